"""gsx_prop_traffic on the GPU: the copies of a propagation call per message, per node
and per link, by class, and their bytes, bit for bit against the expectation of
traffic_cases.py (FIRST / INVALID / DUP from the CPU oracle's first deliverers and
duplicate rows, GRAYLISTED from traffic_model.py; where the model does not apply and the
call graylists copies, that column is checked through its sum).  All integers: equality
is exact."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library loads: both then share one HIP runtime)

import gsx
import oracle as orc
import propagation_cases as pc
import traffic_cases as tc
import traffic_model as tm
from gsx import abi, shard, synth

pytestmark = pytest.mark.gpu

SENT, FIRST, DUP, INVALID, GRAY = range(5)


def engine(key, **kw):
    e = gsx.Engine(1)
    ov, ms, cfg = tc.load(e, key, **kw)
    return e, ov, ms, cfg


def check_identities(t, out, ov, st=None, sizes=None):
    """What holds of every call, whatever the expectation: `out` the call's gsx_prop_out."""
    o = out if isinstance(out, dict) else out.as_dict()
    want = [o["transmissions"], o["deliveries"], o["duplicates"], o["rejected"] + o["ignored"], o["graylisted"]]
    assert t.msg.sum(0, dtype=np.int64).tolist() == want
    assert t.node.sum(0, dtype=np.int64).tolist() == want
    assert int(t.pair.sum(dtype=np.int64)) == o["transmissions"]
    obs = ov.pair_observer()
    by_col = np.bincount(ov.col, weights=t.pair, minlength=ov.n).astype(np.int64)
    by_obs = np.bincount(obs, weights=t.pair, minlength=ov.n).astype(np.int64)
    assert np.array_equal(t.node[:, SENT], by_col)
    assert np.array_equal(t.node[:, FIRST:].sum(1, dtype=np.int64), by_obs)
    assert np.array_equal(t.msg[:, SENT], t.msg[:, FIRST:].sum(1, dtype=np.int64))
    if st is not None:
        assert np.array_equal(t.node[:, FIRST].astype(np.int64) + t.node[:, INVALID], st.node_received)
    up = np.zeros(ov.n, dtype=np.uint64)
    down = np.zeros(ov.n, dtype=np.uint64)
    np.add.at(up, ov.col, t.pair_bytes)
    np.add.at(down, obs, t.pair_bytes)
    assert np.array_equal(t.node_bytes[:, 0], up) and np.array_equal(t.node_bytes[:, 1], down)
    if sizes is None:
        assert np.array_equal(t.pair_bytes, t.pair) and np.array_equal(t.node_bytes[:, 0], t.node[:, SENT])


def check(t, x, ov, sizes=None):
    """t against the expectation x (traffic_cases.Expect), every table bit for bit."""
    msg, node, nbytes, pair, pbytes = tm.tables(x.B, ov.row_ptr, ov.col, sizes)
    cols = slice(None) if x.gray_known else [FIRST, DUP, INVALID]
    assert np.array_equal(t.msg[:, cols], msg[:, cols]), np.argwhere(t.msg != msg)[:5]
    assert np.array_equal(t.node[:, cols], node[:, cols]), np.argwhere(t.node != node)[:5]
    if x.gray_known:
        assert np.array_equal(t.pair, pair), np.argwhere(t.pair != pair)[:5]
        assert np.array_equal(t.node_bytes, nbytes), np.argwhere(t.node_bytes != nbytes)[:5]
        assert np.array_equal(t.pair_bytes, pbytes), np.argwhere(t.pair_bytes != pbytes)[:5]
    else:  # the graylisted copies only through their sum (check_identities: == out.graylisted)
        assert (t.pair >= pair).all() and (t.msg[:, SENT] >= msg[:, SENT]).all()


@pytest.mark.parametrize("key", list(tc.CASES))
def test_every_table_of_every_case(gpu_ok, key):
    x = tc.reference(key)
    e, ov, ms, cfg = engine(key)
    out = e.propagate(ms, cfg)[0]
    assert out.as_dict() == x.out
    sz = tc.sizes("planes", len(ms))
    t = e.prop_traffic(len(ms), sz, per_node=True, per_pair=True)
    check_identities(t, out, ov, e.prop_stats(len(ms), per_node=True), sz)
    check(t, x, ov, sz)
    assert not t.node[tc.LONE].any() and not t.node_bytes[tc.LONE].any()
    if key in ("invalid", "random-invalid", "cut1", "fanout"):
        assert t.total(INVALID) > 0
    if key in ("gossip-m300", "invalid", "cut2"):
        assert t.total(GRAY) > 0 and x.gray_known
    if key == "fanout":
        assert (tc.joined_mask()[ms["source"]] == 0).any()  # a publisher that has not joined: its fanout


@pytest.mark.parametrize("key", ["gossip-m129", "gossip-m300", "invalid"])
def test_sizes(gpu_ok, key):
    """The copy tables do not depend on the sizes; the byte tables are the copies weighted by them."""
    x = tc.reference(key)
    e, ov, ms, cfg = engine(key)
    out = e.propagate(ms, cfg)[0]
    first = None
    for kind in tc.SIZE_KINDS:
        sz = tc.sizes(kind, len(ms))
        t = e.prop_traffic(len(ms), sz, per_node=True, per_pair=True)
        check(t, x, ov, sz)
        check_identities(t, out, ov, None, sz)
        if kind == "zero":
            assert not t.node_bytes.any() and not t.pair_bytes.any() and t.sent() > 0
        if kind == "equal":
            assert np.array_equal(t.pair_bytes, t.pair.astype(np.uint64) * np.uint64(1500))
        if kind == "planes":
            assert int(t.pair_bytes.max()) >= 1 << 33  # sums past 32 bits
        first = first or t
        for a, b in ((t.msg, first.msg), (t.node, first.node), (t.pair, first.pair)):
            assert np.array_equal(a, b)


def test_enforced_gater(gpu_ok):
    """gsx_gater_enforce with AcceptControl pairs: every edge gossipsub, no direct peer, no flood
    publish, no credits, so the oracle with exactly the throttled pairs pushed below
    GraylistThreshold is the reference (test_gpu_gater.py), and the model's gin_extra the
    GRAYLISTED rows."""
    import ctypes as C

    e, ov, ms, _ = engine("plain", score_spread=False)
    ora = orc.Oracle(1)
    tc.load(ora, "plain", score_spread=False)
    ora.set_dup_tracking(True)
    cfg = pc.config(tc.GOSSIP, credit=0, flood_publish=0)
    gp = abi.GaterParams()
    assert e.lib.gsx_default_gater_params(C.byref(gp)) == 0
    gp.threshold, gp.quiet_ns = 0.1, abi.HOUR
    e.set_gater_params(gp)
    E = ov.n_pairs
    rng = np.random.default_rng(41)
    ev = [(abi.GATER_ADD_PEER, 0, p, pc.T0, 0, 0) for p in range(E)]
    ev += [(abi.GATER_REJECT, 0, int(ov.row_ptr[u]), pc.T0, 7, 0) for u in range(ov.n) if ov.row_ptr[u] < ov.row_ptr[u + 1]]
    ev += [(abi.GATER_REJECT, 0, int(p), pc.T0, 8, 0) for p in np.nonzero(rng.random(E) < 0.3)[0]]
    e.gater_events(np.array(ev, dtype=abi.gater_event_dtype()))
    throttled = e.accept_from(pc.T0 + 3 * pc.S, 9, 0) == 1  # GSX_ACCEPT_CONTROL
    assert throttled.any() and not throttled.all()
    e.gater_enforce(True)
    model = tm.run_on(ora, ov, ms, cfg, gin_extra=throttled)
    ora.set_app_scores(np.where(throttled, -1000.0, 0.0))
    x = tc.expect_from(ora, ov, ms, cfg, model)
    out = e.propagate(ms, cfg)[0]
    for f in ("deliveries", "duplicates", "graylisted", "transmissions"):
        assert getattr(out, f) == x.out[f], f
    assert out.graylisted > 0
    t = e.prop_traffic(len(ms), per_node=True, per_pair=True)
    check_identities(t, out, ov, e.prop_stats(len(ms), per_node=True))
    check(t, x, ov)
    obs = ov.pair_observer()
    assert np.array_equal(t.node[:, GRAY], np.bincount(obs, weights=t.pair * throttled, minlength=ov.n).astype(np.int64))


def duplicate_rows(e, m):
    """gsx_prop_duplicates with the call's own row length (abi.prop_words: padded above two words)."""
    import ctypes as C

    W = abi.prop_words(m)
    rows = np.zeros((e.n_pairs, W), dtype=np.uint64)
    e._chk(e.lib.gsx_prop_duplicates(e.h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), W), "gsx_prop_duplicates")
    return rows


def test_stale_state(gpu_ok):
    """One engine through calls of m = 130, 5, 64 with router and topic-independent state changing:
    the traffic after each call is that call's alone, twice the same, and nothing else moves."""
    ov = tc.overlay(True)
    e, ora = gsx.Engine(1), orc.Oracle(1)
    for be in (e, ora):
        pc.setup(be, ov, 1, tc.SEED)
    ora.set_dup_tracking(True)
    for m, router, fp in ((130, tc.GOSSIP, 1), (5, tc.FLOOD, 0), (64, tc.RANDOM, 0), (130, tc.GOSSIP, 0)):
        ms = pc.messages(tc.N, m, 90 + m, invalid=0.2 if m == 130 else 0.0)
        cfg = pc.config(router, flood_publish=fp, size=8, credit=0, delay_ms=1.0)
        model = tm.run_on(ora, ov, ms, cfg) if router != tc.RANDOM else None
        x = tc.expect_from(ora, ov, ms, cfg, model)
        out = e.propagate(ms, cfg)[0]
        assert out.as_dict() == x.out
        before = (e.prop_results(m), e.prop_stats(m, per_node=True), duplicate_rows(e, m), e.export_state(), e.scores())
        assert np.array_equal(tm.bits_of_words(before[2], m), x.B[DUP])
        sz = tc.sizes("random", m)
        a = e.prop_traffic(m, sz, per_node=True, per_pair=True)
        b = e.prop_traffic(m, sz, per_node=True, per_pair=True)
        check(a, x, ov, sz)
        check_identities(a, out, ov, before[1], sz)
        for f in ("msg", "node", "node_bytes", "pair", "pair_bytes"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        after = (e.prop_results(m), e.prop_stats(m, per_node=True), duplicate_rows(e, m), e.export_state(), e.scores())
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
        assert np.array_equal(before[1].hop_hist, after[1].hop_hist)
        assert np.array_equal(before[2], after[2])
        for k, v in before[3].items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v.view(np.uint8), after[3][k].view(np.uint8)), k
        assert np.array_equal(before[4].view(np.uint64), after[4].view(np.uint64))


@pytest.mark.parametrize("credit", [abi.GSX_CREDIT_NOW, abi.GSX_CREDIT_DEFER])
def test_credit_modes(gpu_ok, credit):
    """The scores move after the call (folded or deferred credits); the traffic describes the call."""
    key = "invalid"
    res = []
    for c in (abi.GSX_CREDIT_OFF, credit):
        e, ov, ms, cfg = engine(key)
        cfg.credit_scores = c
        out = e.propagate(ms, cfg)[0]
        t = e.prop_traffic(len(ms), per_node=True, per_pair=True)
        check_identities(t, out, ov)
        res.append((t, e.scores()))
    check(res[1][0], tc.reference(key), ov)
    for f in ("msg", "node", "node_bytes", "pair", "pair_bytes"):
        assert np.array_equal(getattr(res[0][0], f), getattr(res[1][0], f)), f
    if credit == abi.GSX_CREDIT_NOW:
        assert not np.array_equal(res[0][1], res[1][1])  # the credits did move scores


def test_device_pointers_and_null_outputs(gpu_ok):
    import itertools

    import torch

    key = "gossip-m129"
    e, ov, ms, cfg = engine(key)
    e.propagate(ms, cfg)
    m, n, E = len(ms), ov.n, ov.n_pairs
    sz = tc.sizes("random", m)
    host = e.prop_traffic(m, sz, per_node=True, per_pair=True)
    check(host, tc.reference(key), ov, sz)
    names = ("msg", "node", "node_bytes", "pair", "pair_bytes")
    shapes = ((m, 5), (n, 5), (n, 2), (E,), (E,))
    dts = (torch.int32, torch.int32, torch.int64, torch.int32, torch.int64)
    for mask in itertools.product((0, 1), repeat=5):  # every subset of NULL outputs, on the device
        bufs = [torch.full(s, -1, dtype=d, device="cuda:0") if on else None for s, d, on in zip(shapes, dts, mask)]
        torch.cuda.synchronize()
        assert e.prop_traffic(m, sz, out_ptrs=bufs) is None
        e.sync()
        for name, b in zip(names, bufs):
            if b is not None:
                want = getattr(host, name)
                assert np.array_equal(b.cpu().numpy().view(want.dtype).reshape(want.shape), want), (mask, name)
    # host outputs: the per_node / per_pair subsets
    only_msg = e.prop_traffic(m, sz, per_node=False)
    assert only_msg.node is None and only_msg.pair is None and np.array_equal(only_msg.msg, host.msg)
    pairs = e.prop_traffic(m, sz, per_node=False, per_pair=True)
    assert np.array_equal(pairs.pair_bytes, host.pair_bytes) and np.array_equal(pairs.pair, host.pair)
    # one host output alone, the others NULL
    nb = np.zeros((n, 2), dtype=np.uint64)
    e._chk(e.lib.gsx_prop_traffic(e.h, sz.ctypes.data, None, None, nb.ctypes.data, None, None), "gsx_prop_traffic")
    assert np.array_equal(nb, host.node_bytes)


def test_refusals(gpu_ok):
    key = "gossip-m65"
    e, ov, ms, cfg = engine(key)
    want = tc.reference(key)

    def refused(code, quiet=True):
        st = e.export_state() if quiet else None
        with pytest.raises(gsx.GsxError) as ei:
            e.prop_traffic(len(ms))
        assert ei.value.code == code, ei.value
        if quiet:  # the engine is as it was
            for k, v in e.export_state().items():
                if isinstance(v, np.ndarray):
                    assert np.array_equal(v.view(np.uint8), st[k].view(np.uint8)), k

    refused(abi.GSX_ESTATE)  # before any propagation
    e.prop_begin(ms, cfg)
    e.prop_step(0)
    refused(abi.GSX_ESTATE, quiet=False)  # a stepped call in flight
    for _ in range(cfg.max_hops - 1):
        e.prop_step(0)
    out = e.prop_end()
    t = e.prop_traffic(len(ms), per_node=True, per_pair=True)  # the stepped call's traffic
    check(t, want, ov)
    check_identities(t, out, ov)
    lat = np.ones(ov.n_pairs, dtype=np.uint8)
    e.set_link_latency(lat)
    e.propagate_timed(ms, cfg, 8)
    refused(abi.GSX_ESTATE)  # after a timed call
    e.set_prop_tracking(False)
    cfg2 = pc.config(tc.GOSSIP, credit=0)
    e.propagate(ms, cfg2)
    refused(abi.GSX_ESTATE)  # first deliverers not tracked
    e.set_prop_tracking(True)
    cfg3 = pc.config(tc.RANDOM, credit=0, size=8)
    e.set_prop_tracking(False)
    out = e.propagate(ms, cfg3)[0]  # RandomSub always keeps them
    check_identities(e.prop_traffic(len(ms), per_node=True, per_pair=True), out, ov)
    assert e.lib.gsx_prop_traffic(None, None, None, None, None, None, None) == abi.GSX_EINVAL


def test_range_shard_is_refused(gpu_ok):
    """A loaded range shard refuses the call, whatever else its state is."""
    ov = tc.overlay(True)
    e = gsx.Engine(1)
    e.set_peer_params(synth.bench_peer_params())
    e.set_topic_params(0, synth.spam_test_topic_params())
    lo, hi = 0, ov.n // 2
    sh = synth.shard_of(ov, lo, hi)
    e.load_overlay_shard(ov.n, lo, sh.row_ptr, sh.col, sh.edge_flags, sh.node_ips)
    with pytest.raises(gsx.GsxError) as ei:
        e.prop_traffic(10)
    assert ei.value.code == abi.GSX_EINVAL


@pytest.mark.parametrize("world,m", [(2, 130), (3, 131)])
def test_message_parallel(gpu_ok, world, m):
    ov = tc.overlay(True)
    ms = pc.messages(tc.N, m, 50 + m, invalid=0.1)
    cfg = pc.config(tc.GOSSIP, flood_publish=1, delay_ms=1.0)
    sz = tc.sizes("random", m)
    full = gsx.Engine(1)
    pc.setup(full, ov, 1, tc.SEED)
    out = full.propagate(ms, cfg)[0]
    want = full.prop_traffic(m, sz, per_node=True, per_pair=True)
    check_identities(want, out, ov, None, sz)
    reps = []
    for _ in range(world):
        e = gsx.Engine(1)
        pc.setup(e, ov, 1, tc.SEED)
        reps.append(e)

    def run(tp, e):
        mp = shard.MessageParallel(e, tp)
        mp.propagate(ms, cfg)
        return mp.prop_traffic(m, sz, per_node=True, per_pair=True)

    for t in shard.run_local(world, "cuda:0", run, [(e,) for e in reps]):
        for f in ("msg", "node", "node_bytes", "pair", "pair_bytes"):
            assert np.array_equal(getattr(t, f), getattr(want, f)), f

    def untracked(tp, e):
        e.set_prop_tracking(False)
        mp = shard.MessageParallel(e, tp)
        mp.propagate(ms, cfg)
        return mp.prop_traffic(m)

    if world == 2:
        with pytest.raises(gsx.GsxError) as ei:
            shard.run_local(world, "cuda:0", untracked, [(e,) for e in reps])
        assert ei.value.code == abi.GSX_ESTATE


def test_n_msgs_must_be_the_last_calls(gpu_ok):
    e, ov, ms, cfg = engine("gossip-m65")
    e.propagate(ms, cfg)
    with pytest.raises(ValueError):
        e.prop_traffic(len(ms) - 1)
    assert e.prop_traffic(len(ms)).msg.shape == (len(ms), 5)


def test_overflow_refusal(gpu_ok):
    """(longest row) x n_msgs >= 2^32 is refused with GSX_EINVAL: a hub of 2^16 peers and 2^16
    messages, one hop from a leaf (the smallest shape that trips the product; the call itself
    is 2^16 copies).  One message fewer passes that test and meets the next one (tracking is
    off: GSX_ESTATE), so the bound is exact.  The engine is as it was after either refusal."""
    D = 1 << 16
    n = D + 1
    row_ptr = np.concatenate([[0], D + np.arange(n)]).astype(np.int64)  # node 0: the hub; every other node: one pair
    col = np.concatenate([np.arange(1, n), np.zeros(D)]).astype(np.int32)
    ips, _ = synth._ips(n, 0.0, 50)
    e = gsx.Engine(1)
    e.set_peer_params(synth.bench_peer_params())
    e.set_topic_params(0, synth.spam_test_topic_params())
    e.load_overlay(row_ptr, col, np.full(2 * D, abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8), ips)
    ev = np.zeros(2 * D, dtype=abi.event_dtype())
    ev["kind"], ev["pair"], ev["now_ns"] = abi.EV_ADD_PEER, np.arange(2 * D), pc.T0
    e.apply_events(ev)
    e.refresh(pc.T0 + pc.S)
    e.set_prop_tracking(False)
    cfg = pc.config(tc.FLOOD, max_hops=1, credit=0)
    for m, code in ((D - 1, abi.GSX_ESTATE), (D, abi.GSX_EINVAL)):
        ms = np.zeros(m, dtype=abi.msg_dtype())
        ms["source"], ms["msg_id"] = 1, np.arange(m) + 1
        out = e.propagate(ms, cfg)[0]
        assert out.deliveries == m and out.transmissions == m  # the leaf's one peer, the hub
        st = e.export_state()
        with pytest.raises(gsx.GsxError) as ei:
            e.prop_traffic(m)
        assert ei.value.code == code, ei.value
        for k, v in e.export_state().items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v.view(np.uint8), st[k].view(np.uint8)), k
    e.close()

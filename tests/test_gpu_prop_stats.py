"""gsx_prop_stats on the GPU: the per-message hop histogram and the per-node
receipt counts / hop sums of a propagation call, reduced on the device, against
numpy on the CPU oracle's [message][node] hop matrix.  All integers: equality is
exact."""
import functools

import numpy as np
import pytest

import gsx
import oracle as orc
import propagation_cases as pc
from gsx import abi, synth

pytestmark = pytest.mark.gpu

H = abi.GSX_MAX_HOPS + 1
FLOOD, GOSSIP, RANDOM = abi.GSX_ROUTER_FLOODSUB, abi.GSX_ROUTER_GOSSIPSUB, abi.GSX_ROUTER_RANDOMSUB


def expected(hop):
    """hop [m, n] u8 (0xFF never) -> (hist [m, 65] u32, node_received [n] u32, node_hop_sum [n] u64)"""
    hist = np.zeros((hop.shape[0], H), dtype=np.uint32)
    for k, row in enumerate(hop):
        hist[k] = np.bincount(row, minlength=256)[:H]
    got = (hop >= 1) & (hop <= abi.GSX_MAX_HOPS)
    return hist, got.sum(0).astype(np.uint32), (hop.astype(np.uint64) * got).sum(0).astype(np.uint64)


def check(st, hop):
    hist, recv, hsum = expected(hop)
    assert np.array_equal(st.hop_hist, hist), np.argwhere(st.hop_hist != hist)[:5]
    assert np.array_equal(st.node_received, recv), np.argwhere(st.node_received != recv)[:5]
    assert np.array_equal(st.node_hop_sum, hsum), np.argwhere(st.node_hop_sum != hsum)[:5]


def one_node_overlay():
    ips, sybil = synth._ips(1, 0.0, 50)
    return synth.Overlay(1, np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8),
                         ips, sybil)


def path_overlay(n):
    """0 - 1 - 2 - ... - (n - 1), gossipsub peers."""
    deg = np.full(n, 2, dtype=np.int64)
    deg[0] = deg[-1] = 1
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([[v for v in (i - 1, i + 1) if 0 <= v < n] for i in range(n)]).astype(np.int32)
    ips, sybil = synth._ips(n, 0.0, 50)
    return synth.Overlay(n, row_ptr, col, np.full(len(col), abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8), ips, sybil)


def make_overlay(n, d, seed, mix):
    if n == 1:
        return one_node_overlay()
    return pc.overlay(n, d, seed, mix_protocols=mix, direct_frac=0.02 if mix else 0.0)


def long_window(be, T=1):
    """A 5-minute P3 window: every duplicate inside it (the lean hop kernels, with tracking off)."""
    for t in range(T):
        tp = synth.spam_test_topic_params()
        tp.mesh_message_deliveries_window_ns = 300_000 * abi.MILLISECOND
        be.set_topic_params(t, tp)


# key -> n, d, router, m, mix, disconnect, invalid, max_hops, lean
CASES = {
    # tile and word edges: every n of {1, 63, 64, 65, 130, 1500} and every m of {1, 63, 64, 65, 130, 1024}
    "n1-m1": (1, 0, FLOOD, 1, False, 0.0, 0.0, 40, False),
    "n63-m65": (63, 3, GOSSIP, 65, False, 0.0, 0.0, 40, False),
    "n64-m63": (64, 3, FLOOD, 63, False, 0.0, 0.0, 40, False),
    "n65-m64": (65, 3, GOSSIP, 64, True, 0.0, 0.0, 40, False),
    "n130-m130": (130, 3, RANDOM, 130, False, 0.05, 0.0, 40, False),
    "n64-m1024": (64, 3, FLOOD, 1024, False, 0.0, 0.0, 40, False),
    "n130-m1": (130, 3, GOSSIP, 1, True, 0.0, 0.0, 40, False),
    # every router, mixed protocols, removed peers: some nodes never receive
    "n1500-flood-m1024": (1500, 2, FLOOD, 1024, True, 0.4, 0.0, 40, False),
    "n1500-gossip-m130": (1500, 2, GOSSIP, 130, True, 0.4, 0.0, 40, False),
    "n1500-random-m64": (1500, 2, RANDOM, 64, True, 0.4, 0.0, 40, False),
    # dropped / rejected messages, a call cut by max_hops, the lean path
    "invalid": (500, 5, GOSSIP, 200, True, 0.03, 0.25, 40, False),
    "cut": (1500, 4, GOSSIP, 130, True, 0.02, 0.0, 3, False),
    "lean-m40": (1500, 6, GOSSIP, 40, True, 0.02, 0.0, 40, True),
    "lean-m200": (1500, 6, GOSSIP, 200, True, 0.02, 0.0, 40, True),
    # the base of the API tests
    "base": (500, 5, GOSSIP, 130, True, 0.05, 0.0, 40, False),
    "base-m200": (500, 5, GOSSIP, 200, True, 0.05, 0.0, 40, False),
    "base-m40": (500, 5, GOSSIP, 40, True, 0.05, 0.0, 40, False),
}
NEVER = ("n1500-flood-m1024", "n1500-gossip-m130", "n1500-random-m64")


def inputs(key):
    n, d, router, m, mix, disc, invalid, max_hops, lean = CASES[key]
    seed = 7 * n + m
    ov = make_overlay(n, d, seed, mix)
    ms = pc.messages(n, m, seed, invalid=invalid)
    cfg = pc.config(router, max_hops=max_hops, size=50, delay_ms=2.0 if invalid else 0.0)
    return ov, ms, cfg, seed, disc, lean


def load(be, key):
    ov, ms, cfg, seed, disc, lean = inputs(key)
    pc.setup(be, ov, 1, seed, disconnect_frac=disc)
    if lean:
        long_window(be)
    return ms, cfg


@functools.lru_cache(maxsize=None)
def reference(key):
    """The CPU oracle's run of a case, computed once: (PropOut dict, hop [m, n] u8)."""
    o = orc.Oracle(1)
    ms, cfg = load(o, key)
    out, hop, _ = o.propagate(ms, cfg, want_results=True)
    hop.setflags(write=False)
    return out.as_dict(), hop


def engine(key, track=True):
    e = gsx.Engine(1)
    ms, cfg = load(e, key)
    if CASES[key][8]:
        track = False
    e.set_prop_tracking(track)
    return e, ms, cfg


@pytest.mark.parametrize("key", [k for k in CASES if k.startswith("n")])
def test_tile_and_word_edges(gpu_ok, key):
    want_out, hop = reference(key)
    e, ms, cfg = engine(key)
    out = e.propagate(ms, cfg)[0]
    assert out.as_dict() == want_out
    st = e.prop_stats(len(ms), per_node=True)
    check(st, hop)
    assert np.array_equal(st.hop_hist[:, 0], np.ones(len(ms), dtype=np.uint32))  # one source each
    if key in NEVER:
        assert (hop == 0xFF).any()  # the complement n - sum(row) is exercised
        assert (st.hop_hist.sum(1) < CASES[key][0]).any()
        assert want_out["deliveries"] > 0


def test_dropped_messages(gpu_ok):
    want_out, hop = reference("invalid")
    e, ms, cfg = engine("invalid")
    out = e.propagate(ms, cfg)[0]
    st = e.prop_stats(len(ms), per_node=True)
    check(st, hop)
    bad = ms["validation"] != abi.GSX_VALIDATION_ACCEPT
    assert bad.any() and (st.hop_hist[bad, 1] > 0).any()  # received at hop 1, never forwarded
    assert not st.hop_hist[bad, 2:].any()
    assert st.hop_hist[:, 1:].sum() == out.deliveries + out.rejected + out.ignored
    assert out.rejected > 0 and out.ignored > 0 and out.deliveries > 0


def test_call_cut_by_max_hops(gpu_ok):
    want_out, hop = reference("cut")
    e, ms, cfg = engine("cut")
    out = e.propagate(ms, cfg)[0]
    assert out.hops == 3
    st = e.prop_stats(len(ms), per_node=True)
    check(st, hop)
    assert st.hop_hist[:, 3].any() and not st.hop_hist[:, 4:].any()
    assert (st.last_hop() <= 3).all()


def test_row_64_of_a_path(gpu_ok):
    """70 nodes in a line, one message from node 0, max_hops = 64: one node at every hop
    0 .. 64 (the history's last row, GSX_MAX_HOPS, included), the other five never reached."""
    ov = path_overlay(70)
    ms = np.zeros(1, dtype=abi.msg_dtype())
    ms["msg_id"] = 1
    cfg = pc.config(FLOOD, max_hops=abi.GSX_MAX_HOPS, credit=0)
    res = []
    for be in (gsx.Engine(1), orc.Oracle(1)):
        pc.setup(be, ov, 1, 3, score_spread=False)
        res.append((be, be.propagate(ms, cfg, want_results=True)))
    e, (out, ghop, _) = res[0]
    hop = res[1][1][1]
    assert np.array_equal(hop[0], np.concatenate([np.arange(65), [0xFF] * 5]).astype(np.uint8))
    assert np.array_equal(ghop, hop)
    st = e.prop_stats(1, per_node=True)
    check(st, hop)
    assert np.array_equal(st.hop_hist[0], np.ones(H, dtype=np.uint32))
    assert 70 - int(st.hop_hist[0].sum()) == 5
    assert st.last_hop()[0] == 64 and st.reached()[0] == 64


def test_tracking_off_gives_the_same(gpu_ok):
    _, hop = reference("base")
    for track in (True, False):
        e, ms, cfg = engine("base", track=track)
        e.propagate(ms, cfg)
        check(e.prop_stats(len(ms), per_node=True), hop)


@pytest.mark.parametrize("key", ["lean-m40", "lean-m200"])
def test_lean_path(gpu_ok, key):
    want_out, hop = reference(key)
    e, ms, cfg = engine(key)
    out = e.propagate(ms, cfg)[0]
    assert out.as_dict() == want_out and out.deliveries > 0
    check(e.prop_stats(len(ms), per_node=True), hop)


def test_stepped_api(gpu_ok):
    _, hop = reference("base")
    e, ms, cfg = engine("base")
    e.prop_begin(ms, cfg)
    for _ in range(cfg.max_hops):
        e.prop_step(0)
    e.prop_end()
    check(e.prop_stats(len(ms), per_node=True), hop)


def test_device_pointer_output(gpu_ok):
    import torch

    _, hop = reference("base")
    e, ms, cfg = engine("base")
    e.propagate(ms, cfg)
    host = e.prop_stats(len(ms), per_node=True)
    hist = torch.full((len(ms), H), -1, dtype=torch.int32, device="cuda:0")
    recv = torch.full((e.n_nodes,), -1, dtype=torch.int32, device="cuda:0")
    hsum = torch.full((e.n_nodes,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert e.prop_stats(len(ms), out_ptrs=(hist, recv, hsum)) is None
    e.sync()
    dev = gsx.PropStats(hist.cpu().numpy().view(np.uint32), recv.cpu().numpy().view(np.uint32),
                        hsum.cpu().numpy().view(np.uint64))
    check(dev, hop)
    assert np.array_equal(dev.hop_hist, host.hop_hist)
    # one output alone
    hist.fill_(-1)
    torch.cuda.synchronize()
    e.prop_stats(len(ms), out_ptrs=(hist, None, None))
    e.sync()
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), host.hop_hist)


def test_two_calls_with_different_m(gpu_ok):
    """m = 200 then m = 40 on one engine: nothing of the first call in the second result
    (the scratch, the rows' stride, the last word's upper bits)."""
    n = CASES["base-m200"][0]
    ms40 = pc.messages(n, 40, 7 * n + 40)
    o = orc.Oracle(1)
    ms200, cfg = load(o, "base-m200")
    _, hop200, _ = o.propagate(ms200, cfg, want_results=True)
    _, hop40, _ = o.propagate(ms40, cfg, want_results=True)  # (on the scores the first call credited)
    e, _, _ = engine("base-m200")
    e.propagate(ms200, cfg)
    check(e.prop_stats(200, per_node=True), hop200)
    e.propagate(ms40, cfg)
    st = e.prop_stats(40, per_node=True)
    check(st, hop40)
    assert st.hop_hist.shape == (40, H) and st.reached().sum() > 0


def test_state_errors(gpu_ok):
    e, ms, cfg = engine("base-m40")
    with pytest.raises(gsx.GsxError) as ei:
        e.prop_stats(len(ms))
    assert ei.value.code == abi.GSX_ESTATE
    e.prop_begin(ms, cfg)
    e.prop_step(0)
    with pytest.raises(gsx.GsxError) as ei:
        e.prop_stats(len(ms))
    assert ei.value.code == abi.GSX_ESTATE
    for _ in range(cfg.max_hops - 1):
        e.prop_step(0)
    e.prop_end()
    check(e.prop_stats(len(ms), per_node=True), reference("base-m40")[1])
    assert e.lib.gsx_prop_stats(None, None, None, None) == abi.GSX_EINVAL


def test_repeatable_and_consistent_with_prop_out(gpu_ok):
    want_out, hop = reference("base")
    e, ms, cfg = engine("base")
    out = e.propagate(ms, cfg)[0]
    a = e.prop_stats(len(ms), per_node=True)
    b = e.prop_stats(len(ms), per_node=True)
    for x, y in ((a.hop_hist, b.hop_hist), (a.node_received, b.node_received), (a.node_hop_sum, b.node_hop_sum)):
        assert np.array_equal(x, y)
    check(a, hop)
    assert np.array_equal(a.hop_hist[:, 1:].sum(0), np.array(out.hop_deliveries, dtype=np.int64)[1:])
    assert a.reached().sum() == out.deliveries > 0
    assert int(a.node_received.sum()) == out.deliveries

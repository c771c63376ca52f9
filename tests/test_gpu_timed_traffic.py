"""gsx_timed_traffic on the GPU against the copy-by-copy model (timed_traffic_model.py,
itself checked against timed_model.py and traffic_model.py in test_timed_traffic_model.py):
every table bit for bit, on the small shapes of test_gpu_timed_prop.py.  All integers:
equality is exact everywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import gsx
import propagation_cases as pc
import timed_traffic_model as ttm
from gsx import abi, synth
from test_gpu_timed_prop import SHAPES, DevBuf, make, rc_of, same_state, shape, tcfg

pytestmark = pytest.mark.gpu

TT = gsx.TimedTraffic
NAMES = ttm.Tables.NAMES
GS = abi.GSX_ROUTER_GOSSIPSUB


def sizes_of(kind, m):
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros(m, dtype=np.uint32)
    if kind == "1500":
        return np.full(m, 1500, dtype=np.uint32)
    if kind == "huge":  # the sums pass 2^32 at once
        return np.full(m, 2 ** 32 - 1, dtype=np.uint32)
    return ((np.arange(m, dtype=np.uint64) * 977 + 13) % 1500).astype(np.uint32)


def same_tables(t, want, names=NAMES):
    for f in names:
        a, b = getattr(t, f), getattr(want, f)
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape, f
        assert np.array_equal(a, b), (f, np.argwhere(a != b)[:5])


def identities(t, out):
    for tab in (t.msg, t.node, t.bins):
        s = tab.astype(np.int64).sum(0)
        assert s[TT.SENT] == s[TT.FIRST:TT.IN_FLIGHT + 1].sum()
        assert s[TT.SENT] - s[TT.IN_FLIGHT] == out.transmissions
        assert (s[TT.FIRST], s[TT.DUP], s[TT.INVALID], s[TT.GRAYLISTED], s[TT.DUP_IN_WINDOW]) == \
            (out.deliveries, out.duplicates, out.rejected + out.ignored, out.graylisted, out.dup_in_window)
    assert t.bin_bytes.sum(0).tolist() == t.node_bytes.sum(0).tolist()


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_table_equals_the_model(gpu_ok, name, symmetric):
    ov, ms = shape(name)
    T, m = SHAPES[name][3], len(shape(name)[1])
    lat = synth.link_latency(ov, 11, 1, 9, symmetric=symmetric)
    sz = sizes_of("random", m)
    with make(gsx.Engine(T), name) as e:
        R = ttm.run_on(e, ov, lat, ms, tcfg(name), 65534, T=T)
        e.set_link_latency(lat)
        out, _, _ = e.propagate_timed(ms, tcfg(name, credit=abi.GSX_CREDIT_DEFER), 65534)
        for bin_ticks, n_bins in ((1, 64), (3, 20)):
            t = e.timed_traffic(m, sz, bin_ticks, n_bins, per_pair=True)
            same_tables(t, ttm.tables(R, sz, bin_ticks, n_bins))
            identities(t, out)
        again = e.timed_traffic(m, sz, 3, 20, per_pair=True)
        for f in NAMES:
            assert getattr(t, f).tobytes() == getattr(again, f).tobytes(), f
        if name == "gossipsub":  # a late duplicate outside the window
            assert 0 < t.total(TT.DUP_IN_WINDOW) < t.total(TT.DUP)
        assert t.in_flight() == 0 and t.tick_ns == SHAPES[name][9] * abi.MILLISECOND


def test_max_ticks_cut(gpu_ok):
    """The cut of test_max_ticks_cuts_the_call, without and with a validation delay of 3 ticks
    (with it, the nodes that got a message in the last 3 ticks never send it)."""
    name = "gossipsub"
    ov, ms = shape(name)
    m = len(ms)
    lat = synth.link_latency(ov, 11, 1, 9)
    own = np.zeros(ov.n, dtype=bool)
    own[ms["source"]] = True
    for vd in (0, 3):
        cfg = pc.config(GS, latency_ms=5, delay_ms=5.0 * vd, credit=abi.GSX_CREDIT_DEFER)
        with make(gsx.Engine(2), name) as e:
            full = ttm.run_on(e, ov, lat, ms, cfg, 65534, T=2)
            cut = max(int(full.tick[full.tick != 0xFFFF].max()) // 2, 1)
            R = ttm.run_on(e, ov, lat, ms, cfg, cut, T=2)
            e.set_link_latency(lat)
            out, tick, _ = e.propagate_timed(ms, cfg, cut, want_results=True)
            t = e.timed_traffic(m, None, 1, 64, per_pair=True)
            same_tables(t, ttm.tables(R, None, 1, 64))
            identities(t, out)
            assert t.in_flight() > 0 and t.sent() - t.in_flight() == out.transmissions
            # a node whose every send tick is past the cut sent nothing
            got = tick != 0xFFFF
            first_send = np.where(got, tick.astype(np.int64) + vd, 1 << 30).min(0)
            silent = ~own & (first_send > cut)
            assert got[:, silent].any() or vd == 0
            assert not t.node[silent, TT.SENT].any() and not t.node_bytes[silent, 0].any()
            assert not t.bins[cut + 1:].any()  # nothing is sent or arrives after the cut


@pytest.mark.parametrize("name", ["floodsub", "gossipsub", "floodpub", "delay-invalid"])
def test_uniform_latency_twin_of_prop_traffic(gpu_ok, name):
    """gsx_propagate + gsx_prop_traffic on one engine, the timed call over links of 1 tick +
    gsx_timed_traffic on its twin: copies and bytes are equal column for column."""
    ov, ms = shape(name)
    T, m = SHAPES[name][3], len(ms)
    sz = sizes_of("random", m)
    with make(gsx.Engine(T), name) as a, make(gsx.Engine(T), name) as b:
        a.propagate(ms, tcfg(name, credit=abi.GSX_CREDIT_DEFER))
        p = a.prop_traffic(m, sz, per_node=True, per_pair=True)
        b.set_link_latency(np.ones(ov.n_pairs, dtype=np.uint8))
        b.propagate_timed(ms, tcfg(name, credit=abi.GSX_CREDIT_DEFER), 65534)
        t = b.timed_traffic(m, sz, per_pair=True)
        assert np.array_equal(t.msg[:, :5], p.msg) and np.array_equal(t.node[:, :5], p.node)
        assert np.array_equal(t.node_bytes, p.node_bytes)
        assert np.array_equal(t.pair, p.pair) and np.array_equal(t.pair_bytes, p.pair_bytes)
        assert t.in_flight() == 0 and not t.node[:, TT.IN_FLIGHT].any() and p.sent() > 0


@functools.lru_cache(maxsize=None)
def floodpub_run():
    """One timed call (floodpub: 130 messages, a padded multi-word row) cut at 12 ticks, its engine and model."""
    name = "floodpub"
    ov, ms = shape(name)
    lat = synth.link_latency(ov, 11, 1, 9, symmetric=False)
    e = make(gsx.Engine(1), name)
    R = ttm.run_on(e, ov, lat, ms, tcfg(name), 12)
    e.set_link_latency(lat)
    out, _, _ = e.propagate_timed(ms, tcfg(name, credit=abi.GSX_CREDIT_DEFER), 12)
    return e, ov, ms, R, out


@pytest.mark.parametrize("bin_ticks,n_bins", [(1, 1), (1, 7), (1, 128), (1, 129), (2, 1024), (5, 3)])
def test_bins(gpu_ok, bin_ticks, n_bins):
    """One bin; fewer bins than ticks (the last clamps); both sides of the 128 bins the block
    counts in LDS; the most bins allowed.  The peaks are the row maxima of the model's
    per-(node, bin) table, at the lowest such bin."""
    e, ov, ms, R, out = floodpub_run()
    sz = sizes_of("random", len(ms))
    t = e.timed_traffic(len(ms), sz, bin_ticks, n_bins)
    want = ttm.tables(R, sz, bin_ticks, n_bins)
    same_tables(t, want, [f for f in NAMES if not f.startswith("pair")])
    identities(t, out)
    assert t.in_flight() > 0
    assert np.array_equal(t.node_peak, want.node_bin.max(1))
    low = np.where(want.node_bin.max(1) > 0, (want.node_bin == want.node_bin.max(1)[:, None, :]).argmax(1), 0)
    assert np.array_equal(t.node_peak_bin, low)
    if (bin_ticks, n_bins) == (1, 7):
        assert t.bins[6].astype(np.int64).sum() > t.bins[5].astype(np.int64).sum()  # ticks 6 .. 21 fell into it


@pytest.mark.parametrize("kind", [None, "zero", "1500", "huge"])
def test_sizes(gpu_ok, kind):
    e, ov, ms, R, out = floodpub_run()
    m = len(ms)
    sz = sizes_of(kind, m)
    t = e.timed_traffic(m, sz, 1, 16, per_pair=True)
    same_tables(t, ttm.tables(R, sz, 1, 16))
    base = e.timed_traffic(m, None, 1, 16, per_pair=True)
    for f in ("msg", "node", "pair", "bins"):  # the copies do not depend on the sizes
        assert np.array_equal(getattr(t, f), getattr(base, f)), f
    if kind is None:
        assert np.array_equal(t.node_bytes[:, 0], t.node[:, TT.SENT]) and np.array_equal(t.pair_bytes, t.pair)
    if kind == "huge":
        assert int(t.bin_bytes[:, 0].sum()) > 2 ** 32 and t.node_bytes.max() > 2 ** 32


def test_device_pointers_and_single_outputs(gpu_ok):
    e, ov, ms, R, out = floodpub_run()
    m, B = len(ms), 9
    sz = sizes_of("random", m)
    host = e.timed_traffic(m, sz, 2, B, per_pair=True)
    same_tables(host, ttm.tables(R, sz, 2, B))

    def check_dev(f, b):
        want = getattr(host, f)
        assert np.array_equal(b.read(want.dtype).reshape(want.shape), want), f

    bufs = {f: DevBuf(getattr(host, f).nbytes) for f in NAMES}  # every output in device memory (preset to 0x07 bytes)
    assert e.timed_traffic(m, sz, 2, B, out_ptrs={f: b.ptr for f, b in bufs.items()}) is None
    e.sync()
    for f in NAMES:
        check_dev(f, bufs[f])
    for f in NAMES:  # each output alone, the others NULL: on the device and in host memory
        bufs[f].fill(7)
        e.timed_traffic(m, sz, 2, B, out_ptrs={f: bufs[f].ptr})
        e.sync()
        check_dev(f, bufs[f])
        one = e.timed_traffic(m, sz, 2, B, outputs=[f])
        assert np.array_equal(getattr(one, f), getattr(host, f)), f
        assert all(getattr(one, g) is None for g in NAMES if g != f)
    for b in bufs.values():
        b.free()
    no_bins = e.timed_traffic(m, sz, 2, B, per_bin=False)
    assert no_bins.bins is None and no_bins.node_peak is None and np.array_equal(no_bins.node, host.node)


def test_long_row(gpu_ok):
    """400 nodes, one linked to all others (a row of 399 pairs), gossipsub, 70 messages."""
    ov = pc.with_hub(pc.overlay(400, 6, seed=3, mix_protocols=True), 7, 399, seed=3)
    assert ov.row_ptr[8] - ov.row_ptr[7] == 399
    ms = pc.messages(400, 70, seed=3, invalid=0.1)
    lat = synth.link_latency(ov, 3, 1, 9, symmetric=False)
    cfg = pc.config(GS, latency_ms=5, credit=abi.GSX_CREDIT_DEFER)
    sz = sizes_of("random", 70)
    with gsx.Engine(1) as e:
        pc.setup(e, ov, 1, seed=3)
        R = ttm.run_on(e, ov, lat, ms, cfg, 65534)
        e.set_link_latency(lat)
        out, _, _ = e.propagate_timed(ms, cfg, 65534)
        t = e.timed_traffic(70, sz, 1, 32, per_pair=True)
        same_tables(t, ttm.tables(R, sz, 1, 32))
        identities(t, out)
        assert t.busiest(1, by="sent")[0] == 7


def test_more_words_than_the_block_table_holds(gpu_ok):
    """1100 messages are 18 words: the last two are counted past the block's 16-word table."""
    ov = pc.overlay(40, 5, seed=9)
    m = 1100
    ms = pc.messages(40, m, seed=9, invalid=0.05)
    lat = synth.link_latency(ov, 9, 1, 5)
    cfg = pc.config(abi.GSX_ROUTER_FLOODSUB, latency_ms=5, credit=abi.GSX_CREDIT_DEFER)
    sz = sizes_of("random", m)
    with gsx.Engine(1) as e:
        pc.setup(e, ov, 1, seed=9)
        R = ttm.run_on(e, ov, lat, ms, cfg, 65534)
        e.set_link_latency(lat)
        out, _, _ = e.propagate_timed(ms, cfg, 65534)
        t = e.timed_traffic(m, sz, 1, 16, per_pair=True)
        same_tables(t, ttm.tables(R, sz, 1, 16))
        identities(t, out)
        assert t.msg[1024:, TT.SENT].all()


def test_refusals(gpu_ok):
    name = "floodsub"
    ov, ms = shape(name)
    m = len(ms)
    lat = synth.link_latency(ov, 11, 1, 9)
    with make(gsx.Engine(1), name) as e:
        ask = lambda **kw: rc_of(lambda: e.timed_traffic(m, **kw))  # noqa: E731
        assert ask() == abi.GSX_ESTATE  # before any timed call
        e.set_link_latency(lat)
        e.propagate_timed(ms, tcfg(name), 65534)
        assert ask() == 0
        assert ask(n_bins=0) == abi.GSX_EINVAL and ask(n_bins=1025) == abi.GSX_EINVAL and ask(bin_ticks=0) == abi.GSX_EINVAL
        assert ask(n_bins=1024) == 0
        e.propagate(ms, tcfg(name, l=3))
        assert ask() == abi.GSX_ESTATE  # the last propagation is gsx_propagate's
        e.propagate_timed(ms, tcfg(name), 65534)
        assert ask() == 0
        e.prop_begin(ms, tcfg(name, l=3))
        assert ask() == abi.GSX_ESTATE  # a stepped call
        for _ in range(40):
            e.prop_step(0)
        e.prop_end()
        assert ask() == abi.GSX_ESTATE
        e.propagate_timed(ms, tcfg(name), 65534)
        e.set_link_latency(lat)
        assert ask() == abi.GSX_ESTATE  # the latencies were set again
        e.propagate_timed(ms, tcfg(name), 65534)
        assert ask() == 0
        e.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
        assert ask() == abi.GSX_ESTATE  # an overlay load
    o = abi.TimedTrafficOut()
    assert gsx.load_library().gsx_timed_traffic(None, None, 1, 64, C.byref(o)) == abi.GSX_EINVAL


def test_a_range_shard_refuses(gpu_ok):
    ov, ms = shape("floodsub")
    with gsx.Engine(1) as e:
        e.set_peer_params(synth.bench_peer_params())
        e.set_topic_params(0, synth.spam_test_topic_params())
        lo, hi = 0, ov.n // 2
        sh = synth.shard_of(ov, lo, hi)
        e.load_overlay_shard(ov.n, lo, sh.row_ptr, sh.col, sh.edge_flags, sh.node_ips)
        assert rc_of(lambda: e.timed_traffic(len(ms))) == abi.GSX_EINVAL


def test_the_engine_is_unchanged(gpu_ok):
    name = "delay-invalid"
    ov, ms = shape(name)
    m = len(ms)
    lat = synth.link_latency(ov, 11, 1, 9, symmetric=False)
    with make(gsx.Engine(1), name) as a, make(gsx.Engine(1), name) as b:
        for e in (a, b):
            e.set_link_latency(lat)
        ra = a.propagate_timed(ms, tcfg(name), 65534, want_results=True)
        rb = b.propagate_timed(ms, tcfg(name), 65534, want_results=True)
        t1 = a.timed_traffic(m, sizes_of("random", m), 2, 200, per_pair=True)
        same_state(a, b)
        res = a.timed_results(m)
        assert np.array_equal(res[0], rb[1]) and np.array_equal(res[1], rb[2])
        assert np.array_equal(a.timed_stats(m, 1, 64).tick_hist, b.timed_stats(m, 1, 64).tick_hist)
        ra2 = a.propagate_timed(ms, tcfg(name), 65534, want_results=True)
        rb2 = b.propagate_timed(ms, tcfg(name), 65534, want_results=True)
        assert ra[0].as_dict() == rb[0].as_dict() and ra2[0].as_dict() == rb2[0].as_dict()
        assert np.array_equal(ra2[1], rb2[1]) and np.array_equal(ra2[2], rb2[2])
        same_state(a, b)
        assert t1.sent() > 0


def test_credit_now_moves_a_score_across_the_publish_threshold(gpu_ok):
    """Flood publish: a peer is published to iff its score is >= PublishThreshold.  The call's own
    P2 credits lift a peer over the threshold; the tables still follow the eligibility the call had."""
    import timed_model as tm

    name = "floodpub"
    ov, ms = shape(name)
    m = len(ms)
    lat = synth.link_latency(ov, 11, 1, 9)
    cfg = tcfg(name, credit=abi.GSX_CREDIT_NOW)

    def thresholds(pub):
        return abi.Thresholds(gossip_threshold=-100, publish_threshold=pub, graylist_threshold=-1000,
                              accept_px_threshold=0, opportunistic_graft_threshold=0)

    with make(gsx.Engine(1), name) as probe:
        probe.set_thresholds(thresholds(-900.0))
        probe.set_link_latency(lat)
        s0 = probe.scores().copy()
        probe.propagate_timed(ms, cfg, 65534)
        s1 = probe.scores().copy()
    direct = (ov.edge_flags & abi.GSX_EDGE_DIRECT) != 0
    cand = np.nonzero((s1 > s0 + 1.0) & (s0 < -150.0) & ~direct)[0]
    assert len(cand)
    q = int(cand[0])
    pub = float((s0[q] + s1[q]) / 2)
    with make(gsx.Engine(1), name) as e:
        e.set_thresholds(thresholds(pub))
        b0 = e.scores().copy()
        st = e.export_state()
        R = ttm.run_on(e, ov, lat, ms, cfg, 65534, thresholds=(pub, -1000.0))
        e.set_link_latency(lat)
        out, _, _ = e.propagate_timed(ms, cfg, 65534)
        b1 = e.scores().copy()
        crossed = np.nonzero((b0 < pub) & (b1 >= pub) & ~direct)[0]
        assert len(crossed)  # the credits did move a score across the threshold
        in_mesh = st["rec_flags"].reshape(1, -1)[0] & abi.GSX_REC_IN_MESH
        byte = lambda s, p: tm.fwd_byte(GS, 1, int(st["pair_flags"][p]), int(ov.edge_flags[p]), int(in_mesh[p]),  # noqa: E731
                                        float(s[p]), pub, -1000.0)
        assert any(byte(b0, int(p)) != byte(b1, int(p)) for p in crossed)  # ... and an eligibility byte with it
        t = e.timed_traffic(m, None, 1, 64, per_pair=True)
        same_tables(t, ttm.tables(R, None, 1, 64))
        identities(t, out)

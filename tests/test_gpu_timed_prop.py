"""gsx_propagate_timed on the GPU: with every link the same latency it must equal
gsx_propagate as the CPU oracle pins it, bit for bit; with different latencies
it must equal the Python model of the rule (timed_model.py, itself checked
against the oracle and Dijkstra in test_timed_model.py).  All integers and
bit-exact doubles: equality is exact everywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import gsx
import oracle as orc
import propagation_cases as pc
import timed_model as tm
from gsx import abi, synth

pytestmark = pytest.mark.gpu

FS, GS = abi.GSX_ROUTER_FLOODSUB, abi.GSX_ROUTER_GOSSIPSUB
MS = abi.MILLISECOND

# name -> router, n, d, T, m, overlay kw, setup kw, invalid, flood publish, tick (ms), vd (ticks)
SHAPES = {
    "floodsub": (FS, 300, 6, 1, 64, {}, {}, 0.0, 0, 5, 0),
    "gossipsub": (GS, 500, 6, 2, 100, dict(mix_protocols=True, direct_frac=0.05), dict(disconnect_frac=0.05), 0.0, 0, 5, 0),
    "floodpub": (GS, 500, 6, 1, 130, dict(mix_protocols=True), {}, 0.0, 1, 5, 0),
    "delay-invalid": (GS, 500, 6, 1, 100, dict(mix_protocols=True, direct_frac=0.05), dict(disconnect_frac=0.05), 0.25, 0,
                      1, 7),
    "one-word": (GS, 1500, 7, 1, 50, dict(mix_protocols=True), {}, 0.0, 0, 5, 0),
}


@functools.lru_cache(maxsize=None)
def shape(name):
    router, n, d, T, m, okw, skw, invalid, fp, tick_ms, vd = SHAPES[name]
    ov = pc.overlay(n, d, seed=11, **okw)
    ms = pc.messages(n, m, seed=11, invalid=invalid)
    return ov, ms


def make(be, name):
    router, n, d, T, m, okw, skw, invalid, fp, tick_ms, vd = SHAPES[name]
    ov, _ = shape(name)
    pc.setup(be, ov, T, seed=11, **skw)
    return be


def tcfg(name, credit=abi.GSX_CREDIT_NOW, l=1):
    """The timed call's config (l = 1), or gsx_propagate's for hops of l ticks."""
    router, n, d, T, m, okw, skw, invalid, fp, tick_ms, vd = SHAPES[name]
    return pc.config(router, flood_publish=fp, latency_ms=tick_ms * l, delay_ms=float(tick_ms * vd), credit=credit)


def ticks_of_hops(hop, l, vd):
    h = hop.astype(np.int64)
    return np.where(hop == 0xFF, 0xFFFF, np.where(h == 0, 0, h * l + (h - 1) * vd)).astype(np.uint16)


def same_state(a, b):
    sa, sb = a.export_state(), b.export_state()
    for f in abi.STATE_FIELDS:
        assert np.array_equal(np.asarray(sa[f]).view(np.uint8), np.asarray(sb[f]).view(np.uint8)), f
    assert np.array_equal(a.scores().view(np.uint64), b.scores().view(np.uint64))


@functools.lru_cache(maxsize=None)
def oracle_run(name, l):
    o = make(orc.Oracle(SHAPES[name][3]), name)
    out, hop, frm = o.propagate(shape(name)[1], tcfg(name, l=l), want_results=True)
    assert out.hops < 40
    return o, out, hop, frm


@pytest.mark.parametrize("l", [1, 3])
@pytest.mark.parametrize("name", ["floodsub", "gossipsub", "floodpub", "delay-invalid"])
def test_uniform_latency_equals_the_oracle(gpu_ok, name, l):
    ov, ms = shape(name)
    vd = SHAPES[name][10]
    o, out, hop, frm = oracle_run(name, l)
    with make(gsx.Engine(SHAPES[name][3]), name) as e:
        e.set_link_latency(np.full(ov.n_pairs, l, dtype=np.uint8))
        t, tick, tfrm = e.propagate_timed(ms, tcfg(name), 65534, want_results=True)
        want, got = out.as_dict(), t.as_dict()
        print(name, l, got)
        for k in ("deliveries", "duplicates", "transmissions", "rejected", "ignored", "graylisted"):
            assert got[k] == want[k], k
        assert np.array_equal(tick, ticks_of_hops(hop, l, vd))
        assert np.array_equal(tfrm, frm)
        assert t.last_tick == (out.hops * l + (out.hops - 1) * vd if out.hops else 0)
        same_state(e, o)


def pending(e, E):
    f, d, i = (np.zeros(E, dtype=np.uint32) for _ in range(3))
    e.pending_credits(f.ctypes.data, d.ctypes.data)
    e.pending_invalid(i.ctypes.data)
    return f, d, i


def check_model(e, r, t, tick, frm):
    got, want = t.as_dict(), tm.counters(r)
    print(got)
    assert got == want, (got, want)
    assert np.array_equal(tick, r.tick), np.argwhere(tick != r.tick)[:5]
    assert np.array_equal(frm, r.first_from), np.argwhere(frm != r.first_from)[:5]


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_heterogeneous_latency_equals_the_model(gpu_ok, name, symmetric):
    """Latencies 1 .. 9 ticks of 5 ms (1 ms in the delayed case) against the 25 ms window: the
    window splits the copies of a message (asserted for gossipsub, so the case is not vacuous)."""
    ov, ms = shape(name)
    T = SHAPES[name][3]
    lat = synth.link_latency(ov, 11, 1, 9, symmetric=symmetric)
    E = ov.n_pairs
    with make(gsx.Engine(T), name) as a, make(gsx.Engine(T), name) as b:
        r = tm.run_on(a, ov, lat, ms, tcfg(name), 65534, T=T)
        if SHAPES[name][0] == GS and SHAPES[name][9] == 5:
            assert 0 < r.dup_in_window < r.duplicates
        a.set_link_latency(lat)
        t, tick, frm = a.propagate_timed(ms, tcfg(name, credit=abi.GSX_CREDIT_DEFER), 65534, want_results=True)
        check_model(a, r, t, tick, frm)
        f, d, i = pending(a, E)
        assert np.array_equal(f, r.first) and np.array_equal(d, r.dup_in) and np.array_equal(i, r.inv)
        a.fold_credits()
        f, d, i = pending(a, E)
        assert not f.any() and not d.any() and not i.any()
        b.set_link_latency(lat)
        t2, _, _ = b.propagate_timed(ms, tcfg(name), 65534)
        assert t2.as_dict() == t.as_dict()
        same_state(a, b)


def cycle_overlay(n):
    col = np.array([[min((i - 1) % n, (i + 1) % n), max((i - 1) % n, (i + 1) % n)] for i in range(n)],
                   dtype=np.int32).reshape(-1)
    ips, sybil = synth._ips(n, 0.0, 50)
    return synth.Overlay(n, np.arange(n + 1, dtype=np.int64) * 2, col,
                         np.full(2 * n, abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8), ips, sybil)


@pytest.mark.parametrize("kind", ["short-ring", "sparse-ring"])
def test_ring_wrap_on_a_cycle(gpu_ok, kind):
    """200 nodes in a cycle, floodsub: a call of hundreds of ticks over a ring of 8 slots
    (latencies 1 .. 3, no delay), and one over a ring of 256 slots of which few are occupied
    (latencies 1 or 200, 50 ticks of validation)."""
    ov = cycle_overlay(200)
    lat = synth.link_latency(ov, 5, 1, 3)
    vd = 0
    if kind == "sparse-ring":
        lat = np.where(lat == 2, 200, 1).astype(np.uint8)
        vd = 50
    ms = pc.messages(200, 70, seed=5)
    cfg = pc.config(FS, latency_ms=5, delay_ms=5.0 * vd, credit=abi.GSX_CREDIT_DEFER)
    with gsx.Engine(1) as e:
        pc.setup(e, ov, 1, seed=5, score_spread=False)
        r = tm.run_on(e, ov, lat, ms, cfg, 65534)
        e.set_link_latency(lat)
        t, tick, frm = e.propagate_timed(ms, cfg, 65534, want_results=True)
        check_model(e, r, t, tick, frm)
        assert t.ticks_run >= 100 and t.deliveries == 70 * 199
        f, d, i = pending(e, ov.n_pairs)
        assert np.array_equal(f, r.first) and np.array_equal(d, r.dup_in)


def test_max_ticks_cuts_the_call(gpu_ok):
    name = "gossipsub"
    ov, ms = shape(name)
    lat = synth.link_latency(ov, 11, 1, 9)
    with make(gsx.Engine(2), name) as e:
        full = tm.run_on(e, ov, lat, ms, tcfg(name), 65534, T=2)
        cut = max(full.last_tick // 2, 1)
        r = tm.run_on(e, ov, lat, ms, tcfg(name), cut, T=2)
        assert 0 < r.deliveries < full.deliveries
        e.set_link_latency(lat)
        t, tick, frm = e.propagate_timed(ms, tcfg(name, credit=abi.GSX_CREDIT_DEFER), cut, want_results=True)
        check_model(e, r, t, tick, frm)
        assert t.ticks_run <= cut and (tick[tick != 0xFFFF] <= cut).all() and (tick == 0xFFFF).any()
        f, d, i = pending(e, ov.n_pairs)
        assert np.array_equal(f, r.first) and np.array_equal(d, r.dup_in) and np.array_equal(i, r.inv)


def stats_expected(tick, bin_ticks, n_bins):
    m, n = tick.shape
    hist = np.zeros((m, n_bins), dtype=np.uint32)
    got = tick != 0xFFFF
    b = np.minimum(tick.astype(np.int64) // bin_ticks, n_bins - 1)
    for k in range(m):
        hist[k] = np.bincount(b[k][got[k]], minlength=n_bins)
    rx = got & (tick >= 1)
    return hist, rx.sum(0).astype(np.uint32), (tick.astype(np.uint64) * rx).sum(0).astype(np.uint64)


class DevBuf:
    """Device memory from the HIP runtime the engine's library already has loaded, preset to 0x07 bytes."""
    hip = None

    def __init__(self, nbytes):
        if DevBuf.hip is None:
            DevBuf.hip = C.CDLL("libamdhip64.so")
        self.nbytes = nbytes
        p = C.c_void_p()
        assert DevBuf.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        self.ptr = p.value
        self.fill(7)

    def fill(self, byte):
        assert DevBuf.hip.hipMemset(C.c_void_p(self.ptr), byte, C.c_size_t(self.nbytes)) == 0
        assert DevBuf.hip.hipDeviceSynchronize() == 0

    def read(self, dtype):
        out = np.empty(self.nbytes, dtype=np.uint8)
        assert DevBuf.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.ptr), C.c_size_t(self.nbytes), 2) == 0
        return out.view(dtype)

    def free(self):
        DevBuf.hip.hipFree(C.c_void_p(self.ptr))


def test_timed_stats_equal_numpy_over_the_results(gpu_ok):
    name = "floodpub"  # m = 130: three words, the last partial
    ov, ms = shape(name)
    lat = synth.link_latency(ov, 11, 1, 9)
    with make(gsx.Engine(1), name) as e:
        e.set_link_latency(lat)
        t, tick, _ = e.propagate_timed(ms, tcfg(name), 10, want_results=True)  # cut short: some nodes never reached
        assert (tick == 0xFFFF).any() and t.last_tick > 7  # ... and a clamp at 7 bins of 1 tick
        for bin_ticks in (1, 4):
            for n_bins in (1, 7, 1024):
                hist, recv, tsum = stats_expected(tick, bin_ticks, n_bins)
                st = e.timed_stats(len(ms), bin_ticks, n_bins, per_node=True)
                assert np.array_equal(st.tick_hist, hist), (bin_ticks, n_bins)
                assert np.array_equal(st.node_received, recv) and np.array_equal(st.node_tick_sum, tsum)
                again = e.timed_stats(len(ms), bin_ticks, n_bins, per_node=True)
                assert st.tick_hist.tobytes() == again.tick_hist.tobytes()
                assert st.node_tick_sum.tobytes() == again.node_tick_sum.tobytes()
                only = e.timed_stats(len(ms), bin_ticks, n_bins)
                assert np.array_equal(only.tick_hist, hist) and only.node_received is None
                # device outputs, with and without the per-node ones
                dh, dr, dsum = DevBuf(4 * hist.size), DevBuf(4 * ov.n), DevBuf(8 * ov.n)
                e.timed_stats(len(ms), bin_ticks, n_bins, out_ptrs=(dh.ptr, dr.ptr, dsum.ptr))
                e.sync()
                assert np.array_equal(dh.read(np.uint32).reshape(hist.shape), hist)
                assert np.array_equal(dr.read(np.uint32), recv) and np.array_equal(dsum.read(np.uint64), tsum)
                dh.fill(7)
                e.timed_stats(len(ms), bin_ticks, n_bins, out_ptrs=(dh.ptr, None, None))
                e.sync()
                assert np.array_equal(dh.read(np.uint32).reshape(hist.shape), hist)
                for b in (dh, dr, dsum):
                    b.free()
        assert st.reached().tolist() == ((tick != 0xFFFF).sum(1) - 1).tolist()
        assert st.tick_ns == 5 * MS


def rc_of(fn):
    try:
        fn()
    except abi.GsxError as ex:
        return ex.code
    return 0


def test_refusals_leave_the_engine_unchanged(gpu_ok):
    name = "gossipsub"
    ov, ms = shape(name)
    lat = synth.link_latency(ov, 11, 1, 9)
    cfg = tcfg(name)
    with make(gsx.Engine(2), name) as e, make(gsx.Engine(2), name) as fresh:
        assert rc_of(lambda: e.propagate_timed(ms, cfg, 1000)) == abi.GSX_ESTATE  # no latencies set
        bad = lat.copy()
        bad[len(bad) // 2] = 0
        assert rc_of(lambda: e.set_link_latency(bad)) == abi.GSX_EINVAL
        assert rc_of(lambda: e.propagate_timed(ms, cfg, 1000)) == abi.GSX_ESTATE  # still none
        e.set_link_latency(lat)
        rs = pc.config(abi.GSX_ROUTER_RANDOMSUB, latency_ms=5, size=500)
        assert rc_of(lambda: e.propagate_timed(ms, rs, 1000)) == abi.GSX_EINVAL
        odd = pc.config(GS, latency_ms=5, delay_ms=7.0)  # 7 ms is no multiple of the 5 ms tick
        assert rc_of(lambda: e.propagate_timed(ms, odd, 1000)) == abi.GSX_EINVAL
        assert rc_of(lambda: e.propagate_timed(ms, cfg, 65535)) == abi.GSX_EINVAL
        gp = abi.GaterParams()
        assert gsx.load_library().gsx_default_gater_params(C.byref(gp)) == 0
        e.set_gater_params(gp)
        e.accept_from(pc.T0 + 3 * pc.S, 1, 0)
        e.gater_enforce(True)
        assert rc_of(lambda: e.propagate_timed(ms, cfg, 1000)) == abi.GSX_ESTATE
        e.gater_enforce(False)
        e.set_gater_params(None)
        e.set_link_latency(None)
        assert rc_of(lambda: e.propagate_timed(ms, cfg, 1000)) == abi.GSX_ESTATE  # removed again
        # a valid call after all that equals a fresh engine's
        e.set_link_latency(lat)
        fresh.set_link_latency(lat)
        t, tick, frm = e.propagate_timed(ms, cfg, 65534, want_results=True)
        t2, tick2, frm2 = fresh.propagate_timed(ms, cfg, 65534, want_results=True)
        assert t.as_dict() == t2.as_dict() and np.array_equal(tick, tick2) and np.array_equal(frm, frm2)
        same_state(e, fresh)
        # gsx_propagate's readers never see a timed call's rows
        for fn in (lambda: e.prop_stats(len(ms)), lambda: e.prop_results(len(ms)), lambda: e.prop_duplicates(len(ms)),
                   e.gater_fold_prop, e.tag_fold_prop):
            assert rc_of(fn) == abi.GSX_ESTATE
        out, hop, _ = e.propagate(ms, tcfg(name, l=3), want_results=True)
        out2, hop2, _ = fresh.propagate(ms, tcfg(name, l=3), want_results=True)
        assert out.as_dict() == out2.as_dict() and np.array_equal(hop, hop2)
        assert e.prop_stats(len(ms)).hop_hist.sum() == (hop != 0xFF).sum()
        assert e.prop_duplicates(len(ms)).shape[0] == ov.n_pairs
        same_state(e, fresh)


def test_a_range_shard_refuses(gpu_ok):
    name = "floodsub"
    ov, ms = shape(name)
    with gsx.Engine(1) as e:
        sh = synth.overlay_shard(ov, 0, ov.n // 2) if hasattr(synth, "overlay_shard") else None
        if sh is None:
            lo, hi = 0, ov.n // 2
            e.load_overlay_shard(ov.n, lo, ov.row_ptr[lo:hi + 1] - ov.row_ptr[lo], ov.col[ov.row_ptr[lo]:ov.row_ptr[hi]],
                                 ov.edge_flags[ov.row_ptr[lo]:ov.row_ptr[hi]], ov.node_ips)
        else:
            e.load_overlay_shard(sh.n, sh.node_lo, sh.row_ptr, sh.col, sh.edge_flags, sh.node_ips)
        e.set_link_latency(np.ones(e.n_pairs, dtype=np.uint8))
        assert rc_of(lambda: e.propagate_timed(ms, tcfg(name), 1000)) == abi.GSX_ESTATE


def test_engine_reuse_across_plain_and_timed_calls(gpu_ok):
    """propagate (m = 1024), timed (m = 50), propagate (m = 64), timed (m = 130, other latencies) on
    one engine: every call equals the same call on an engine that ran only the calls before it with
    the same effect on the state (the twin replays them, so both start each step from equal states)."""
    name = "gossipsub"
    ov, _ = shape(name)
    steps = [("p", 1024, None), ("t", 50, synth.link_latency(ov, 1, 1, 9)), ("p", 64, None),
             ("t", 130, synth.link_latency(ov, 2, 1, 5, symmetric=False))]
    with make(gsx.Engine(2), name) as e:
        for i, (kind, m, lat) in enumerate(steps):
            ms = pc.messages(ov.n, m, seed=20 + i, invalid=0.1)
            with make(gsx.Engine(2), name) as twin:
                twin.import_state(e.export_state())
                same_state(e, twin)
                if kind == "p":
                    a = e.propagate(ms, tcfg(name, l=2), want_results=True)
                    b = twin.propagate(ms, tcfg(name, l=2), want_results=True)
                else:
                    e.set_link_latency(lat)
                    twin.set_link_latency(lat)
                    a = e.propagate_timed(ms, tcfg(name), 65534, want_results=True)
                    b = twin.propagate_timed(ms, tcfg(name), 65534, want_results=True)
                assert a[0].as_dict() == b[0].as_dict(), (i, a[0].as_dict(), b[0].as_dict())
                assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), i
                same_state(e, twin)

"""gsx_score_stats on the GPU: the selected pairs per score bin for the engine,
per observer row and per peer, and the row / peer minima, against the numpy
reference (score_stats_cases.reference) on the engine's own scores() and
export_state().  Counters are integers and the minima are picked, not computed:
every comparison is on the raw bytes."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library loads: both then share one HIP runtime)

import gsx
import propagation_cases as pc
import score_stats_cases as sc
from gsx import abi

pytestmark = pytest.mark.gpu

S = abi.SECOND
PC = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
GOSSIP = abi.GSX_ROUTER_GOSSIPSUB


def snapshot(e):
    """What the reference reads: the scores and the exported flags, read-only."""
    s, st = e.scores(), e.export_state()
    for a in (s, st["pair_flags"], st["rec_flags"]):
        a.setflags(write=False)
    return s, st


def want(snap, ov, edges, select="present", topic=0):
    s, st = snap
    return sc.reference(s, st["pair_flags"], st["rec_flags"], ov.row_ptr, ov.col, ov.n, edges, select, topic)


def selected(snap, select="present"):
    pf = snap[1]["pair_flags"]
    return (pf & abi.GSX_PAIR_PRESENT) != 0 if select == "present" else pf == PC


# ---- 1. parity on a mixed state ------------------------------------------------------------------
T_MIXED, HUB, LONER = 3, 7, 13


@functools.lru_cache(maxsize=None)
def mixed():
    """700 nodes of mixed protocols, a hub row of >= 600 pairs, a node with an empty row; absent,
    retained and connected pairs; scores spread by a credited propagation and two heartbeats.
    -> (engine, overlay, snapshot); score_stats changes nothing, so the tests share it."""
    seed = 11
    ov = sc.isolate(pc.with_hub(pc.overlay(700, 3, seed, mix_protocols=True), HUB, 640, seed), LONER)
    e = gsx.Engine(T_MIXED)
    pc.setup(e, ov, T_MIXED, seed, disconnect_frac=0.1)
    out = e.propagate(pc.messages(ov.n, 100, seed), pc.config(GOSSIP, topic=0, latency_ms=5))[0]
    assert out.deliveries > 0
    e.heartbeat(1, pc.T0 + 4 * S, 3)
    e.heartbeat(2, pc.T0 + 5 * S, 3)
    e.refresh(pc.T0 + 6 * S)
    return e, ov, snapshot(e)


def test_mixed_state_shape(gpu_ok):
    e, ov, (s, st) = mixed()
    deg = np.diff(ov.row_ptr)
    assert deg[HUB] >= 600 and deg[LONER] == 0 and not (ov.col == LONER).any()
    pf = st["pair_flags"]
    assert (pf == 0).any() and (pf == abi.GSX_PAIR_PRESENT).any() and (pf == PC).any()
    assert len(np.unique(s[pf != 0])) > 100  # the scores are spread


@pytest.mark.parametrize("select,topic", [("present", 0), ("connected", 0), ("mesh", 0), ("mesh", T_MIXED - 1)])
def test_parity_on_a_mixed_state(gpu_ok, select, topic):
    e, ov, snap = mixed()
    s = snap[0]
    edges = sc.edges_from(s[selected(snap)], 7)
    for x in edges:
        assert (s[selected(snap)] == x).any()  # a score on every edge
    st = e.score_stats(edges, select, topic)
    ref = want(snap, ov, edges, select, topic)
    sc.assert_equal(st, ref, what=(select, topic))
    assert np.array_equal(st.edges, edges)
    n_sel = int(ref["hist"].sum())
    assert n_sel > 0 and int(st.hist.sum()) == n_sel
    assert int(st.obs_bins.sum(dtype=np.int64)) == n_sel == int(st.peer_bins.sum(dtype=np.int64))
    assert np.isinf(st.obs_min[LONER]) and np.isinf(st.peer_min[LONER]) and not st.peer_bins[LONER].any()
    if select == "present":
        assert n_sel == int(selected(snap).sum()) and (st.hist > 0).all()  # every bin in use
        assert st.obs_bins[HUB].sum() >= 500


@pytest.mark.parametrize("topic", [0, T_MIXED - 1])
def test_mesh_degree_without_edges(gpu_ok, topic):
    e, ov, snap = mixed()
    st = e.score_stats([], "mesh", topic)
    sc.assert_equal(st, want(snap, ov, [], "mesh", topic))
    rf = snap[1]["rec_flags"].reshape(T_MIXED, -1)[topic]
    in_mesh = ((rf & abi.GSX_REC_IN_MESH) != 0) & (snap[1]["pair_flags"] == PC)
    per_node = np.bincount(ov.pair_observer()[in_mesh], minlength=ov.n)
    assert per_node.sum() > 0 and np.array_equal(st.degree(), per_node)
    assert st.hist.shape == (1,) and st.obs_bins.shape == (ov.n, 1)


# ---- 2. sizes that break the segmentation -----------------------------------------------------------
SEG_ROWS = {  # the first rows' degrees; the rest are drawn (0 .. 5)
    1: [0],
    63: [62, 2, 0, 0, 0, 40, 24],       # row 1 ends on pair 64, row 6 on pair 128
    64: [63, 1, 0, 0, 60, 4, 0, 0],     # rows 1 and 5 end on a wave's edge
    65: [64, 0, 0, 64, 3],              # rows 0 and 3 are exactly one wave each
    130: [62, 2, 0, 0, 100, 36, 129],   # row 6 = pairs 200 .. 328: waves 3, 4, 5 and the block edge at 256
}


@functools.lru_cache(maxsize=None)
def seg_overlay(n):
    rng = np.random.default_rng(n)
    degs = SEG_ROWS[n] + [int(x) for x in rng.integers(0, min(6, n), n - len(SEG_ROWS[n]))]
    if n > 1 and sum(degs) % 64 == 0:
        degs[-1] += 1
    return sc.degrees_overlay(n, degs, seed=n)


def seg_engine(n, T=1, e=None):
    ov = seg_overlay(n)
    e = e or gsx.Engine(T)
    pc.setup(e, ov, T, seed=n, disconnect_frac=0.2)
    return e, ov, snapshot(e)


@pytest.mark.parametrize("n", sorted(SEG_ROWS))
def test_sizes_that_break_segmentation(gpu_ok, n):
    e, ov, snap = seg_engine(n)
    E, rp, deg = ov.n_pairs, ov.row_ptr, np.diff(ov.row_ptr)
    if n > 1:
        assert E % 64 != 0
        assert ((rp[1:][deg > 0] % 64) == 0).any()  # a row ends exactly on a wave's edge
        assert ((deg[:-1] == 0) & (deg[1:] == 0)).any()  # consecutive empty rows
        key = set(zip(ov.pair_observer().tolist(), ov.col.tolist()))
        assert any((v, u) not in key for u, v in key)  # directed: some u -> v without v -> u
    else:
        assert E == 0
    if n == 130:
        a, b = rp[:-1][deg > 0], rp[1:][deg > 0] - 1
        assert (((b // 64) - (a // 64) >= 2) & ((a // 256) != (b // 256))).any()  # three waves, two blocks
    s = snap[0]
    sel = s[selected(snap)]
    for select in ("present", "connected", "mesh"):
        edges = sc.edges_from(sel, 3) if len(np.unique(sel)) >= 5 else [-1.0, 0.0]
        st = e.score_stats(edges, select, 0)
        sc.assert_equal(st, want(snap, ov, edges, select, 0), what=(n, select))
    if n == 1:
        assert st.hist.tolist() == [0, 0, 0] and np.isinf(st.obs_min).all() and np.isinf(st.peer_min).all()


# ---- 3. edge counts 0, 1 and 7 --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zeros_state():
    """Present pairs with all-zero records; a third of them without an app score: exactly +0.0."""
    ov = pc.overlay(130, 3, 5)
    e = gsx.Engine(1)
    pc.setup(e, ov, 1, 5, mesh_degree=0, score_spread=False)
    rng = np.random.default_rng(5)
    app = np.where(rng.random(ov.n_pairs) < 0.33, 0.0, rng.integers(-9, 10, ov.n_pairs).astype(np.float64))
    e.set_app_scores(app)
    return e, ov, snapshot(e)


def test_one_edge_at_zero(gpu_ok):
    e, ov, snap = zeros_state()
    s = snap[0]
    zero = s.view(np.uint64) == 0  # +0.0
    assert zero.sum() > 20 and (s < 0).any() and (s > 0).any()
    st = e.score_stats([0.0])
    sc.assert_equal(st, want(snap, ov, [0.0]))
    assert int(st.hist[0]) == int((s < 0).sum()) and int(st.hist[1]) == int((s >= 0).sum())  # +0.0: the upper bin
    assert st.below(0.0)[0] == int((s < 0).sum())


@pytest.mark.parametrize("k", [0, 7])
def test_zero_and_seven_edges(gpu_ok, k):
    e, ov, snap = zeros_state()
    edges = sc.edges_from(snap[0], k) if k else []
    st = e.score_stats(edges)
    sc.assert_equal(st, want(snap, ov, edges))
    assert st.hist.shape == (k + 1,) and int(st.hist.sum()) == ov.n_pairs
    if k == 0:
        assert np.array_equal(st.degree(), np.diff(ov.row_ptr))


def test_default_edges(gpu_ok):
    e, ov, snap = zeros_state()
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                    accept_px_threshold=0, opportunistic_graft_threshold=5))
    assert e.score_stats_edges().tolist() == [-300.0, -200.0, -100.0, 0.0, 5.0]
    sp = abi.ScoreStatsSpec(select=2, topic=9)
    assert e.lib.gsx_score_stats_edges(e.h, C.byref(sp)) == 0
    assert (sp.select, sp.topic, sp.n_edges) == (2, 9, 5)  # select and topic are left alone
    st = e.score_stats()
    assert st.edges.tolist() == [-300.0, -200.0, -100.0, 0.0, 5.0]
    sc.assert_equal(st, want(snapshot(e), ov, st.edges))


# ---- 4. reads what the score readers read, and changes nothing ------------------------------------
@pytest.mark.parametrize("mode", ["defer", "defer-wb4-pending", "late"])
def test_reads_settled_scores_and_changes_nothing(gpu_ok, mode):
    """Queued events and an unflushed credited propagation: the call equals the reference on the
    scores() taken afterwards, and the engine goes on exactly as its twin that never made the call."""
    seed, n = 17, 130
    ov = pc.overlay(n, 3, seed)
    twins = []
    for _ in range(2):
        e = gsx.Engine(1)
        if mode == "late":
            e.set_prop_tracking(False)  # the lean path: the credit folds are left to the next reader
        pc.setup(e, ov, 1, seed, disconnect_frac=0.05)
        now = pc.T0 + 2 * S
        if mode == "defer-wb4-pending":
            e.set_decay_writeback(4)
            for _ in range(2):  # phase 2 of 4: the stored counters lag by two decays
                now += S
                e.refresh(now)
        conn = np.nonzero(e.export_state()["pair_flags"] == PC)[0]
        e.apply_events(np.array([(abi.EV_INVALID_DELIVERY, 0, int(p), now, 0) for p in conn[:9] for _ in range(4)]
                                + [(abi.EV_PENALTY, 0, int(conn[11]), now, 3)], dtype=abi.event_dtype()))
        cfg = pc.config(GOSSIP, latency_ms=0 if mode == "late" else 10,
                        credit=abi.GSX_CREDIT_NOW if mode == "late" else abi.GSX_CREDIT_DEFER)
        cfg.now_ns = now + S // 2
        assert e.propagate(pc.messages(n, 40, seed), cfg)[0].deliveries > 0
        e.apply_events(np.array([(abi.EV_INVALID_DELIVERY, 0, int(conn[20]), now + S, 0)] * 5
                                + [(abi.EV_PENALTY, 0, int(conn[21]), now + S, 2)], dtype=abi.event_dtype()))
        twins.append(e)
    a, b = twins
    edges = [-300.0, -100.0, -5.0, 0.0, 5.0]
    st = a.score_stats(edges)
    snap = snapshot(a)
    sc.assert_equal(st, want(snap, ov, edges), what=mode)
    assert int(st.hist[:3].sum()) > 0  # the penalties and the -500 app scores are in
    sb, stb = b.scores(), b.export_state()
    assert np.array_equal(snap[0].view(np.uint64), sb.view(np.uint64))
    for f in abi.STATE_FIELDS:
        assert np.array_equal(np.ascontiguousarray(snap[1][f]).view(np.uint8),
                              np.ascontiguousarray(stb[f]).view(np.uint8)), f
    assert snap[1]["last_refresh_ns"] == stb["last_refresh_ns"]
    assert a.zero_map_violations() == b.zero_map_violations() == 0
    for e in twins:  # and they stay together
        e.refresh(pc.T0 + 9 * S)
    assert np.array_equal(a.scores().view(np.uint64), b.scores().view(np.uint64))


# ---- 5. output plumbing -----------------------------------------------------------------------------
EDGES5 = [-200.0, -1.0, 0.0, 1.0]
DTYPES = {"hist": np.uint64, "obs_bins": np.uint32, "obs_min": np.float64, "peer_bins": np.uint32,
          "peer_min": np.float64}


def raw_call(e, edges, arrays, select=abi.GSX_SS_PRESENT, topic=0):
    sp = abi.ScoreStatsSpec(select=select, topic=topic, n_edges=len(edges))
    for k, x in enumerate(edges):
        sp.edges[k] = x
    out = abi.ScoreStatsOut(**{f: a.ctypes.data for f, a in arrays.items()})
    return e.lib.gsx_score_stats(e.h, C.byref(sp), C.byref(out))


def test_every_subset_of_null_outputs(gpu_ok):
    e, ov, snap = seg_engine(130)
    ref = want(snap, ov, EDGES5)
    for r in range(len(sc.FIELDS) + 1):
        for fields in itertools.combinations(sc.FIELDS, r):
            arrays = {f: np.full(ref[f].nbytes, 0xAB, dtype=np.uint8).view(DTYPES[f]).reshape(ref[f].shape)
                      for f in fields}  # (garbage: the call zeroes / fills what it is asked for)
            assert raw_call(e, EDGES5, arrays) == 0, fields
            for f in fields:
                got, w = arrays[f], ref[f]
                assert np.array_equal(got.view(np.uint8), w.view(np.uint8)), fields


def test_device_pointer_outputs_and_repeat(gpu_ok):
    import torch

    e, ov, snap = seg_engine(130)
    host = e.score_stats(EDGES5)
    again = e.score_stats(EDGES5)  # the outputs are zeroed / filled anew
    ref = want(snap, ov, EDGES5)
    sc.assert_equal(host, ref)
    sc.assert_equal(again, ref)
    B, n = len(EDGES5) + 1, ov.n
    t = (torch.full((B,), -1, dtype=torch.int64, device="cuda:0"),
         torch.full((n, B), -1, dtype=torch.int32, device="cuda:0"),
         torch.full((n,), -1.0, dtype=torch.float64, device="cuda:0"),
         torch.full((n, B), -1, dtype=torch.int32, device="cuda:0"),
         torch.full((n,), -1.0, dtype=torch.float64, device="cuda:0"))
    torch.cuda.synchronize()
    for _ in range(2):
        assert e.score_stats(EDGES5, out_ptrs=t) is None
    e.sync()
    dev = gsx.ScoreStats(EDGES5, t[0].cpu().numpy().view(np.uint64), t[1].cpu().numpy().view(np.uint32),
                         t[2].cpu().numpy(), t[3].cpu().numpy().view(np.uint32), t[4].cpu().numpy())
    sc.assert_equal(dev, ref)
    # one device output alone, beside host outputs
    t[3].fill_(-1)
    torch.cuda.synchronize()
    hist = np.zeros(B, dtype=np.uint64)
    out = abi.ScoreStatsOut(hist=hist.ctypes.data, peer_bins=t[3].data_ptr())
    sp = abi.ScoreStatsSpec(n_edges=len(EDGES5))
    for k, x in enumerate(EDGES5):
        sp.edges[k] = x
    assert e.lib.gsx_score_stats(e.h, C.byref(sp), C.byref(out)) == 0
    e.sync()
    assert np.array_equal(hist, ref["hist"])
    assert np.array_equal(t[3].cpu().numpy().view(np.uint32), ref["peer_bins"])


def test_engine_reused_with_a_smaller_overlay(gpu_ok):
    e, ov, snap = seg_engine(130)
    sc.assert_equal(e.score_stats(EDGES5), want(snap, ov, EDGES5))
    e, ov, snap = seg_engine(63, e=e)
    st = e.score_stats(EDGES5)
    sc.assert_equal(st, want(snap, ov, EDGES5))
    assert st.obs_bins.shape == (63, 5) and st.peer_min.shape == (63,)


def test_inside_a_timing_region(gpu_ok):
    e, ov, snap = seg_engine(130)
    e.timing_begin(3)
    for _ in range(2):
        st = e.score_stats(EDGES5)
    tot, lo, hi, k = e.timing_end()
    assert k == 2 and tot > 0  # each call is one timed launch
    sc.assert_equal(st, want(snap, ov, EDGES5))


# ---- 6. errors -----------------------------------------------------------------------------------
def test_errors(gpu_ok):
    e, ov, snap = seg_engine(65, T=2)
    hist = {"hist": np.zeros(8, dtype=np.uint64)}
    assert raw_call(e, [0.0], hist) == 0
    assert raw_call(e, [0.0], hist, select=3) == abi.GSX_EINVAL  # unknown selection
    assert raw_call(e, [0.0], hist, select=abi.GSX_SS_MESH, topic=2) == abi.GSX_EINVAL  # topic >= n_topics
    assert raw_call(e, [0.0], hist, select=abi.GSX_SS_MESH, topic=1) == 0
    assert raw_call(e, [0.0], hist, select=abi.GSX_SS_PRESENT, topic=99) == 0  # (the topic is MESH's alone)
    for bad in ([np.nan], [np.inf], [-np.inf, 0.0], [0.0, 0.0], [1.0, 0.0], [0.0, 1.0, 1.0]):
        assert raw_call(e, bad, hist) == abi.GSX_EINVAL, bad
    sp = abi.ScoreStatsSpec(n_edges=8)
    out = abi.ScoreStatsOut(hist=hist["hist"].ctypes.data)
    assert e.lib.gsx_score_stats(e.h, C.byref(sp), C.byref(out)) == abi.GSX_EINVAL  # n_edges > 7
    with pytest.raises(gsx.GsxError) as ei:
        e.score_stats(list(range(8)))
    assert ei.value.code == abi.GSX_EINVAL
    ok = abi.ScoreStatsSpec()
    assert e.lib.gsx_score_stats(None, C.byref(ok), C.byref(out)) == abi.GSX_EINVAL
    assert e.lib.gsx_score_stats(e.h, None, C.byref(out)) == abi.GSX_EINVAL
    assert e.lib.gsx_score_stats(e.h, C.byref(ok), None) == abi.GSX_EINVAL
    assert e.lib.gsx_score_stats_edges(e.h, None) == abi.GSX_EINVAL
    assert e.lib.gsx_score_stats(e.h, C.byref(ok), C.byref(abi.ScoreStatsOut())) == 0  # all NULL: nothing to do
    sc.assert_equal(e.score_stats([0.0]), want(snap, ov, [0.0]))  # the engine is as it was
    fresh = gsx.Engine(1)
    assert fresh.lib.gsx_score_stats(fresh.h, C.byref(ok), C.byref(out)) == abi.GSX_ESTATE  # no overlay loaded
    assert fresh.score_stats_edges().tolist() == [0.0]  # (the thresholds need none)

"""gsx_score_parts on the GPU: the parts of every pair's score, its cause and
worst topic, and the four tables, against the model of the contract
(score_parts_model.py) fed from the engine's own export_state() and snapshot().
The parts are the very products score() adds and the counters are integers:
every comparison is on the raw bytes, a NaN equal to any NaN."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library loads: both then share one HIP runtime)

import gsx
import nonfinite_cases as nf
import propagation_cases as pc
import score_parts_model as spm
import score_stats_cases as sc
from gsx import abi, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND
PC = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
GOSSIP = abi.GSX_ROUTER_GOSSIPSUB
OUT = {"pair_parts": "parts", "pair_cause": "cause", "pair_topic": "worst_topic", "cause_hist": "cause_hist",
       "topic_hist": "topic_hist", "obs_cause": "obs_cause", "peer_cause": "peer_cause"}
EDGES = [-300.0, -100.0, -5.0, 0.0, 5.0]


def assert_parts(got, ref, what=""):
    for f, attr in OUT.items():
        g = getattr(got, attr)
        assert g is not None, (what, f)
        if g.shape != ref[f].shape or g.dtype != ref[f].dtype:
            raise AssertionError(f"{what} {f}: got {g.shape} {g.dtype}, want {ref[f].shape} {ref[f].dtype}")
        if not spm.same_bytes(g, ref[f]):
            bad = np.argwhere(~nf.same_mask(g, ref[f]))[:5]
            raise AssertionError(f"{what} {f}: differs at {bad.tolist()}: got {[g[tuple(i)].item() for i in bad]} "
                                 f"want {[ref[f][tuple(i)].item() for i in bad]}")


def want(e, ov, pp, tps, edges, select="present", topic=0):
    rec, pair = spm.engine_inputs(e)
    return spm.reference(rec, pair, pp, tps, e.n_topics, ov.row_ptr, ov.col, ov.n, edges, select, topic)


def same_scores(a, b):
    return bool(nf.same_mask(a, b).all())


def setup(e, ov, T, scored, seed, disconnect_frac=0.0, mesh_degree=6):
    """propagation_cases.setup with some topics left unscored -> (PeerScoreParams, {t: TopicScoreParams})."""
    rng = np.random.default_rng(seed + 1)
    pp = synth.bench_peer_params()
    e.set_peer_params(pp)
    tps = {}
    for t in scored:
        tp = synth.spam_test_topic_params()
        tp.mesh_message_deliveries_window_ns = 25 * abi.MILLISECOND
        tp.mesh_message_deliveries_activation_ns = 2 * S  # some records are active by the last refresh
        tp.topic_weight = 0.25 * (t + 1)
        e.set_topic_params(t, tp)
        tps[t] = tp
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                    accept_px_threshold=0, opportunistic_graft_threshold=0))
    e.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    E = ov.n_pairs
    ev = [(abi.EV_ADD_PEER, 0, p, pc.T0, 0) for p in range(E)]
    for t in range(T):
        for i in range(ov.n):
            row = np.arange(ov.row_ptr[i], ov.row_ptr[i + 1])
            row = row[(ov.edge_flags[row] & abi.GSX_EDGE_GOSSIPSUB) != 0]
            ev += [(abi.EV_GRAFT, t, int(q), pc.T0, 0) for q in rng.permutation(row)[:mesh_degree]]
    e.apply_events(np.array(ev, dtype=abi.event_dtype()))
    e.set_app_scores(np.where(rng.random(E) < 0.08, -500.0, rng.normal(0, 2, E)))
    if disconnect_frac > 0:
        rm = np.nonzero(rng.random(E) < disconnect_frac)[0]
        e.apply_events(np.array([(abi.EV_REMOVE_PEER, 0, int(q), pc.T0 + S, 0) for q in rm], dtype=abi.event_dtype()))
    e.refresh(pc.T0 + 2 * S)
    return pp, tps


# ---- 1. parity on a mixed state ------------------------------------------------------------------
T_MIXED, HUB, LONER = 3, 7, 13


@functools.lru_cache(maxsize=None)
def mixed():
    """test_gpu_score_stats.py's recipe with topic 1 left unscored -> (engine, overlay, pp, tps)."""
    seed = 11
    ov = sc.isolate(pc.with_hub(pc.overlay(700, 3, seed, mix_protocols=True), HUB, 640, seed), LONER)
    e = gsx.Engine(T_MIXED)
    pp, tps = setup(e, ov, T_MIXED, (0, 2), seed, disconnect_frac=0.1)
    out = e.propagate(pc.messages(ov.n, 100, seed, invalid=0.1), pc.config(GOSSIP, topic=0, latency_ms=5))[0]
    assert out.deliveries > 0
    ev = np.nonzero(e.export_state()["pair_flags"] == PC)[0][::37]
    e.apply_events(np.array([(abi.EV_PENALTY, 0, int(p), pc.T0 + 3 * S, 1 + int(p) % 3) for p in ev],
                            dtype=abi.event_dtype()))
    e.heartbeat(1, pc.T0 + 4 * S, 3)
    e.heartbeat(2, pc.T0 + 5 * S, 3)
    e.refresh(pc.T0 + 6 * S)
    return e, ov, pp, tps


@pytest.mark.parametrize("select,topic", [("present", 0), ("connected", 0), ("mesh", 0), ("mesh", T_MIXED - 1)])
def test_parity_on_a_mixed_state(gpu_ok, select, topic):
    e, ov, pp, tps = mixed()
    deg = np.diff(ov.row_ptr)
    assert deg[HUB] >= 600 and deg[LONER] == 0
    scores = e.scores()
    pf = e.export_state()["pair_flags"]
    assert (pf == 0).any() and (pf == abi.GSX_PAIR_PRESENT).any() and (pf == PC).any()
    edges = sc.edges_from(scores[(pf & abi.GSX_PAIR_PRESENT) != 0], 7)
    got = e.score_parts(edges, select, topic, per_pair=True)
    ref = want(e, ov, pp, tps, edges, select, topic)
    assert_parts(got, ref, what=(select, topic))
    assert same_scores(got.parts[:, abi.GSX_PART_SCORE], scores)
    st = e.score_stats(edges, select, topic)
    assert st.hist.sum() > 0
    assert np.array_equal(got.cause_hist.sum(1), st.hist) and np.array_equal(got.topic_hist.sum(1), st.hist)
    assert np.array_equal(got.obs_cause.sum(1), st.obs_bins.sum(1)) and np.array_equal(got.peer_cause.sum(1), st.peer_bins.sum(1))
    assert not got.topic_hist[:, 1].any()  # the unscored topic is nobody's worst
    if select == "present":
        assert len(np.unique(got.cause[pf != 0])) >= 3 and got.obs_cause[HUB].sum() >= 500
        assert (got.cause[pf == 0] == abi.GSX_CAUSE_NONE).all() and not got.parts[pf == 0].view(np.uint64).any()


# ---- 2. every cause occurs ------------------------------------------------------------------------
def causes_case(be):
    """A hand-made imported state on 40 nodes, T = 3 with topic 1 unscored, negative P1 / P2 weights
    on topic 0 -> (overlay, pp, tps, {what: pair})."""
    T, now = 3, pc.T0
    ov = pc.overlay(40, 3, 3)
    ov.node_ips = ov.node_ips.copy()
    ov.node_ips[:, 0] = 1000 + np.arange(ov.n) // 8  # eight nodes to an IP: P6 where an observer sees two of them
    E = ov.n_pairs
    pp = synth.bench_peer_params()
    pp.topic_score_cap = 6.0
    pp.ip_colocation_factor_weight = -0.125
    pp.behaviour_penalty_weight = -1.0
    be.set_peer_params(pp)
    tps = {}
    for t in (0, 2):
        tp = synth.spam_test_topic_params()
        tp.topic_weight = 1.0
        tp.time_in_mesh_weight, tp.time_in_mesh_cap = (-0.5, 100.0) if t == 0 else (0.0, 100.0)
        tp.first_message_deliveries_weight = -1.0 if t == 0 else 1.0
        tp.mesh_message_deliveries_weight, tp.mesh_message_deliveries_threshold = -1.0, 4.0
        tp.mesh_failure_penalty_weight = -1.0
        tp.invalid_message_deliveries_weight = -1.0
        be.set_topic_params(t, tp)
        tps[t] = tp
    be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    st = {f: np.zeros(T * E if f in abi.RECORD_FIELDS else E, dtype=abi.STATE_DTYPES[f]) for f in abi.STATE_FIELDS}
    st["pair_flags"][:] = PC
    st["graft_time_ns"][:] = now
    st["last_refresh_ns"] = now
    r = {f: st[f].reshape(T, E) for f in abi.RECORD_FIELDS}
    app = np.zeros(E)
    MESH, ACT = abi.GSX_REC_IN_MESH, abi.GSX_REC_IN_MESH | abi.GSX_REC_ACTIVE

    def mesh(t, p, flags, secs, mmd):
        r["rec_flags"][t, p], r["mesh_time_ns"][t, p], r["graft_time_ns"][t, p] = flags, secs * S, now - secs * S
        r["mesh_message_deliveries"][t, p] = mmd

    who = dict(p1=0, p2=1, p3=2, p3_inactive=3, p3b=4, p4=5, p5=6, p7=7, tie=8, cap=9, topic_tie=10, unscored=11,
               absent=12, retained=13)
    mesh(0, who["p1"], MESH, 9, 10.0)                       # P1 = 9 * -0.5
    r["first_message_deliveries"][0, who["p2"]] = 3.0       # P2 = 3 * -1
    mesh(2, who["p3"], ACT, 0, 1.0)                         # P3 = -(4 - 1)^2 on topic 2 (no P1 weight there)
    mesh(2, who["p3_inactive"], MESH, 0, 1.0)               # below the threshold, not yet active: no P3
    r["mesh_failure_penalty"][2, who["p3b"]] = 2.5          # P3b
    r["invalid_message_deliveries"][0, who["p4"]] = 1.5     # P4 = -2.25
    app[who["p5"]] = -7.0                                   # P5
    st["behaviour_penalty"][who["p7"]] = 3.0                # P7 = -9
    r["mesh_failure_penalty"][0, who["tie"]] = 4.0          # P3b == P4 == -4: the lower index
    r["invalid_message_deliveries"][2, who["tie"]] = 2.0
    r["first_message_deliveries"][2, who["cap"]] = 50.0     # topic sum 50 - 1 > cap 6
    r["mesh_failure_penalty"][0, who["cap"]] = 1.0
    r["mesh_failure_penalty"][0, who["topic_tie"]] = 2.0    # topics 0 and 2 both -2: the lower t
    r["mesh_failure_penalty"][2, who["topic_tie"]] = 2.0
    r["invalid_message_deliveries"][1, who["unscored"]] = 9.0  # on the unscored topic: nothing
    st["pair_flags"][who["absent"]] = 0
    r["invalid_message_deliveries"][0, who["absent"]] = 5.0
    st["pair_flags"][who["retained"]] = abi.GSX_PAIR_PRESENT
    st["expire_ns"][who["retained"]] = now + 100 * S
    r["invalid_message_deliveries"][0, who["retained"]] = 2.0
    be.import_state(st)
    be.set_app_scores(app)
    return ov, pp, tps, who


def check_causes(ref, who, p6_pairs):
    """What the model alone says about the hand-made pairs: all nine causes, the ties, the cap."""
    c, w, parts = ref["pair_cause"], ref["pair_topic"], ref["pair_parts"]
    assert set(c.tolist()) == set(range(abi.GSX_CAUSES))
    for name, j in (("p1", 0), ("p2", 1), ("p3", 2), ("p3b", 3), ("p4", 4), ("p5", 5), ("p7", 7)):
        assert c[who[name]] == j, (name, parts[who[name]].tolist())
    assert len(p6_pairs) and (c[p6_pairs] == abi.GSX_PART_P6).any()
    assert (w[who["p1"]], w[who["p3"]], w[who["p4"]]) == (0, 2, 0)
    q = who["p3_inactive"]
    assert not parts[q, abi.GSX_PART_P3] and c[q] in (abi.GSX_CAUSE_NONE, abi.GSX_PART_P6)
    q = who["tie"]
    assert parts[q, abi.GSX_PART_P3B] == parts[q, abi.GSX_PART_P4] == -4.0 and c[q] == abi.GSX_PART_P3B
    q = who["cap"]
    assert parts[q, abi.GSX_PART_TOPICS] == 6.0 and parts[q, :5].sum() == 49.0
    q = who["topic_tie"]
    assert w[q] == 0 and c[q] == abi.GSX_PART_P3B
    q = who["unscored"]
    assert w[q] == abi.GSX_TOPIC_NONE and not parts[q, :5].any()
    assert c[who["absent"]] == abi.GSX_CAUSE_NONE and not parts[who["absent"]].any()
    assert c[who["retained"]] == abi.GSX_PART_P4
    assert (c == abi.GSX_CAUSE_NONE).sum() > 20


def test_every_cause_occurs(gpu_ok):
    e = gsx.Engine(3)
    ov, pp, tps, who = causes_case(e)
    got = e.score_parts(EDGES, per_pair=True)
    ref = want(e, ov, pp, tps, EDGES)
    p6_pairs = np.nonzero(e.snapshot()["ip_colocation_factor"] > 0)[0]
    check_causes(ref, who, p6_pairs)
    assert_parts(got, ref)
    assert same_scores(got.parts[:, abi.GSX_PART_SCORE], e.scores())
    present = e.export_state()["pair_flags"] != 0
    assert got.blame().tolist() == np.bincount(ref["pair_cause"][present], minlength=9).tolist()
    assert ov.col[who["p7"]] in got.peers_blamed("p7") and got.fraction("p7") > 0
    for select, topic in (("connected", 0), ("mesh", 2)):
        assert_parts(e.score_parts(EDGES, select, topic, per_pair=True), want(e, ov, pp, tps, EDGES, select, topic), select)


# ---- 3. sizes that break the segmentation -----------------------------------------------------------
# Exactly 1, 63, 64, 65 and 129 pairs: one lane; a wave short of one lane; one full tile and no tail;
# a tail of one lane; two tiles and a tail of one lane.  The rows end on, and straddle, a wave's edge.
PAIR_COUNTS = {  # n_pairs: (nodes, the first rows' degrees; the other rows are empty)
    1: (2, [1]),
    63: (70, [40, 0, 0, 23]),
    64: (70, [63, 1]),                 # row 0 ends one lane short of the edge, row 1 on it
    65: (70, [64, 0, 1]),              # row 0 is exactly the wave, row 2 the one-lane tail
    129: (70, [60, 8, 0, 60, 1]),      # row 1 straddles the edge at 64, row 3 ends on 128, a one-lane tail
}


def seg_check(e, ov, pp, tps, what):
    conn = np.nonzero(e.export_state()["pair_flags"] == PC)[0]
    if len(conn):
        e.apply_events(np.array([(abi.EV_INVALID_DELIVERY, 0, int(p), pc.T0 + 2 * S, 0) for p in conn[::5]]
                                + [(abi.EV_PENALTY, 0, int(p), pc.T0 + 2 * S, 2) for p in conn[2::7]], dtype=abi.event_dtype()))
    for select in ("present", "connected", "mesh"):
        got = e.score_parts(EDGES, select, 0, per_pair=True)
        assert_parts(got, want(e, ov, pp, tps, EDGES, select, 0), what=(what, select))
    return got  # (the mesh selection's)


@pytest.mark.parametrize("E", sorted(PAIR_COUNTS))
def test_pair_counts_at_a_waves_edge(gpu_ok, E):
    n, degs = PAIR_COUNTS[E]
    ov = sc.degrees_overlay(n, degs + [0] * (n - len(degs)), seed=E)
    assert ov.n_pairs == E == sum(degs)
    e = gsx.Engine(1)
    pp, tps = setup(e, ov, 1, (0,), seed=E, disconnect_frac=0.2 if E > 1 else 0.0)
    seg_check(e, ov, pp, tps, E)
    got = e.score_parts(EDGES, per_pair=True)
    present = int((e.export_state()["pair_flags"] != 0).sum())  # (a disconnected pair of positive score is forgotten)
    assert got.parts.shape == (E, 10) and int(got.cause_hist.sum()) == int(got.obs_cause.sum()) == present > 0
    assert same_scores(got.parts[:, abi.GSX_PART_SCORE], e.scores())
    if E > 1:
        assert len(np.unique(got.cause)) >= 2


SEG_ROWS = {  # score_stats_cases' row shapes by node count; the rest of the rows are drawn (0 .. 5)
    1: [0],
    63: [62, 2, 0, 0, 0, 40, 24],
    64: [63, 1, 0, 0, 60, 4, 0, 0],
    65: [64, 0, 0, 64, 3],
    129: [62, 2, 0, 0, 100, 36, 128],  # row 6: three waves, across the block edge at 256
}


@pytest.mark.parametrize("n", sorted(SEG_ROWS))
def test_row_shapes_that_break_segmentation(gpu_ok, n):
    rng = np.random.default_rng(n)
    degs = SEG_ROWS[n] + [int(x) for x in rng.integers(0, min(6, n), n - len(SEG_ROWS[n]))]
    ov = sc.degrees_overlay(n, degs, seed=n)
    e = gsx.Engine(1)
    pp, tps = setup(e, ov, 1, (0,), seed=n, disconnect_frac=0.2)
    if n > 1:
        rp, deg = ov.row_ptr, np.diff(ov.row_ptr)
        assert ((rp[1:][deg > 0] % 64) == 0).any()  # a row ends exactly on a wave's edge
    got = seg_check(e, ov, pp, tps, n)
    if n == 1:
        assert ov.n_pairs == 0 and not got.cause_hist.any() and not got.topic_hist.any() and got.parts.shape == (0, 10)
    else:
        assert len(np.unique(got.cause)) >= 3


# ---- 4. topic counts: the specialised instances and the general loop -------------------------------
@pytest.mark.parametrize("T", [1, 2, 4, 8, 9, 64])
def test_topic_counts(gpu_ok, T):
    ov = pc.overlay(50, 3, T)
    e = gsx.Engine(T)
    scored = tuple(t for t in range(T) if T < 3 or t % 5 != 1)
    pp, tps = setup(e, ov, T, scored, seed=T, disconnect_frac=0.1, mesh_degree=3)
    conn = np.nonzero(e.export_state()["pair_flags"] == PC)[0]
    e.apply_events(np.array([(abi.EV_INVALID_DELIVERY, int(p) % T, int(p), pc.T0 + 2 * S, 0) for p in conn[::3]]
                            + [(abi.EV_FIRST_DELIVERY, T - 1, int(p), pc.T0 + 2 * S, 0) for p in conn[1::4]],
                           dtype=abi.event_dtype()))
    e.refresh(pc.T0 + 5 * S)
    for select, topic in (("present", 0), ("mesh", T - 1)):
        got = e.score_parts(EDGES, select, topic, per_pair=True)
        assert_parts(got, want(e, ov, pp, tps, EDGES, select, topic), what=(T, select))
    assert got.topic_hist.shape == (len(EDGES) + 1, T + 1)
    worst = e.score_parts(EDGES, per_pair=True).worst_topic
    assert set(worst.tolist()) - {abi.GSX_TOPIC_NONE}
    assert set(worst.tolist()) - {abi.GSX_TOPIC_NONE} <= set(scored)


# ---- 5. deferred write-back -------------------------------------------------------------------------
def test_deferred_write_back(gpu_ok):
    seed, n, T = 23, 130, 2
    ov = pc.overlay(n, 3, seed)
    twins = []
    for k in (4, 1):
        e = gsx.Engine(T)
        e.set_decay_writeback(k)
        pp, tps = setup(e, ov, T, (0, 1), seed, disconnect_frac=0.1)
        conn = np.nonzero(e.export_state()["pair_flags"] == PC)[0]
        e.apply_events(np.array([(abi.EV_INVALID_DELIVERY, int(p) % T, int(p), pc.T0 + 2 * S, 0) for p in conn[::3] for _ in range(3)]
                                + [(abi.EV_PENALTY, 0, int(p), pc.T0 + 2 * S, 5) for p in conn[1::4]], dtype=abi.event_dtype()))
        twins.append(e)
    a, b = twins
    for step in (1, 2, 3):  # the stored counters and bp lag by 1, 2, 3 decays
        for e in twins:
            e.refresh(pc.T0 + (2 + step) * S)
        marks = a.zero_map_marked(), a.pair_zero_map_marked(abi.GSX_PZ_APP), a.pair_zero_map_marked(abi.GSX_PZ_P6)
        before, s_before = a.export_state(), a.scores()
        got = a.score_parts(EDGES, per_pair=True)
        ref = want(a, ov, pp, tps, EDGES)
        assert_parts(got, ref, what=step)
        assert_parts(b.score_parts(EDGES, per_pair=True), ref, what=("k = 1", step))
        assert (got.cause == abi.GSX_PART_P4).any() and (got.cause == abi.GSX_PART_P7).any()
        after = a.export_state()
        for f in abi.STATE_FIELDS:
            assert np.array_equal(before[f].view(np.uint8), after[f].view(np.uint8)), (step, f)
        assert same_scores(s_before, a.scores()) and same_scores(got.parts[:, abi.GSX_PART_SCORE], s_before)
        assert marks == (a.zero_map_marked(), a.pair_zero_map_marked(abi.GSX_PZ_APP), a.pair_zero_map_marked(abi.GSX_PZ_P6))
        assert a.zero_map_violations() == 0 and a.pair_zero_map_violations() == 0


# ---- 6. unsettled state ------------------------------------------------------------------------------
def test_unsettled_state(gpu_ok):
    seed, n = 17, 130
    ov = pc.overlay(n, 3, seed)
    e = gsx.Engine(1)
    e.set_prop_tracking(False)  # the lean path: the credit folds are left to the next reader
    pp, tps = setup(e, ov, 1, (0,), seed, disconnect_frac=0.05)
    now = pc.T0 + 2 * S
    conn = np.nonzero(e.export_state()["pair_flags"] == PC)[0]
    cfg = pc.config(GOSSIP, latency_ms=0, credit=abi.GSX_CREDIT_NOW)
    cfg.now_ns = now + S // 2
    assert e.propagate(pc.messages(n, 40, seed, invalid=0.2), cfg)[0].deliveries > 0
    e.apply_events(np.array([(abi.EV_INVALID_DELIVERY, 0, int(conn[20]), now + S, 0)] * 5
                            + [(abi.EV_PENALTY, 0, int(conn[21]), now + S, 2)], dtype=abi.event_dtype()))
    got = e.score_parts(EDGES, per_pair=True)  # before any score reader
    assert same_scores(got.parts[:, abi.GSX_PART_SCORE], e.scores())
    assert_parts(got, want(e, ov, pp, tps, EDGES))
    assert got.cause[conn[20]] == abi.GSX_PART_P4 and got.cause[conn[21]] == abi.GSX_PART_P7
    assert np.array_equal(got.cause_hist.sum(1), e.score_stats(EDGES).hist)


# ---- 7. non-finite values ----------------------------------------------------------------------------
@pytest.mark.parametrize("T,variant", nf.CASES)
def test_non_finite(gpu_ok, T, variant):
    ov = nf.overlay()
    e = gsx.Engine(T)
    nf.load(e, ov, T, variant)
    pp, tpl = nf.params(T, variant)
    tps = dict(enumerate(tpl))
    got = e.score_parts(EDGES, per_pair=True)
    ref = want(e, ov, pp, tps, EDGES)
    assert_parts(got, ref, what=(T, variant))
    scores = e.scores()
    assert same_scores(got.parts[:, abi.GSX_PART_SCORE], scores)
    nan_score = np.isnan(scores) & (e.export_state()["pair_flags"] != 0)
    assert nan_score.any() and np.isinf(scores).any()
    assert int(got.cause_hist[-1].sum()) >= int(nan_score.sum())  # a NaN score: the top bin
    assert np.array_equal(got.cause_hist.sum(1), e.score_stats(EDGES).hist)
    nan_part = np.isnan(got.parts[:, :8])
    assert nan_part.any() and not nan_part[np.arange(ov.n_pairs), np.minimum(got.cause, 7)][got.cause != 8].any()
    both = nan_part.any(1) & (got.cause != abi.GSX_CAUSE_NONE)
    assert both.any()  # a pair with a NaN part whose cause is another, negative part
    if variant == "w5zero":  # +inf * 0: P5 is its NaN
        p = 65  # recipes()[0]: app = +inf
        assert np.isnan(got.parts[p, abi.GSX_PART_P5]) and np.isnan(scores[p])


# ---- 8. the interface --------------------------------------------------------------------------------
DTYPES = {"pair_parts": np.float64, "pair_cause": np.uint8, "pair_topic": np.uint8, "cause_hist": np.uint64,
          "topic_hist": np.uint64, "obs_cause": np.uint32, "peer_cause": np.uint32}


@functools.lru_cache(maxsize=None)
def small():
    ov = pc.overlay(130, 3, 29)
    e = gsx.Engine(2)
    pp, tps = setup(e, ov, 2, (0, 1), 29, disconnect_frac=0.1)
    return e, ov, pp, tps


def raw_call(e, edges, arrays, select=abi.GSX_SS_PRESENT, topic=0):
    sp = abi.ScoreStatsSpec(select=select, topic=topic, n_edges=len(edges))
    for k, x in enumerate(edges[: abi.GSX_SS_MAX_EDGES]):
        sp.edges[k] = x
    out = abi.ScorePartsOut(**{f: a.ctypes.data for f, a in arrays.items()})
    return e.lib.gsx_score_parts(e.h, C.byref(sp), C.byref(out))


def test_each_output_alone_and_repeat(gpu_ok):
    e, ov, pp, tps = small()
    ref = want(e, ov, pp, tps, EDGES)
    assert_parts(e.score_parts(EDGES, per_pair=True), ref)
    assert_parts(e.score_parts(EDGES, per_pair=True), ref, "again")  # the outputs are overwritten
    for f in spm.FIELDS:
        a = np.full(ref[f].nbytes, 0xAB, dtype=np.uint8).view(DTYPES[f]).reshape(ref[f].shape)  # garbage in
        assert raw_call(e, EDGES, {f: a}) == 0, f
        assert spm.same_bytes(a, ref[f]), f
    e.timing_begin(3)
    for _ in range(2):
        e.score_parts(EDGES)
    tot, lo, hi, k = e.timing_end()
    assert k == 2 and tot > 0  # each call is one timed launch


def test_device_pointer_outputs(gpu_ok):
    import torch

    e, ov, pp, tps = small()
    ref = want(e, ov, pp, tps, EDGES)
    B, n, E, T = len(EDGES) + 1, ov.n, ov.n_pairs, e.n_topics
    t = (torch.full((E, 10), -1.0, dtype=torch.float64, device="cuda:0"),
         torch.full((E,), 77, dtype=torch.uint8, device="cuda:0"), torch.full((E,), 77, dtype=torch.uint8, device="cuda:0"),
         torch.full((B, 9), -1, dtype=torch.int64, device="cuda:0"), torch.full((B, T + 1), -1, dtype=torch.int64, device="cuda:0"),
         torch.full((n, 9), -1, dtype=torch.int32, device="cuda:0"), torch.full((n, 9), -1, dtype=torch.int32, device="cuda:0"))
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        assert e.score_parts(EDGES, out_ptrs=t) is None
        e.sync()
        runs.append([x.cpu().numpy().copy() for x in t])
    for f, a, b in zip(spm.FIELDS, *runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f  # two calls: byte-identical
        assert spm.same_bytes(a.view(DTYPES[f]).reshape(ref[f].shape), ref[f]), f
    # one device output beside a host output
    t[6].fill_(-1)
    torch.cuda.synchronize()
    ch = np.zeros((B, 9), dtype=np.uint64)
    sp = abi.ScoreStatsSpec(n_edges=len(EDGES))
    for k, x in enumerate(EDGES):
        sp.edges[k] = x
    out = abi.ScorePartsOut(cause_hist=ch.ctypes.data, peer_cause=t[6].data_ptr())
    assert e.lib.gsx_score_parts(e.h, C.byref(sp), C.byref(out)) == 0
    e.sync()
    assert np.array_equal(ch, ref["cause_hist"]) and np.array_equal(t[6].cpu().numpy().view(np.uint32), ref["peer_cause"])


def test_errors_and_empty_engines(gpu_ok):
    e, ov, pp, tps = small()
    ch = {"cause_hist": np.zeros((8, 9), dtype=np.uint64)}
    assert raw_call(e, [0.0], ch) == 0
    assert raw_call(e, [0.0], ch, select=3) == abi.GSX_EINVAL
    assert raw_call(e, [0.0], ch, select=abi.GSX_SS_MESH, topic=2) == abi.GSX_EINVAL  # topic >= n_topics
    assert raw_call(e, [0.0], ch, select=abi.GSX_SS_MESH, topic=1) == 0
    assert raw_call(e, [0.0], ch, select=abi.GSX_SS_PRESENT, topic=99) == 0
    for bad in ([np.nan], [np.inf], [0.0, 0.0], [1.0, 0.0]):
        assert raw_call(e, bad, ch) == abi.GSX_EINVAL, bad
    sp, ok = abi.ScoreStatsSpec(n_edges=8), abi.ScoreStatsSpec()
    out = abi.ScorePartsOut(cause_hist=ch["cause_hist"].ctypes.data)
    assert e.lib.gsx_score_parts(e.h, C.byref(sp), C.byref(out)) == abi.GSX_EINVAL  # n_edges > 7
    with pytest.raises(gsx.GsxError) as ei:
        e.score_parts(list(range(8)))
    assert ei.value.code == abi.GSX_EINVAL
    assert e.lib.gsx_score_parts(None, C.byref(ok), C.byref(out)) == abi.GSX_EINVAL
    assert e.lib.gsx_score_parts(e.h, None, C.byref(out)) == abi.GSX_EINVAL
    assert e.lib.gsx_score_parts(e.h, C.byref(ok), None) == abi.GSX_EINVAL
    assert e.lib.gsx_score_parts(e.h, C.byref(ok), C.byref(abi.ScorePartsOut())) == 0  # all NULL: nothing to do
    assert_parts(e.score_parts(EDGES, per_pair=True), want(e, ov, pp, tps, EDGES))  # the engine is as it was
    fresh = gsx.Engine(1)
    assert fresh.lib.gsx_score_parts(fresh.h, C.byref(ok), C.byref(out)) == abi.GSX_ESTATE  # no overlay loaded
    # a range shard: not offered
    shard = gsx.Engine(1)
    half = ov.n // 2
    rp = ov.row_ptr[: half + 1]
    shard.load_overlay_shard(ov.n, 0, rp, ov.col[: rp[-1]], ov.edge_flags[: rp[-1]], ov.node_ips)
    assert shard.lib.gsx_score_parts(shard.h, C.byref(ok), C.byref(out)) == abi.GSX_EINVAL
    # an engine of no nodes, and one of nodes without pairs: zeroed tables
    for nn in (0, 3):
        empty = gsx.Engine(2)
        empty.set_peer_params(synth.bench_peer_params())
        empty.load_overlay(np.zeros(nn + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
        tabs = {f: np.full((8, 9) if f == "cause_hist" else (8, 3), 0xAB, dtype=np.uint64) for f in ("cause_hist", "topic_hist")}
        assert raw_call(empty, [0.0], tabs) == 0
        assert not tabs["cause_hist"][:2].any() and not tabs["topic_hist"].reshape(-1)[:6].any()
        got = empty.score_parts([0.0], per_pair=True)
        assert got.parts.shape == (0, 10) and not got.cause_hist.any() and got.obs_cause.shape == (nn, 9)


def test_refused_while_a_sharded_exchange_is_in_flight(gpu_ok):
    """test_gpu_shard.py's probe: between gsx_hb_end and gsx_gx_end the call is refused with GSX_ESTATE
    (the exchange holds the round's sets), and on the same range shard with nothing in flight with
    GSX_EINVAL."""
    import gossip_cases as gc
    from gsx import shard

    n, d, seed, T, world = 600, 6, 53, 1, 2
    ov = pc.overlay(n, d, seed)
    full = gsx.Engine(T)
    app = pc.setup(full, ov, T, seed, mesh_degree=6)
    st0 = full.export_state()
    E = ov.n_pairs
    rank_lo = synth.shard_ranges(n, world)
    engines = []
    for k in range(world):
        lo, hi = int(rank_lo[k]), int(rank_lo[k + 1])
        sh = synth.shard_of(ov, lo, hi)
        a, b = int(ov.row_ptr[lo]), int(ov.row_ptr[hi])
        e = gsx.Engine(T)
        e.set_peer_params(synth.bench_peer_params())
        tp = synth.spam_test_topic_params()
        tp.mesh_message_deliveries_window_ns = 25 * abi.MILLISECOND
        e.set_topic_params(0, tp)
        e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                        accept_px_threshold=0, opportunistic_graft_threshold=0))
        e.load_overlay_shard(n, lo, sh.row_ptr, sh.col, sh.edge_flags, sh.node_ips)
        st = {f: (st0[f].reshape(T, E)[:, a:b].reshape(-1).copy() if f in abi.RECORD_FIELDS else st0[f][a:b].copy())
              for f in abi.STATE_FIELDS}
        st["last_refresh_ns"] = st0["last_refresh_ns"]
        e.import_state(st)
        e.set_app_scores(app[a:b])
        e.set_gossipsub_params(gc.params())
        engines.append(e)

    def call(be):
        ch = np.zeros((2, 9), dtype=np.uint64)
        return raw_call(be, [0.0], {"cause_hist": ch})

    codes = []

    class Probe(shard.RangeSharded):
        def _gx_exchange(self, n_sets):
            assert self.be.gx_pending() is not None
            codes.append(call(self.be))
            return super()._gx_exchange(n_sets)

    runners = shard.run_local(world, "cuda:0", lambda tp, e: Probe(e, rank_lo, tp), [(e,) for e in engines])
    cfg = pc.config(GOSSIP, topic=0, max_hops=2, latency_ms=5, seed=seed)
    ms = pc.messages(n, 40, seed)
    shard.run_local(world, "cuda:0", lambda tp, r: (setattr(r, "tp", tp), r.propagate(ms, cfg))[1], [(r,) for r in runners])
    shard.run_local(world, "cuda:0", lambda tp, r: (setattr(r, "tp", tp), r.heartbeat(1, pc.T0 + S, 5))[1],
                    [(r,) for r in runners])
    assert codes and all(c == abi.GSX_ESTATE for c in codes), codes
    assert all(e.gx_pending() is None for e in engines)
    assert [call(e) for e in engines] == [abi.GSX_EINVAL] * world  # a range shard, nothing in flight


@pytest.mark.parametrize("T", [2, 8])
def test_an_overlay_of_no_pairs_loads_with_many_topics(gpu_ok, T):
    """The loader's per-(topic, pair) arrays are sized for their clears when there is no pair: nodes
    without links load under any topic count, and every reader sees empty or zeroed results."""
    e = gsx.Engine(T)
    e.set_peer_params(synth.bench_peer_params())
    for t in range(T):
        e.set_topic_params(t, synth.spam_test_topic_params())
    e.load_overlay(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32))
    e.refresh(pc.T0 + S)
    assert e.n_pairs == 0 and e.scores().shape == (0,)
    assert e.score_stats([0.0]).hist.tolist() == [0, 0]
    got = e.score_parts([0.0], per_pair=True)
    assert not got.cause_hist.any() and not got.topic_hist.any() and got.topic_hist.shape == (2, T + 1)
    assert got.obs_cause.shape == (5, 9) and not got.obs_cause.any() and not got.peer_cause.any()

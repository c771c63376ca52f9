"""Non-finite and extreme score values on every path that reads a score: the
engine against the oracle (which test_nonfinite_oracle.py holds to the plain
model, score_model.py) on the cases of nonfinite_cases.py.

The rules ("non-finite values"): scores, counters and snapshots
equal the oracle's, a NaN matching any NaN (x86 and gfx950 make different
default NaNs) and everything else as raw bits; a NaN score is below no
threshold and at or above none, as the reference's comparisons evaluate;
gsx_score_stats counts a NaN in the top bin and leaves it out of the minima.
zero_map_violations() stays 0 throughout."""
import numpy as np
import pytest

import gossip_cases as gc
import gsx
import heartbeat_cases as hc
import nonfinite_cases as nc
import oracle as orc
import propagation_cases as pc
import score_stats_cases as sc
import test_gpu_gater as tg
from gsx import abi

pytestmark = pytest.mark.gpu

S = abi.SECOND
T0 = nc.T0
INF = np.inf
GOSSIP = abi.GSX_ROUTER_GOSSIPSUB
THRESHOLDS = dict(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300, accept_px_threshold=0,
                  opportunistic_graft_threshold=0)


def same(eng, ora, where):
    nc.assert_same(eng.scores(), ora.scores(), f"{where}: scores")
    gs, ws = eng.export_state(), ora.export_state()
    for f in abi.STATE_FIELDS:
        nc.assert_same(gs[f], ws[f], f"{where}: state field {f}")
    assert gs["last_refresh_ns"] == ws["last_refresh_ns"], where
    assert eng.zero_map_violations() == 0, where
    return ws


def backends(T, variant, writeback=None):
    ov = nc.overlay()
    st, app = nc.state(ov, T, variant)
    eng, ora = gsx.Engine(T), orc.Oracle(T)
    for be in (eng, ora):
        nc.load(be, ov, T, variant, st, app)
        be.set_thresholds(abi.Thresholds(**THRESHOLDS))
    if writeback is not None:
        eng.set_decay_writeback(writeback)
    return ov, st, app, eng, ora


def refresh_both(eng, ora, now):
    for be in (eng, ora):
        be.refresh(now)


# ---- refresh ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("writeback", [None, 1])
@pytest.mark.parametrize("T,variant", nc.CASES)
def test_refresh(gpu_ok, T, variant, writeback):
    """After the import and after each of five refreshes (a whole write-back cycle and one
    more), with the deferred write-back at its default and off."""
    ov, st, app, eng, ora = backends(T, variant, writeback)
    same(eng, ora, f"T={T} {variant}: imported")
    now = T0
    for i in range(5):
        now += S
        refresh_both(eng, ora, now)
        ws = same(eng, ora, f"T={T} {variant} wb={writeback}: refresh {i + 1}")
    sc_ = ora.scores()
    assert np.isnan(sc_).any() and (sc_ == INF).any() and (sc_ == -INF).any()
    assert (ws["pair_flags"][128:192] == 0).sum() > (st["pair_flags"][128:192] == 0).sum()  # a retention ran out


# ---- score, score_many, peer_score_snapshot -----------------------------------------------------------
@pytest.mark.parametrize("T,variant", nc.CASES)
def test_direct_score_reads(gpu_ok, T, variant):
    """The single reads, with decays pending (two refreshes into the write-back cycle)."""
    ov, st, app, eng, ora = backends(T, variant)
    special = sorted(nc.special_lanes(variant)) + [1, 64, 129, 130, 131, 191]  # and ordinary, absent, retained ones
    for step in range(3):
        if step:
            refresh_both(eng, ora, T0 + step * S)
        want = ora.score_many(special)
        assert np.isnan(want).any() and (want == INF).any() and (want == -INF).any()
        nc.assert_same(eng.score_many(special), want, f"step {step}: score_many")
        nc.assert_same(np.array([eng.score(p) for p in special]), want, f"step {step}: score")
        gs, ws = eng.snapshot(), ora.snapshot()
        for f in ws:
            nc.assert_same(gs[f], ws[f], f"step {step}: snapshot {f}")
        nc.assert_same(gs["app_specific_score"][gs["present"] != 0], app[gs["present"] != 0], f"step {step}: P5")
    assert eng.zero_map_violations() == 0


# ---- events on special records -------------------------------------------------------------------------
@pytest.mark.parametrize("T,variant", nc.CASES)
def test_events_on_special_records(gpu_ok, T, variant):
    """A first delivery, an invalid delivery and a prune on records whose counters are inf, NaN,
    1e200 or subnormal, with a decay pending (rec_materialize, then the capped + 1)."""
    ov, st, app, eng, ora = backends(T, variant)
    now = T0 + S
    refresh_both(eng, ora, now)
    same(eng, ora, "one refresh")
    t = nc.special_topics(T)[-1]
    pairs = [p for p, r in nc.special_lanes(variant).items() if set(r) & set(nc.FIELD)]
    assert len(pairs) >= 15
    for kind in (abi.EV_FIRST_DELIVERY, abi.EV_INVALID_DELIVERY, abi.EV_MESH_DELIVERY, abi.EV_PRUNE):
        ev = np.array([(kind, t, p, now, 0) for p in pairs], dtype=abi.event_dtype())
        for be in (eng, ora):
            be.apply_events(ev)
        same(eng, ora, f"T={T} {variant}: event kind {kind}")
    refresh_both(eng, ora, now + S)
    same(eng, ora, "refresh after the events")


@pytest.mark.parametrize("T,variant", nc.CASES)
def test_remove_peer_on_special_scores(gpu_ok, T, variant):
    """RemovePeer on pairs scoring NaN, +inf, -inf and +0.0 + -0.0, with a decay pending: the
    reference forgets a peer if `score > 0` (score.go:615), so the NaN and the zero are
    retained like the -inf."""
    ov, st, app, eng, ora = backends(T, variant)
    now = T0 + S
    refresh_both(eng, ora, now)
    sc_ = ora.scores()
    conn = ora.export_state()["pair_flags"] == nc.CONNECTED
    pick = {"nan": np.nonzero(np.isnan(sc_) & conn)[0], "+inf": np.nonzero((sc_ == INF) & conn)[0],
            "-inf": np.nonzero((sc_ == -INF) & conn)[0], "zero": np.array([nc.ZERO_PAIR])}
    assert all(len(v) for v in pick.values()), {k: len(v) for k, v in pick.items()}
    assert sc_[nc.ZERO_PAIR] == 0.0 and not np.signbit(sc_[nc.ZERO_PAIR])
    rm = np.concatenate(list(pick.values()))
    ev = np.array([(abi.EV_REMOVE_PEER, 0, int(p), now + S, 0) for p in rm], dtype=abi.event_dtype())
    for be in (eng, ora):
        be.apply_events(ev)
    ws = same(eng, ora, f"T={T} {variant}: RemovePeer")
    pf = ws["pair_flags"]
    assert (pf[pick["nan"]] == abi.GSX_PAIR_PRESENT).all() and (pf[pick["-inf"]] == abi.GSX_PAIR_PRESENT).all()
    assert (pf[pick["+inf"]] == 0).all() and pf[nc.ZERO_PAIR] == abi.GSX_PAIR_PRESENT
    refresh_both(eng, ora, now + 2 * S)
    same(eng, ora, "refresh after RemovePeer")


# ---- accept_from ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,variant", [(1, "w5"), (3, "w5zero")])
def test_accept_from(gpu_ok, T, variant):
    """AcceptFrom with the gater set, on every pair, against gater_model.py and the oracle's
    scores: `score < graylist` (gossipsub.go:583-594) is false for a NaN, which reaches the gate."""
    ov, st, app, eng, ora = backends(T, variant)
    present = st["pair_flags"] != 0
    gp, mp = tg.gater_params()
    mr = tg.Mirror(eng, ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips, present, gp, mp, seed=5)
    obs = ov.pair_observer()
    first = [int(ov.row_ptr[u]) for u in range(ov.n) if ov.row_ptr[u] < ov.row_ptr[u + 1]]
    evs = [(abi.GATER_ADD_PEER, 0, int(p), T0, 0) for p in np.nonzero(present)[0]]
    evs += [(abi.GATER_REJECT, 0, p, T0, 7) for p in first for _ in range(4)]  # every observer throttles
    evs += [(abi.GATER_REJECT, 0, int(p), T0, 8) for p in np.nonzero(present)[0] if p % 2 for _ in range(40)]
    mr.check_export(mr.events(evs))
    sc_ = ora.scores()
    seen = set()
    nan_ok = 0
    for draw in range(4):
        got = eng.accept_from(T0 + S, 5, draw)
        want = mr.expected_status(np.arange(nc.E), T0 + S, draw, sc_)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        seen |= set(got.tolist())
        nan_ok += int((got[np.isnan(sc_)] != abi.GSX_ACCEPT_NONE).sum())
        assert (got[np.isnan(sc_)] != abi.GSX_ACCEPT_NONE).all()
        assert (got[sc_ == -INF] == abi.GSX_ACCEPT_NONE).all()
    assert seen == {abi.GSX_ACCEPT_NONE, abi.GSX_ACCEPT_CONTROL, abi.GSX_ACCEPT_ALL} and nan_ok > 0
    assert len(obs) == nc.E and eng.zero_map_violations() == 0


# ---- score_stats -----------------------------------------------------------------------------------------
def check_stats(eng, ora, ov, T, where):
    st = ora.export_state()
    s = ora.scores()
    for select, topic in (("present", 0), ("mesh", 0), ("mesh", T - 1)):
        got = eng.score_stats(None, select, topic)
        assert got.edges.tolist() == [-300.0, -200.0, -100.0, 0.0]  # the thresholds and 0.0
        ref = sc.reference(s, st["pair_flags"], st["rec_flags"], ov.row_ptr, ov.col, ov.n, got.edges, select, topic)
        sc.assert_equal(got, ref, what=(where, select, topic))
        assert not np.isnan(got.obs_min).any() and not np.isnan(got.peer_min).any()
        # below(graylist) is what the router's gate refuses: `score < graylist`
        pf = st["pair_flags"]
        sel = (pf & abi.GSX_PAIR_PRESENT) != 0
        if select == "mesh":
            sel = (pf == nc.CONNECTED) & ((st["rec_flags"].reshape(T, -1)[topic] & abi.GSX_REC_IN_MESH) != 0)
        with np.errstate(invalid="ignore"):
            gray = sel & (s < -300.0)
        h, o, p = got.below(-300.0)
        assert h == int(gray.sum())
        assert np.array_equal(o, np.bincount(ov.pair_observer()[gray], minlength=ov.n))
        assert np.array_equal(p, np.bincount(ov.col[gray], minlength=ov.n))
    return s, st


@pytest.mark.parametrize("T,variant", nc.CASES)
def test_score_stats_on_the_cases(gpu_ok, T, variant):
    ov, st, app, eng, ora = backends(T, variant)
    refresh_both(eng, ora, T0 + S)
    s, _ = check_stats(eng, ora, ov, T, f"T={T} {variant}")
    got = eng.score_stats(None, "present")
    assert got.hist[-1] >= np.isnan(s[st["pair_flags"] != 0]).sum() > 0  # the NaNs are in the top bin
    assert (got.obs_min == -INF).any() and (got.peer_min == -INF).any()  # -inf minimises as a value


def test_score_stats_nan_rows(gpu_ok):
    """A row whose only selected pair is a NaN; a row of 80 pairs, NaN in every one, that starts
    at pair 61 and so spans three waves (the row's segments add up through the atomics, the
    `shared` path); a peer, node 80, that only NaN-scored observers point at.  NaNs of both
    signs: a sign-set one would sort below -inf as a key, a sign-clear one above +inf."""
    n = 90
    rows = [[80], list(range(2, 62)), list(range(3, 83))] + [[0, 1] for _ in range(3, 10)] + [[] for _ in range(10, n)]
    ov = sc.overlay_from_rows(rows)
    E = ov.n_pairs
    obs = ov.pair_observer()
    assert ov.row_ptr[2] == 61 and ov.row_ptr[3] == 141 and E == 155
    rng = np.random.default_rng(3)
    app = rng.normal(0, 200, E)
    app[rng.random(E) < 0.1] = -INF
    app[rng.random(E) < 0.1] = INF
    nan_rows = (obs == 0) | (obs == 2)
    app[nan_rows] = np.where(np.arange(E) % 2 == 0, nc.POS_NAN, nc.NEG_NAN)[nan_rows]
    assert np.isnan(app[ov.col == 80]).all() and (ov.col == 80).sum() == 2
    eng, ora = gsx.Engine(2), orc.Oracle(2)
    ev = [(abi.EV_ADD_PEER, 0, p, T0, 0) for p in range(E)]
    ev += [(abi.EV_GRAFT, 1, p, T0, 0) for p in range(E) if p % 3 != 1]
    for be in (eng, ora):
        pp, tps = nc.params(2, "w5")
        be.set_peer_params(pp)
        for t, tp in enumerate(tps):
            be.set_topic_params(t, tp)
        be.set_thresholds(abi.Thresholds(**THRESHOLDS))
        be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
        be.apply_events(np.array(ev, dtype=abi.event_dtype()))
        be.set_app_scores(app)
    nc.assert_same(eng.scores(), ora.scores(), "scores")
    check_stats(eng, ora, ov, 2, "nan rows")
    for select, topic in (("present", 0), ("mesh", 1)):
        got = eng.score_stats(None, select, topic)
        B = len(got.edges) + 1
        for u in (0, 2):
            k = got.obs_bins[u].sum()
            assert k > 0 and got.obs_bins[u, B - 1] == k and got.obs_min[u] == INF, (select, u)
        assert got.peer_bins[80, B - 1] == got.peer_bins[80].sum() > 0 and got.peer_min[80] == INF
        _, o, p = got.below(0.0)
        assert o[0] == 0 and o[2] == 0 and p[80] == 0
        _, fo, fp = got.fraction_below(-300.0)
        assert fo[0] == 0.0 and fo[2] == 0.0 and fp[80] == 0.0


# ---- propagation -------------------------------------------------------------------------------------------
def special_app(ov, rf, base, seed):
    """NaN of either sign, +inf and -inf on a part of the floodsub pairs, of the mesh pairs and of
    the direct pairs (the score a pair holds is its observer's of the pair's peer: the sender)."""
    app = base.copy()
    vals = [nc.POS_NAN, INF, -INF, nc.NEG_NAN]
    ef = ov.edge_flags
    groups = {"floodsub": np.nonzero(ef & abi.GSX_EDGE_FLOODSUB)[0],
              "direct": np.nonzero(ef & abi.GSX_EDGE_DIRECT)[0],
              "mesh": np.nonzero((rf & abi.GSX_REC_IN_MESH) != 0)[0]}
    for name, g in groups.items():
        assert len(g) >= 12, name
        for j, q in enumerate(g[::3]):
            app[q] = vals[j % 4]
    return app, groups


@pytest.mark.parametrize("flood", [0, 1])
@pytest.mark.parametrize("m", [40, 130])
def test_propagation(gpu_ok, m, flood):
    """Three credited gossipsub calls in a row, of 40 messages (one word) or 130 (two), with no
    score read in between (the lazy and deferred folds and the term cache carry the credits; the
    130-message run defers its folds to the end), then settled: counters, hops, first senders,
    state and scores.  NaN and +-inf scores sit on floodsub, mesh and direct senders."""
    n, seed = 150, 23
    ov = pc.overlay(n, 4, seed, mix_protocols=True, direct_frac=0.08)
    eng, ora = gsx.Engine(1), orc.Oracle(1)
    late = m == 130
    if late:
        eng.set_prop_tracking(False)
    for be in (eng, ora):
        base = pc.setup(be, ov, 1, seed)
        rf = be.export_state()["rec_flags"]
        app, groups = special_app(ov, rf, base, seed)
        be.set_app_scores(app)
    same(eng, ora, "set up")
    sc0 = ora.scores()
    obs = ov.pair_observer()
    # (a floodsub peer the setup's GRAFT replies put in a mesh is sent to as a mesh peer)
    nan_fs = [q for q in groups["floodsub"] if np.isnan(sc0[q]) and not ov.edge_flags[q] & abi.GSX_EDGE_DIRECT
              and not rf[q] & abi.GSX_REC_IN_MESH]
    assert nan_fs and (sc0 == INF).any() and (sc0 == -INF).any()
    accepted = refused = 0
    for k in range(3):
        ms = pc.messages(n, m, seed + k, invalid=0.1)
        for j, q in enumerate(nan_fs[: m // 4]):  # publishers with a NaN-scored floodsub peer
            ms["source"][j] = obs[q]
        cfg = pc.config(GOSSIP, flood_publish=flood, latency_ms=0 if late else 5, seed=seed + k)
        cfg.now_ns = T0 + 3 * S + k * 10 * abi.MILLISECOND
        wo, whop, wfrm = ora.propagate(ms, cfg, want_results=True)
        go, ghop, gfrm = eng.propagate(ms, cfg, want_results=True)
        assert go.as_dict() == wo.as_dict(), (k, go.as_dict(), wo.as_dict())
        assert np.array_equal(ghop, whop), k
        assert late or np.array_equal(gfrm, wfrm), k  # (the late run keeps counts, no first senders)
        assert wo.deliveries > 0 and wo.graylisted > 0
        # on the oracle: AcceptFrom accepts a NaN-scored sender, the publish threshold refuses one
        for q in np.nonzero(np.isnan(sc0) & ((ov.edge_flags & abi.GSX_EDGE_DIRECT) == 0))[0]:
            accepted += int((wfrm[:, obs[q]] == ov.col[q]).sum())
        for j, q in enumerate(nan_fs[: m // 4]):
            assert wfrm[j, ov.col[q]] != obs[q], (k, j, q)
            refused += 1
    assert accepted > 0 and refused > 0
    eng.settle_scores()
    same(eng, ora, f"m={m} flood={flood}: settled")
    refresh_both(eng, ora, T0 + 4 * S)
    same(eng, ora, f"m={m} flood={flood}: refreshed")


# ---- one heartbeat with the gossip exchange -------------------------------------------------------------------
def test_heartbeat_extreme_scores(gpu_ok):
    """Scores of +-inf, +-DBL_MAX, +-0.0 and subnormals, and NO NaN: the reference sorts the mesh
    candidates by score (gossipsub.go, heartbeat: sort.Slice), and Go's sort is unspecified
    under an order that a NaN breaks, so there is no answer to compare with.  Mesh degree 14 is
    above Dhi: the over-subscription sort runs, and on tick 60 the opportunistic-graft median."""
    n, seed, T = 80, 31, 1
    ov = pc.overlay(n, 10, seed)
    vals = [INF, -INF, nc.DBL_MAX, -nc.DBL_MAX, 0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310]
    res = []
    for be in (gsx.Engine(T), orc.Oracle(T)):
        base = pc.setup(be, ov, T, seed, mesh_degree=14)
        app = np.abs(base)
        app[::2] = np.array(vals)[np.arange(len(app[::2])) % len(vals)]
        be.set_app_scores(app)
        th = dict(THRESHOLDS, opportunistic_graft_threshold=5.0)
        be.set_thresholds(abi.Thresholds(**th))
        be.set_gossipsub_params(gc.params())
        cfg = pc.config(GOSSIP, max_hops=2, latency_ms=5, seed=seed)
        be.propagate(pc.messages(n, 24, seed), cfg)
        outs = [be.heartbeat(tick, T0 + (3 + i) * S, seed * 31 + 7).as_dict() for i, tick in enumerate((59, 60))]
        res.append((outs, hc.snapshot(be)))
    (go, gs), (wo, ws) = res
    assert go == wo, [(k, go[i][k], wo[i][k]) for i in (0, 1) for k in wo[i] if go[i][k] != wo[i][k]]
    assert wo[0]["prunes"] > 0 and wo[0]["ihave_msgs"] > 0 and wo[1]["grafts"] > 0
    assert not np.isnan(ws["scores"]).any() and (ws["scores"] == INF).any() and (ws["scores"] == -INF).any()
    for f in ws:
        if f == "last_refresh_ns":
            assert gs[f] == ws[f]
        else:
            nc.assert_same(gs[f], ws[f], f"heartbeat: {f}")

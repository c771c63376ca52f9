"""The oracle against score_model.py (the plain restatement of score() and of
refreshScores' decay) on the non-finite / extreme cases of nonfinite_cases.py:
scores and every exported state array, after the import and after each of five
refreshes (a whole write-back cycle of the engine and one more, so the GPU
tests can take the oracle's word at every step they compare).

It also holds, on the oracle's scores alone, what keeps the GPU tests from
going hollow: every case contains a NaN score, a +inf, a -inf, a NaN that
arithmetic made from inputs that hold none, and at least half of the pairs
finite."""
import numpy as np
import pytest

import nonfinite_cases as nc
import oracle as orc
import score_model as sm
from gsx import abi

S = abi.SECOND


def model_of(ov, T, st, tps):
    """{pair: sm.PeerStats} of the present pairs of an import_state dict."""
    peers = {}
    for p in range(nc.E):
        pf = int(st["pair_flags"][p])
        if not pf & abi.GSX_PAIR_PRESENT:
            continue
        ps = sm.PeerStats()
        ps.connected = bool(pf & abi.GSX_PAIR_CONNECTED)
        ps.expire = int(st["expire_ns"][p])
        ps.behaviour_penalty = float(st["behaviour_penalty"][p])
        for t in range(T):
            r = t * nc.E + p
            ts = sm.TopicStats()
            ts.in_mesh = bool(st["rec_flags"][r] & abi.GSX_REC_IN_MESH)
            ts.mesh_message_deliveries_active = bool(st["rec_flags"][r] & abi.GSX_REC_ACTIVE)
            ts.graft_time = int(st["graft_time_ns"][r])
            ts.mesh_time = int(st["mesh_time_ns"][r])
            ts.first_message_deliveries = float(st["first_message_deliveries"][r])
            ts.mesh_message_deliveries = float(st["mesh_message_deliveries"][r])
            ts.mesh_failure_penalty = float(st["mesh_failure_penalty"][r])
            ts.invalid_message_deliveries = float(st["invalid_message_deliveries"][r])
            ps.topics[t] = ts
        peers[p] = ps
    return peers


def count_ips(peers, ov):
    """len(ps.peerIPs[ip]) for each peer's one IP: the observer's tracked peers on it, retained
    ones included (removeIPs runs when a peerStats is deleted, score.go:507, 617)."""
    obs = ov.pair_observer()
    ip = ov.node_ips[ov.col, 0]
    for p, ps in peers.items():
        ps.peers_in_ip = [sum(1 for q in peers if obs[q] == obs[p] and ip[q] == ip[p])]


def model_export(peers, T):
    """The model's state in gsx_export_state's form, for the present pairs (-> arrays, present mask)."""
    out = {f: np.zeros(T * nc.E if f in abi.RECORD_FIELDS else nc.E, dtype=abi.STATE_DTYPES[f])
           for f in abi.STATE_FIELDS}
    for p, ps in peers.items():
        out["pair_flags"][p] = abi.GSX_PAIR_PRESENT | (abi.GSX_PAIR_CONNECTED if ps.connected else 0)
        out["expire_ns"][p] = ps.expire
        out["behaviour_penalty"][p] = ps.behaviour_penalty
        for t, ts in ps.topics.items():
            r = t * nc.E + p
            out["first_message_deliveries"][r] = ts.first_message_deliveries
            out["mesh_message_deliveries"][r] = ts.mesh_message_deliveries
            out["mesh_failure_penalty"][r] = ts.mesh_failure_penalty
            out["invalid_message_deliveries"][r] = ts.invalid_message_deliveries
            out["graft_time_ns"][r] = ts.graft_time
            out["mesh_time_ns"][r] = ts.mesh_time if ts.in_mesh else 0  # (the view's rule, gsx.h)
            out["rec_flags"][r] = (abi.GSX_REC_IN_MESH if ts.in_mesh else 0) | \
                (abi.GSX_REC_ACTIVE if ts.mesh_message_deliveries_active else 0)
    present = np.zeros(nc.E, dtype=bool)
    present[list(peers)] = True
    return out, present


def check(ora, peers, pp, tpd, app, T, where):
    want = np.array([sm.score(peers.get(p), pp, tpd, float(app[p])) for p in range(nc.E)])
    got = ora.scores()
    nc.assert_same(got, want, f"{where}: scores")
    exp, present = model_export(peers, T)
    st = ora.export_state()
    nc.assert_same(st["pair_flags"], exp["pair_flags"], f"{where}: pair_flags")
    for f in abi.STATE_FIELDS:  # (a deleted peerStats has no state to compare)
        m = np.tile(present, T) if f in abi.RECORD_FIELDS else present
        nc.assert_same(st[f][m], exp[f][m], f"{where}: {f}")
    return got


def inputs_hold_nan(st, app, T, p):
    return bool(np.isnan(app[p]) or np.isnan(st["behaviour_penalty"][p]) or
                any(np.isnan(st[f].reshape(T, nc.E)[:, p]).any() for f in nc.FIELD.values()))


@pytest.mark.parametrize("T,variant", nc.CASES)
def test_oracle_equals_model(T, variant):
    ov = nc.overlay()
    ora = orc.Oracle(T)
    st, app = nc.load(ora, ov, T, variant)
    pp, tps = nc.params(T, variant)
    tpd = dict(enumerate(tps))
    peers = model_of(ov, T, st, tps)
    count_ips(peers, ov)
    assert (ora.snapshot()["ip_colocation_factor"] > 0).sum() >= 10  # P6 is in play
    scores = [check(ora, peers, pp, tpd, app, T, f"T={T} {variant}: imported")]
    now = nc.T0
    for i in range(5):
        now += S
        ora.refresh(now)
        peers = {p: ps for p, ps in peers.items() if sm.refresh(ps, pp, tpd, now)}
        count_ips(peers, ov)
        scores.append(check(ora, peers, pp, tpd, app, T, f"T={T} {variant}: refresh {i + 1}"))
    assert len(peers) < int((st["pair_flags"] != 0).sum())  # a retention ran out on the way

    # what the GPU tests rest on, step by step
    for k, sc in enumerate(scores):
        nan = np.isnan(sc)
        assert nan.any(), k
        assert (sc == np.inf).any() and (sc == -np.inf).any(), k
        made = [p for p in np.nonzero(nan)[0] if not inputs_hold_nan(st, app, T, p)]
        assert made, k
        assert np.isfinite(sc).sum() * 2 >= nc.E, (k, int(np.isfinite(sc).sum()))
    # the special values did land where they were aimed
    lanes = nc.special_lanes(variant)
    assert all(64 < p < 128 or p in (0, 63) or p >= 192 for p in lanes)
    assert np.isnan(scores[0][0]) and np.isnan(scores[-1][0])  # lane 0 of tile 0: a NaN app score


def test_go_div_truncates():
    assert [sm.go_div(a, b) for a, b in ((7, 2), (-7, 2), (7, -2), (-7, -2), (0, 5), (-1, 3))] == [3, -3, -3, 3, 0, 0]


def test_score_stats_reference_rules():
    """The numpy reference of gsx_score_stats: a NaN in the top bin and out of the minima,
    +-inf as ordered values."""
    import score_stats_cases as sc

    s = np.array([nc.NEG_NAN, -np.inf, nc.POS_NAN, np.inf, -5.0, nc.POS_NAN])
    pf = np.full(6, abi.GSX_PAIR_PRESENT, dtype=np.uint8)
    ref = sc.reference(s, pf, np.zeros(6, dtype=np.uint8), [0, 2, 3, 6], [3, 4, 3, 4, 5, 5], 6, [-10.0, 0.0])
    assert ref["hist"].tolist() == [1, 1, 4]
    assert ref["obs_bins"].tolist() == [[1, 0, 1], [0, 0, 1], [0, 1, 2]]
    assert ref["obs_min"].tolist() == [-np.inf, np.inf, -5.0]
    assert ref["peer_min"].tolist() == [np.inf, np.inf, np.inf, np.inf, -np.inf, -5.0]


def test_same_mask_rules():
    a = np.array([nc.POS_NAN, 0.0, 1.0, np.inf, nc.NEG_NAN])
    b = np.array([nc.NEG_NAN, -0.0, 1.0, np.inf, 5.0])
    assert nc.same_mask(a, b).tolist() == [True, False, True, True, False]

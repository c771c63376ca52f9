"""A plain restatement of gsx_score_parts' contract (include/gsx.h), written
against score.go:258-335 and score_model.py's types: what score() adds up for
one peer as one observer sees it, part by part, which part is to blame and on
which topic.  Python floats are IEEE binary64 and nothing is contracted, so
every product and sum rounds as Go's does.  It knows nothing of the engine's
layout.

pair_parts() is the model, for one pair.  parts_arrays() is the same
arithmetic on numpy arrays over all pairs at once (element-wise ufuncs round
like the scalar operations), pinned to pair_parts() by test_score_parts_model.py;
reference() builds every output table of the call from it."""
from __future__ import annotations

import numpy as np

import score_model as sm

P1, P2, P3, P3B, P4, P5, P6, P7, TOPICS, SCORE = range(10)
PARTS = 10
CAUSE_NONE = 8
CAUSES = 9
TOPIC_NONE = 0xFF
PRESENT, CONNECTED = 0x01, 0x02  # GSX_PAIR_*
IN_MESH, ACTIVE = 0x01, 0x02  # GSX_REC_*
SELECT = {"present": 0, "connected": 1, "mesh": 2}


def cause_of(parts) -> int:
    """The lowest j in 0..7 whose part is < 0 and not above any other; a NaN is below nothing."""
    lowest, cause = 0.0, CAUSE_NONE
    for j in range(CAUSE_NONE):
        if parts[j] < lowest:
            lowest, cause = parts[j], j
    return cause


def pair_parts(pstats, pp, topic_params, app_score: float, p6=None):
    """-> (parts [10], cause, worst topic).  pstats None: no peerStats.  topic_params: {topic
    index: TopicScoreParams} of the scored topics.  p6: the IP colocation factor if it is known
    (PeerScoreSnapshot), else computed from pstats.peers_in_ip."""
    parts = [0.0] * PARTS
    if pstats is None:
        return parts, CAUSE_NONE, TOPIC_NONE
    score, low, worst = 0.0, 0.0, TOPIC_NONE
    for topic in sorted(pstats.topics):
        tstats = pstats.topics[topic]
        tp = topic_params.get(topic)
        if tp is None:
            continue
        tw = tp.topic_weight
        topic_score = 0.0
        if tstats.in_mesh:
            p1 = float(sm.go_div(tstats.mesh_time, tp.time_in_mesh_quantum_ns))
            if p1 > tp.time_in_mesh_cap:
                p1 = tp.time_in_mesh_cap
            t1 = p1 * tp.time_in_mesh_weight
            topic_score += t1
            parts[P1] += t1 * tw
        t2 = tstats.first_message_deliveries * tp.first_message_deliveries_weight
        topic_score += t2
        parts[P2] += t2 * tw
        if tstats.mesh_message_deliveries_active:
            if tstats.mesh_message_deliveries < tp.mesh_message_deliveries_threshold:
                deficit = tp.mesh_message_deliveries_threshold - tstats.mesh_message_deliveries
                t3 = (deficit * deficit) * tp.mesh_message_deliveries_weight
                topic_score += t3
                parts[P3] += t3 * tw
        t3b = tstats.mesh_failure_penalty * tp.mesh_failure_penalty_weight
        topic_score += t3b
        parts[P3B] += t3b * tw
        t4 = (tstats.invalid_message_deliveries * tstats.invalid_message_deliveries) * tp.invalid_message_deliveries_weight
        topic_score += t4
        parts[P4] += t4 * tw
        ts = topic_score * tw
        score += ts
        if ts < low:
            low, worst = ts, topic
    if pp.topic_score_cap > 0 and score > pp.topic_score_cap:
        score = pp.topic_score_cap
    parts[TOPICS] = score
    parts[P5] = app_score * pp.app_specific_weight
    score += parts[P5]
    if pp.ip_colocation_factor_weight != 0:
        if p6 is None:
            p6 = sm.ip_colocation_factor(pstats, pp)
        parts[P6] = p6 * pp.ip_colocation_factor_weight
        score += parts[P6]
    if pstats.behaviour_penalty > pp.behaviour_penalty_threshold:
        excess = pstats.behaviour_penalty - pp.behaviour_penalty_threshold
        parts[P7] = (excess * excess) * pp.behaviour_penalty_weight
        score += parts[P7]
    parts[SCORE] = score
    return parts, cause_of(parts), worst


def _go_div(a, b: int):
    """Go's int64 `/` (truncated towards zero) on an int64 array."""
    q = np.abs(a) // abs(b)
    return np.where((a < 0) == (b < 0), q, -q)


def parts_arrays(rec, pair, pp, topic_params):
    """pair_parts() over all pairs.  rec: [T, E] arrays first_message_deliveries,
    mesh_message_deliveries, mesh_failure_penalty, invalid_message_deliveries, mesh_time_ns,
    rec_flags (GSX_REC_*); pair: [E] arrays pair_flags (GSX_PAIR_*), behaviour_penalty,
    app_specific_score, ip_colocation_factor.  -> (parts [E, 10] f64, cause [E] u8, topic [E] u8)"""
    pf = np.asarray(pair["pair_flags"], dtype=np.uint8)
    E = len(pf)
    f = {k: np.asarray(rec[k]).reshape(-1, max(E, 1)) for k in rec}  # (no pairs: no rows, the loop below is empty)
    parts = np.zeros((E, PARTS))
    score, low = np.zeros(E), np.zeros(E)
    worst = np.full(E, TOPIC_NONE, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for t in sorted(topic_params) if E else ():
            tp = topic_params[t]
            tw = tp.topic_weight
            in_mesh = (f["rec_flags"][t] & IN_MESH) != 0
            active = (f["rec_flags"][t] & ACTIVE) != 0
            ts = np.zeros(E)
            p1 = np.zeros(E)
            if in_mesh.any():
                p1[in_mesh] = _go_div(f["mesh_time_ns"][t][in_mesh].astype(np.int64),
                                      int(tp.time_in_mesh_quantum_ns)).astype(np.float64)
            p1 = np.where(p1 > tp.time_in_mesh_cap, tp.time_in_mesh_cap, p1)
            t1 = p1 * tp.time_in_mesh_weight
            ts = np.where(in_mesh, ts + t1, ts)
            parts[:, P1] = np.where(in_mesh, parts[:, P1] + t1 * tw, parts[:, P1])
            t2 = f["first_message_deliveries"][t] * tp.first_message_deliveries_weight
            ts = ts + t2
            parts[:, P2] += t2 * tw
            mmd = f["mesh_message_deliveries"][t]
            has3 = active & (mmd < tp.mesh_message_deliveries_threshold)
            deficit = tp.mesh_message_deliveries_threshold - mmd
            t3 = (deficit * deficit) * tp.mesh_message_deliveries_weight
            ts = np.where(has3, ts + t3, ts)
            parts[:, P3] = np.where(has3, parts[:, P3] + t3 * tw, parts[:, P3])
            t3b = f["mesh_failure_penalty"][t] * tp.mesh_failure_penalty_weight
            ts = ts + t3b
            parts[:, P3B] += t3b * tw
            imd = f["invalid_message_deliveries"][t]
            t4 = (imd * imd) * tp.invalid_message_deliveries_weight
            ts = ts + t4
            parts[:, P4] += t4 * tw
            ts = ts * tw
            score = score + ts
            m = ts < low
            low = np.where(m, ts, low)
            worst = np.where(m, np.uint8(t), worst)
        if pp.topic_score_cap > 0:
            score = np.where(score > pp.topic_score_cap, pp.topic_score_cap, score)
        parts[:, TOPICS] = score
        parts[:, P5] = np.asarray(pair["app_specific_score"], dtype=np.float64) * pp.app_specific_weight
        score = score + parts[:, P5]
        if pp.ip_colocation_factor_weight != 0:
            parts[:, P6] = np.asarray(pair["ip_colocation_factor"], dtype=np.float64) * pp.ip_colocation_factor_weight
            score = score + parts[:, P6]
        bp = np.asarray(pair["behaviour_penalty"], dtype=np.float64)
        has7 = bp > pp.behaviour_penalty_threshold
        excess = bp - pp.behaviour_penalty_threshold
        t7 = (excess * excess) * pp.behaviour_penalty_weight
        parts[:, P7] = np.where(has7, t7, 0.0)
        score = np.where(has7, score + t7, score)
        parts[:, SCORE] = score
        lowest = np.zeros(E)
        cause = np.full(E, CAUSE_NONE, dtype=np.uint8)
        for j in range(CAUSE_NONE):
            m = parts[:, j] < lowest
            lowest = np.where(m, parts[:, j], lowest)
            cause = np.where(m, np.uint8(j), cause)
    absent = (pf & PRESENT) == 0
    parts[absent] = 0.0
    cause[absent] = CAUSE_NONE
    worst[absent] = TOPIC_NONE
    return parts, cause.astype(np.uint8), worst.astype(np.uint8)


FIELDS = ("pair_parts", "pair_cause", "pair_topic", "cause_hist", "topic_hist", "obs_cause", "peer_cause")


def reference(rec, pair, pp, topic_params, n_topics, row_ptr, col, n_total, edges, select="present", topic=0):
    """Every output of gsx_score_parts -> dict(pair_parts [E, 10] f64, pair_cause [E] u8,
    pair_topic [E] u8, cause_hist [B, 9] u64, topic_hist [B, T + 1] u64, obs_cause [n, 9] u32,
    peer_cause [n_total, 9] u32), B = len(edges) + 1."""
    parts, cause, worst = parts_arrays(rec, pair, pp, topic_params)
    pf = np.asarray(pair["pair_flags"], dtype=np.uint8)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    E, n_local, B = len(pf), len(row_ptr) - 1, len(edges) + 1
    sel = (pf & PRESENT) != 0
    if SELECT.get(select, select) != SELECT["present"]:
        sel &= (pf & CONNECTED) != 0
    if SELECT.get(select, select) == SELECT["mesh"] and E:
        sel &= (np.asarray(rec["rec_flags"], dtype=np.uint8).reshape(-1, E)[topic] & IN_MESH) != 0
    obs = np.repeat(np.arange(n_local, dtype=np.int64), np.diff(row_ptr))
    q = np.nonzero(sel)[0]
    b = np.searchsorted(edges, parts[q, SCORE], side="right")  # a NaN: the top bin
    c = cause[q].astype(np.int64)
    w = np.where(worst[q] == TOPIC_NONE, n_topics, worst[q]).astype(np.int64)
    cause_hist = np.zeros((B, CAUSES), dtype=np.uint64)
    np.add.at(cause_hist, (b, c), np.uint64(1))
    topic_hist = np.zeros((B, n_topics + 1), dtype=np.uint64)
    np.add.at(topic_hist, (b, w), np.uint64(1))
    obs_cause = np.zeros((n_local, CAUSES), dtype=np.uint32)
    np.add.at(obs_cause, (obs[q], c), np.uint32(1))
    peer_cause = np.zeros((n_total, CAUSES), dtype=np.uint32)
    np.add.at(peer_cause, (col[q], c), np.uint32(1))
    return {"pair_parts": parts, "pair_cause": cause, "pair_topic": worst, "cause_hist": cause_hist,
            "topic_hist": topic_hist, "obs_cause": obs_cause, "peer_cause": peer_cause}


def same_bytes(got, ref) -> bool:
    """Raw bytes, NaN == NaN whatever its payload."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    if got.dtype == np.float64:
        gn, rn = np.isnan(got), np.isnan(ref)
        return bool(np.array_equal(gn, rn) and np.array_equal(got[~gn].view(np.uint64), ref[~rn].view(np.uint64)))
    return bool(np.array_equal(got, ref))


def engine_inputs(e):
    """(rec, pair) for parts_arrays / reference from the engine's own export_state() and snapshot()."""
    st, sn = e.export_state(), e.snapshot()
    rec = {k: st[k] for k in ("first_message_deliveries", "mesh_message_deliveries", "mesh_failure_penalty",
                              "invalid_message_deliveries", "mesh_time_ns", "rec_flags")}
    pair = {"pair_flags": st["pair_flags"], "behaviour_penalty": st["behaviour_penalty"],
            "app_specific_score": sn["app_specific_score"], "ip_colocation_factor": sn["ip_colocation_factor"]}
    return rec, pair

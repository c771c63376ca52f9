"""A plain restatement, for one peer as one observer sees it, of the reference's
score() (score.go:258-335, with ipColocationFactor :337-381 reduced to the
counts it reads) and of refreshScores' share for that peer (:495-558): the
retention check, the per-record decay, mesh time and activation, and the P7
decay.  Python floats are IEEE binary64 and nothing here is contracted, so
every product and sum rounds as Go's does; Duration arithmetic is on Python
ints with Go's truncating division.  The counterpart of gater_model.py: it
knows nothing of the oracle's C or of the engine's layout, and it is the
checker of both where the values are not finite (Go's comparisons with a NaN
are all false but `!=`, as Python's are).

Parameters are any objects with the fields of score_params.go in snake case
(PeerScoreParams: topic_score_cap, app_specific_weight, ...; TopicScoreParams:
topic_weight, time_in_mesh_quantum_ns, ...); durations and times are ns.
"""
from __future__ import annotations


def go_div(a: int, b: int) -> int:
    """Go's int64 `/`: truncated towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class TopicStats:
    """topicStats, score.go:37-62"""

    def __init__(self):
        self.in_mesh = False
        self.graft_time = 0
        self.mesh_time = 0
        self.first_message_deliveries = 0.0
        self.mesh_message_deliveries = 0.0
        self.mesh_message_deliveries_active = False
        self.mesh_failure_penalty = 0.0
        self.invalid_message_deliveries = 0.0


class PeerStats:
    """peerStats, score.go:17-35.  topics: {topic index: TopicStats}; peers_in_ip: for each of
    the peer's IPs that is not whitelisted, len(ps.peerIPs[ip])."""

    def __init__(self):
        self.connected = True
        self.expire = 0
        self.topics = {}
        self.peers_in_ip = []
        self.behaviour_penalty = 0.0


def ip_colocation_factor(pstats: PeerStats, pp) -> float:
    """:337-381"""
    result = 0.0
    for peers_in_ip in pstats.peers_in_ip:
        if peers_in_ip > pp.ip_colocation_factor_threshold:  # :374
            surpluss = float(peers_in_ip - pp.ip_colocation_factor_threshold)
            result += surpluss * surpluss
    return result


def score(pstats, pp, topic_params, app_score: float) -> float:
    """:258-335.  pstats None: no peerStats, 0 (:259-262).  topic_params: {topic index:
    TopicScoreParams} of the scored topics, visited in ascending index (the order the
    engine and the oracle fix for Go's map range)."""
    if pstats is None:
        return 0.0
    score = 0.0
    for topic in sorted(pstats.topics):
        tstats = pstats.topics[topic]
        tp = topic_params.get(topic)
        if tp is None:  # :269-273
            continue
        topic_score = 0.0
        if tstats.in_mesh:  # P1 :279-285
            p1 = float(go_div(tstats.mesh_time, tp.time_in_mesh_quantum_ns))
            if p1 > tp.time_in_mesh_cap:
                p1 = tp.time_in_mesh_cap
            topic_score += p1 * tp.time_in_mesh_weight
        p2 = tstats.first_message_deliveries  # P2 :288-289
        topic_score += p2 * tp.first_message_deliveries_weight
        if tstats.mesh_message_deliveries_active:  # P3 :292-298
            if tstats.mesh_message_deliveries < tp.mesh_message_deliveries_threshold:
                deficit = tp.mesh_message_deliveries_threshold - tstats.mesh_message_deliveries
                p3 = deficit * deficit
                topic_score += p3 * tp.mesh_message_deliveries_weight
        p3b = tstats.mesh_failure_penalty  # P3b :302-303
        topic_score += p3b * tp.mesh_failure_penalty_weight
        p4 = tstats.invalid_message_deliveries * tstats.invalid_message_deliveries  # P4 :307-308
        topic_score += p4 * tp.invalid_message_deliveries_weight
        score += topic_score * tp.topic_weight  # :311
    if pp.topic_score_cap > 0 and score > pp.topic_score_cap:  # :315-317
        score = pp.topic_score_cap
    p5 = app_score  # P5 :320-321
    score += p5 * pp.app_specific_weight
    p6 = ip_colocation_factor(pstats, pp)  # P6 :324-325
    score += p6 * pp.ip_colocation_factor_weight
    if pstats.behaviour_penalty > pp.behaviour_penalty_threshold:  # P7 :328-332
        excess = pstats.behaviour_penalty - pp.behaviour_penalty_threshold
        p7 = excess * excess
        score += p7 * pp.behaviour_penalty_weight
    return score


def refresh(pstats: PeerStats, pp, topic_params, now: int) -> bool:
    """One peer's turn of refreshScores' loop, :502-557.  -> False if the peer's retention ran
    out and its peerStats is deleted (:505-509), True if it stays."""
    if not pstats.connected:
        return not now > pstats.expire  # now.After(pstats.expire); retained scores do not decay
    for topic, tstats in pstats.topics.items():
        tp = topic_params.get(topic)
        if tp is None:  # :520-524
            continue
        tstats.first_message_deliveries *= tp.first_message_deliveries_decay  # :527-542
        if tstats.first_message_deliveries < pp.decay_to_zero:
            tstats.first_message_deliveries = 0.0
        tstats.mesh_message_deliveries *= tp.mesh_message_deliveries_decay
        if tstats.mesh_message_deliveries < pp.decay_to_zero:
            tstats.mesh_message_deliveries = 0.0
        tstats.mesh_failure_penalty *= tp.mesh_failure_penalty_decay
        if tstats.mesh_failure_penalty < pp.decay_to_zero:
            tstats.mesh_failure_penalty = 0.0
        tstats.invalid_message_deliveries *= tp.invalid_message_deliveries_decay
        if tstats.invalid_message_deliveries < pp.decay_to_zero:
            tstats.invalid_message_deliveries = 0.0
        if tstats.in_mesh:  # :544-549
            tstats.mesh_time = now - tstats.graft_time
            if tstats.mesh_time > tp.mesh_message_deliveries_activation_ns:
                tstats.mesh_message_deliveries_active = True
    pstats.behaviour_penalty *= pp.behaviour_penalty_decay  # :553-556
    if pstats.behaviour_penalty < pp.decay_to_zero:
        pstats.behaviour_penalty = 0.0
    return True

"""gsx_score_parts without a device: the model of its contract
(score_parts_model.py) against score_model.score on randomized peerStats, its
tie and NaN rules on hand-made cases, its numpy form against its plain form,
the ScoreParts helpers, and the ABI's bookkeeping."""
import ctypes as C
import math
import os
import re
import struct
from types import SimpleNamespace as NS

import numpy as np
import pytest

import gsx
import score_model as sm
import score_parts_model as spm
from gsx import abi

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gsx.h")
INF, NAN = math.inf, math.nan


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def same(a: float, b: float) -> bool:
    return (a != a and b != b) or bits(a) == bits(b)


def topic_params(rng, **kw):
    tp = NS(topic_weight=float(rng.choice([0.25, 0.5, 1.0, 3.0])), time_in_mesh_weight=float(rng.choice([0.0, 0.01, 0.5])),
            time_in_mesh_quantum_ns=int(rng.choice([1, 10**6, 10**9])), time_in_mesh_cap=float(rng.choice([1.0, 10.0, 3600.0])),
            first_message_deliveries_weight=float(rng.choice([0.0, 1.0, 2.5])),
            mesh_message_deliveries_weight=float(rng.choice([0.0, -1.0, -0.3])),
            mesh_message_deliveries_threshold=float(rng.choice([1.0, 4.0, 20.0])),
            mesh_failure_penalty_weight=float(rng.choice([0.0, -1.0, -0.7])),
            invalid_message_deliveries_weight=float(rng.choice([0.0, -1.0, -99.0])))
    tp.__dict__.update(kw)
    return tp


def peer_params(rng, **kw):
    pp = NS(topic_score_cap=float(rng.choice([0.0, 5.0, 100.0])), app_specific_weight=float(rng.choice([0.0, 1.0, 0.5])),
            ip_colocation_factor_weight=float(rng.choice([0.0, -1.0, -5.0])), ip_colocation_factor_threshold=int(rng.choice([1, 3])),
            behaviour_penalty_weight=float(rng.choice([-1.0, -10.0])), behaviour_penalty_threshold=float(rng.choice([0.0, 2.0])))
    pp.__dict__.update(kw)
    return pp


def counter(rng):
    r = rng.random()
    if r < 0.04:
        return float(rng.choice([INF, NAN]))
    if r < 0.4:
        return 0.0
    return float(rng.random() * rng.choice([1.0, 10.0, 1000.0]))


def peer_stats(rng, T):
    ps = sm.PeerStats()
    ps.connected = bool(rng.random() < 0.9)
    ps.behaviour_penalty = counter(rng)
    ps.peers_in_ip = [int(x) for x in rng.integers(1, 8, rng.integers(0, 3))]
    for t in range(T):
        ts = sm.TopicStats()
        ts.in_mesh = bool(rng.random() < 0.6)
        ts.mesh_time = int(rng.integers(0, 10**12)) if ts.in_mesh else 0
        ts.mesh_message_deliveries_active = ts.in_mesh and bool(rng.random() < 0.7)
        ts.first_message_deliveries = counter(rng)
        ts.mesh_message_deliveries = counter(rng)
        ts.mesh_failure_penalty = counter(rng)
        ts.invalid_message_deliveries = counter(rng)
        ps.topics[t] = ts
    return ps


def app_score(rng):
    r = rng.random()
    return float(rng.choice([INF, -INF, NAN])) if r < 0.1 else 0.0 if r < 0.3 else float(rng.normal(0, 50))


def test_model_score_is_score_model_score():
    rng = np.random.default_rng(1)
    T, seen = 4, {"cap": 0, "w6_zero": 0, "nonfinite": 0, "nan_score": 0}
    for i in range(1500):
        pp = peer_params(rng)
        tps = {t: topic_params(rng) for t in range(T) if t != 2}  # topic 2 is not scored
        if i % 3 == 0:  # a cap that bites: positive topic sums above it
            pp.topic_score_cap = 0.5
            for tp in tps.values():
                tp.first_message_deliveries_weight = 2.5
        ps = peer_stats(rng, T)
        app = app_score(rng)
        parts, cause, worst = spm.pair_parts(ps, pp, tps, app)
        want = sm.score(ps, pp, tps, app)
        assert same(parts[spm.SCORE], want), (i, parts[spm.SCORE], want)
        assert len(parts) == spm.PARTS and 0 <= cause <= spm.CAUSE_NONE
        assert worst == spm.TOPIC_NONE or (worst in tps)
        if cause != spm.CAUSE_NONE:
            assert parts[cause] < 0 and not any(parts[cause] > parts[j] for j in range(8))
            assert not any(parts[j] < 0 and not any(parts[j] > parts[k] for k in range(8)) for j in range(cause))
        else:
            assert not any(parts[j] < 0 for j in range(8))
        if pp.ip_colocation_factor_weight == 0:
            assert bits(parts[spm.P6]) == 0
            seen["w6_zero"] += 1
        if pp.topic_score_cap > 0 and parts[spm.TOPICS] == pp.topic_score_cap:
            seen["cap"] += 1
        seen["nonfinite"] += not all(math.isfinite(x) for x in parts)
        seen["nan_score"] += want != want
    assert all(v > 20 for v in seen.values()), seen
    assert spm.pair_parts(None, peer_params(rng), {}, 3.0) == ([0.0] * 10, spm.CAUSE_NONE, spm.TOPIC_NONE)


def flat_case():
    """One topic set where every weight is plain, for the hand-made cases."""
    pp = NS(topic_score_cap=0.0, app_specific_weight=1.0, ip_colocation_factor_weight=-1.0, ip_colocation_factor_threshold=1,
            behaviour_penalty_weight=-1.0, behaviour_penalty_threshold=0.0)
    tp = NS(topic_weight=1.0, time_in_mesh_weight=0.0, time_in_mesh_quantum_ns=1, time_in_mesh_cap=10.0,
            first_message_deliveries_weight=1.0, mesh_message_deliveries_weight=-1.0, mesh_message_deliveries_threshold=2.0,
            mesh_failure_penalty_weight=-1.0, invalid_message_deliveries_weight=-1.0)
    ps = sm.PeerStats()
    for t in range(3):
        ps.topics[t] = sm.TopicStats()
    return pp, {0: tp, 1: NS(**tp.__dict__), 2: NS(**tp.__dict__)}, ps


def test_cause_ties_and_nan():
    pp, tps, ps = flat_case()
    # P3b = -4 on topic 0, P4 = -(2 * 2) on topic 1, P7 = -(2 * 2): three equal lowest parts, the lowest index wins
    ps.topics[0].mesh_failure_penalty = 4.0
    ps.topics[1].invalid_message_deliveries = 2.0
    ps.behaviour_penalty = 2.0
    parts, cause, worst = spm.pair_parts(ps, pp, tps, 0.0)
    assert parts[spm.P3B] == parts[spm.P4] == parts[spm.P7] == -4.0 and cause == spm.P3B
    assert worst == 0  # topics 0 and 1 both weigh -4: the lowest t
    # a lower P5 takes over; an equal one (index above P3b) does not
    assert spm.pair_parts(ps, pp, tps, -4.5)[1] == spm.P5
    assert spm.pair_parts(ps, pp, tps, -4.0)[1] == spm.P3B
    # a NaN part is never the cause and hides none: P5 = NaN, P4 = NaN
    assert spm.pair_parts(ps, pp, tps, NAN)[1] == spm.P3B
    ps.topics[1].invalid_message_deliveries = NAN
    parts, cause, worst = spm.pair_parts(ps, pp, tps, NAN)
    assert parts[spm.P4] != parts[spm.P4] and parts[spm.SCORE] != parts[spm.SCORE] and cause == spm.P3B
    assert worst == 0  # topic 1's score is a NaN: below nothing
    # only NaN and non-negative parts: no cause, no topic
    ps.topics[0].mesh_failure_penalty = 0.0
    ps.behaviour_penalty = 0.0
    assert spm.pair_parts(ps, pp, tps, NAN)[1:] == (spm.CAUSE_NONE, spm.TOPIC_NONE)
    # -inf ties: two parts at -inf, the lowest index
    ps.topics[1].invalid_message_deliveries = INF
    assert spm.pair_parts(ps, pp, tps, -INF)[1:] == (spm.P4, 1)
    # -0.0 is not negative
    ps.topics[1].invalid_message_deliveries = 0.0
    assert spm.pair_parts(ps, pp, tps, -0.0)[1:] == (spm.CAUSE_NONE, spm.TOPIC_NONE)
    assert spm.cause_of([-1.0, -1.0, NAN, -INF, -INF, 0.0, 0.0, 0.0]) == 3


def test_topic_rules_and_cap():
    pp, tps, ps = flat_case()
    ps.topics[0].first_message_deliveries = 9.0
    ps.topics[1].invalid_message_deliveries = 1.0   # -1
    ps.topics[2].mesh_failure_penalty = 3.0         # -3: the worst topic, not the first negative one
    parts, cause, worst = spm.pair_parts(ps, pp, tps, 0.0)
    assert (cause, worst) == (spm.P3B, 2) and parts[spm.TOPICS] == 5.0
    pp.topic_score_cap = 2.0  # the cap cuts the sum; parts 0-4 do not add up to TOPICS any more
    parts = spm.pair_parts(ps, pp, tps, 1.0)[0]
    assert parts[spm.TOPICS] == 2.0 and parts[spm.SCORE] == 3.0 and sum(parts[:5]) == 5.0
    del tps[2]  # an unscored topic adds nothing and is never the worst
    assert spm.pair_parts(ps, pp, tps, 0.0)[1:] == (spm.P4, 1)
    # P3 only for an active record under the threshold; P1 only in the mesh
    tps[0].time_in_mesh_weight = -1.0  # (a negative P1 weight: only the non-validating setters allow it)
    ps.topics[0].in_mesh, ps.topics[0].mesh_time = True, 7
    assert spm.pair_parts(ps, pp, tps, 0.0)[0][spm.P1] == -7.0
    ps.topics[0].mesh_message_deliveries_active = True
    assert spm.pair_parts(ps, pp, tps, 0.0)[0][spm.P3] == -4.0
    ps.topics[0].mesh_message_deliveries = 2.0
    assert bits(spm.pair_parts(ps, pp, tps, 0.0)[0][spm.P3]) == 0
    # w6 == 0: +0.0 whatever the factor; inf * 0 in P5 is its NaN
    pp.ip_colocation_factor_weight, pp.app_specific_weight = 0.0, 0.0
    ps.peers_in_ip = [9]
    parts = spm.pair_parts(ps, pp, tps, INF)[0]
    assert bits(parts[spm.P6]) == 0 and parts[spm.P5] != parts[spm.P5] and parts[spm.SCORE] != parts[spm.SCORE]


def arrays_of(stats, apps, pp, T):
    E = len(stats)
    rec = {k: np.zeros((T, E)) for k in ("first_message_deliveries", "mesh_message_deliveries", "mesh_failure_penalty",
                                         "invalid_message_deliveries")}
    rec["mesh_time_ns"] = np.zeros((T, E), dtype=np.int64)
    rec["rec_flags"] = np.zeros((T, E), dtype=np.uint8)
    pair = {"pair_flags": np.zeros(E, dtype=np.uint8), "behaviour_penalty": np.zeros(E),
            "app_specific_score": np.asarray(apps, dtype=np.float64), "ip_colocation_factor": np.zeros(E)}
    for p, ps in enumerate(stats):
        if ps is None:
            continue
        pair["pair_flags"][p] = spm.PRESENT | (spm.CONNECTED if ps.connected else 0)
        pair["behaviour_penalty"][p] = ps.behaviour_penalty
        pair["ip_colocation_factor"][p] = sm.ip_colocation_factor(ps, pp)
        for t, ts in ps.topics.items():
            rec["first_message_deliveries"][t, p] = ts.first_message_deliveries
            rec["mesh_message_deliveries"][t, p] = ts.mesh_message_deliveries
            rec["mesh_failure_penalty"][t, p] = ts.mesh_failure_penalty
            rec["invalid_message_deliveries"][t, p] = ts.invalid_message_deliveries
            rec["mesh_time_ns"][t, p] = ts.mesh_time
            rec["rec_flags"][t, p] = (spm.IN_MESH if ts.in_mesh else 0) | (spm.ACTIVE if ts.mesh_message_deliveries_active else 0)
    return rec, pair


@pytest.mark.parametrize("seed", [2, 3, 4])
def test_numpy_form_is_the_plain_form(seed):
    rng = np.random.default_rng(seed)
    T, E = 4, 400
    pp = peer_params(rng, topic_score_cap=[0.0, 3.0, 50.0][seed - 2], ip_colocation_factor_weight=[-1.0, 0.0, -5.0][seed - 2])
    tps = {t: topic_params(rng) for t in range(T) if t != 1}
    tps[0].time_in_mesh_weight, tps[0].first_message_deliveries_weight = -0.5, -1.0  # negative P1 / P2
    stats = [None if rng.random() < 0.1 else peer_stats(rng, T) for _ in range(E)]
    apps = [app_score(rng) for _ in range(E)]
    rec, pair = arrays_of(stats, apps, pp, T)
    parts, cause, worst = spm.parts_arrays(rec, pair, pp, tps)
    for p in range(E):
        w = spm.pair_parts(stats[p], pp, tps, apps[p])
        assert all(same(float(parts[p, j]), w[0][j]) for j in range(spm.PARTS)), (p, parts[p].tolist(), w[0])
        assert (int(cause[p]), int(worst[p])) == w[1:], p
    assert len(set(cause.tolist())) >= 6
    # the tables: a ring overlay of E pairs over 40 nodes, counted by hand
    n = 40
    row_ptr = np.arange(0, E + 1, E // n, dtype=np.int64)
    col = rng.integers(0, n, E).astype(np.int32)
    edges = [-100.0, -1.0, 0.0, 10.0]
    for select in ("present", "connected", "mesh"):
        ref = spm.reference(rec, pair, pp, tps, T, row_ptr, col, n, edges, select, topic=3)
        ch = np.zeros((5, 9), dtype=np.uint64)
        th = np.zeros((5, T + 1), dtype=np.uint64)
        oc, pc = np.zeros((n, 9), dtype=np.uint32), np.zeros((n, 9), dtype=np.uint32)
        for p in range(E):
            ps = stats[p]
            if ps is None or (select != "present" and not ps.connected) or (select == "mesh" and not ps.topics[3].in_mesh):
                continue
            s = float(parts[p, spm.SCORE])
            b = sum(1 for x in edges if not s < x)
            ch[b, cause[p]] += 1
            th[b, T if worst[p] == spm.TOPIC_NONE else worst[p]] += 1
            oc[p // (E // n), cause[p]] += 1
            pc[col[p], cause[p]] += 1
        for f, w in (("cause_hist", ch), ("topic_hist", th), ("obs_cause", oc), ("peer_cause", pc)):
            assert spm.same_bytes(ref[f], w), (select, f)
        assert ch.sum() > 0 and (ch.sum(1) == th.sum(1)).all()


def test_score_parts_helpers():
    edges = [-10.0, 0.0]
    ch = np.zeros((3, 9), dtype=np.uint64)
    ch[0, abi.GSX_PART_P4], ch[0, abi.GSX_PART_P7], ch[1, abi.GSX_PART_P4], ch[2, abi.GSX_CAUSE_NONE] = 3, 1, 2, 5
    th = np.zeros((3, 3), dtype=np.uint64)
    th[0, 1], th[1, 0], th[2, 2] = 4, 2, 5
    pc = np.zeros((4, 9), dtype=np.uint32)
    pc[2, abi.GSX_PART_P4], pc[3, abi.GSX_PART_P4], pc[0, abi.GSX_PART_P7] = 4, 1, 1
    sp = gsx.ScoreParts(edges, ch, th, None, pc)
    assert sp.blame(below=-10.0).tolist() == [0, 0, 0, 0, 3, 0, 0, 1, 0]
    assert sp.blame(below=0.0)[abi.GSX_PART_P4] == 5 and sp.blame().sum() == 11
    assert sp.blame_topics(below=0.0).tolist() == [2, 4, 0] and sp.blame_topics().tolist() == [2, 4, 5]
    assert sp.fraction("p4", below=-10.0) == 0.75 and sp.fraction(abi.GSX_PART_P7, below=0.0) == 1 / 6
    assert sp.peers_blamed("p4").tolist() == [2, 3] and sp.peers_blamed("p7").tolist() == [0]
    assert sp.peers_blamed("none").tolist() == [] and sp.obs_cause is None and sp.parts is None
    with pytest.raises(ValueError):
        sp.blame(below=1.0)
    empty = gsx.ScoreParts([0.0], np.zeros((2, 9)), np.zeros((2, 2)))
    assert math.isnan(empty.fraction("p1", below=0.0))


def test_abi_declares_score_parts():
    O = abi.ScorePartsOut
    assert C.sizeof(O) == 7 * C.sizeof(C.c_void_p)
    assert abi.SIGNATURES["gsx_score_parts"] == (C.c_int, [C.c_void_p, C.POINTER(abi.ScoreStatsSpec), C.POINTER(O)])
    src = open(HEADER).read()
    body = re.search(r"typedef struct gsx_score_parts_out \{(.*?)\} gsx_score_parts_out;", src, re.S).group(1)
    assert [f for f, _ in O._fields_] == re.findall(r"\*\s*(\w+);", body)
    for name in ("GSX_PART_P1", "GSX_PART_P2", "GSX_PART_P3", "GSX_PART_P3B", "GSX_PART_P4", "GSX_PART_P5", "GSX_PART_P6",
                 "GSX_PART_P7", "GSX_PART_TOPICS", "GSX_PART_SCORE", "GSX_PARTS", "GSX_CAUSE_NONE", "GSX_CAUSES",
                 "GSX_TOPIC_NONE"):
        v = re.search(rf"#define {name}\s+(\w+)", src).group(1)
        assert int(v.rstrip("u"), 0) == getattr(abi, name), name
    assert len(abi.PART_NAMES) == abi.GSX_PARTS and len(abi.CAUSE_NAMES) == abi.GSX_CAUSES
    assert (spm.PARTS, spm.CAUSES, spm.CAUSE_NONE, spm.TOPIC_NONE) == (abi.GSX_PARTS, abi.GSX_CAUSES, abi.GSX_CAUSE_NONE,
                                                                      abi.GSX_TOPIC_NONE)
    assert re.search(r"#define GSX_ABI_VERSION\s+5\b", src)
    lib = gsx.load_library()
    assert lib.gsx_score_parts(None, None, None) == abi.GSX_EINVAL  # a NULL engine, before any device work
    assert callable(gsx.Engine.score_parts)

"""Shared inputs of the non-finite / extreme value tests (test_nonfinite_oracle.py on
the CPU, test_gpu_nonfinite.py on the GPU), and the one comparison they use.

The overlay is the 197-pair one of test_gpu_refresh_stream.py: three full
64-pair tiles and a 5-lane tail, with T = 1 and 8 (the specialised instances
of the refresh pass) and 3 (the general one).  The special values sit on
single lanes of tile 1 (every other lane from 65 on, ordinary pairs between
them), on lanes 0 and 63 of tile 0 and on the five lanes of the tail; tile 2
mixes absent and retained pairs in.

The application scores go in through set_app_scores and the behaviour penalty
and the counters THROUGH import_state ONLY: no event can put an infinity, a
NaN or a value above its cap into a counter, import_state is the one entry
that takes such a double as it is.

Two variants of every T:
  "w5"      AppSpecificWeight 0.75, TopicScoreCap 30, DecayToZero 1e-300, decays 0.5,
            every weight non-zero;
  "w5zero"  AppSpecificWeight 0 (inf * 0), DecayToZero 1e-320 (a subnormal), decays
            0.999, and the weights of P3 and P4 zero (an overflowed counter times 0).
            With this weight no term after the cap can be +inf, so the variant runs
            without the cap (TopicScoreCap 0: `cap > 0 &&` short-circuits) and its
            +inf scores are topic sums; the capped +inf sum is variant "w5"'s.
"""
from __future__ import annotations

import math
import struct

import numpy as np

import propagation_cases as pc
from gsx import abi, synth

S = abi.SECOND
T0 = pc.T0
E = 197
TOPICS = [1, 8, 3]
VARIANTS = ["w5", "w5zero"]
CASES = [(T, v) for T in TOPICS for v in VARIANTS]
CONNECTED = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
CAP = 30.0
DBL_MAX = 1.7976931348623157e308
NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]  # x86's default NaN
POS_NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]  # gfx950's
INF = math.inf
MESH_ACTIVE = abi.GSX_REC_IN_MESH | abi.GSX_REC_ACTIVE


def same_mask(got, want):
    """Elementwise: equal as raw bits, or both NaN (sign and payload of a NaN are not
    compared: x86 and gfx950 produce different default NaNs)."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
    if g.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        return (g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w))
    return g == w


def assert_same(got, want, what):
    ok = same_mask(got, want)
    if not ok.all():
        bad = np.argwhere(~ok)[:6]
        raise AssertionError(f"{what}: differs at {bad.tolist()}: got "
                             f"{[np.asarray(got)[tuple(i)].item() for i in bad]} want "
                             f"{[np.asarray(want)[tuple(i)].item() for i in bad]}")


def overlay():
    """connectSome over 36 nodes, cut after its first 197 pairs (the scorer needs no reverse pair),
    with shared IPs."""
    ov = synth.connect_some_overlay(36, d=3)
    assert ov.n_pairs >= E
    ov.row_ptr = np.minimum(ov.row_ptr, E)
    ov.col = ov.col[:E].copy()
    ov.edge_flags = ov.edge_flags[:E].copy()
    assert ov.n_pairs == E and E == 3 * 64 + 5
    # six nodes to an IP: some observers see several peers on one, so P6 is not zero everywhere
    ov.node_ips = ov.node_ips.copy()
    ov.node_ips[:, 0] = 1000 + np.arange(ov.n) // 6
    return ov


def params(T, variant):
    """-> (PeerScoreParams, [TopicScoreParams] * T)"""
    b = variant == "w5zero"
    decay = 0.999 if b else 0.5
    pp = synth.bench_peer_params()
    pp.topic_score_cap = 0.0 if b else CAP
    pp.app_specific_weight = 0.0 if b else 0.75
    pp.decay_to_zero = 1e-320 if b else 1e-300
    pp.behaviour_penalty_decay = decay
    pp.retain_score_ns = 3 * S + S // 2
    tps = []
    for _ in range(T):
        tp = synth.spam_test_topic_params()
        tp.first_message_deliveries_decay = decay
        tp.mesh_message_deliveries_decay = decay
        tp.mesh_failure_penalty_decay = decay
        tp.invalid_message_deliveries_decay = decay
        if b:
            tp.mesh_message_deliveries_weight = 0.0
            tp.invalid_message_deliveries_weight = 0.0
        tps.append(tp)
    return pp, tps


def recipes(variant):
    """The special pairs' values: dicts of app (AppSpecificScore), bp (behaviour penalty) and
    the four counters fmd / mmd / mfp / imd (set on the case's special topics, mmd on a
    record that is in the mesh and active)."""
    dtz = 1e-320 if variant == "w5zero" else 1e-300
    up, dn = math.nextafter(dtz, INF), math.nextafter(dtz, 0.0)
    r = [dict(app=x) for x in (INF, -INF, POS_NAN, NEG_NAN, 0.0, -0.0, DBL_MAX, -DBL_MAX, 5e-324, -5e-324,
                               1e-310, -1e-310)]
    r += [dict(bp=1e200), dict(bp=2.0 ** 63)]  # excess squared overflows; 2^63
    r += [dict(app=INF, bp=1e200)]  # +inf + -inf
    r += [dict(imd=1e200), dict(mmd=-1e200), dict(mmd=1e200)]  # P4 and P3 overflow (their weights 0 in "w5zero")
    r += [dict(fmd=INF), dict(mfp=INF), dict(imd=INF), dict(mmd=-INF)]
    r += [dict(fmd=POS_NAN), dict(mmd=NEG_NAN), dict(mfp=POS_NAN), dict(imd=NEG_NAN)]
    r += [dict(fmd=5e-324, mmd=1e-310, mfp=1e-310, imd=5e-324), dict(fmd=1e-310, mmd=5e-324, mfp=5e-324, imd=1e-310)]
    # exactly at DecayToZero and one ulp either side, as stored and as the first decay by 0.5 leaves it
    r += [dict(fmd=dtz, mmd=up, mfp=dn, imd=dtz), dict(fmd=up, mmd=dn, mfp=dtz, imd=up),
          dict(fmd=dn, mmd=dtz, mfp=up, imd=dn),
          dict(fmd=2 * dtz, mmd=2 * up, mfp=2 * dn, imd=2 * dtz)]
    assert len(r) <= 32, len(r)
    return r


# recipes repeated at the tiles' edges: lane 0 and lane 63 of tile 0, and the tail
EDGE_LANES = {0: dict(app=POS_NAN), 63: dict(app=-INF), 192: dict(app=INF), 193: dict(imd=1e200),
              194: dict(fmd=NEG_NAN), 195: dict(bp=1e200), 196: dict(app=-0.0, zero=True)}
ZERO_PAIR = 196  # no counter, no penalty, in no mesh: its score is +0.0 + -0.0 (P5) + -0.0 (P6)


def special_lanes(variant):
    """{pair: recipe}"""
    out = {65 + 2 * j: r for j, r in enumerate(recipes(variant))}
    out.update(EDGE_LANES)
    return out


def special_topics(T):
    return sorted({0, T - 1, T // 2})


FIELD = {"fmd": "first_message_deliveries", "mmd": "mesh_message_deliveries", "mfp": "mesh_failure_penalty",
         "imd": "invalid_message_deliveries"}


def state(ov, T, variant):
    """-> (the state for import_state, the app score vector)"""
    st = synth.synthetic_state(ov, T, T0)
    pf = st["pair_flags"]
    pf[:] = CONNECTED
    # tile 2: absent and retained pairs mixed in (a retained pair's expiry 4 s or -1 s from T0)
    for p in range(128, 192):
        if p % 3 == 0:
            pf[p] = 0
        elif p % 5 == 0:
            pf[p] = abi.GSX_PAIR_PRESENT
            st["expire_ns"][p] = T0 + (4 * S if p % 2 else -S)
            st["rec_flags"][p::E] = 0  # RemovePeer took it out of every mesh
            st["mesh_time_ns"][p::E] = 0
    app = np.zeros(E)
    for p, r in special_lanes(variant).items():
        app[p] = r.get("app", 0.0)
        if r.get("zero"):
            st["behaviour_penalty"][p] = 0.0
            for f in list(FIELD.values()) + ["rec_flags", "mesh_time_ns"]:
                st[f][p::E] = 0
        if "bp" in r:
            st["behaviour_penalty"][p] = r["bp"]
        for t in special_topics(T):
            for k, f in FIELD.items():
                if k in r:
                    st[f].reshape(T, E)[t, p] = r[k]
            if "mmd" in r:  # P3 reads it only from an active record of the mesh
                st["rec_flags"].reshape(T, E)[t, p] = MESH_ACTIVE
                st["mesh_time_ns"].reshape(T, E)[t, p] = T0 - st["graft_time_ns"].reshape(T, E)[t, p]
    return st, app


def load(be, ov, T, variant, st=None, app=None):
    """Parameters, overlay, state and app scores of a case into a backend."""
    pp, tps = params(T, variant)
    be.set_peer_params(pp)
    for t, tp in enumerate(tps):
        be.set_topic_params(t, tp)
    be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    if st is None:
        st, app = state(ov, T, variant)
    be.import_state(st)
    be.set_app_scores(app)
    return st, app

"""The refresh + score pass's instruction stream ("Refresh pass:
exact P1 division by multiply"): P1's mesh_time / quantum without the software
divide (div_q1, gsx_ops.h), the decay loop counted in a scalar register when
the whole wave agrees on the count, and the flag / meshTime update as selects
under one branch on the pair's state.
Nothing a caller sees may change: engine == oracle bit for bit, scores and
every exported state array, after every call.

Shape: 197 pairs (three full tiles and a 5-lane tail) with T = 1, 8 (specialised
instances) and 3 (the general one).  Tile 1 (pairs 64..127) holds the single
lanes with the edge values; tile 2 mixes absent and retained pairs in; tile 0
and the tail are ordinary."""
import numpy as np
import pytest

import gsx
import oracle as orc
import propagation_cases as pc
from gsx import abi, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND
T0 = pc.T0
E = 197
TOPICS = [1, 8, 3]
BOUND = 1 << 50  # div_q1's fast path: |mesh_time| below it (gsx_ops.h DIV_Q1_BOUND)
CAP1 = 10.5      # a TimeInMeshCap that is no integer
ACT3 = 30 * S
QUANTA = {"1ns": 1, "1s": S, "odd": 3_600_000_000_007}
CONNECTED = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(eng, ora, where):
    got, want = eng.scores(), ora.scores()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        f"{where}: scores differ at pairs {np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0][:8]}"
    gs, ws = eng.export_state(), ora.export_state()
    for f in abi.STATE_FIELDS:
        assert np.array_equal(bits(gs[f]), bits(ws[f])), f"{where}: state field {f}"
    assert eng.zero_map_violations() == 0, where
    return ws


def overlay():
    """connectSome over 36 nodes, cut after its first 197 pairs (the scorer needs no reverse pair)."""
    ov = synth.connect_some_overlay(36, d=3)
    assert ov.n_pairs >= E
    ov.row_ptr = np.minimum(ov.row_ptr, E)
    ov.col = ov.col[:E].copy()
    ov.edge_flags = ov.edge_flags[:E].copy()
    assert ov.n_pairs == E and E == 3 * 64 + 5
    return ov


def topic_params(q1, decay):
    tp = synth.spam_test_topic_params()
    tp.time_in_mesh_quantum_ns = q1
    tp.time_in_mesh_cap = CAP1
    tp.mesh_message_deliveries_activation_ns = ACT3
    tp.first_message_deliveries_decay = decay
    tp.mesh_message_deliveries_decay = decay
    tp.mesh_failure_penalty_decay = decay
    tp.invalid_message_deliveries_decay = decay
    return tp


def backends(T, st, ov, q1=S, decay=0.3, dtz=20.0):
    bes = [gsx.Engine(T), orc.Oracle(T)]
    for be in bes:
        pp = synth.bench_peer_params()
        pp.decay_to_zero = dtz
        pp.retain_score_ns = 3 * S + S // 2
        be.set_peer_params(pp)
        for t in range(T):
            be.set_topic_params(t, topic_params(q1, decay))
        be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
        be.import_state(st)
        be.set_app_scores(np.zeros(E))
    return bes


def edge_mesh_times(q1):
    """mesh_time values, as of the first refresh (T0 + 1 s), for single lanes of tile 1."""
    capq = int(CAP1 * q1)  # cap1 * q1, truncated where the product is no integer
    v = [-5 * S, -1, 0, 1,                                   # graftTime after `now`, and around zero
         7 * q1 - 1, 7 * q1, 7 * q1 + 1,                     # a quantum boundary and 1 ns either side
         capq - 1, capq, capq + 1,                           # the cap
         10 * q1 - 1, 10 * q1 + 1, 11 * q1 - 1, 11 * q1, 11 * q1 + 1,  # the whole quanta around the cap
         ACT3 - 1, ACT3, ACT3 + 1,                           # activation: meshTime > activation
         BOUND - 1 - S, BOUND - S, BOUND + 12345, (1 << 52) + 1, (1 << 53) + 1, 3 << 60]  # around and past the bound
    return [int(x) for x in v]


def base_state(ov, T):
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
    return st


@pytest.mark.parametrize("quantum", list(QUANTA))
@pytest.mark.parametrize("T", TOPICS)
def test_mesh_time_edges(gpu_ok, T, quantum):
    q1 = QUANTA[quantum]
    ov = overlay()
    st = base_state(ov, T)
    now1 = T0 + S
    mts = edge_mesh_times(q1)
    assert len(mts) <= 60
    fl = st["rec_flags"].reshape(T, E)
    graft = st["graft_time_ns"].reshape(T, E)
    mesh = st["mesh_time_ns"].reshape(T, E)
    for t in {0, T - 1, T // 2}:
        for j, mt in enumerate(mts):
            p = 64 + 2 + j  # single lanes of tile 1, ordinary records between and around them
            fl[t, p] = abi.GSX_REC_IN_MESH  # not yet active
            graft[t, p] = now1 - mt
            mesh[t, p] = T0 - graft[t, p]  # as the refresh at T0 left it (0 would say: grafted since)
    eng, ora = backends(T, st, ov, q1=q1, decay=0.9)
    out = same(eng, ora, f"T={T} q1={q1}: imported")
    now = T0
    for i in range(5):  # a whole write-back cycle and one more
        now += S
        for be in (eng, ora):
            be.refresh(now)
        out = same(eng, ora, f"T={T} q1={q1}: refresh {i + 1}")
        if i == 0:  # the values did land where they were aimed (the oracle's export)
            got = out["mesh_time_ns"].reshape(T, E)[0, 66:66 + len(mts)]
            assert [int(x) for x in got] == mts
            act = (out["rec_flags"].reshape(T, E)[0, 66:66 + len(mts)] & abi.GSX_REC_ACTIVE) != 0
            assert [bool(a) for a in act] == [mt > ACT3 for mt in mts]


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("T", TOPICS)
def test_mixed_decay_counts(gpu_ok, T, phase):
    """An event materialises one lane's record of tile 1 after `phase` refreshes of
    the cycle.  At phases 1 to 3 that lane's count of pending decays then differs
    from its wave's (the lane-counted loop); at phase 0 nothing is pending, the
    event leaves the record's epoch where the wave's is and the counts stay equal
    (the scalar-counted loop, like tile 0 at every phase).  Lane j's mmd starts at 25 / 0.5^(j % 4): under decay
    0.5 and DecayToZero 20 it reaches zero at its (j % 4 + 1)-th decay, inside the
    multi-decay loop of whichever refresh applies it."""
    ov = overlay()
    st = base_state(ov, T)
    mmd = st["mesh_message_deliveries"].reshape(T, E)
    start = 25.0 / 0.5 ** (np.arange(E) % 4)
    mmd[:] = start
    eng, ora = backends(T, st, ov, decay=0.5)
    same(eng, ora, f"T={T}: imported")
    now = T0
    lane, t = 64 + 13, T - 1
    conn = st["pair_flags"] == CONNECTED
    conn[lane] = False  # (the delivery also counts in its mmd)
    for i in range(9):
        if i == phase:
            ev = np.array([(abi.EV_FIRST_DELIVERY, t, lane, now, 0)], dtype=abi.event_dtype())
            for be in (eng, ora):
                be.apply_events(ev)
            same(eng, ora, f"T={T} phase {phase}: after the event")
        now += S
        for be in (eng, ora):
            be.refresh(now)
        out = same(eng, ora, f"T={T} phase {phase}: refresh {i + 1}")
        if i < 4:  # the counters cross DecayToZero one residue class per decay
            z = out["mesh_message_deliveries"].reshape(T, E)[t] == 0
            assert np.array_equal(z[conn], (np.arange(E) % 4 <= i)[conn]), i

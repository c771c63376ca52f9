"""The 16-refresh write-back period and the decay chain (REC_EPOCH
and PAIR_EPOCH are four bits, gsx_ops.h runs k pending decays as k multiplies
and one zero test).  Nothing a caller sees may change: engine == oracle bit for
bit, scores and every field of abi.STATE_FIELDS, after EVERY call, at k = 16
(and once at k = 4 and k = 1), with up to 15 decays pending; the zero map's and
the pair zero map's invariants hold throughout (pair_epoch_cases.same).

Shapes: 60 nodes, ~360 pairs (full tiles and a partial one); T = 1, 3, 8 (the
specialised kernels) and 9 (the generic one).  Decays of 0.7 against
DecayToZero = 0.3: counters in [0, 1500) and penalties in [0, 5) cross
DecayToZero after 1 .. 24 decays, so many do with 5 .. 15 pending."""
import numpy as np
import pytest

import gsx
import nonfinite_cases as nc
import oracle as orc
import pair_epoch_cases as pe
import propagation_cases as pc
from gsx import abi, synth
from pair_epoch_cases import CONNECTED, RETAINED, S, T0

pytestmark = pytest.mark.gpu

N, D = 60, 3
CASES = [(1, 16), (3, 16), (8, 16), (9, 16), (8, 4), (3, 1)]
PHASES = (0, 3, 4, 8, 15)
DECAY, DTZ = 0.7, 0.3


def peer_params(d7=DECAY, dtz=DTZ, retain_ns=2 * S + S // 2):
    return pe.peer_params(retain_ns=retain_ns, d7=d7, dtz=dtz)


def topic_params(decay=DECAY):
    tp = synth.spam_test_topic_params()
    tp.first_message_deliveries_decay = decay
    tp.mesh_message_deliveries_decay = decay
    tp.mesh_failure_penalty_decay = decay
    tp.invalid_message_deliveries_decay = decay
    return tp


def start(T, k, extra=0, tps=None):
    ov = synth.connect_some_overlay(N, d=D)
    assert 256 < ov.n_pairs and ov.n_pairs % 64 != 0
    st = synth.synthetic_state(ov, T, T0, p_absent=0.1)
    imd = st["invalid_message_deliveries"]
    imd[::7] = 60.0 + np.arange(len(imd[::7]))
    in_mesh = (st["rec_flags"] & abi.GSX_REC_IN_MESH) != 0
    st["rec_flags"] = np.where(in_mesh, abi.GSX_REC_IN_MESH | abi.GSX_REC_ACTIVE, 0).astype(np.uint8)
    bes = [gsx.Engine(T) for _ in range(1 + extra)] + [orc.Oracle(T)]
    for be in bes:
        be.set_peer_params(peer_params())
        for t in range(T):
            be.set_topic_params(t, tps[t] if tps else topic_params())
        be.set_thresholds(abi.Thresholds(**pe.THRESHOLDS))
        be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
        be.import_state(st)
        be.set_app_scores(np.zeros(ov.n_pairs))
    for e in bes[:-1]:
        e.set_decay_writeback(k)
    return ov, bes


def event_batch(ora, T, now, rng):
    """Every event kind, each on a pair of its own: -> (events, retained pair, forgotten pair)."""
    st = ora.export_state()
    pf = st["pair_flags"]
    E = len(pf)
    fl = st["rec_flags"].reshape(T, E)
    conn = [int(p) for p in rng.permutation(np.nonzero(pf == CONNECTED)[0])]
    absent = np.nonzero(pf == 0)[0]
    t = int(rng.integers(T))
    meshed = [p for p in conn if fl[t, p] & abi.GSX_REC_IN_MESH]
    assert len(absent) and len(meshed) >= 2 and len(conn) > 12
    rest = [p for p in conn if p not in meshed[:2]]
    ev = [(abi.EV_ADD_PEER, 0, int(absent[0]), now, 0),
          (abi.EV_PRUNE, t, meshed[0], now, 0),
          (abi.EV_MESH_DELIVERY, t, meshed[1], now, 0),
          (abi.EV_GRAFT, t, rest[0], now, 0),
          (abi.EV_FIRST_DELIVERY, t, rest[1], now, 0),
          (abi.EV_INVALID_DELIVERY, t, rest[2], now, 0),
          (abi.EV_PENALTY, 0, rest[3], now, 3),
          (abi.EV_APP_SCORE, 0, rest[4], now, pe.f64_bits(-2.5))]
    ev += pe.remove_events(rest[5], now, -1e6)  # retained
    ev += pe.remove_events(rest[6], now, 1e9)   # forgotten (above any P4 of nine topics)
    return ev, rest[5], rest[6]


@pytest.mark.parametrize("T,k", CASES)
def test_forty_refreshes_events_at_phases(gpu_ok, T, k):
    """40 refreshes (the phase wraps twice at 16).  Before the refreshes that start at phases
    0, 3, 4, 8 and 15: every event kind, a penalty, a RemovePeer that retains and one that
    forgets; two refreshes later the retained pair reconnects.  An event leaves one lane's count
    different from its wave's, a retained pair makes a wave mix retained and connected lanes.
    Counters and penalties cross DecayToZero while 5 or more decays pend."""
    ov, (eng, ora) = start(T, k)
    ck = pe.Clock(eng, ora)
    rng = np.random.default_rng(100 * T + k)
    reconnect = {}
    cross_rec = cross_bp = 0
    pe.same(eng, ora, "imported")
    for n in range(40):
        where = f"T={T} k={k} before refresh {n + 1} (phase {n % k})"
        if n in reconnect:
            p = reconnect.pop(n)
            pe.events((eng, ora), [(abi.EV_ADD_PEER, 0, p, ck.now, 0), (abi.EV_PENALTY, 0, p, ck.now, 1)])
            assert pe.same(eng, ora, where + ": reconnect")["pair_flags"][p] == CONNECTED
        if n % 16 in PHASES:
            ev, kept, gone = event_batch(ora, T, ck.now, rng)
            pe.events((eng, ora), ev)
            out = pe.same(eng, ora, where + ": events")
            assert out["pair_flags"][kept] == RETAINED and out["pair_flags"][gone] == 0, where
            reconnect[n + 2] = kept
        before = ora.export_state()
        after = ck.step(where)
        if (n + 1) % 16 >= 5:  # (read by scores() and export_state() before the next store)
            for f in ("first_message_deliveries", "mesh_failure_penalty"):
                cross_rec += int(((before[f] >= DTZ) & (after[f] == 0)).sum())
            cross_bp += int(((before["behaviour_penalty"] >= DTZ) & (after["behaviour_penalty"] == 0)).sum())
    assert cross_rec > 0 and cross_bp > 0


@pytest.mark.parametrize("T,k", CASES)
def test_export_import_switches_and_setters_mid_cycle(gpu_ok, T, k):
    """Export at phase 9 into a second engine; the periods switched 16 -> 4 -> 1 -> 16 and both
    parameter setters, each with decays pending."""
    ov, (eng, eng2, ora) = start(T, k, extra=1)
    ck = pe.Clock(eng, ora)
    ck.step(f"T={T} k={k}: to phase 9", 9)
    pe.events((eng, ora), [(abi.EV_INVALID_DELIVERY, T - 1, 70, ck.now, 0), (abi.EV_PRUNE, 0, 3, ck.now, 0),
                           (abi.EV_PENALTY, 0, 9, ck.now, 2)])
    eng2.import_state(eng.export_state())
    eng2.set_decay_writeback(16)
    pe.same(eng2, ora, "importer at phase 9")
    pe.same(eng, ora, "exporter at phase 9")
    clock2 = pe.Clock(eng, eng2, ora, now=ck.now)

    def step(where, n):
        for i in range(n):
            clock2.now += S
            for be in (eng, eng2, ora):
                be.refresh(clock2.now)
            pe.same(eng, ora, f"{where}: exporter + {i}")
            pe.same(eng2, ora, f"{where}: importer + {i}")

    step("after the import", 6)
    for period in (4, 1, 16):  # (each with decays of the period before pending)
        for e in (eng, eng2):
            e.set_decay_writeback(period)
        pe.same(eng, ora, f"switched to {period}")
        pe.same(eng2, ora, f"importer switched to {period}")
        pe.events((eng, eng2, ora), [(abi.EV_FIRST_DELIVERY, 0, 5 + period, clock2.now, 0)])
        step(f"period {period}", 6)
    tp = topic_params(0.8)
    tp.first_message_deliveries_cap = 40.0
    tp.mesh_message_deliveries_cap = 30.0
    for be in (eng, eng2, ora):
        be.set_topic_params(T - 1, tp)
    pe.same(eng, ora, "set_topic_params at phase 6")
    step("after set_topic_params", 7)
    for be in (eng, eng2, ora):
        be.set_peer_params(peer_params(d7=0.6, dtz=0.05))
    pe.same(eng, ora, "set_peer_params at phase 7")
    step("after set_peer_params", 6)


@pytest.mark.parametrize("T", [1, 3, 8, 9])
def test_propagate_credits_at_a_late_phase(gpu_ok, T):
    """A credited gossipsub batch (folds and their re-scores) with 5 and with 12 decays pending."""
    ov = pc.overlay(120, D, seed=17)
    for ph in (5, 12):
        eng, ora = gsx.Engine(T), orc.Oracle(T)
        for be in (eng, ora):
            pc.setup(be, ov, T, seed=17)
            be.set_peer_params(pe.peer_params(retain_ns=10 * S, d7=0.8, dtz=0.3))
        eng.set_decay_writeback(16)
        ck = pe.Clock(eng, ora, now=T0 + 2 * S)
        ck.step(f"T={T} to phase {ph}", ph)
        for j in range(2):
            ms = pc.messages(120, 24, seed=17 + j)
            ms["validation"][5 + j] = abi.GSX_VALIDATION_REJECT
            cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=T - 1, latency_ms=10, seed=9 + j)
            cfg.now_ns = ck.now
            wo, whop, _ = ora.propagate(ms, cfg, want_results=True)
            go, ghop, _ = eng.propagate(ms, cfg, want_results=True)
            assert go.as_dict() == wo.as_dict() and wo.deliveries > 0, (ph, j)
            assert np.array_equal(ghop, whop), (ph, j)
            pe.same(eng, ora, f"T={T} phase {ph}: after batch {j}")
            ck.step(f"T={T} phase {ph}: after batch {j}", 1)
        ck.step(f"T={T} phase {ph}: after", 4)


@pytest.mark.parametrize("T", [1, 3, 8, 9])
def test_heartbeat_prune_at_a_late_phase(gpu_ok, T):
    """A heartbeat prunes a negative-score mesh peer (its own prune: P3b from the record's
    pending-decayed mmd) with 6 and with 13 decays pending."""
    for ph in (6, 13):
        ov, (eng, ora) = start(T, 16)
        E = ov.n_pairs
        st = ora.export_state()
        mmd = st["mesh_message_deliveries"].reshape(T, E)
        ok = ((st["rec_flags"].reshape(T, E) & abi.GSX_REC_ACTIVE) != 0) & (mmd < 100.0)
        ok[:, st["pair_flags"] == 0] = False
        t, p = (int(x) for x in np.argwhere(ok)[0])
        app = np.zeros(E)
        app[p] = -1000.0
        for be in (eng, ora):
            be.set_app_scores(app)
        ck = pe.Clock(eng, ora)
        ck.step(f"T={T} heartbeat at {ph}", ph)
        go = eng.heartbeat(1, ck.now + S // 2, 5).as_dict()
        wo = ora.heartbeat(1, ck.now + S // 2, 5).as_dict()
        assert go == wo and go["prunes"] > 0, ph
        pe.same(eng, ora, f"T={T} heartbeat at {ph}: after the round")
        ck.step(f"T={T} heartbeat at {ph}: after", 4)


@pytest.mark.parametrize("T,variant", [(1, "w5"), (3, "w5zero"), (8, "w5zero"), (9, "w5")])
def test_huge_and_non_finite_penalties(gpu_ok, T, variant):
    """bp of 1e200, 2^63, +inf, a NaN, 1e308 and the smallest subnormal (and the non-finite
    counters of nonfinite_cases.py) through a whole cycle of 16 and into the next, with an
    AddPenalty on each at phases 2 and 9."""
    ov = nc.overlay()
    st, app = nc.state(ov, T, variant)
    special = [p for p, r in nc.special_lanes(variant).items() if "bp" in r]
    extra = [2, 66, 4, 62]
    st["behaviour_penalty"][extra] = [np.inf, nc.POS_NAN, 1e308, 5e-324]
    st["pair_flags"][extra] = CONNECTED
    eng, ora = gsx.Engine(T), orc.Oracle(T)
    for be in (eng, ora):
        nc.load(be, ov, T, variant, st, app)
    eng.set_decay_writeback(16)

    def same(where):
        nc.assert_same(eng.scores(), ora.scores(), f"{where}: scores")
        gs, ws = eng.export_state(), ora.export_state()
        for f in abi.STATE_FIELDS:
            nc.assert_same(gs[f], ws[f], f"{where}: state field {f}")
        assert (gs["pair_flags"] & ~np.uint8(CONNECTED)).max() == 0, where
        assert eng.zero_map_violations() == 0 and eng.pair_zero_map_violations() == 0, where
        return ws

    same("imported")
    now = T0
    for i in range(19):
        now += S
        for be in (eng, ora):
            be.refresh(now)
        ws = same(f"T={T} {variant}: refresh {i + 1}")
        if i in (1, 8):
            ev = np.array([(abi.EV_PENALTY, 0, p, now, 1 + i) for p in special + extra], dtype=abi.event_dtype())
            for be in (eng, ora):
                be.apply_events(ev)
            same(f"T={T} {variant}: penalties after refresh {i + 1}")
    bp = ws["behaviour_penalty"]
    assert np.isinf(bp[2]) and np.isnan(bp[66])


@pytest.mark.parametrize("T", [3, 9])
def test_unvalidated_decays_keep_the_stepwise_form(gpu_ok, T):
    """A decay is validated only where its weight is not zero: topics with P2 / P3 weights of
    zero and decays of 3, -0.5 and 0 (values climb back over DecayToZero, change sign) still
    equal the oracle, which tests after every multiply, with up to 15 decays pending."""
    tps = []
    for t in range(T):
        tp = topic_params()
        if t % 2 == 0:
            tp.first_message_deliveries_weight = 0.0
            tp.first_message_deliveries_decay = 3.0 if t % 4 == 0 else 0.0
            tp.mesh_message_deliveries_weight = 0.0
            tp.mesh_message_deliveries_decay = -0.5
        tps.append(tp)
    ov, (eng, ora) = start(T, 16, tps=tps)
    ck = pe.Clock(eng, ora)
    pe.same(eng, ora, "imported")
    for n in range(20):
        if n in (3, 9):
            pe.events((eng, ora), [(abi.EV_FIRST_DELIVERY, t, 11 + t, ck.now, 0) for t in range(T)])
            pe.same(eng, ora, f"T={T}: deliveries before refresh {n + 1}")
        ck.step(f"T={T} unvalidated decays")


def test_setter_accepts_16_and_rejects_the_rest(gpu_ok):
    e = gsx.Engine(1)
    assert e.decay_writeback() == 16  # the default
    for k in (16, 4, 2, 1, 16):
        e.set_decay_writeback(k)
        assert e.decay_writeback() == k
    for held in (16, 4):
        e.set_decay_writeback(held)
        for k in (5, 8, 12, 17, 32):
            with pytest.raises(abi.GsxError, match="decay write-back period must be 1, 2, 4 or 16") as ex:
                e.set_decay_writeback(k)
            assert ex.value.code == abi.GSX_EINVAL
            assert e.decay_writeback() == held  # a refused value leaves the period in force

"""The behaviour penalty under the deferred write-back (PAIR_EPOCH):
the refresh pass stores bp only every k-th refresh and the stored value lags by
up to k - 1 decays of BehaviourPenaltyDecay in between, counted in two bits of
the device's pair flag byte.  Nothing a caller sees may change: every case
compares the engine with the oracle bit for bit, scores and every exported
state array, after every call, for the write-back periods 1, 2 and 4, with the
actions that read or write bp placed at every phase of a cycle.  The exported
pair flags never carry more than PRESENT | CONNECTED (pair_epoch_cases.same).

Shapes: 197 pairs (three full tiles and a partial one), T = 1 and T = 8; bp in
[0, 5) decays by 0.5 against DecayToZero = 0.3, so that penalties of every size
cross DecayToZero within one to five refreshes, in the middle of a cycle."""
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

PERIODS = [1, 2, 4]


def start(T, k, extra=0):
    ov, bes = pe.backends(T, pe.peer_params(retain_ns=3 * S + S // 2), extra=extra)
    for e in bes[:-1]:
        e.set_decay_writeback(k)
    return ov, bes


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("k", PERIODS)
def test_penalties_removals_and_reconnects_at_every_phase(gpu_ok, T, k):
    """AddPenalty on connected, retained and absent pairs, RemovePeer (retained and forgotten)
    and a reconnect two refreshes later, each started at every phase of the cycle and followed
    by five refreshes; bp values cross DecayToZero on the way."""
    ov, (eng, ora) = start(T, k)
    ck = pe.Clock(eng, ora)
    rng = np.random.default_rng(3 + k)
    zero_seen = crossing = 0
    for ph in range(k):
        for kind in ("penalty", "remove", "forget", "reconnect"):
            where = f"T={T} k={k} phase {ph} {kind}"
            while ck.n % k != ph:
                ck.step(where + ": aligning")
            st = ora.export_state()
            pf = st["pair_flags"]
            conn = np.nonzero(pf == CONNECTED)[0]
            if kind == "penalty":
                some = [int(p) for p in rng.choice(conn, 12, replace=False)]
                ev = [(abi.EV_PENALTY, 0, p, ck.now, 1 + i % 4) for i, p in enumerate(some)]
                ev += [(abi.EV_PENALTY, 0, some[0], ck.now, 2)]  # twice on one pair in one batch
                ev += [(abi.EV_PENALTY, 0, int(p), ck.now, 3) for p in np.nonzero(pf != CONNECTED)[0][:6]]
                pe.events((eng, ora), ev)
                pe.same(eng, ora, where)
            else:
                p = int(rng.choice(conn))
                pe.events((eng, ora), pe.remove_events(p, ck.now, 1e6 if kind == "forget" else -1e6))
                out = pe.same(eng, ora, where)
                assert out["pair_flags"][p] == (0 if kind == "forget" else RETAINED), where
                if kind == "reconnect":  # at another phase than the removal (k > 1)
                    ck.step(where + ": retained", 1 if k == 2 else 2)
                    pe.events((eng, ora), [(abi.EV_PENALTY, 0, p, ck.now, 2), (abi.EV_ADD_PEER, 0, p, ck.now, 0),
                                           (abi.EV_PENALTY, 0, p, ck.now, 1)])
                    assert pe.same(eng, ora, where + ": reconnected")["pair_flags"][p] == CONNECTED
                if kind == "forget":  # a new peerStats on the forgotten pair, mid-cycle
                    ck.step(where + ": forgotten", 1)
                    pe.events((eng, ora), [(abi.EV_APP_SCORE, 0, p, ck.now, 0), (abi.EV_ADD_PEER, 0, p, ck.now, 0),
                                           (abi.EV_PENALTY, 0, p, ck.now, 4)])
                    pe.same(eng, ora, where + ": added again")
            for _ in range(5):
                before = ora.export_state()["behaviour_penalty"]
                after = ck.step(where)["behaviour_penalty"]
                crossing += int(((before > 0) & (after == 0) & (ck.n % k != 0)).sum())
            zero_seen += int((after == 0).sum())
    assert zero_seen > 0 and (k == 1 or crossing > 0)  # penalties reached DecayToZero, some mid-cycle


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("k", PERIODS)
def test_export_import_and_period_switch_at_every_phase(gpu_ok, T, k):
    """An export in the middle of a cycle imported into a second engine, and a switch of the
    period there; both engines go on with the oracle."""
    for ph in range(k):
        ov, (eng, eng2, ora) = start(T, k, extra=1)
        ck = pe.Clock(eng, ora)
        where = f"T={T} k={k} phase {ph}"
        ck.step(where, ph + 1)
        pe.events((eng, ora), [(abi.EV_PENALTY, 0, p, ck.now, 2) for p in range(5, ov.n_pairs, 17)])
        if ph:
            ck.step(where + ": penalties", 1)
        st = eng.export_state()
        assert (st["pair_flags"] & ~np.uint8(CONNECTED)).max() == 0
        eng2.import_state(st)
        pe.same(eng2, ora, where + ": importer")
        pe.same(eng, ora, where + ": exporter")
        for i in range(6):
            if i == 2:  # the importer switches its period with decays pending, the exporter later
                eng2.set_decay_writeback(PERIODS[(PERIODS.index(k) + 1) % 3])
                pe.same(eng2, ora, where + ": importer switched")
            if i == 3:
                eng.set_decay_writeback(PERIODS[(PERIODS.index(k) + 2) % 3])
                pe.same(eng, ora, where + ": exporter switched")
            ck.now += S
            for be in (eng, eng2, ora):
                be.refresh(ck.now)
            pe.same(eng, ora, f"{where}: exporter + {i}")
            pe.same(eng2, ora, f"{where}: importer + {i}")
            pe.events((eng, eng2, ora), [(abi.EV_PENALTY, 0, 7 + 3 * i, ck.now, 1)])


@pytest.mark.parametrize("k", PERIODS)
def test_peer_params_switch_mid_cycle(gpu_ok, k):
    """Another BehaviourPenaltyDecay and DecayToZero while decays of the old ones pend."""
    ov, (eng, ora) = start(3, k)
    ck = pe.Clock(eng, ora)
    for ph in range(1, 4):
        ck.step(f"k={k} start {ph}", ph)
        for be in (eng, ora):
            be.set_peer_params(pe.peer_params(retain_ns=3 * S, d7=0.5 + 0.1 * ph, dtz=0.3 / ph))
        pe.same(eng, ora, f"k={k} set_peer_params after {ph}")
        pe.events((eng, ora), [(abi.EV_PENALTY, 0, p, ck.now, 3) for p in range(ph, ov.n_pairs, 11)])
        ck.step(f"k={k} after {ph}", 5)


@pytest.mark.parametrize("k", PERIODS)
@pytest.mark.parametrize("T,variant", [(1, "w5"), (8, "w5zero")])
def test_huge_and_non_finite_penalties(gpu_ok, T, variant, k):
    """bp of 1e200 and 2^63 (the cases of nonfinite_cases.py), and +inf and a NaN beside them,
    through a whole cycle and one more, with an AddPenalty on each in the middle."""
    ov = nc.overlay()
    st, app = nc.state(ov, T, variant)
    special = [p for p, r in nc.special_lanes(variant).items() if "bp" in r]
    assert len(special) >= 3
    extra = [2, 66, 4, 62]
    st["behaviour_penalty"][extra] = [np.inf, nc.POS_NAN, 1e308, 5e-324]
    st["pair_flags"][extra] = CONNECTED
    eng, ora = gsx.Engine(T), orc.Oracle(T)
    for be in (eng, ora):
        nc.load(be, ov, T, variant, st, app)
    eng.set_decay_writeback(k)

    def same(where):
        nc.assert_same(eng.scores(), ora.scores(), f"{where}: scores")
        gs, ws = eng.export_state(), ora.export_state()
        for f in abi.STATE_FIELDS:
            nc.assert_same(gs[f], ws[f], f"{where}: state field {f}")
        assert (gs["pair_flags"] & ~np.uint8(CONNECTED)).max() == 0, where
        return ws

    same("imported")
    now = T0
    for i in range(6):
        now += S
        for be in (eng, ora):
            be.refresh(now)
        ws = same(f"T={T} {variant} k={k}: refresh {i + 1}")
        if i in (1, 2):
            ev = np.array([(abi.EV_PENALTY, 0, p, now, 1 + i) for p in special + extra], dtype=abi.event_dtype())
            for be in (eng, ora):
                be.apply_events(ev)
            same(f"T={T} {variant} k={k}: penalties after refresh {i + 1}")
    bp = ws["behaviour_penalty"]
    assert np.isinf(bp[2]) and np.isnan(bp[66]) and (bp[special] > 1e15).all()


@pytest.mark.parametrize("k", PERIODS)
@pytest.mark.parametrize("T", [1, 3])
def test_propagate_mid_cycle(gpu_ok, T, k):
    """A credited gossipsub batch in the middle of a cycle, on pairs whose behaviour penalty puts
    them around the publish and graylist thresholds (P7 = -10 bp^2): the folds' re-scores read bp
    with its pending decays (k_prop_count: T = 1 its fused fold, T = 3 fold_pair), so the
    counters, the hops and the scores equal the oracle's."""
    n = 120
    ov = pc.overlay(n, 3, seed=17)
    for ph in range(k):
        eng, ora = gsx.Engine(T), orc.Oracle(T)
        for be in (eng, ora):
            pc.setup(be, ov, T, seed=17, score_spread=False)
            be.set_peer_params(pe.peer_params(retain_ns=10 * S, d7=0.8, dtz=0.01))
        eng.set_decay_writeback(k)
        rng = np.random.default_rng(ph)
        ev = [(abi.EV_PENALTY, 0, int(p), T0 + 2 * S, int(rng.integers(3, 30))) for p in range(0, ov.n_pairs, 2)]
        pe.events((eng, ora), ev)
        ck = pe.Clock(eng, ora, now=T0 + 2 * S)
        ck.step(f"T={T} k={k} start {ph}", ph + 1)
        sc = ora.scores()  # 29 * 0.8^4 = 11.9: P7 = -1411; the pairs without a penalty are near 0
        assert (sc < -300).any() and (sc > -100).any()  # either side of every threshold
        for j in range(2):
            ms = pc.messages(n, 24, seed=17 + j)
            ms["validation"][5 + j] = abi.GSX_VALIDATION_REJECT
            cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=T - 1, latency_ms=10, seed=9 + j)
            cfg.now_ns = ck.now
            wo, whop, _ = ora.propagate(ms, cfg, want_results=True)
            go, ghop, _ = eng.propagate(ms, cfg, want_results=True)
            assert go.as_dict() == wo.as_dict(), (ph, j, go.as_dict(), wo.as_dict())
            assert np.array_equal(ghop, whop), (ph, j)
            assert wo.deliveries > 0
            pe.same(eng, ora, f"T={T} k={k} start {ph}: after batch {j}")
            if j == 0:
                ck.step(f"T={T} k={k} start {ph}: between the batches", 1)
        ck.step(f"T={T} k={k} start {ph}: after", 4)

"""Deferred write-back of the decayed counters (REC_EPOCH): the
refresh pass stores fmd / mmd / mfp / imd every k-th refresh (k = 4 by default)
and the stored values lag by up to k - 1 decays in between.  Nothing a caller
sees may change: every case compares the engine with the oracle bit for bit
(scores and every exported state array) after EVERY call, with an event, a
setter, an import, a propagation or a heartbeat landing at each phase of the
cycle, and checks the zero map's invariant at every step.

Shapes: ~180 pairs (two full tiles and a partial one), T = 1, 3, 8 (the
specialised and the general kernel instances), decays of 0.3 against
DecayToZero = 20 so that counters of every size reach zero within a cycle."""
import copy

import numpy as np
import pytest

import gsx
import oracle as orc
import propagation_cases as pc
import randomized as R
from gsx import abi, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND
T0 = pc.T0
N, D = 30, 3
TOPICS = [1, 3, 8]
THRESHOLDS = dict(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300, accept_px_threshold=0,
                  opportunistic_graft_threshold=5)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(eng, ora, where):
    """Scores and every state array bit-identical; the zero map's invariant holds."""
    got, want = eng.scores(), ora.scores()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        f"{where}: scores differ at pairs {np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0][:8]}"
    gs, ws = eng.export_state(), ora.export_state()
    for f in abi.STATE_FIELDS:
        assert np.array_equal(bits(gs[f]), bits(ws[f])), f"{where}: state field {f}"
    if hasattr(eng, "zero_map_violations"):
        assert eng.zero_map_violations() == 0, where
    return gs


def peer_params(dtz=20.0):
    pp = synth.bench_peer_params()
    pp.decay_to_zero = dtz
    pp.retain_score_ns = 3 * S + S // 2  # a retained pair is purged by the 4th refresh after its removal
    return pp


def topic_params(decay=0.3):
    tp = synth.spam_test_topic_params()
    tp.first_message_deliveries_decay = decay
    tp.mesh_message_deliveries_decay = decay
    tp.mesh_failure_penalty_decay = decay
    tp.invalid_message_deliveries_decay = decay
    return tp


def state(ov, T):
    st = synth.synthetic_state(ov, T, T0, p_absent=0.15)
    # a few records with an invalid-delivery counter, so that every counter decays
    imd = st["invalid_message_deliveries"]
    imd[::7] = 60.0 + np.arange(len(imd[::7]))
    in_mesh = (st["rec_flags"] & abi.GSX_REC_IN_MESH) != 0
    st["rec_flags"] = np.where(in_mesh, abi.GSX_REC_IN_MESH | abi.GSX_REC_ACTIVE, 0).astype(np.uint8)
    return st


def backends(T, k=None, extra=0):
    ov = synth.connect_some_overlay(N, d=D)
    assert 128 < ov.n_pairs < 256 and ov.n_pairs % 64 != 0
    st = state(ov, T)
    bes = [gsx.Engine(T) for _ in range(1 + extra)] + [orc.Oracle(T)]
    for be in bes:
        be.set_peer_params(peer_params())
        for t in range(T):
            be.set_topic_params(t, topic_params())
        be.set_thresholds(abi.Thresholds(**THRESHOLDS))
        be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
        be.import_state(st)
        be.set_app_scores(np.zeros(ov.n_pairs))
    if k is not None:
        bes[0].set_decay_writeback(k)
    return ov, st, bes


def events(bes, ev):
    for be in bes:
        be.apply_events(np.array(ev, dtype=abi.event_dtype()))


class Clock:
    """Refreshes both backends one second apart and counts them (the phase of the
    default period is refreshes % 4 after an import)."""

    def __init__(self, *bes):
        self.bes, self.now, self.n = bes, T0, 0

    def refresh(self, where, k=1):
        for i in range(k):
            self.now += S
            for be in self.bes:
                be.refresh(self.now)
            self.n += 1
            st = same(self.bes[0], self.bes[-1], f"{where}: refresh {i + 1} of {k} (#{self.n})")
        return st

    def to_phase(self, ph, where):
        while self.n % 4 != ph:
            self.refresh(where + ": aligning")


KINDS = ["add_new", "remove_negative", "reconnect", "graft", "prune", "first", "mesh", "invalid", "penalty",
         "purge_add"]


@pytest.mark.parametrize("T", TOPICS)
def test_event_at_every_phase(gpu_ok, T):
    """Every event kind injected at every phase of the write-back cycle, then at
    least five more refreshes; engine == oracle after every call."""
    ov, st, (eng, ora) = backends(T)
    ck = Clock(eng, ora)
    E = ov.n_pairs
    rng = np.random.default_rng(5)
    NEG = int(np.float64(-1e6).view(np.int64))
    zero_seen = 0
    for ph in range(4):
        for kind in KINDS:
            where = f"T={T} phase {ph} {kind}"
            ck.to_phase(ph, where)
            cur = eng.export_state()
            pf = cur["pair_flags"]
            fl = cur["rec_flags"].reshape(T, E)
            conn = np.nonzero(pf == (abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED))[0]
            t = int(rng.integers(T))
            now = ck.now
            if kind == "add_new":
                absent = np.nonzero(pf == 0)[0]
                assert len(absent), where
                ev = [(abi.EV_ADD_PEER, 0, int(absent[0]), now, 0)]
            elif kind in ("remove_negative", "reconnect", "purge_add"):
                p = int(rng.choice(conn))
                ev = [(abi.EV_APP_SCORE, 0, p, now, NEG), (abi.EV_REMOVE_PEER, 0, p, now, 0)]
            elif kind in ("prune", "mesh"):
                cand = conn[(fl[t, conn] & abi.GSX_REC_IN_MESH) != 0]
                assert len(cand), where
                ev = [(abi.EV_PRUNE if kind == "prune" else abi.EV_MESH_DELIVERY, t, int(rng.choice(cand)), now, 0)]
            else:
                code = dict(graft=abi.EV_GRAFT, first=abi.EV_FIRST_DELIVERY, invalid=abi.EV_INVALID_DELIVERY,
                            penalty=abi.EV_PENALTY)[kind]
                ev = [(code, t, int(rng.choice(conn)), now, 3 if kind == "penalty" else 0)]
            events((eng, ora), ev)
            out = same(eng, ora, where + ": after the event")
            if kind in ("remove_negative", "reconnect", "purge_add"):
                assert out["pair_flags"][p] == abi.GSX_PAIR_PRESENT, where  # retained
            if kind == "reconnect":  # two refreshes later, so at another phase than the removal
                ck.refresh(where + ": retained", 2)
                events((eng, ora), [(abi.EV_ADD_PEER, 0, p, ck.now, 0)])
                out = same(eng, ora, where + ": after the reconnect")
                assert out["pair_flags"][p] == abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
            if kind == "purge_add":  # retained for 3.5 s: the 4th refresh purges it, then AddPeer mid-phase
                ck.refresh(where + ": until the purge", 4)
                assert eng.export_state()["pair_flags"][p] == 0, where
                ck.refresh(where + ": purged", 1)
                events((eng, ora), [(abi.EV_APP_SCORE, 0, p, ck.now, 0), (abi.EV_ADD_PEER, 0, p, ck.now, 0)])
                same(eng, ora, where + ": AddPeer after the purge")
            out = ck.refresh(where, 5)
            zero_seen += int(np.count_nonzero(out["first_message_deliveries"] == 0))
    assert zero_seen > 0  # counters did reach DecayToZero


@pytest.mark.parametrize("T", TOPICS)
def test_param_setters_mid_phase(gpu_ok, T):
    """SetTopicScoreParams (other decays, lower caps: the recap runs) and the peer
    parameters (another DecayToZero) while decays are pending."""
    ov, st, (eng, ora) = backends(T)
    ck = Clock(eng, ora)
    for ph in (1, 2, 3):
        ck.refresh(f"setters, start {ph}", ph)
        tp = topic_params(0.6 + 0.1 * ph)
        tp.first_message_deliveries_cap = 40.0 / ph
        tp.mesh_message_deliveries_cap = 30.0 / ph
        for be in (eng, ora):
            be.set_topic_params(T - 1, tp)
        same(eng, ora, f"set_topic_params after {ph}")
        ck.refresh(f"after set_topic_params {ph}", ph)
        for be in (eng, ora):
            be.set_peer_params(peer_params(dtz=5.0 / ph))
        same(eng, ora, f"set_peer_params after {ph}")
        ck.refresh(f"after set_peer_params {ph}", 5)
        # fresh counters for the next round
        events((eng, ora), [(abi.EV_FIRST_DELIVERY, T - 1, p, ck.now, 0) for p in range(0, ov.n_pairs, 3)] * 30)
        same(eng, ora, f"deliveries {ph}")


@pytest.mark.parametrize("T", TOPICS)
def test_export_import_mid_phase(gpu_ok, T):
    """The exported state of an engine with pending decays, imported into a second
    engine: both continue with the oracle."""
    for ph in (1, 2, 3):
        ov, st, (eng, eng2, ora) = backends(T, extra=1)
        ck = Clock(eng, ora)
        ck.refresh(f"export at {ph}", ph)
        events((eng, ora), [(abi.EV_INVALID_DELIVERY, T - 1, 70, ck.now, 0), (abi.EV_PRUNE, 0, 3, ck.now, 0)])
        ck.refresh(f"export at {ph}", 1)
        eng2.import_state(eng.export_state())
        same(eng2, ora, f"imported at {ph}")
        same(eng, ora, f"exporter at {ph}")
        for i in range(5):
            ck.now += S
            for be in (eng, eng2, ora):
                be.refresh(ck.now)
            same(eng, ora, f"exporter, {ph} + {i}")
            same(eng2, ora, f"importer, {ph} + {i}")
            events((eng, eng2, ora), [(abi.EV_FIRST_DELIVERY, 0, 5 + i, ck.now, 0)])


@pytest.mark.parametrize("T,mode", [(1, "per-hop"), (3, "per-hop"), (1, "late"), (3, "late")])
def test_propagate_credits_mid_phase(gpu_ok, T, mode):
    """One credited gossipsub batch with decays pending: per-hop accounting folds in
    k_prop_count (T = 1: its fused fold; T = 3: fold_pair); `late` defers the
    folds, which settle_scores / the next refresh folds."""
    ov = pc.overlay(120, D, seed=17)
    for ph in (1, 2, 3):
        eng, ora = gsx.Engine(T), orc.Oracle(T)
        if mode == "late":
            eng.set_prop_tracking(False)
        for be in (eng, ora):
            pc.setup(be, ov, T, seed=17)
            pp = synth.bench_peer_params()
            pp.decay_to_zero = 0.3
            be.set_peer_params(pp)  # (restarts the cycle: the phase below is the refreshes since)
        ck = Clock(eng, ora)
        ck.now = T0 + 2 * S
        for k in range(2):
            ms = pc.messages(120, 24, seed=17 + k)
            ms["validation"][5 + k] = abi.GSX_VALIDATION_REJECT
            cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=T - 1, latency_ms=0 if mode == "late" else 10, seed=9 + k)
            cfg.now_ns = ck.now
            want = ora.propagate(ms, cfg)[0].as_dict()
            got = eng.propagate(ms, cfg)[0].as_dict()
            assert got == want, (ph, k)
            ck.refresh(f"{mode} T={T} start {ph} batch {k}", ph)  # (folds a deferred batch)
        cfg.now_ns = ck.now
        assert eng.propagate(ms, cfg)[0].as_dict() == ora.propagate(ms, cfg)[0].as_dict()
        eng.settle_scores()
        same(eng, ora, f"{mode} T={T} start {ph}: after the batch")
        ck.refresh(f"{mode} T={T} start {ph}: after", 5)


@pytest.mark.parametrize("T", TOPICS)
def test_heartbeat_prune_mid_phase(gpu_ok, T):
    """A heartbeat prunes a negative-score mesh peer whose active record is under the
    P3 threshold while decays are pending (the heartbeat's own prune)."""
    for ph in (1, 2, 3):
        ov, st, (eng, ora) = backends(T)
        E = ov.n_pairs
        mmd = st["mesh_message_deliveries"].reshape(T, E)
        ok = ((st["rec_flags"].reshape(T, E) & abi.GSX_REC_ACTIVE) != 0) & (mmd < 100.0)
        ok[:, st["pair_flags"] == 0] = False
        t, p = (int(x) for x in np.argwhere(ok)[0])
        app = np.zeros(E)
        app[p] = -1000.0
        for be in (eng, ora):
            be.set_app_scores(app)
        ck = Clock(eng, ora)
        ck.refresh(f"heartbeat at {ph}", ph)
        go = eng.heartbeat(1, ck.now + S // 2, 5).as_dict()
        wo = ora.heartbeat(1, ck.now + S // 2, 5).as_dict()
        assert go == wo and go["prunes"] > 0, ph
        same(eng, ora, f"heartbeat at {ph}: after the round")
        ck.refresh(f"heartbeat at {ph}: after", 5)


def test_random_calls_same_for_every_period(gpu_ok):
    """The same random call sequence under write-back periods 1, 2 and 4 (and the
    oracle): identical scores and exports at every check.  Every refresh of the
    sequence is run three times over, so the checks fall on every phase."""
    T = 3
    ov = R.small_overlay(60, 3, 7, 10)
    ops = []
    for op in R.make_ops(ov, T, 7, n_steps=300):
        if op[0] == "refresh":
            for j in range(3):
                ops += [("refresh", op[1] + j * abi.MILLISECOND), ("check",)]
        elif op[0] != "check":
            ops.append(op)
    runs = []
    for k in (1, 2, 4):
        e = gsx.Engine(T)
        e.set_decay_writeback(k)
        runs.append(R.replay(e, ov, T, copy.deepcopy(ops)))
        assert e.zero_map_violations() == 0
    want = R.replay(orc.Oracle(T), ov, T, copy.deepcopy(ops))
    for got in runs:
        assert len(got) == len(want) > 12
        for i, ((gs, gst, gn), (ws, wst, wn)) in enumerate(zip(got, want)):
            assert gn == wn, i
            assert np.array_equal(gs.view(np.uint64), ws.view(np.uint64)), f"check {i}: scores"
            for f in abi.STATE_FIELDS:
                assert np.array_equal(bits(gst[f]), bits(wst[f])), f"check {i}: state field {f}"


def test_setter_rejects_other_periods(gpu_ok):
    e = gsx.Engine(1)
    for k in (0, 3, 8):
        with pytest.raises(Exception):
            e.set_decay_writeback(k)

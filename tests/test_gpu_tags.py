"""The tag tracer on the device (gsx_set_tag_params .. gsx_conn_trim) against
the line-by-line model of tag_tracer.go (tests/tag_model.py), the values the
reference's own tests assert (tests/golden/tag_kat.json), and, for
gsx_tag_fold_prop, the model fed event by event from the ORACLE's propagation
results."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch  # (initialised before any engine: the device-pointer outputs of the trim test)

import gsx
import oracle as orc
import propagation_cases as pc
import tag_model as tm
from gsx import abi, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND
T0 = pc.T0
KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tag_kat.json")))
REASONS = {v: k for k, v in abi.REJECT_REASONS.items()}
BOTH = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED


def tag_params(bump=1, decay=1, cap=15):
    return abi.TagParams(bump=bump, decay_amount=decay, cap=cap, decay_interval_ns=600 * S), tm.Params(bump, decay, cap)


def plain_engine(T, row_ptr, col, ef=None, ips=None, present=None):
    e = gsx.Engine(T, device=0)
    e.set_peer_params(synth.bench_peer_params())
    for t in range(T):
        e.set_topic_params(t, synth.spam_test_topic_params())
    e.load_overlay(row_ptr, col, ef, ips)
    present = np.arange(e.n_pairs) if present is None else present
    if len(present):
        e.apply_events(np.array([(abi.EV_ADD_PEER, 0, int(p), T0, 0) for p in present], dtype=abi.event_dtype()))
    return e


class Mirror:
    """Drives the engine's tag tracer and one model tracer per observer with the same calls."""

    def __init__(self, eng, row_ptr, col, ef, T, tp, mp, present=None):
        self.e, self.T, self.col = eng, T, np.asarray(col)
        self.row_ptr = np.asarray(row_ptr)
        self.n, self.E = len(row_ptr) - 1, len(col)
        self.obs = np.repeat(np.arange(self.n), np.diff(row_ptr))
        self.ef = np.zeros(self.E, dtype=np.uint8) if ef is None else np.asarray(ef)
        self.models = [tm.ModelBackend(mp) for _ in range(self.n)]
        self.joined = np.full(self.n, (1 << T) - 1, dtype=object)
        self.present = np.zeros(self.E, dtype=bool)
        for u, m in enumerate(self.models):
            b, en = self.row_ptr[u], self.row_ptr[u + 1]
            m.set_direct(int(v) for v, f in zip(self.col[b:en], self.ef[b:en]) if f & abi.GSX_EDGE_DIRECT)
            for t in range(T):
                m.join(t)
        for p in (range(self.E) if present is None else present):
            self.add_peer(int(p))
        eng.set_tag_params(tp)

    def add_peer(self, p):
        self.present[p] = True
        self.models[self.obs[p]].add_peer(int(self.col[p]))

    def set_joined(self, u, mask):
        for t in range(self.T):
            was, now = (self.joined[u] >> t) & 1, (mask >> t) & 1
            if was and not now:
                self.models[u].leave(t)
            if now and not was:
                self.models[u].join(t)
        self.joined[u] = mask

    def sync_mesh(self):
        """The mesh protections are the scorer's in-mesh bits, which Join / Leave move on the
        device (their equality with the oracle's is test_gpu_membership's subject)."""
        rf = self.e.export_state()["rec_flags"].reshape(self.T, self.E)
        for p in range(self.E):
            m, v = self.models[self.obs[p]], int(self.col[p])
            for t in range(self.T):
                (m.graft if rf[t, p] & abi.GSX_REC_IN_MESH else m.prune)(v, t)

    def expect(self):
        tags = np.zeros((self.T, self.E), dtype=np.uint8)
        prot = np.zeros(self.E, dtype=np.uint8)
        for p in range(self.E):
            m, v = self.models[self.obs[p]], int(self.col[p])
            for t in range(self.T):
                tags[t, p] = m.value(v, t)
            if self.present[p]:
                prot[p] = (abi.GSX_CONN_DIRECT if m.direct_protected(v) else 0) | \
                          (abi.GSX_CONN_MESH if m.mesh_protected(v) else 0)
        val = np.where(self.present, tags.sum(axis=0, dtype=np.uint32), 0).astype(np.uint32)
        return tags, val, prot

    def check(self, what=""):
        tags, val, prot = self.expect()
        got = self.e.tag_export()
        assert np.array_equal(got, tags), (what, np.argwhere(got != tags)[:5])
        v, p = self.e.conn_values()
        assert np.array_equal(v, val), what
        assert np.array_equal(p, prot), (what, np.nonzero(p != prot)[0][:5])
        assert self.e.tag_num_pending() == sum(len(m.tt.near_first) for m in self.models), what
        return got


# ---- the reference's four tests through the ABI -------------------------------------------
class EngineBackend:
    """tag_model's backend interface over observer 0 of a 4-node star (peers 1, 2, 3), 2 topics."""

    def __init__(self):
        self.direct = []
        self.e = None
        self.joined = 0
        self.pending = []

    def _engine(self):
        if self.e is None:
            row_ptr = np.array([0, 3, 4, 5, 6], dtype=np.int64)
            col = np.array([1, 2, 3, 0, 0, 0], dtype=np.int32)
            ef = np.full(6, abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8)
            for p in self.direct:
                ef[p - 1] |= abi.GSX_EDGE_DIRECT
            self.e = plain_engine(2, row_ptr, col, ef, present=[])
            p = KAT["params"]
            self.e.set_tag_params(abi.TagParams(bump=p["bump"], decay_amount=p["decay_amount"], cap=p["cap"],
                                                decay_interval_ns=p["decay_interval_ns"]))
            self.e.set_subscriptions(np.array([self.joined, 3, 3, 3], dtype=np.uint64))
        return self.e

    def set_direct(self, peers):
        assert self.e is None
        self.direct = list(peers)

    def join(self, topic):
        self.joined |= 1 << topic
        if self.e is not None:
            self.e.set_subscriptions(np.array([self.joined, 3, 3, 3], dtype=np.uint64))

    def leave(self, topic):
        self.joined &= ~(1 << topic)
        self._engine().set_subscriptions(np.array([self.joined, 3, 3, 3], dtype=np.uint64))

    def _ev(self, kind, p, topic):
        self._engine().apply_events(np.array([(kind, topic, p - 1, T0, 0)], dtype=abi.event_dtype()))

    def add_peer(self, p):
        self._ev(abi.EV_ADD_PEER, p, 0)

    def graft(self, p, topic):
        self._ev(abi.EV_ADD_PEER, p, 0)
        self._ev(abi.EV_GRAFT, p, topic)

    def prune(self, p, topic):
        self._ev(abi.EV_PRUNE, p, topic)

    def validate(self, p, msg, topic):
        self._engine().tag_trace_validate(p - 1, msg, topic, T0)

    def duplicate(self, p, msg, topic):
        self._engine().tag_trace_duplicate(p - 1, msg, topic, T0)

    def deliver(self, p, msg, topic):
        self._engine().tag_trace_deliver(p - 1, msg, topic, T0)

    def decay(self, steps):
        self._engine().tag_decay(steps)

    def value(self, p, topic):
        return int(self._engine().tag_export()[topic, p - 1])

    def mesh_protected(self, p):
        return bool(self._engine().conn_values()[1][p - 1] & abi.GSX_CONN_MESH)

    def direct_protected(self, p):
        return bool(self._engine().conn_values()[1][p - 1] & abi.GSX_CONN_DIRECT)


def test_the_reference_tests_through_the_abi(gpu_ok):
    made = []

    def make():
        made.append(EngineBackend())
        return made[-1]

    got = tm.run_kat(make, KAT)
    for be in made:
        be.e.close()
    for name, g in got.items():
        assert g == KAT[name]["expect"], name


# ---- seeded random call sequences against the model ----------------------------------------
@pytest.mark.parametrize("T", [1, 3, 9, 64])
def test_random_call_sequences(gpu_ok, T):
    ov = pc.overlay(40, 4, seed=11 + T, direct_frac=0.1)
    E, n = ov.n_pairs, ov.n
    rng = np.random.default_rng(100 + T)
    present = np.nonzero(rng.random(E) < 0.9)[0]
    e = plain_engine(T, ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips, present)
    e.set_gossipsub_params(orc.default_gossipsub_params())
    tp, mp = tag_params(cap=3)
    mr = Mirror(e, ov.row_ptr, ov.col, ov.edge_flags, T, tp, mp, present)
    mr.check("fresh")
    kinds = ["trace"] * 6 + ["events"] * 3 + ["decay", "leave", "join", "subs", "mesh", "mesh"]
    saw_cap = saw_zero_again = saw_drop = False
    for step in range(90):
        k = kinds[int(rng.integers(len(kinds)))]
        if k == "trace":
            for _ in range(int(rng.integers(1, 12))):
                p, t, msg = int(rng.integers(E)), int(rng.integers(T)), int(rng.integers(6))
                m, v = mr.models[mr.obs[p]], int(ov.col[p])
                c = int(rng.integers(5))
                if c == 0:
                    e.tag_trace_validate(p, msg, t, T0)
                    m.validate(v, msg, t)
                elif c in (1, 2):
                    e.tag_trace_duplicate(p, msg, t, T0)
                    m.duplicate(v, msg, t)
                elif c == 3:
                    saw_drop |= not ((mr.joined[mr.obs[p]] >> t) & 1)
                    e.tag_trace_deliver(p, msg, t, T0)
                    m.deliver(v, msg, t)
                else:
                    r = int(rng.choice([2, 6, 7, 8, 9]))
                    e.tag_trace_reject(p, msg, t, r, T0)
                    m.tt.reject_message(msg, REASONS[r])
        elif k == "events":
            ev = [(int(rng.integers(E)) if rng.random() < 0.7 else 0, int(rng.integers(T)), int(rng.integers(5)))
                  for _ in range(int(rng.integers(1, 25)))]
            e.tag_events(np.array(ev, dtype=abi.tag_event_dtype()))
            for p, t, c in ev:
                for _ in range(c):
                    mr.models[mr.obs[p]].tt.bump_delivery_tag(int(ov.col[p]), t)
        elif k == "decay":
            steps = int(rng.choice([1, 1, 2, 3, 300, int(rng.integers(1, 301))]))
            before = e.tag_export()
            e.tag_decay(steps)
            for m in mr.models:
                m.decay(min(steps, 4))  # (cap 3: four steps empty every tag)
            saw_zero_again |= bool(before.any()) and steps >= 3
        elif k in ("leave", "join"):
            nodes = rng.choice(n, 5, replace=False).astype(np.uint32)
            topics = rng.integers(0, T, 5).astype(np.uint32)
            if k == "leave":
                e.leave(nodes, topics, T0 + step * S)
            else:
                e.join(nodes, topics, T0 + step * S, 5 + step)
            for u, t in zip(nodes, topics):
                mr.set_joined(int(u), (mr.joined[u] & ~(1 << int(t))) if k == "leave" else (mr.joined[u] | (1 << int(t))))
            mr.sync_mesh()
        elif k == "subs":
            masks = [((int(rng.integers(1 << 32)) << 32) | int(rng.integers(1 << 32))) & ((1 << T) - 1) for _ in range(n)]
            e.set_subscriptions(np.array(masks, dtype=np.uint64))
            for u in range(n):
                mr.set_joined(u, masks[u])
        else:
            ps = rng.choice(present, 6)
            ts = rng.integers(0, T, 6)
            graft = rng.random(6) < 0.6
            e.apply_events(np.array([(abi.EV_GRAFT if g else abi.EV_PRUNE, int(t), int(p), T0, 0)
                                     for p, t, g in zip(ps, ts, graft)], dtype=abi.event_dtype()))
            for p, t, g in zip(ps, ts, graft):
                m = mr.models[mr.obs[p]]
                (m.graft if g else m.prune)(int(ov.col[p]), int(t))
        got = mr.check((step, k))
        saw_cap |= bool((got == 3).any())
        # the invariant: no tag at an unjoined observer
        for t in range(T):
            unj = np.array([not ((mr.joined[u] >> t) & 1) for u in mr.obs])
            assert not got[t][unj].any(), (step, k, t)
    assert saw_cap and saw_zero_again and saw_drop
    e.close()


def test_decay_of_every_byte_value(gpu_ok):
    """Tags 0 .. 255 next to each other in one 16-byte word, every amount that matters."""
    ov = pc.overlay(100, 6, seed=2)
    e = plain_engine(3, ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips, present=[])
    E = e.n_pairs
    rng = np.random.default_rng(2)
    for amount, steps in ((1, 1), (1, 127), (1, 128), (7, 18), (1, 254), (1, 255), (3, 100), (1, 10 ** 12)):
        e.set_tag_params(abi.TagParams(bump=1, decay_amount=amount, cap=255, decay_interval_ns=S))
        want = np.zeros((3, E), dtype=np.int64)
        want[0, :256] = np.arange(256)
        want[1] = rng.integers(0, 256, E)
        want[2, ::3] = 255
        ev = [(p, t, int(want[t, p])) for t in range(3) for p in range(E) if want[t, p]]
        e.tag_events(np.array(ev, dtype=abi.tag_event_dtype()))
        assert E >= 256 and np.array_equal(e.tag_export(), want)
        e.tag_decay(steps)
        assert np.array_equal(e.tag_export(), np.maximum(want - amount * steps, 0)), (amount, steps)
    e.close()


# ---- gsx_tag_fold_prop ---------------------------------------------------------------------
N_FOLD = 200
FOLD_T = 3
FOLD_TOPIC = 1


@pytest.fixture(scope="module", params=[abi.GSX_ROUTER_GOSSIPSUB, abi.GSX_ROUTER_FLOODSUB], ids=["gossipsub", "floodsub"])
def fold_world(request, gpu_ok):
    ov = pc.overlay(N_FOLD, 10, seed=41, mix_protocols=True)
    eng, ora = gsx.Engine(FOLD_T, device=0), orc.Oracle(FOLD_T)
    rng = np.random.default_rng(6)
    joined = np.full(N_FOLD, (1 << FOLD_T) - 1, dtype=np.uint64)
    joined[rng.random(N_FOLD) < 0.1] &= np.uint64(~(1 << FOLD_TOPIC) & 7)  # some observers have not joined the topic
    for be in (eng, ora):
        pc.setup(be, ov, FOLD_T, seed=41)
        be.set_subscriptions(joined)
    ora.set_dup_tracking(True)
    yield request.param, ov, eng, ora, joined
    eng.close()


def model_fold(ov, joined, mp, ms, hop, frm, dup, delayed, topic):
    """The tracer calls of the batch per (node, message) from the oracle's results: Validate, the
    duplicates that came in the first copy's hop (while it was validating, if validation takes
    time), Deliver / Reject, the later duplicates.  -> (tags [E], near-first copies, later copies)"""
    E, n = ov.n_pairs, ov.n
    obs, col = ov.pair_observer(), np.asarray(ov.col)
    pair_of = {(int(u), int(v)): p for p, (u, v) in enumerate(zip(obs, col))}
    dups = {}
    for p in np.nonzero(dup.any(axis=1))[0]:
        for w in range(dup.shape[1]):
            x = int(dup[p, w])
            while x:
                b = (x & -x).bit_length() - 1
                x &= x - 1
                dups.setdefault((int(obs[p]), w * 64 + b), []).append(int(p))
    models = [tm.ModelBackend(mp) for _ in range(n)]
    for u, m in enumerate(models):
        for t in range(FOLD_T):
            if (int(joined[u]) >> t) & 1:
                m.join(t)
    n_near = n_late = 0
    for k in range(len(ms)):
        val = int(ms["validation"][k])
        for u in np.nonzero(frm[k] >= 0)[0]:
            u = int(u)
            m, v = models[u], int(frm[k, u])
            d = dups.get((u, k), [])
            same = [p for p in d if int(hop[k, col[p]]) + 1 == int(hop[k, u])]
            late = [p for p in d if p not in same]
            if not delayed:  # inline validation: every duplicate comes after the outcome
                same, late = [], d
            m.validate(v, k, topic)
            for p in same:
                m.duplicate(int(col[p]), k, topic)
            if val == abi.GSX_VALIDATION_ACCEPT:
                m.deliver(v, k, topic)
                n_near += len(same)
                n_late += len(late)
            else:
                m.tt.reject_message(k, {abi.GSX_VALIDATION_REJECT: tm.REJECT_FAILED, abi.GSX_VALIDATION_IGNORE: tm.REJECT_IGNORED,
                                        abi.GSX_VALIDATION_THROTTLE: tm.REJECT_THROTTLED}[val])
            for p in late:
                m.duplicate(int(col[p]), k, topic)
        assert not any(mm.tt.near_first for mm in models)
    tags = np.array([models[obs[p]].value(int(col[p]), topic) for p in range(E)], dtype=np.uint8)
    return tags, n_near, n_late


@pytest.mark.parametrize("m", [1, 64, 65, 200])
def test_fold_prop_equals_the_model_fed_from_the_oracle(fold_world, m):
    router, ov, eng, ora, joined = fold_world
    E = ov.n_pairs
    ms = pc.messages(N_FOLD, m, seed=m, invalid=0.3 if m > 1 else 0.0)
    if m > 1:  # all four outcomes
        ms["validation"][1:4] = [abi.GSX_VALIDATION_REJECT, abi.GSX_VALIDATION_IGNORE, abi.GSX_VALIDATION_THROTTLE]
    while not (int(joined[ms["source"][0]]) >> FOLD_TOPIC) & 1:
        ms["source"][0] = (ms["source"][0] + 1) % N_FOLD  # (a joined publisher, so that m = 1 travels)
    tp, mp = tag_params(cap=255)
    got = {}
    for delay_ms in (2.0, 0.0):
        cfg = pc.config(router, topic=FOLD_TOPIC, credit=0, delay_ms=delay_ms)
        _, hop, frm = ora.propagate(ms, cfg, want_results=True)
        dup = ora.prop_duplicates(m)
        eng.propagate(ms, cfg)
        eng.set_tag_params(tp)
        eng.tag_fold_prop()
        want, n_near, n_late = model_fold(ov, joined, mp, ms, hop, frm, dup, delay_ms > 0, FOLD_TOPIC)
        x = eng.tag_export()
        assert not x[0].any() and not x[2].any()
        assert np.array_equal(x[FOLD_TOPIC], want), (delay_ms, np.nonzero(x[FOLD_TOPIC] != want)[0][:5])
        assert want.any()
        if delay_ms > 0:
            assert n_near >= 1 and n_late >= 1, (n_near, n_late)  # both kinds of duplicate are in the batch
        eng.tag_fold_prop()  # a second call folds the same batch again
        assert np.array_equal(eng.tag_export()[FOLD_TOPIC], np.minimum(2 * want.astype(np.int64), 255))
        got[delay_ms] = want
    # the near-first path is not vacuous: without a validation delay some tag is strictly smaller
    assert (got[0.0] <= got[2.0]).all() and (got[0.0] < got[2.0]).any()
    unj = np.array([not ((int(joined[u]) >> FOLD_TOPIC) & 1) for u in ov.pair_observer()])
    assert unj.any() and not got[2.0][unj].any()


def test_fold_prop_saturates_at_the_cap(fold_world):
    router, ov, eng, ora, joined = fold_world
    ms = pc.messages(N_FOLD, 130, seed=8)
    cfg = pc.config(router, topic=FOLD_TOPIC, credit=0, delay_ms=2.0)
    _, hop, frm = ora.propagate(ms, cfg, want_results=True)
    dup = ora.prop_duplicates(130)
    eng.propagate(ms, cfg)
    tp, mp = tag_params(bump=2, cap=5)
    eng.set_tag_params(tp)
    eng.tag_fold_prop()
    want, _, _ = model_fold(ov, joined, mp, ms, hop, frm, dup, True, FOLD_TOPIC)
    assert np.array_equal(eng.tag_export()[FOLD_TOPIC], want)
    assert (want == 5).any() and (want == 2).any() and (want == 4).any()


# ---- gsx_conn_trim ---------------------------------------------------------------------------
DEGS = [0, 1, 63, 64, 65, 300, 5000]


def star_overlay():
    """Hub i has DEGS[i] leaves (the first of the 5000), so the leaves' rows hold 0 .. 6 hubs."""
    H, L = len(DEGS), max(DEGS)
    rows = [np.arange(H, H + d) for d in DEGS] + [np.array([i for i, d in enumerate(DEGS) if d > j]) for j in range(L)]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return row_ptr, np.concatenate(rows).astype(np.int32)


def test_conn_trim_equals_the_model(gpu_ok):
    row_ptr, col = star_overlay()
    n, E, T = len(row_ptr) - 1, len(col), 2
    rng = np.random.default_rng(17)
    ef = np.full(E, abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8)
    ef[rng.random(E) < 0.05] |= abi.GSX_EDGE_DIRECT
    r = rng.random(E)
    absent, retained = r < 0.1, (r >= 0.1) & (r < 0.2)
    e = plain_engine(T, row_ptr, col, ef, present=np.nonzero(~absent)[0])
    tp, mp = tag_params(cap=3)
    mr = Mirror(e, row_ptr, col, ef, T, tp, mp, np.nonzero(~absent)[0])
    grafted = np.nonzero(~absent & ~retained & (rng.random(E) < 0.1))[0]
    e.apply_events(np.array([(abi.EV_GRAFT, int(p) % T, int(p), T0, 0) for p in grafted], dtype=abi.event_dtype()))
    for p in grafted:
        mr.models[mr.obs[p]].graft(int(col[p]), int(p) % T)
    e.apply_events(np.array([(abi.EV_REMOVE_PEER, 0, int(p), T0 + S, 0) for p in np.nonzero(retained)[0]],
                            dtype=abi.event_dtype()))
    ev = [(p, int(rng.integers(T)), int(rng.integers(1, 4))) for p in np.nonzero(rng.random(E) < 0.7)[0]]
    e.tag_events(np.array(ev, dtype=abi.tag_event_dtype()))
    for p, t, c in ev:
        for _ in range(c):
            mr.models[mr.obs[p]].tt.bump_delivery_tag(int(col[p]), t)
    mr.check("trim world")
    pf = e.export_state()["pair_flags"]
    conn = (pf & BOTH) == BOTH
    assert not (pf[absent] & abi.GSX_PAIR_PRESENT).any()
    assert ((pf[retained] & BOTH) == abi.GSX_PAIR_PRESENT).all() and conn[~absent & ~retained].all()
    _, val, prot = mr.expect()
    saw = set()
    for low in (0, 2, 40, 64, 150, 4500, 5000, 6000):
        want = np.zeros(E, dtype=np.uint8)
        want_n = np.zeros(n, dtype=np.uint32)
        for u in range(n):
            b, en = int(row_ptr[u]), int(row_ptr[u + 1])
            idx = b + np.nonzero(conn[b:en])[0]
            closed = mr.models[u].cm.trim([int(col[p]) for p in idx], low)
            want[idx[closed]] = 1
            want_n[u] = len(closed)
            if closed and u < len(DEGS):
                cut = max(val[idx[closed]])
                keep = np.setdiff1d(idx, idx[closed])
                if ((val[keep] == cut) & (prot[keep] == 0)).any():
                    saw.add("tie across the cut")
                if ((prot[idx] != 0) & (val[idx] < cut)).any() and ((prot[idx] != 0) & (val[idx] > cut)).any():
                    saw.add("protected on both sides")
        ct = e.conn_trim(low)
        assert np.array_equal(ct.trim, want), (low, np.nonzero(ct.trim != want)[0][:5])
        assert np.array_equal(ct.node_trimmed, want_n), low
        assert not (want[~conn]).any()
        u = len(DEGS) - 2
        assert np.array_equal(ct.trimmed(u), np.nonzero(want)[0][(np.nonzero(want)[0] >= row_ptr[u]) & (np.nonzero(want)[0] < row_ptr[u + 1])])
        assert len(ct.kept(u)) + len(ct.trimmed(u)) == conn[row_ptr[u]:row_ptr[u + 1]].sum()
        # device outputs
        d_trim = torch.full((E,), 7, dtype=torch.uint8, device="cuda:0")
        d_n = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
        assert e.conn_trim(low, trim_ptr=d_trim, node_trimmed_ptr=d_n) is None
        e.sync()
        torch.cuda.synchronize()
        assert np.array_equal(d_trim.cpu().numpy(), want) and np.array_equal(d_n.cpu().numpy().astype(np.uint32), want_n)
    assert saw == {"tie across the cut", "protected on both sides"}
    d_val = torch.zeros(E, dtype=torch.int32, device="cuda:0")
    d_prot = torch.zeros(E, dtype=torch.uint8, device="cuda:0")
    e.conn_values(value_ptr=d_val, protect_ptr=d_prot)
    e.sync()
    torch.cuda.synchronize()
    assert np.array_equal(d_val.cpu().numpy().astype(np.uint32), val) and np.array_equal(d_prot.cpu().numpy(), prot)
    e.close()


# ---- TestGossipsubConnTagMessageDeliveries, restated -------------------------------------------
def test_sybil_squatters_are_trimmed_and_honest_peers_kept(gpu_ok):
    n_honest, n_squat = 5, 10
    n = n_honest + n_squat
    row_ptr = np.arange(0, n * (n - 1) + 1, n - 1, dtype=np.int64)
    col = np.concatenate([np.setdiff1d(np.arange(n), [u]) for u in range(n)]).astype(np.int32)
    ef = np.full(len(col), abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8)
    e = plain_engine(1, row_ptr, col, ef)
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                    accept_px_threshold=0, opportunistic_graft_threshold=0))
    e.set_app_scores(np.zeros(e.n_pairs))
    gp = orc.default_gossipsub_params()
    gp.d = gp.d_lo = gp.d_hi = 3
    gp.d_score = gp.d_out = 0
    e.set_gossipsub_params(gp)
    joined = np.zeros(n, dtype=np.uint64)
    joined[:n_honest] = 1  # the squatters connect and subscribe to nothing
    e.set_subscriptions(joined)
    e.refresh(T0 + S)
    e.heartbeat(1, T0 + 2 * S, 3)
    e.set_tag_params(abi.TagParams(bump=1, decay_amount=1, cap=50, decay_interval_ns=600 * S))
    for u in range(n_honest):
        ms = np.zeros(100, dtype=abi.msg_dtype())
        ms["source"], ms["msg_id"] = u, 1000 * u + np.arange(100)
        e.propagate(ms, pc.config(abi.GSX_ROUTER_GOSSIPSUB, flood_publish=1, credit=0, delay_ms=1.0))
        e.tag_fold_prop()
    e.tag_decay(1)
    tags = e.tag_export()[0]
    obs = np.repeat(np.arange(n), n - 1)
    hh = (obs < n_honest) & (col < n_honest)
    assert (tags[hh] > 0).all()
    assert not tags[col >= n_honest].any()
    ct = e.conn_trim(5)
    for u in range(n_honest):
        kept = col[ct.kept(u)]
        assert set(range(n_honest)) - {u} <= set(kept.tolist())
        assert (kept >= n_honest).sum() <= 5
        assert len(kept) == 5
    e.close()


# ---- lifetime and refusals ---------------------------------------------------------------------
def test_refusals_and_lifetime(gpu_ok):
    lib = gsx.load_library()
    ov = pc.overlay(40, 4, seed=3)
    e = gsx.Engine(2, device=0)
    pc.setup(e, ov, 2, seed=3)
    E = e.n_pairs
    buf = np.zeros(2 * E + 64, dtype=np.uint32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    one = np.array([(0, 0, 1)], dtype=abi.tag_event_dtype())
    n64 = C.c_uint64()

    def calls():
        return [lib.gsx_tag_trace_validate(e.h, 0, 1, 0, T0), lib.gsx_tag_trace_duplicate(e.h, 0, 1, 0, T0),
                lib.gsx_tag_trace_deliver(e.h, 0, 1, 0, T0), lib.gsx_tag_trace_reject(e.h, 0, 1, 0, 8, T0),
                lib.gsx_tag_num_pending(e.h, C.byref(n64)), lib.gsx_tag_events(e.h, one.ctypes.data_as(C.c_void_p), 1),
                lib.gsx_tag_decay(e.h, 1), lib.gsx_tag_fold_prop(e.h), lib.gsx_tag_export(e.h, ptr),
                lib.gsx_conn_values(e.h, ptr, None), lib.gsx_conn_trim(e.h, 1, ptr, None)]

    assert calls() == [abi.GSX_ESTATE] * 11  # no tracer yet
    tp = abi.TagParams()
    assert lib.gsx_default_tag_params(C.byref(tp)) == 0
    assert (tp.bump, tp.decay_amount, tp.cap, tp.decay_interval_ns) == (1, 1, 15, 600 * S)
    for bad in ((0, 1, 15), (16, 1, 15), (1, 1, 256), (1, 0, 15), (1, 1, 0)):
        assert lib.gsx_set_tag_params(e.h, C.byref(abi.TagParams(bump=bad[0], decay_amount=bad[1], cap=bad[2]))) == abi.GSX_EINVAL
    assert lib.gsx_set_tag_params(None, C.byref(tp)) == abi.GSX_EINVAL
    fresh = gsx.Engine(1, device=0)
    assert lib.gsx_set_tag_params(fresh.h, C.byref(tp)) == abi.GSX_ESTATE  # no overlay
    fresh.close()
    e.set_tag_params(tp)
    assert lib.gsx_tag_fold_prop(e.h) == abi.GSX_ESTATE  # no propagation yet
    for pair, topic in ((E, 0), (0, 2)):
        one[0] = (pair, topic, 1)
        assert lib.gsx_tag_events(e.h, one.ctypes.data_as(C.c_void_p), 1) == abi.GSX_EINVAL
    two = np.array([(1, 0, 2), (E, 0, 1)], dtype=abi.tag_event_dtype())
    assert lib.gsx_tag_events(e.h, two.ctypes.data_as(C.c_void_p), 2) == abi.GSX_EINVAL
    assert not e.tag_export().any()  # nothing was applied
    assert lib.gsx_tag_events(e.h, None, 1) == abi.GSX_EINVAL
    assert lib.gsx_tag_export(e.h, None) == abi.GSX_EINVAL
    assert lib.gsx_conn_trim(e.h, 1, None, None) == abi.GSX_EINVAL
    assert lib.gsx_tag_trace_deliver(e.h, E, 1, 0, T0) == abi.GSX_ERANGE
    assert lib.gsx_tag_trace_deliver(e.h, 0, 1, 2, T0) == abi.GSX_EINVAL
    assert lib.gsx_tag_trace_reject(e.h, 0, 1, 0, 11, T0) == abi.GSX_EINVAL
    # the fold needs the first-deliverer rows of the call it folds
    ms = pc.messages(40, 10, seed=3)
    e.set_prop_tracking(False)
    e.propagate(ms, pc.config(abi.GSX_ROUTER_GOSSIPSUB, credit=0))
    assert lib.gsx_tag_fold_prop(e.h) == abi.GSX_ESTATE
    e.set_prop_tracking(True)
    e.propagate(ms, pc.config(abi.GSX_ROUTER_GOSSIPSUB, credit=0))
    assert lib.gsx_tag_fold_prop(e.h) == 0 and e.tag_export().any()
    e.tag_trace_validate(0, 5, 0, T0)
    assert e.tag_num_pending() == 1
    # NULL drops the tracer; a new one starts empty
    e.set_tag_params(None)
    assert calls() == [abi.GSX_ESTATE] * 11
    e.set_tag_params(tp)
    assert not e.tag_export().any() and e.tag_num_pending() == 0
    e.tag_events(np.array([(3, 1, 2)], dtype=abi.tag_event_dtype()))
    assert e.tag_export()[1, 3] == 2
    # an overlay load drops it
    e.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    assert calls() == [abi.GSX_ESTATE] * 11
    e.close()
    # a range shard keeps tags but folds and trims nothing
    sh = gsx.Engine(1, device=0)
    sh.set_peer_params(synth.bench_peer_params())
    sh.set_topic_params(0, synth.spam_test_topic_params())
    lo, hi = 0, 20
    rp = (ov.row_ptr[lo:hi + 1] - ov.row_ptr[lo]).astype(np.int64)
    sh.load_overlay_shard(40, lo, rp, ov.col[ov.row_ptr[lo]:ov.row_ptr[hi]], ov.edge_flags[ov.row_ptr[lo]:ov.row_ptr[hi]],
                          ov.node_ips)
    sh.set_tag_params(tp)
    sh.tag_events(np.array([(0, 0, 20)], dtype=abi.tag_event_dtype()))
    assert sh.tag_export()[0, 0] == 15
    assert lib.gsx_tag_fold_prop(sh.h) == abi.GSX_ESTATE
    assert lib.gsx_conn_trim(sh.h, 1, ptr, None) == abi.GSX_ESTATE
    sh.close()


def test_a_stepped_call_in_flight_refuses_the_fold(gpu_ok):
    lib = gsx.load_library()
    ov = pc.overlay(40, 4, seed=3)
    e = gsx.Engine(1, device=0)
    pc.setup(e, ov, 1, seed=3)
    e.set_tag_params(e.default_tag_params())
    ms = pc.messages(40, 10, seed=3)
    cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, credit=0)
    e.propagate(ms, cfg)
    assert lib.gsx_tag_fold_prop(e.h) == 0
    e.prop_begin(ms, cfg)
    assert lib.gsx_tag_fold_prop(e.h) == abi.GSX_ESTATE
    e.prop_end()
    assert lib.gsx_tag_fold_prop(e.h) == 0
    e.close()


def test_the_tracer_leaves_the_scorer_alone(gpu_ok):
    """Tracer on, none of its calls made: events, refresh, a credited propagation and a heartbeat
    leave scores and state equal to the oracle's."""
    ov = pc.overlay(300, 6, seed=23, mix_protocols=True)
    ms = pc.messages(300, 100, seed=23, invalid=0.1)
    cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, latency_ms=5, delay_ms=2.0)
    res = []
    for be in (gsx.Engine(2, device=0), orc.Oracle(2)):
        pc.setup(be, ov, 2, seed=23)
        be.set_gossipsub_params(orc.default_gossipsub_params())
        if isinstance(be, gsx.Engine):
            be.set_tag_params(be.default_tag_params())
        be.apply_events(np.array([(abi.EV_PRUNE, 0, p, T0 + 2 * S, 0) for p in range(0, ov.n_pairs, 7)],
                                 dtype=abi.event_dtype()))
        be.refresh(T0 + 3 * S)
        out, hop, _ = be.propagate(ms, cfg, want_results=True)
        hb = be.heartbeat(1, T0 + 4 * S, 9)
        be.refresh(T0 + 5 * S)
        res.append((out.as_dict(), hop, hb.as_dict(), be.scores(), be.export_state()))
    (o1, h1, b1, s1, x1), (o2, h2, b2, s2, x2) = res
    assert o1 == o2 and b1 == b2 and np.array_equal(h1, h2)
    assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64))
    for k in abi.STATE_FIELDS:
        assert np.array_equal(x1[k].view(np.uint8), x2[k].view(np.uint8)), k

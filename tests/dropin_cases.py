"""Shared drivers of test_gpu_dropin.py and test_dropin_oracle.py: the drop-in
Score() path (gsx_score / gsx_score_many on an engine of at most 65,536 pairs:
the host score copy, the shortcut that skips the device, and k_dropin).

Every driver takes a Lockstep over one backend (the oracle alone: the CPU test
pins the preconditions) or over engine + oracle (every read is compared with
the oracle's bit for bit where it is made, and the engine's dropin_launches()
must move by what the driver expects: which path answered)."""
from __future__ import annotations

import numpy as np

import gossip_cases as gc
import membership_cases as mc
import pair_epoch_cases as pe
import propagation_cases as pc
import randomized as rz
import test_gpu_wb16 as wb
from gsx import abi, synth

S = abi.SECOND
MS = abi.MILLISECOND
T0 = rz.T0
CONNECTED = pe.CONNECTED
GOSSIP, FLOOD = abi.GSX_ROUTER_GOSSIPSUB, abi.GSX_ROUTER_FLOODSUB

# k_dropin's limits (gsx_engine.cpp)
MAX_PAIRS, MAX_EVENTS, MAX_OBS, BLOCK = 65536, 4096, 64, 1024


def evs(ev):
    return np.array(ev, dtype=abi.event_dtype())


class Lockstep:
    """The same calls on every backend; the last one is the oracle, the first (when there are
    two) the engine.  Reads return the oracle's values."""

    def __init__(self, *bes):
        self.bes = bes
        self.ora = bes[-1]
        self.eng = bes[0] if len(bes) > 1 else None
        self.counted = []  # (where, expected launches) of every read that named an expectation

    def call(self, name, *a, **kw):
        return [getattr(be, name)(*a, **kw) for be in self.bes][-1]

    def events(self, ev):
        self.call("apply_events", evs(ev))

    def launches(self):
        return self.eng.dropin_launches() if self.eng is not None else 0

    def _read(self, fn, where, expect):
        n0 = self.launches()
        got = [np.asarray(fn(be), dtype=np.float64) for be in self.bes]
        if expect is not None:
            self.counted.append((where, expect))
            if self.eng is not None:
                assert self.launches() - n0 == expect, f"{where}: k_dropin launches {self.launches() - n0} != {expect}"
        if self.eng is not None:
            g, w = got[0].view(np.uint64), got[-1].view(np.uint64)
            assert np.array_equal(g, w), f"{where}: differs from the oracle at {np.nonzero(g != w)[0][:8]}"
        return got[-1]

    def many(self, pairs, where, expect=None):
        ps = np.asarray(pairs, dtype=np.uint64)
        return self._read(lambda be: be.score_many(ps), f"{where}: score_many", expect)

    def one(self, pair, where, expect=None):
        return float(self._read(lambda be: be.score(int(pair)), f"{where}: score({pair})", expect))

    def full(self, where, n_pairs):
        """score_many(all), scores() and export_state(): both score copies and the records."""
        a = self.many(np.arange(n_pairs), f"{where}: all pairs")
        b = self._read(lambda be: be.scores(), f"{where}: scores()", None)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), where
        sts = [be.export_state() for be in self.bes]
        if self.eng is not None:
            for f in abi.STATE_FIELDS:
                assert np.array_equal(pe.bits(sts[0][f]), pe.bits(sts[-1][f])), f"{where}: state field {f}"
            assert sts[0]["last_refresh_ns"] == sts[-1]["last_refresh_ns"], where
        return b, sts[-1]


def configure(ls, ov, T):
    pp, tps = rz.scenario_params(T)
    ls.call("set_peer_params", pp)
    for t, tp in tps.items():
        ls.call("set_topic_params", t, tp)
    ls.call("load_overlay", ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    ls.call("set_ip_whitelist", [3])


# ---- mixed(): ~9,500 pairs, a hub row longer than k_dropin's block ------------------------
MIXED_N, MIXED_SEED, HUB, HUB_LINKS, IP_POOL = 1200, 11, 5, 1100, 40


def mixed():
    ov = pc.with_hub(rz.small_overlay(MIXED_N, 3, MIXED_SEED, IP_POOL), HUB, HUB_LINKS, MIXED_SEED)
    assert ov.n % 64 != 0 and ov.n_pairs % 64 != 0 and 9000 < ov.n_pairs < MAX_PAIRS
    assert ov.row_ptr[HUB + 1] - ov.row_ptr[HUB] >= HUB_LINKS > BLOCK
    return ov


def grafted(p, T):
    """mixed_setup grafts every third pair, on topic p % T."""
    return p % 3 == 0


def mixed_setup(ls, ov, T):
    """AddPeer every pair, graft every third, forget every tenth (the later AddPeers' pairs), one
    refresh: all through apply_events + scores() (the general path); then the host copy."""
    E = ov.n_pairs
    configure(ls, ov, T)
    ls.events([(abi.EV_ADD_PEER, 0, p, T0, 0) for p in range(E)])
    ls.events([(abi.EV_GRAFT, p % T, p, T0, 0) for p in range(E) if grafted(p, T)])
    ls.events([(abi.EV_FIRST_DELIVERY, p % T, p, T0, 0) for p in range(0, E, 4)])
    ls.call("scores")
    ls.events([e for p in range(7, E, 10) for e in pe.remove_events(p, T0, 1e9)])
    ls.call("refresh", T0 + 2 * S)
    ls.call("scores")
    ls.many(np.arange(E), "prime")


class Batch:
    def __init__(self, name, events, expect, rows, ov):
        self.name, self.events, self.expect, self.rows = name, events, expect, sorted(rows)
        obs = ov.pair_observer()
        self.pairs = sorted({e[2] for e in events})
        self.observers = sorted({int(obs[p]) for p in self.pairs})
        rng = np.random.default_rng(len(events) + 7 * len(self.observers))
        named = set(self.pairs)
        near = [p for u in self.rows for p in range(ov.row_ptr[u], ov.row_ptr[u + 1]) if p not in named]
        touched = set(self.observers)
        far = [p for p in rng.permutation(ov.n_pairs).tolist() if int(obs[p]) not in touched][:16]
        self.near = [int(p) for p in rng.permutation(near)[:16]] if near else []
        self.far = far
        self.unnamed = self.near + self.far


class _World:
    """The pairs' standing as the batches leave it (they are built in the order they run)."""

    def __init__(self, ov, T):
        self.ov, self.T, self.E = ov, T, ov.n_pairs
        self.rng = np.random.default_rng(MIXED_SEED + 1)
        self.absent = set(range(7, self.E, 10))
        self.retained = set()
        self.now = T0 + 2 * S
        self.batches = []

    def row(self, u):
        return list(range(int(self.ov.row_ptr[u]), int(self.ov.row_ptr[u + 1])))

    def conn(self, u):
        return [p for p in self.row(u) if p not in self.absent and p not in self.retained]

    def topic(self, p):
        return p % self.T

    def ev(self, kind, p, arg=0):
        t = self.topic(p) if kind in (3, 4, 5, 6, 7) else 0
        return (kind, t, int(p), self.now, int(arg))

    def remove(self, p, keep):
        (self.retained if keep else self.absent).add(p)
        return [self.ev(9, p, pe.f64_bits(-1e6 if keep else 1e9)), self.ev(2, p)]

    def add(self, p):
        self.absent.discard(p)
        self.retained.discard(p)
        return [self.ev(1, p)]

    def group(self, u, row, kinds, keep=False):
        """Events of observer u: `kinds` (of 3 .. 9) each on a pair of its own while the row has
        one; with `row`, also a RemovePeer and, where the row holds an absent pair, an AddPeer."""
        free = [int(p) for p in self.rng.permutation(self.conn(u))]
        out = []
        if row:
            gone = [p for p in self.row(u) if p in self.absent]
            if gone:
                out += self.add(gone[0])
            if len(free) > 1:
                out += self.remove(free.pop(), keep)
        for i, k in enumerate(kinds):
            if not free:
                break
            p = free[i % len(free)]
            arg = {8: 1 + i % 3, 9: pe.f64_bits(-1.5 - i)}.get(k, 0)
            out.append(self.ev(k, p, arg))
        return out

    def emit(self, name, groups, expect=1):
        """Round-robin over the groups: each keeps its order, the issue order mixes them."""
        ev, i = [], 0
        while any(i < len(g) for g in groups):
            ev += [g[i] for g in groups if i < len(g)]
            i += 1
        obs = self.ov.pair_observer()
        rows = {int(obs[e[2]]) for e in ev if e[0] in (1, 2)}
        self.batches.append(Batch(name, ev, expect, rows, self.ov))
        self.now += 100 * MS

    def observers(self, n):
        """n observers other than the hub with at least three connected pairs."""
        out = []
        for u in self.rng.permutation(self.ov.n).tolist():
            if u != HUB and len(self.conn(u)) >= 3:
                out.append(u)
            if len(out) == n:
                return out
        raise AssertionError("not enough observers")


def spread(w, n):
    """n observers: every other one with an AddPeer / RemovePeer (its row is re-scored), the
    rest pairs only; kinds 3 .. 9 in rotating windows of three."""
    groups = []
    for i, u in enumerate(w.observers(n)):
        kinds = [3 + (i + j) % 7 for j in range(3)]
        groups.append(w.group(u, row=i % 2 == 0, kinds=kinds, keep=i % 4 == 0))
    return groups


def mixed_batches(ov, T):
    w = _World(ov, T)
    hub_mesh = [p for p in w.conn(HUB) if grafted(p, T) and w.topic(p) < max(T - 1, 1)]
    hub_rest = [p for p in w.conn(HUB) if not grafted(p, T)]
    # every kind on a pair of its own in the hub's row, a retaining and a forgetting RemovePeer
    g = w.add([p for p in w.row(HUB) if p in w.absent][0])
    g += [w.ev(4, hub_mesh[0]), w.ev(6, hub_mesh[1]), w.ev(3, hub_rest[0]), w.ev(5, hub_rest[1]), w.ev(7, hub_rest[2]),
          w.ev(8, hub_rest[3], 3), w.ev(9, hub_rest[4], pe.f64_bits(-2.5))]
    g += w.remove(hub_rest[5], keep=True) + w.remove(hub_rest[6], keep=False)
    w.emit("every kind in the hub's row", [g])
    for n in (2, 63, 64):
        w.emit(f"{n} observers", spread(w, n))
    w.emit("65 observers", spread(w, 65), expect=0)
    # the hub is the only row re-scored: P6 moves for pairs the batch never names
    gone = [p for p in w.row(HUB) if p in w.absent]
    g = [e for p in gone[:40] for e in w.add(p)]
    g += [e for p in w.conn(HUB)[100:120] for e in w.remove(p, keep=False)]
    w.emit("hub row only", [g] + [w.group(u, False, [8, 5, 7]) for u in w.observers(10)])
    # 300 events on one pair: deliveries to and past their caps, a PRUNE in the middle
    p = hub_mesh[2]
    kinds = [5] * 60 + [6] * 60 + [7] * 29 + [4] + [6, 5, 7] * 10 + [3] + [6] * 60 + [7] * 59
    assert len(kinds) == 300
    w.emit("300 events on one pair", [[w.ev(k, p) for k in kinds]])
    # duplicates in one group; EV_APP_SCORE twice on one pair (the last one wins)
    u = w.observers(1)[0]
    a, b, c = w.conn(u)[:3]
    g = [w.ev(8, a, 2), w.ev(5, a), w.ev(9, a, pe.f64_bits(2.5)), w.ev(8, a, 1), w.ev(5, b), w.ev(5, b),
         w.ev(9, a, pe.f64_bits(-4.25)), w.ev(7, b)]
    v = w.observers(1)[0]
    y = w.conn(v)[0]
    g2 = w.remove(y, keep=False) + w.add(y) + [w.ev(8, y, 2)] + w.remove(y, keep=True) + w.add(y)
    w.emit("duplicate pairs", [g, g2])
    # no row: the 256-thread launch
    w.emit("pairs only, one event", [[w.ev(8, c, 3)]])
    w.emit("pairs only, five observers", [w.group(x, False, [5, 8, 9]) for x in w.observers(5)])
    # the event limit, on the hub's row (one RemovePeer: the row is re-scored)
    for n in (MAX_EVENTS, MAX_EVENTS + 1):
        hub = w.conn(HUB)
        g = w.remove(hub[-1], keep=False)
        g += [w.ev((5, 6, 7, 8)[i % 4], hub[i % 500], 1) for i in range(n - len(g))]
        w.emit(f"{n} events", [g], expect=1 if n <= MAX_EVENTS else 0)
    return w.batches


def run_mixed(ls, T=3):
    """-> [(batch, the oracle's scores before it, after it)]."""
    ov = mixed()
    mixed_setup(ls, ov, T)
    out = []
    before = ls.ora.scores()
    for b in mixed_batches(ov, T):
        ls.events(b.events)
        ls.many(b.pairs + b.unnamed, b.name, expect=b.expect)
        after, st = ls.full(b.name, ov.n_pairs)
        out.append((b, before, after, st))
        before = after
    return out


# ---- exact(E): 65,536 pairs exactly, and one more ----------------------------------------
EXACT_N = 8192


def exact(E):
    """Circulant: node i sees i +- 1 .. 4; E = 65,537 adds the one-directional pair 0 -> 100."""
    n = EXACT_N
    assert E in (MAX_PAIRS, MAX_PAIRS + 1)
    nb = [sorted((i + k) % n for k in (-4, -3, -2, -1, 1, 2, 3, 4)) for i in range(n)]
    if E == MAX_PAIRS + 1:
        nb[0] = sorted(nb[0] + [100])
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum([len(r) for r in nb])
    col = np.array([v for r in nb for v in r], dtype=np.int32)
    ips = np.full((n, 2), abi.GSX_NO_IP, dtype=np.uint32)
    ips[:, 0] = (np.arange(n) // 3) % 700  # neighbours share addresses in threes
    return synth.Overlay(n=n, row_ptr=row_ptr, col=col, edge_flags=np.full(len(col), abi.GSX_EDGE_GOSSIPSUB, np.uint8),
                         node_ips=ips, sybil=np.zeros(n, dtype=bool))


def run_exact(ls, E):
    ov = exact(E)
    assert ov.n_pairs == E
    configure(ls, ov, 1)
    ls.events([(abi.EV_ADD_PEER, 0, p, T0, 0) for p in range(E)])
    ls.call("scores")
    ls.many(np.arange(E), "prime")
    before = ls.ora.scores()
    p, q = 5, 8 * 4000 + 2
    ls.events([(abi.EV_PENALTY, 0, p, T0 + S, 3)] + pe.remove_events(q, T0 + S, 1e9))
    ls.many([p, q, q + 1, 8 * 4000, E - 1, 0], f"exact({E})", expect=1 if E <= MAX_PAIRS else 0)
    after, _ = ls.full(f"exact({E})", E)
    return ov, before, after


# ---- (b) k_dropin with decays pending -----------------------------------------------------
def wb_load(ls, T):
    """test_gpu_wb16.start's state on every backend of ls (the engines at a period of 16)."""
    ov = synth.connect_some_overlay(wb.N, d=wb.D)
    st = synth.synthetic_state(ov, T, T0, p_absent=0.1)
    imd = st["invalid_message_deliveries"]
    imd[::7] = 60.0 + np.arange(len(imd[::7]))
    in_mesh = (st["rec_flags"] & abi.GSX_REC_IN_MESH) != 0
    st["rec_flags"] = np.where(in_mesh, abi.GSX_REC_IN_MESH | abi.GSX_REC_ACTIVE, 0).astype(np.uint8)
    ls.call("set_peer_params", wb.peer_params())
    for t in range(T):
        ls.call("set_topic_params", t, wb.topic_params())
    ls.call("set_thresholds", abi.Thresholds(**pe.THRESHOLDS))
    ls.call("load_overlay", ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    ls.call("import_state", st)
    ls.call("set_app_scores", np.zeros(ov.n_pairs))
    if ls.eng is not None:
        ls.eng.set_decay_writeback(16)
    return ov


def run_pending_decays(ls, T, phase, check=None):
    """Events through k_dropin with `phase` decays pending.  check(where): the caller's
    comparison of engine and oracle (pair_epoch_cases.same).  -> (crossings of DecayToZero by a
    touched counter, by a touched penalty, retained pair's flags, forgotten pair's flags)."""
    ov = wb_load(ls, T)
    E = ov.n_pairs
    every = np.arange(E)
    ls.many(every, "prime")
    now = T0
    for _ in range(phase):
        now += S
        ls.call("refresh", now)
    ls.many(every, f"phase {phase}: re-prime")
    ev, kept, gone = wb.event_batch(ls.ora, T, now, np.random.default_rng(100 * T + phase))
    pairs = sorted({e[2] for e in ev})
    touched = np.zeros(E, dtype=bool)
    touched[pairs] = True
    ls.events(ev)
    ls.many(pairs, f"T={T} phase {phase}: events", expect=1)
    if check:
        check(f"T={T} phase {phase}: after the events")
    _, st = ls.full(f"T={T} phase {phase}: after the events", E)
    flags = (int(st["pair_flags"][kept]), int(st["pair_flags"][gone]))
    cross_rec = cross_bp = 0
    for i in range(4):
        before = ls.ora.export_state()
        now += S
        ls.call("refresh", now)
        if check:
            check(f"T={T} phase {phase}: refresh + {i + 1}")
        _, after = ls.full(f"T={T} phase {phase}: refresh + {i + 1}", E)
        if phase + i + 1 >= 5:  # (the phase wraps at 16: 12 + 4 = 16 stores, still >= 5 pending before it)
            tt = np.tile(touched, T)
            for f in ("first_message_deliveries", "mesh_message_deliveries", "mesh_failure_penalty",
                      "invalid_message_deliveries"):
                cross_rec += int(((before[f] >= wb.DTZ) & (after[f] == 0) & tt).sum())
            cross_bp += int(((before["behaviour_penalty"] >= wb.DTZ) & (after["behaviour_penalty"] == 0) & touched).sum())
    return cross_rec, cross_bp, flags


# ---- (c) no mutator leaves a stale host copy ----------------------------------------------
C_N, C_D, C_T, C_SEED = 600, 5, 2, 23


class Ctx:
    def __init__(self, ls):
        self.ls = ls
        self.T = C_T
        self.ov = pc.overlay(C_N, C_D, C_SEED, mix_protocols=True)
        self.now = T0 + 3 * S
        self.rng = np.random.default_rng(C_SEED)

    @property
    def E(self):
        return self.ov.n_pairs

    def setup(self):
        for be in self.ls.bes:
            pc.setup(be, self.ov, self.T, C_SEED)
        # a few addresses shared by many pairs: P6 and the whitelist matter
        rng = np.random.default_rng(C_SEED + 2)
        pairs = rng.choice(self.E, 300, replace=False)
        ips = np.full((300, 2), abi.GSX_NO_IP, dtype=np.uint32)
        ips[:, 0] = rng.integers(0, 6, 300)
        self.ls.call("set_pair_ips", pairs, ips)

    def prop(self, router, credit=abi.GSX_CREDIT_NOW, latency_ms=10, seed=0, topic=0, hops=40, m=48):
        ms = pc.messages(self.ov.n, m, C_SEED + seed, invalid=0.1)
        cfg = pc.config(router, topic=topic, latency_ms=latency_ms, credit=credit, seed=9 + seed, max_hops=hops)
        cfg.now_ns = self.now
        return ms, cfg

    def propagate(self, *a, **kw):
        ms, cfg = self.prop(*a, **kw)
        outs = [be.propagate(ms, cfg)[0].as_dict() for be in self.ls.bes]
        assert outs[0] == outs[-1] and outs[-1]["deliveries"] > 0, outs
        self.now += 50 * MS


def _m_refresh(c):
    c.now += S
    c.ls.call("refresh", c.now)


def _m_app(c):
    c.ls.call("set_app_scores", c.rng.normal(0, 3, c.E))


def _m_pair_ips(c):
    pairs = c.rng.choice(c.E, 60, replace=False)
    ips = np.full((60, 2), abi.GSX_NO_IP, dtype=np.uint32)
    ips[:, 0] = c.rng.integers(0, 3, 60)
    ips[::5, 1] = 4
    c.ls.call("set_pair_ips", pairs, ips)


def _m_whitelist(c):
    c.ls.call("set_ip_whitelist", [0, 2, 4])


def _m_peer_params(c):
    pp = synth.bench_peer_params()
    pp.app_specific_weight = pp.app_specific_weight * 2 + 0.5
    pp.ip_colocation_factor_weight = pp.ip_colocation_factor_weight * 0.5 - 1.0
    pp.topic_score_cap = 5.0
    c.ls.call("set_peer_params", pp)


def _m_topic_params(c):
    tp = synth.spam_test_topic_params()
    tp.mesh_message_deliveries_window_ns = 25 * MS
    tp.topic_weight = tp.topic_weight * 0.5 + 0.125
    tp.first_message_deliveries_cap = 1.0
    tp.mesh_message_deliveries_cap = 1.0
    tp.time_in_mesh_cap = 0.5
    c.ls.call("set_topic_params", 0, tp)


def _pre_lazy(c):
    c.propagate(GOSSIP)
    c.propagate(GOSSIP, seed=1)


def _m_thresholds(c):
    c.ls.call("set_thresholds", abi.Thresholds(gossip_threshold=-0.5, publish_threshold=-1, graylist_threshold=-2,
                                               accept_px_threshold=100, opportunistic_graft_threshold=50))


def _m_import(c):
    st = c.ls.ora.export_state()
    st["first_message_deliveries"] = st["first_message_deliveries"] * 0.5 + 1.0
    st["behaviour_penalty"] = st["behaviour_penalty"] + 2.0
    c.ls.call("import_state", st)


def _pre_three_refreshes(c):
    for _ in range(3):
        _m_refresh(c)


def _m_writeback(c):
    if c.ls.eng is not None:  # (the oracle stores at every refresh: it has no period)
        c.ls.eng.set_decay_writeback(4)
        c.ls.eng.set_decay_writeback(16)


def _m_gossip_once(c):
    c.propagate(GOSSIP)


def _m_gossip_thrice(c):
    for k in range(3):
        c.propagate(GOSSIP, seed=k, topic=k % c.T)


def _m_gossip_late(c):
    if c.ls.eng is not None:  # (the oracle keeps no first-deliverer rows to turn off)
        c.ls.eng.set_prop_tracking(False)
    c.propagate(GOSSIP, latency_ms=0)
    c.propagate(GOSSIP, latency_ms=0, seed=1)


def _m_flood(c):
    c.propagate(FLOOD)


def _m_defer_fold(c):
    ms, cfg = c.prop(GOSSIP, credit=abi.GSX_CREDIT_DEFER)
    _, now = c.prop(GOSSIP, credit=abi.GSX_CREDIT_NOW)
    outs = []
    for be in c.ls.bes:  # (the oracle credits at once: GSX_CREDIT_DEFER + fold is the engine's split of it)
        if be is c.ls.eng:
            outs.append(be.propagate(ms, cfg)[0].as_dict())
            be.fold_credits()
        else:
            outs.append(be.propagate(ms, now)[0].as_dict())
    assert outs[0] == outs[-1], outs


def _m_heartbeat(c):
    tot = {}
    for k in range(3):
        # round 0 serves its IWANTs; with no retransmission the later promises break (P7)
        c.ls.call("set_gossipsub_params", gc.params(iwant_followup_ns=S // 2, **({"gossip_retransmission": 0} if k else {})))
        ms, cfg = c.prop(GOSSIP, seed=k, topic=k % c.T, hops=2, latency_ms=5)
        outs = [be.propagate(ms, cfg)[0].as_dict() for be in c.ls.bes]
        assert outs[0] == outs[-1], k
        hb = [be.heartbeat(61 + k, c.now + 500 * MS, C_SEED).as_dict() for be in c.ls.bes]
        assert hb[0] == hb[-1], (k, hb)
        c.now += S
        for x, v in hb[-1].items():
            tot[x] = tot.get(x, 0) + v
    c.hb_totals = tot


def _m_join_leave(c):
    c.ls.call("set_subscriptions", mc.joined_bits(c.ov.n, c.T, C_SEED))
    rng = np.random.default_rng(C_SEED + 4)
    nodes = rng.choice(c.ov.n, 40, replace=False).astype(np.uint32)
    topics = rng.integers(0, c.T, 40).astype(np.uint32)
    outs = [be.join(nodes, topics, c.now, C_SEED + 1).as_dict() for be in c.ls.bes]
    assert outs[0] == outs[-1], outs
    nodes = rng.choice(c.ov.n, 200, replace=False).astype(np.uint32)
    topics = rng.integers(0, c.T, 200).astype(np.uint32)
    outs = [be.leave(nodes, topics, c.now + 100 * MS).as_dict() for be in c.ls.bes]
    assert outs[0] == outs[-1], outs
    c.now += 200 * MS


def _m_trace(c):
    ls, now = c.ls, c.now
    row = np.arange(c.ov.row_ptr[9], c.ov.row_ptr[10])
    a, b, d = (int(x) for x in row[:3])
    ls.call("trace_validate", a, 1, 0, now)
    ls.call("trace_duplicate", b, 1, 0, now)
    ls.call("trace_deliver", a, 1, 0, now)
    ls.call("trace_duplicate", d, 1, 0, now + MS)
    ls.call("trace_validate", b, 2, 1, now)
    ls.call("trace_duplicate", a, 2, 1, now)
    ls.call("trace_reject", b, 2, 1, rz.REASONS[0], now)
    for r in rz.REASONS:
        ls.call("trace_reject", d, 3, 0, int(r), now)
    ls.call("gc_deliveries", now + 200 * S)
    c.now += 10 * MS


def _m_reload(c):
    """A smaller overlay (its host copy primed), then a larger one, on the same backends."""
    for n in (300, 800):
        c.ov = pc.overlay(n, C_D, C_SEED + n, mix_protocols=True)
        c.setup()
        c.ls.many(np.arange(c.E), f"overlay of {n}: all pairs")
        c.ls.events([(abi.EV_PENALTY, 0, c.E - 1, c.now, 2), (abi.EV_FIRST_DELIVERY, 0, 0, c.now, 0)])
        c.ls.many([0, c.E - 1], f"overlay of {n}: an event", expect=1)


# name -> (what runs after the priming read and before the mutator, the mutator, whether the
# oracle's scores must change)
MUTATORS = {
    "refresh": (None, _m_refresh, True),
    "set_app_scores": (None, _m_app, True),
    "set_pair_ips": (None, _m_pair_ips, True),
    "set_ip_whitelist": (None, _m_whitelist, True),
    "set_peer_params": (None, _m_peer_params, True),
    "set_topic_params": (None, _m_topic_params, True),
    "set_thresholds above the lazy bound": (_pre_lazy, _m_thresholds, False),
    "import_state": (None, _m_import, True),
    "set_decay_writeback 4 then 16": (_pre_three_refreshes, _m_writeback, False),
    "gossipsub credits once": (None, _m_gossip_once, True),
    "gossipsub credits three times": (None, _m_gossip_thrice, True),
    "gossipsub late accounting": (None, _m_gossip_late, True),
    "floodsub credits": (None, _m_flood, True),
    "deferred credits folded": (None, _m_defer_fold, True),
    "heartbeat with the gossip exchange": (None, _m_heartbeat, True),
    "join and leave": (None, _m_join_leave, True),
    "tracer calls and gc": (None, _m_trace, True),
    "load_overlay smaller then larger": (None, _m_reload, True),
}


def kinds_batch(st, T, now, rng):
    """One event of each kind 1 .. 9 on pairs of their own, from the exported state `st`."""
    pf = st["pair_flags"]
    E = len(pf)
    conn = [int(p) for p in rng.permutation(np.nonzero(pf == CONNECTED)[0])]
    assert len(conn) > 12
    t = int(rng.integers(T))
    absent = np.nonzero(pf == 0)[0]
    first = int(absent[0]) if len(absent) else conn[9]
    assert first < E
    return [(abi.EV_ADD_PEER, 0, first, now, 0), (abi.EV_REMOVE_PEER, 0, conn[0], now, 0),
            (abi.EV_GRAFT, t, conn[1], now, 0), (abi.EV_PRUNE, t, conn[2], now, 0),
            (abi.EV_FIRST_DELIVERY, t, conn[3], now, 0), (abi.EV_MESH_DELIVERY, t, conn[4], now, 0),
            (abi.EV_INVALID_DELIVERY, t, conn[5], now, 0), (abi.EV_PENALTY, 0, conn[6], now, 2),
            (abi.EV_APP_SCORE, 0, conn[7], now, pe.f64_bits(-3.25))]


def run_mutator(ls, name):
    """-> (the oracle's scores before the mutator, after it, the context)."""
    pre, mutate, _ = MUTATORS[name]
    c = Ctx(ls)
    c.setup()
    ls.many(np.arange(c.E), f"{name}: prime")
    if pre:
        pre(c)
    before = ls.ora.scores()
    mutate(c)
    rng = np.random.default_rng(C_SEED + 3)
    for p in rng.integers(0, c.E, 64).tolist():
        ls.one(p, name)
    ls.many(np.arange(c.E), f"{name}: all pairs")
    after, st = ls.full(name, c.E)
    ev = kinds_batch(st, c.T, c.now, rng)
    ls.events(ev)
    ls.many(sorted({e[2] for e in ev}), f"{name}: then one event of each kind")
    ls.full(f"{name}: then one event of each kind", c.E)
    return before, after, c


# ---- (d) the shortcut that skips the device -----------------------------------------------
def shares_ip(ov, p, q):
    a = {int(x) for x in ov.node_ips[ov.col[p]] if x != abi.GSX_NO_IP and x != 3}
    b = {int(x) for x in ov.node_ips[ov.col[q]] if x != abi.GSX_NO_IP and x != 3}
    return bool(a & b)


def run_shortcut(ls, T=3):
    """-> {step: (the oracle's score of the pair read before the events, after them)}."""
    ov = mixed()
    E = ov.n_pairs
    mixed_setup(ls, ov, T)
    now = T0 + 3 * S
    obs = ov.pair_observer()
    hub = range(int(ov.row_ptr[HUB]), int(ov.row_ptr[HUB + 1]))
    p = int(ov.row_ptr[40]) + 1
    q = int(ov.row_ptr[41]) + 1
    assert p % 10 != 7 and q % 10 != 7 and obs[p] != obs[q] and HUB not in (obs[p], obs[q])
    out = {}
    base = ls.ora.scores()
    # an event on p leaves q alone: answered from the host copy, the event stays queued
    ls.events([(abi.EV_PENALTY, 0, p, now, 3)])
    out["other row"] = (base[q], ls.one(q, "event on p, read q", expect=0))
    ls.many([q, q + 1], "event on p, read q", expect=0)
    out["the pair"] = (base[p], ls.one(p, "event on p, read p", expect=1))
    # an AddPeer in the hub's row moves the P6 of another pair of the row
    a = next(x for x in hub if x % 10 == 7)
    r = next(x for x in hub if x % 10 != 7 and x != a and shares_ip(ov, a, x))
    base = ls.ora.scores()
    ls.events([(abi.EV_ADD_PEER, 0, a, now, 0)])
    out["AddPeer in the row"] = (base[r], ls.one(r, "AddPeer in the row", expect=1))
    # a RemovePeer that forgets likewise (its EV_APP_SCORE names only the pair itself)
    x = next(y for y in hub if y % 10 != 7 and y not in (a, r) and shares_ip(ov, r, y))
    base = ls.ora.scores()
    ls.events(pe.remove_events(x, now, 1e9))
    out["RemovePeer in the row"] = (base[r], float(ls.many([r], "RemovePeer in the row", expect=1)[0]))
    # an out-of-range pair: GSX_ERANGE, the queued events stay queued, later reads are right
    ls.events([(abi.EV_PENALTY, 0, p, now, 1)])
    if ls.eng is not None:
        n0 = ls.launches()
        try:
            ls.eng.score_many(np.array([q, E], dtype=np.uint64))
            raise AssertionError("score_many took a pair out of range")
        except abi.GsxError as ex:
            assert ex.code == abi.GSX_ERANGE
        assert ls.launches() == n0
    ls.many([q], "after GSX_ERANGE, read q", expect=0)
    ls.many([p, q], "after GSX_ERANGE, read p", expect=1)  # (+1: the event was still queued)
    ls.full("after GSX_ERANGE", E)
    return out


# ---- (e) a seeded router session ----------------------------------------------------------
SESSION_N, SESSION_STEPS = 400, 150


def run_session(ls, T, seed):
    """-> the oracle's reads.  Every read of every backend is compared as it is made."""
    ov = rz.small_overlay(SESSION_N, 3, seed, 40)
    ops = rz.session_ops(ov, T, seed, SESSION_STEPS)
    reads = [rz.session_replay(be, ov, T, ops) for be in ls.bes]
    if ls.eng is not None:
        assert len(reads[0]) == len(reads[-1])
        for i, ((kg, g), (kw, w)) in enumerate(zip(reads[0], reads[-1])):
            assert kg == kw, i
            if isinstance(w, dict):
                assert set(g) == set(w), (i, kw)
                for f in w:
                    assert np.array_equal(pe.bits(np.asarray(g[f])), pe.bits(np.asarray(w[f]))), (i, kw, f)
            else:
                g, w = np.atleast_1d(np.asarray(g)), np.atleast_1d(np.asarray(w))
                assert np.array_equal(pe.bits(g), pe.bits(w)), f"read {i} ({kw}): differs from the oracle"
    return ops, reads[-1]

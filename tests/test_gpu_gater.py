"""The peer gater and gsx_accept_from on the device against tests/gater_model.py
(a restatement of peer_gater.go): every status and the exported state bit for
bit, call by call; and gsx_gater_fold_prop against the model fed event by event
from the ORACLE's propagation results."""
import ctypes as C

import numpy as np
import pytest

import gater_model as gm
import gsx
import oracle as orc
import propagation_cases as pc
from gsx import abi, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND
T0 = 1_700_000_000 * S
NO_IP = abi.GSX_NO_IP
REASONS = {v: k for k, v in abi.REJECT_REASONS.items()}
GRAYLIST = -300.0


def gater_params(threshold=0.1, gdecay=0.9, sdecay=0.95, retain=8 * S, quiet=6 * S, weights=None):
    p = abi.GaterParams()
    assert gsx.load_library().gsx_default_gater_params(C.byref(p)) == 0
    p.threshold, p.global_decay, p.source_decay = threshold, gdecay, sdecay
    p.retain_stats_ns, p.quiet_ns = retain, quiet
    for t, w in (weights or {}).items():
        p.topic_delivery_weight[t] = w
    m = gm.Params(threshold, gdecay, sdecay, retain_stats=retain, quiet=quiet, topic_delivery_weights=weights)
    return p, m


def scored_engine(T, row_ptr, col, ef, ips, present=None, app=None):
    """An engine with the scorer set up so that a present pair's score is its app score."""
    e = gsx.Engine(T, device=0)
    pp = synth.bench_peer_params()
    pp.ip_colocation_factor_weight = 0.0
    e.set_peer_params(pp)
    for t in range(T):
        e.set_topic_params(t, synth.spam_test_topic_params())
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=GRAYLIST,
                                    accept_px_threshold=0, opportunistic_graft_threshold=0))
    e.load_overlay(row_ptr, col, ef, ips)
    E = e.n_pairs
    present = np.ones(E, dtype=bool) if present is None else present
    e.apply_events(np.array([(abi.EV_ADD_PEER, 0, int(p), T0, 0) for p in np.nonzero(present)[0]],
                            dtype=abi.event_dtype()))
    e.set_app_scores(np.zeros(E) if app is None else app)
    return e


class Mirror:
    """Drives the engine's gater and one model gater per observer with the same calls."""

    def __init__(self, eng, row_ptr, col, ef, node_ips, present, gp, mp, seed):
        self.e, self.col, self.ef, self.present, self.seed = eng, np.asarray(col), np.asarray(ef), present, seed
        self.n = len(row_ptr) - 1
        self.E = len(col)
        self.obs = np.repeat(np.arange(self.n), np.diff(row_ptr))
        self.ips = np.asarray(node_ips, dtype=np.uint32).reshape(-1, 2)[self.col].copy()  # per pair
        self.pair_of = {(int(self.obs[p]), int(self.col[p])): p for p in range(self.E)}
        self.models = [gm.PeerGater(mp, (lambda v, u=u: self.ip_name(self.pair_of[(u, v)]))) for u in range(self.n)]
        self.gid = {}        # (observer, ip name) -> the engine's group id, learnt at binding
        self.bound_key = {}  # pair -> (observer, ip name) it is bound to
        self.draw = 0
        self.seen = set()
        eng.set_gater_params(gp)

    def ip_name(self, p):
        for k in (0, 1):
            if self.ips[p, k] != NO_IP:
                return str(int(self.ips[p, k]))
        return "<unknown>"

    def events(self, evs):
        """evs: (kind, topic, pair, now, reason).  A pair-level event of an unbound pair goes to
        the engine only: it must be ignored there (gsx.h), and a router never issues one."""
        self.e.gater_events(np.array([(k, t, p, now, r, 0) for k, t, p, now, r in evs], dtype=abi.gater_event_dtype()))
        new = []
        for k, t, p, now, r in evs:
            u, v = int(self.obs[p]), int(self.col[p])
            m = self.models[u]
            bound = p in self.bound_key
            if k == abi.GATER_VALIDATE:
                m.validate_message()
            elif k == abi.GATER_REJECT and r in (6, 7):
                m.reject_message(v, REASONS[r], now)
            elif k == abi.GATER_ADD_PEER:
                if not bound:
                    self.bound_key[p] = (u, self.ip_name(p))
                    new.append(p)
                m.add_peer(v)
            elif not bound:
                continue
            elif k == abi.GATER_REMOVE_PEER:
                m.remove_peer(v, now)
                del self.bound_key[p]
            elif k == abi.GATER_DELIVER:
                m.deliver_message(v, t)
            elif k == abi.GATER_DUPLICATE:
                m.duplicate_message(v)
            else:
                m.reject_message(v, REASONS[r], now)
        return new

    def check_export(self, new=()):
        x = self.e.gater_export()
        for p in new:  # learn the group of a fresh binding: peers of one (observer, IP) must share it
            g = int(x["bound_group"][p])
            assert g != abi.GSX_GATER_UNBOUND
            assert self.gid.setdefault(self.bound_key[p], g) == g
        assert len(set(self.gid.values())) == len(self.gid)
        n, G = self.n, len(x["connected"])
        want = {k: np.zeros_like(v) for k, v in x.items()}
        want["bound_group"][:] = abi.GSX_GATER_UNBOUND
        for p, key in self.bound_key.items():
            want["bound_group"][p] = self.gid[key]
        for u, m in enumerate(self.models):
            want["validate"][u], want["throttle"][u] = m.validate, m.throttle
            want["last_throttle_ns"][u] = abi.GSX_GATER_NEVER if m.last_throttle is None else m.last_throttle
            assert set(m.peer_stats) == {int(self.col[p]) for p, k in self.bound_key.items() if k[0] == u}
        for (u, ip), g in self.gid.items():
            assert g < G and (g == u if ip == "<unknown>" else g >= n)
            st = self.models[u].ip_stats.get(ip)
            if st is not None:
                want["connected"][g], want["expire_ns"][g] = st.connected, st.expire
                want["deliver"][g], want["duplicate"][g] = st.deliver, st.duplicate
                want["ignore"][g], want["reject"][g] = st.ignore, st.reject
        for k in x:
            a, b = x[k], want[k]
            if a.dtype == np.float64:
                a, b = a.view(np.uint64), b.view(np.uint64)
            assert np.array_equal(a, b), (k, np.nonzero(a != b)[0][:8])
        return x

    def expected_status(self, pairs, now, draw, scores):
        out = np.empty(len(pairs), dtype=np.uint8)
        for i, p in enumerate(pairs):
            p = int(p)
            if self.ef[p] & abi.GSX_EDGE_DIRECT:
                out[i] = gm.ACCEPT_ALL
            elif scores[p] < GRAYLIST:
                out[i] = gm.ACCEPT_NONE
            elif not self.present[p] or p not in self.bound_key:
                out[i] = gm.ACCEPT_ALL
            else:
                out[i] = self.models[int(self.obs[p])].accept_from(int(self.col[p]), now,
                                                                  gm.canonical_u(self.seed, p, draw))
        return out

    def accept(self, now, pairs=None):
        draw, self.draw = self.draw, self.draw + 1
        got = self.e.accept_from(now, self.seed, draw, pairs)
        want = self.expected_status(np.arange(self.E) if pairs is None else pairs, now, draw, self.e.scores())
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        self.seen |= set(int(s) for s in got)
        return got


def test_kat_TestPeerGater_through_the_abi(gpu_ok):
    """peer_gater_test.go:11-128 on pair 0 of a two-node overlay."""
    row_ptr, col = [0, 1, 2], [1, 0]
    ips = np.array([[7, NO_IP], [1234, NO_IP]], dtype=np.uint32)  # peerA = node 1 on "1.2.3.4"
    ef = np.full(2, abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8)
    e = scored_engine(1, row_ptr, col, ef, ips)
    gp, mp = gater_params(0.1, 0.9, 0.999, retain=6 * abi.HOUR, quiet=abi.MINUTE)  # NewPeerGaterParams(.1, .9, .999)
    assert gsx.load_library().gsx_validate_gater_params(C.byref(gp)) == 0
    mr = Mirror(e, row_ptr, col, ef, ips, np.ones(2, dtype=bool), gp, mp, seed=0x9A7E5)
    now = T0
    A = [0]

    def ev(kind, reason=0):
        mr.check_export(mr.events([(kind, 0, 0, now, reason)]))

    ev(abi.GATER_ADD_PEER)
    assert mr.accept(now, A)[0] == gm.ACCEPT_ALL
    ev(abi.GATER_VALIDATE)
    assert mr.accept(now, A)[0] == gm.ACCEPT_ALL
    ev(abi.GATER_REJECT, abi.REJECT_REASONS["validation queue full"])
    assert mr.accept(now, A)[0] == gm.ACCEPT_ALL
    ev(abi.GATER_REJECT, abi.REJECT_REASONS["validation throttled"])
    assert mr.accept(now, A)[0] == gm.ACCEPT_ALL
    def accept_checked():
        st = mr.accept(now, A)[0]
        mr.check_export()
        return st

    for _ in range(100):
        ev(abi.GATER_REJECT, abi.REJECT_REASONS["validation ignored"])
        ev(abi.GATER_REJECT, abi.REJECT_REASONS["validation failed"])
    assert any(accept_checked() == gm.ACCEPT_CONTROL for _ in range(1000))
    for _ in range(100):
        ev(abi.GATER_DELIVER)
    assert any(accept_checked() == gm.ACCEPT_ALL for _ in range(1000))
    for _ in range(100):
        now += S
        e.gater_decay(now)
        mr.models[0].decay_stats(now)
        mr.check_export()
    x = mr.check_export()
    assert x["throttle"][0] == 0.0
    assert mr.accept(now, A)[0] == gm.ACCEPT_ALL
    assert mr.accept(now)[0] == gm.ACCEPT_ALL  # (the full set as well)
    ev(abi.GATER_REMOVE_PEER)
    x = mr.check_export()
    g = mr.gid[(0, "1234")]
    assert x["bound_group"][0] == abi.GSX_GATER_UNBOUND  # no stat record for peerA ...
    assert x["connected"][g] == 0 and x["reject"][g] > 0  # ... but still one for its IP
    now += 6 * abi.HOUR + 2 * S  # past the retention (the reference's test moves expire instead)
    e.gater_decay(now)
    mr.models[0].decay_stats(now)
    x = mr.check_export()
    assert "1234" not in mr.models[0].ip_stats and x["reject"][g] == 0 and x["deliver"][g] == 0
    e.close()


def random_overlay(seed):
    """70 nodes of degree ~6; IPs so that some observers see 3-5 peers on one IP, some peers have none."""
    ov = synth.connect_some_overlay(70, d=3, seed=seed)
    rng = np.random.default_rng(seed)
    ips = np.full((70, 2), NO_IP, dtype=np.uint32)
    ips[:, 0] = 100 + np.arange(70)
    ips[:, 1] = np.where(rng.random(70) < 0.3, 500 + np.arange(70), NO_IP)  # (an IPv6 /64 beside the address)
    ips[rng.random(70) < 0.12] = NO_IP
    hub = int(np.argmax(np.diff(ov.row_ptr)))
    nb = ov.col[ov.row_ptr[hub]:ov.row_ptr[hub + 1]]
    ips[nb[:5], 0] = 900  # the hub sees five peers on one IP ...
    ips[nb[5:8], 0] = 901  # ... and three on another
    ef = ov.edge_flags.copy()
    ef[rng.random(len(ef)) < 0.06] |= abi.GSX_EDGE_DIRECT
    return ov, ips, ef, hub


def test_random_call_sequences(gpu_ok):
    seed = 11
    ov, ips, ef, hub = random_overlay(seed)
    rng = np.random.default_rng(seed + 1)
    E = ov.n_pairs
    assert E > 128 and E % 64 != 0  # more than one 64-pair tile, ragged last tile
    obs = ov.pair_observer()
    cnt = {}
    for p in range(E):
        cnt[(obs[p], ips[ov.col[p], 0])] = cnt.get((obs[p], ips[ov.col[p], 0]), 0) + 1
    assert any(3 <= c <= 5 for (u, ip), c in cnt.items() if ip != NO_IP)
    assert any(ips[ov.col[p], 0] == NO_IP and ips[ov.col[p], 1] == NO_IP for p in range(E))
    present = rng.random(E) > 0.05
    app = np.where(rng.random(E) < 0.1, -500.0, 0.0)
    e = scored_engine(3, ov.row_ptr, ov.col, ef, ips, present, app)
    gp, mp = gater_params(weights={1: 0.3})
    mr = Mirror(e, ov.row_ptr, ov.col, ef, ips, present, gp, mp, seed=77)
    busy = np.concatenate([[hub], rng.choice(70, 11, replace=False)])
    busy_pairs = np.nonzero(np.isin(obs, busy))[0]
    now = T0
    groups0 = e.gater_num_groups()
    mr.check_export(mr.events([(abi.GATER_ADD_PEER, 0, int(p), now, 0) for p in np.nonzero(rng.random(E) < 0.8)[0]]))
    deleted = kept_undecayed = moved = 0
    was_hot, quiet_again = set(), set()
    kinds = [abi.GATER_ADD_PEER, abi.GATER_REMOVE_PEER, abi.GATER_VALIDATE, abi.GATER_DELIVER, abi.GATER_DUPLICATE,
             abi.GATER_REJECT]
    for step in range(400):
        now += int(rng.integers(2, 30)) * S // 10
        r = rng.random()
        new = ()
        if r < 0.45:  # a batch of events of every kind and every reject reason
            evs = []
            for _ in range(int(rng.integers(1, 40))):
                p = int(rng.choice(busy_pairs) if rng.random() < 0.8 else rng.integers(E))
                k = int(rng.choice(kinds, p=[0.1, 0.1, 0.2, 0.2, 0.1, 0.3]))
                if k == abi.GATER_ADD_PEER and p in mr.bound_key and rng.random() < 0.9:
                    k = abi.GATER_VALIDATE  # (a second AddPeer of a bound peer only now and then)
                if k == abi.GATER_REMOVE_PEER and p not in mr.bound_key:
                    k = abi.GATER_DUPLICATE  # (bound in this very batch: the check below learns its group first)
                reason = int(rng.integers(0, 11)) if rng.random() < 0.6 else int(rng.choice([6, 7, 8, 9]))
                evs.append((k, int(rng.integers(3)), p, now, reason))
            new = mr.events(evs)
        elif r < 0.65:
            before = [{ip: (st.connected, st.deliver, st.duplicate, st.ignore, st.reject) for ip, st in m.ip_stats.items()}
                      for m in mr.models]
            e.gater_decay(now)
            for u, m in enumerate(mr.models):
                m.decay_stats(now)
                for ip, (c, *vals) in before[u].items():
                    if c == 0 and ip not in m.ip_stats:
                        deleted += 1
                    elif c == 0 and any(vals):
                        st = m.ip_stats[ip]
                        assert (st.deliver, st.duplicate, st.ignore, st.reject) == tuple(vals)
                        kept_undecayed += 1
        elif r < 0.72 and mr.bound_key:  # an IP move of a bound pair: it stays bound to its old group
            p = int(rng.choice(sorted(mr.bound_key)))
            new_ip = int(rng.choice([900, 901, 2000 + step, NO_IP]))
            mr.ips[p] = (new_ip, NO_IP)
            e.set_pair_ips([p], [[new_ip, NO_IP]])
            moved += 1
        elif r < 0.86:
            mr.accept(now)
            for u, m in enumerate(mr.models):
                quiet = m.last_throttle is None or now - m.last_throttle > mp.quiet
                if not quiet:
                    was_hot.add(u)
                elif u in was_hot:
                    quiet_again.add(u)
        else:
            mr.accept(now, rng.integers(0, E, int(rng.integers(1, 100))))
        mr.check_export(new)
    assert mr.seen == {gm.ACCEPT_NONE, gm.ACCEPT_CONTROL, gm.ACCEPT_ALL}
    assert deleted > 0 and kept_undecayed > 0 and quiet_again and moved > 0
    assert e.gater_num_groups() > groups0  # an IP move brought an observer a new IP
    assert any(ip == "<unknown>" for _, ip in mr.gid)
    e.close()


def test_stage_order(gpu_ok):
    """direct beats graylist beats the gate; without a gater the statuses follow the scores alone."""
    row_ptr, col = [0, 3, 4, 5, 6], [1, 2, 3, 0, 0, 0]
    ips = np.array([[1, NO_IP], [2, NO_IP], [3, NO_IP], [4, NO_IP]], dtype=np.uint32)
    ef = np.full(6, abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8)
    ef[0] |= abi.GSX_EDGE_DIRECT
    app = np.array([-500.0, -500.0, 0.0, 0.0, 0.0, 0.0])
    e = scored_engine(1, row_ptr, col, ef, ips, None, app)
    none_gater = e.accept_from(T0, 1, 0)
    assert none_gater.tolist() == [2, 0, 2, 2, 2, 2]
    assert np.array_equal(none_gater == 0, (e.scores() < GRAYLIST) & ((ef & abi.GSX_EDGE_DIRECT) == 0))
    gp, mp = gater_params()
    mr = Mirror(e, row_ptr, col, ef, ips, np.ones(6, dtype=bool), gp, mp, seed=5)
    bad = [(abi.GATER_ADD_PEER, 0, p, T0, 0) for p in range(3)]
    bad += [(abi.GATER_REJECT, 0, 0, T0, 7)] * 4  # the observer throttles: the gate is on
    bad += [(abi.GATER_REJECT, 0, p, T0, 8) for p in range(3) for _ in range(200)]  # every group is bad
    mr.check_export(mr.events(bad))
    got = [mr.accept(T0 + S) for _ in range(8)]
    assert all(g[0] == gm.ACCEPT_ALL for g in got)      # direct, graylisted score, bad group
    assert all(g[1] == gm.ACCEPT_NONE for g in got)     # graylisted, whatever the gate says
    assert any(g[2] == gm.ACCEPT_CONTROL for g in got)  # the gate alone
    e.set_gater_params(None)
    assert np.array_equal(e.accept_from(T0 + S, 5, 0), none_gater)
    e.close()


# ---- gsx_gater_fold_prop ----------------------------------------------------------------
N_FOLD = 200
BIG = float(2 ** 53 - 2)


@pytest.fixture(scope="module", params=[abi.GSX_ROUTER_GOSSIPSUB, abi.GSX_ROUTER_FLOODSUB], ids=["gossipsub", "floodsub"])
def fold_world(request, gpu_ok):
    ov = pc.overlay(N_FOLD, 6, seed=31, mix_protocols=True)
    rng = np.random.default_rng(5)
    ov.node_ips = np.asarray(ov.node_ips, dtype=np.uint32).reshape(-1, 2).copy()
    ov.node_ips[:, 0] = rng.integers(0, 60, N_FOLD)  # shared IPs: several pairs of an observer in one group
    ov.node_ips[rng.random(N_FOLD) < 0.1] = NO_IP
    eng, ora = gsx.Engine(3, device=0), orc.Oracle(3)
    for be in (eng, ora):
        pc.setup(be, ov, 3, seed=31)
    ora.set_dup_tracking(True)
    yield request.param, ov, eng, ora
    eng.close()


def fold_messages(m, seed):
    ms = pc.messages(N_FOLD, m, seed)
    ms["validation"] = (np.arange(m) + seed) % 4 if m > 1 else seed % 4  # all four outcomes
    return ms


@pytest.mark.parametrize("topic", [0, 1], ids=["w1", "w0.3"])
@pytest.mark.parametrize("m", [1, 64, 65, 130])
def test_fold_prop_equals_the_model_fed_from_the_oracle(fold_world, m, topic):
    router, ov, eng, ora = fold_world
    E = ov.n_pairs
    ef = np.asarray(ov.edge_flags)
    gp, mp = gater_params(weights={1: 0.3, 2: BIG})
    ms = fold_messages(m, seed=m + topic)
    cfg = pc.config(router, topic=topic, credit=0)
    _, _, frm = ora.propagate(ms, cfg, want_results=True)
    dup = ora.prop_duplicates(m)
    eng.propagate(ms, cfg)
    # the pair whose group starts above 2^53 - 2: one that gets an ACCEPT first receipt, if any
    bp = 0
    acc = np.nonzero(ms["validation"] == abi.GSX_VALIDATION_ACCEPT)[0]
    if len(acc) and (frm[acc[0]] >= 0).any():
        u0 = int(np.nonzero(frm[acc[0]] >= 0)[0][0])
        bp = {(int(o), int(c)): q for q, (o, c) in enumerate(zip(ov.pair_observer(), ov.col))}[(u0, int(frm[acc[0], u0]))]
    exports = []
    for run in range(2):
        mr = Mirror(eng, ov.row_ptr, ov.col, ef, ov.node_ips, np.ones(E, dtype=bool), gp, mp, seed=3)
        rng = np.random.default_rng(9)
        bound = np.union1d(np.nonzero(rng.random(E) < 0.9)[0], [bp])
        new = mr.events([(abi.GATER_ADD_PEER, 0, int(p), T0, 0) for p in bound])
        pre = [(int(rng.choice([abi.GATER_DELIVER, abi.GATER_DUPLICATE, abi.GATER_VALIDATE])), int(rng.integers(2)),
                int(rng.integers(E)), T0, 0) for _ in range(600)]
        pre += [(abi.GATER_REJECT, 0, int(rng.integers(E)), T0, int(rng.choice([7, 8, 9]))) for _ in range(300)]
        mr.events(pre)
        eng.gater_decay(T0 + S)  # fractional starting values
        for mdl in mr.models:
            mdl.decay_stats(T0 + S)
        mr.events([(abi.GATER_DELIVER, 2, bp, T0 + S, 0)])  # one group above 2^53 - 2: its +1 steps round
        mr.check_export(new)
        eng.gater_fold_prop()
        # the model, event by event from the oracle's results
        for k in range(m):
            for u in np.nonzero(frm[k] >= 0)[0]:
                u, v = int(u), int(frm[k, u])
                p = mr.pair_of[(u, v)]
                mdl = mr.models[u]
                mdl.validate_message()
                val = int(ms["validation"][k])
                if val == abi.GSX_VALIDATION_THROTTLE:
                    mdl.reject_message(v, gm.REJECT_THROTTLED, cfg.now_ns)
                elif p not in mr.bound_key:
                    continue
                elif val == abi.GSX_VALIDATION_ACCEPT:
                    mdl.deliver_message(v, topic)
                else:
                    mdl.reject_message(v, gm.REJECT_FAILED if val == abi.GSX_VALIDATION_REJECT else gm.REJECT_IGNORED,
                                       cfg.now_ns)
        for p in np.nonzero(dup.any(axis=1))[0]:
            if int(p) in mr.bound_key:
                for _ in range(sum(bin(int(w)).count("1") for w in dup[p])):
                    mr.models[int(mr.obs[p])].duplicate_message(int(ov.col[p]))
        x = mr.check_export()
        exports.append(x)
        assert x["deliver"][mr.gid[mr.bound_key[bp]]] >= BIG
    assert (frm >= 0).sum() > 0
    for k in exports[0]:
        assert np.array_equal(exports[0][k].view(np.uint8), exports[1][k].view(np.uint8)), k


# ---- gsx_gater_enforce --------------------------------------------------------------------
def test_enforcement_equals_the_oracle_with_the_throttled_pairs_graylisted(gpu_ok):
    """Every edge gossipsub, no direct peer, no flood publish, no credits: a pair's score decides
    nothing but AcceptFrom, so the oracle with exactly the throttled pairs pushed below
    GraylistThreshold by their app score is the reference of an enforced call."""
    n = 200
    ov = pc.overlay(n, 6, seed=41)
    assert ((ov.edge_flags & abi.GSX_EDGE_GOSSIPSUB) != 0).all() and not (ov.edge_flags & abi.GSX_EDGE_DIRECT).any()
    eng, ora = gsx.Engine(1, device=0), orc.Oracle(1)
    for be in (eng, ora):
        pc.setup(be, ov, 1, seed=41, score_spread=False)
    E = ov.n_pairs
    rng = np.random.default_rng(41)
    gp, _ = gater_params(quiet=abi.HOUR)
    eng.set_gater_params(gp)
    dt = abi.gater_event_dtype()
    ev = [(abi.GATER_ADD_PEER, 0, p, pc.T0, 0, 0) for p in range(E)]
    ev += [(abi.GATER_REJECT, 0, int(ov.row_ptr[u]), pc.T0, 7, 0) for u in range(n) if ov.row_ptr[u] < ov.row_ptr[u + 1]]
    ev += [(abi.GATER_REJECT, 0, int(p), pc.T0, 8, 0) for p in np.nonzero(rng.random(E) < 0.3)[0]]
    eng.gater_events(np.array(ev, dtype=dt))
    connected = (eng.export_state()["pair_flags"] & abi.GSX_PAIR_CONNECTED) != 0
    now = pc.T0 + 3 * S

    def cfg():
        return pc.config(abi.GSX_ROUTER_GOSSIPSUB, credit=0, flood_publish=0)

    def run(be, ms):
        out, hop, frm = be.propagate(ms, cfg(), want_results=True)
        return out, hop, frm

    def same(a, b):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        for f in ("deliveries", "duplicates", "graylisted"):
            assert getattr(a[0], f) == getattr(b[0], f), f

    msgs = {m: pc.messages(n, m, seed=41 + m) for m in (1, 65, 130)}
    plain = {m: run(ora, ms) for m, ms in msgs.items()}  # the unmodified oracle
    decisions = []
    for draw in (0, 1):  # the second round: the same engine after a DIFFERENT decision set (incremental pins)
        st = eng.accept_from(now, 9, draw)
        decisions.append(st.copy())
        throttled = st == gm.ACCEPT_CONTROL
        assert not (st == gm.ACCEPT_NONE).any()
        share = throttled[connected].mean()
        assert 0.05 <= share <= 0.60, share
        assert eng.gater_gate_pairs() == (0, int(throttled.sum()))
        eng.gater_enforce(True)
        ora.set_app_scores(np.where(throttled, -1000.0, 0.0))
        for m, ms in msgs.items():
            got, want = run(eng, ms), run(ora, ms)
            same(got, want)
            assert got[0].graylisted > 0 or m == 1
            if m > 1:  # the gate changes what is delivered
                assert got[0].deliveries != plain[m][0].deliveries or not np.array_equal(got[1], plain[m][1])
        ora.set_app_scores(np.zeros(E))
    assert not np.array_equal(decisions[0], decisions[1])
    eng.gater_enforce(False)  # off again: the unmodified oracle
    for m, ms in msgs.items():
        same(run(eng, ms), plain[m])
    eng.close()


def test_refusals(gpu_ok):
    lib = gsx.load_library()
    ov = pc.overlay(40, 4, seed=3)
    e = gsx.Engine(1, device=0)
    pc.setup(e, ov, 1, seed=3)
    E = e.n_pairs
    out = np.zeros(E, dtype=np.uint8)
    one = np.array([(abi.GATER_VALIDATE, 0, 0, T0, 0, 0)], dtype=abi.gater_event_dtype())

    def events(a):
        return lib.gsx_gater_events(e.h, a.ctypes.data_as(C.c_void_p), len(a))

    assert events(one) == abi.GSX_ESTATE  # no gater yet
    assert lib.gsx_gater_decay(e.h, T0) == abi.GSX_ESTATE
    assert lib.gsx_gater_fold_prop(e.h) == abi.GSX_ESTATE
    gp, _ = gater_params()
    e.set_gater_params(gp)
    assert lib.gsx_gater_fold_prop(e.h) == abi.GSX_ESTATE  # no propagation yet
    assert lib.gsx_gater_enforce(e.h, 1) == abi.GSX_ESTATE  # no decision set
    assert lib.gsx_gater_gate_pairs(e.h, None, None) == abi.GSX_ESTATE
    e.accept_from(T0, 1, 0, [0, 1])  # (a listed call leaves none either)
    assert lib.gsx_gater_enforce(e.h, 1) == abi.GSX_ESTATE
    assert lib.gsx_gater_enforce(e.h, 0) == 0
    assert lib.gsx_gater_enforce(None, 1) == abi.GSX_EINVAL
    e.accept_from(T0, 1, 0)
    assert lib.gsx_gater_enforce(e.h, 1) == 0
    e.set_gater_params(gp)  # a decision set belongs to the gater it was computed under
    assert lib.gsx_gater_enforce(e.h, 1) == abi.GSX_ESTATE
    # NULL arguments
    assert lib.gsx_accept_from(e.h, None, E, T0, 1, 0, None) == abi.GSX_EINVAL
    assert lib.gsx_accept_from(None, None, E, T0, 1, 0, out.ctypes.data_as(C.c_void_p)) == abi.GSX_EINVAL
    assert lib.gsx_gater_events(e.h, None, 1) == abi.GSX_EINVAL
    assert lib.gsx_gater_export(e.h, None) == abi.GSX_EINVAL
    assert lib.gsx_gater_num_groups(e.h, None) == abi.GSX_EINVAL
    assert lib.gsx_set_gater_params(None, C.byref(gp)) == abi.GSX_EINVAL
    # a pair out of range, a short full set
    bad = np.array([E], dtype=np.uint64)
    assert lib.gsx_accept_from(e.h, bad.ctypes.data_as(C.c_void_p), 1, T0, 1, 0, out.ctypes.data_as(C.c_void_p)) == abi.GSX_EINVAL
    assert lib.gsx_accept_from(e.h, None, E - 1, T0, 1, 0, out.ctypes.data_as(C.c_void_p)) == abi.GSX_EINVAL
    for kind, pair, reason in ((abi.GATER_VALIDATE, E, 0), (0, 0, 0), (7, 0, 0), (abi.GATER_REJECT, 0, 11),
                               (abi.GATER_REJECT, 0, -1)):
        one[0] = (kind, 0, pair, T0, reason, 0)
        assert events(one) == abi.GSX_EINVAL, (kind, pair, reason)
    x = e.gater_export()
    assert not x["validate"].any() and (x["bound_group"] == abi.GSX_GATER_UNBOUND).all()  # nothing was applied
    # the fold needs the first-deliverer rows of the call it folds
    ms = pc.messages(40, 10, seed=3)
    e.set_prop_tracking(False)
    e.propagate(ms, pc.config(abi.GSX_ROUTER_GOSSIPSUB, credit=0))
    assert lib.gsx_gater_fold_prop(e.h) == abi.GSX_ESTATE
    e.set_prop_tracking(True)
    e.propagate(ms, pc.config(abi.GSX_ROUTER_GOSSIPSUB, credit=0))
    assert lib.gsx_gater_fold_prop(e.h) == 0
    e.close()
    # a range shard keeps gater state but folds nothing
    sh = gsx.Engine(1, device=0)
    sh.set_peer_params(synth.bench_peer_params())
    sh.set_topic_params(0, synth.spam_test_topic_params())
    lo, hi = 0, 20
    rp = (ov.row_ptr[lo:hi + 1] - ov.row_ptr[lo]).astype(np.int64)
    sh.load_overlay_shard(40, lo, rp, ov.col[ov.row_ptr[lo]:ov.row_ptr[hi]], ov.edge_flags[ov.row_ptr[lo]:ov.row_ptr[hi]],
                          ov.node_ips)
    sh.set_gater_params(gp)
    assert lib.gsx_gater_fold_prop(sh.h) == abi.GSX_ESTATE
    sh.accept_from(T0, 1, 0)  # the decision itself works on a shard; enforcing it does not
    assert lib.gsx_gater_enforce(sh.h, 1) == abi.GSX_ESTATE
    sh.close()

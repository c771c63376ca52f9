"""Every topic-indexed GPU path above 8 topics, up to GSX_MAX_TOPICS = 64, against
the CPU oracle, bit for bit (tests/test_many_topics_oracle.py pins the oracle
itself at these topic counts, and shows on the oracle alone that every scenario
reaches what it is for).

T = 9: one topic in k_hb_scan's second group of eight and in the second backoff
presence chunk (nt = 1); 16: two full groups; 33: bit 32 of the topic masks,
nt = 1 in the fifth group, an odd T for the zero map's aligned 32-bit reads;
64: bit 63, a full kc[3][64] in the gossip exchange's forwarding, eight groups,
the generic refresh+score kernel at its widest."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported on the main thread before the shard threads use it)

import gossip_cases as gc
import gsx
import many_topics_cases as M
import oracle as orc
import propagation_cases as pc
import randomized as R
import score_stats_cases as ssc
from gsx import abi, shard, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND
T0 = pc.T0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_state(got, want, where):
    for f in abi.STATE_FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert np.array_equal(bits(g), bits(w)), (where, f, np.nonzero(g != w)[0][:5].tolist())


def same_scores(eng, ora, where):
    g, w = eng.scores(), ora.scores()
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (where, np.nonzero(g != w)[0][:8].tolist())


# ---- (a) scoring ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [16, 33, 64])
def test_random_scoring_calls_match_oracle(gpu_ok, T):
    """The generic refresh+score kernel (launch_rs: T not in {1, 2, 4, 8}) with every
    topic but the last scored: KernParams.tp[t] and the zero map's offsets up to t = 62."""
    ov = R.small_overlay(300, 3, T, 50)
    ops = R.make_ops(ov, T, T, n_steps=300)
    assert {t for op in ops if op[0] == "events" for _, t, _, _, _ in op[1]} >= set(range(8, T))
    got = R.replay(gsx.Engine(T), ov, T, ops)
    want = R.replay(orc.Oracle(T), ov, T, ops)
    assert len(got) == len(want) > 5
    for i, ((gs, gst, gn), (ws, wst, wn)) in enumerate(zip(got, want)):
        assert gn == wn, f"check {i}: delivery records {gn} vs {wn}"
        assert np.array_equal(gs.view(np.uint64), ws.view(np.uint64)), f"check {i}: scores"
        same_state(gst, wst, f"check {i}")
    last = want[-1][1]
    E = ov.n_pairs
    for f in M.COUNTERS:  # the high topics' counters were in play
        assert any(np.asarray(st[f]).reshape(T, E)[8:].any() for _, st, _ in want), f
    assert (np.asarray(last["rec_flags"]).reshape(T, E)[T - 2] & abi.GSX_REC_IN_MESH).any()


def test_lazy_decay_and_zero_map_at_33_topics(gpu_ok):
    """test_gpu_lazy_decay.test_param_setters_mid_phase at T = 33 from a state whose
    pairs are all present and whose MFP and IMD are zero (test_gpu_zero_map's), with
    invalid deliveries on topics 8 and 32: the zero map's entries tile * T * 2 + 2 t + 1
    of an odd T are marked, and cleared once the counters have decayed to zero;
    engine == oracle and the map's invariant after every call."""
    import test_gpu_lazy_decay as ld
    import test_gpu_zero_map as zm

    T = 33

    def decays(tp):
        for f in ("first_message", "mesh_message"):
            setattr(tp, f + "_deliveries_decay", 0.3)
        tp.mesh_failure_penalty_decay = tp.invalid_message_deliveries_decay = 0.3

    ov, st, eng, ora = zm.backends(T, tp_edit=decays)
    for be in (eng, ora):
        be.set_peer_params(ld.peer_params(dtz=0.5))
    assert eng.zero_map_marked() == 0 and eng.zero_map_violations() == 0
    E = ov.n_pairs
    pairs = [5, 64 + 7, 64 * 3 + 5]  # three tiles, none of them the ragged last one
    assert (st["pair_flags"][pairs] == (abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED)).all() and E > 64 * 5
    ck = ld.Clock(eng, ora)
    for ph in (1, 2, 3):
        ld.events((eng, ora), [(abi.EV_INVALID_DELIVERY, t, p, ck.now, 0) for t in (8, 32) for p in pairs] * 6)
        ld.same(eng, ora, f"invalid deliveries {ph}")
        assert eng.zero_map_marked() == 6, ph  # the IMD entries of (3 tiles) x (topics 8 and 32)
        ck.refresh(f"setters, start {ph}", ph)
        tp = ld.topic_params(0.6 + 0.1 * ph)
        tp.first_message_deliveries_cap = 40.0 / ph
        tp.mesh_message_deliveries_cap = 30.0 / ph
        for be in (eng, ora):
            be.set_topic_params(T - 1, tp)
        ld.same(eng, ora, f"set_topic_params after {ph}")
        ck.refresh(f"after set_topic_params {ph}", ph)
        for be in (eng, ora):
            be.set_peer_params(ld.peer_params(dtz=0.5 / ph))
        ld.same(eng, ora, f"set_peer_params after {ph}")
        ck.refresh(f"after set_peer_params {ph}", 5)
        ld.events((eng, ora), [(abi.EV_FIRST_DELIVERY, T - 1, p, ck.now, 0) for p in range(0, E, 3)] * 30)
        ld.same(eng, ora, f"deliveries {ph}")
        for _ in range(40):  # IMD 6 under decays 0.3 (topic 8) and up to 0.9 (topic 32) down to DecayToZero
            if not ora.export_state()["invalid_message_deliveries"].any():
                break
            ck.refresh(f"decaying {ph}")
        assert not ora.export_state()["invalid_message_deliveries"].any()
        ck.refresh(f"all zero {ph}", 4)  # a whole write-back cycle later at the latest the map says zero again
        assert eng.zero_map_marked() == 0, ph


# ---- relabelling: Engine(64) on topic k == Engine(1), with no oracle in between --------------
@pytest.fixture(scope="module")
def scoring_world(gpu_ok):
    ov = R.small_overlay(300, 3, 5, 50)
    ops = R.make_ops(ov, 1, 5, n_steps=300)
    want = M.one_topic_replay(gsx.Engine(1), ov, 1, 0, ops)
    assert M.counters_seen(want)
    return ov, ops, want


@pytest.mark.parametrize("k", M.RELABEL_TOPICS)
def test_engine_scoring_on_topic_k_of_64_equals_the_one_topic_engine(scoring_world, k):
    ov, ops, want = scoring_world
    got = M.one_topic_replay(gsx.Engine(64), ov, 64, k, ops)
    M.assert_relabelled(got, want, 64, k, ov.n_pairs)


@pytest.mark.parametrize("router", [abi.GSX_ROUTER_GOSSIPSUB, abi.GSX_ROUTER_FLOODSUB], ids=["gossipsub", "floodsub"])
def test_engine_credited_propagation_on_topic_k_of_64_equals_the_one_topic_engine(gpu_ok, router):
    want = M.prop_relabel_run(gsx.Engine(1), 1, 0, router)
    for k in M.RELABEL_TOPICS:
        M.assert_prop_relabelled(M.prop_relabel_run(gsx.Engine(64), 64, k, router), want, k)


# ---- (b) heartbeat -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hb_world(gpu_ok):
    """One engine and one oracle run per case, kept for the score-stats test."""
    runs = {}

    def world(case):
        if case not in runs:
            eng, ora = gsx.Engine(case[0]), orc.Oracle(case[0])
            runs[case] = (eng, ora, M.hb_run(eng, case), M.hb_run(ora, case))
        return runs[case]

    yield world
    for eng, ora, _, _ in runs.values():
        eng.close()
        ora.close()


@pytest.mark.parametrize("case", M.HB_CASES, ids=M.hb_id)
def test_heartbeat_rounds_match_oracle(hb_world, case):
    _, _, (_, gpre, go, gs), (ov, wpre, wo, ws) = hb_world(case)
    same_state(gpre, wpre, "before the first round")
    for k in range(M.HB_TICKS):
        assert go[k] == wo[k], (k, {x: (go[k][x], wo[k][x]) for x in go[k] if go[k][x] != wo[k][x]})
        M.same_snapshot(gs[k], ws[k], f"tick {k}")
    M.hb_reach(case, ov, wpre, wo, ws)


def test_heartbeat_hub_nodes_match_oracle_at_9_topics(gpu_ok):
    """hub_work[t] / n_hub[t] for t = 8: nodes of more than 64 peers, one wave each."""
    ov, n = M.hub_overlay()
    go, gs = M.hub_run(gsx.Engine(9), ov, n)
    wo, ws = M.hub_run(orc.Oracle(9), ov, n)
    for k in range(len(wo)):
        assert go[k] == wo[k], (k, go[k], wo[k])
        M.same_snapshot(gs[k], ws[k], f"tick {k}")
    M.hub_reach(ov, 9, wo, ws)


# ---- (f) score stats on the state the heartbeat cases leave --------------------------------
@pytest.mark.parametrize("T,md,topic", [(9, 2, 8), (64, 2, 63), (64, 14, 63), (64, 14, 8)])
def test_score_stats_of_a_high_topics_mesh(hb_world, T, md, topic):
    eng, ora, _, (ov, _, _, _) = hb_world(M.hb_case(T, md))
    st = ora.export_state()
    same_state(eng.export_state(), st, "after the run")
    scores = ora.scores()
    same_scores(eng, ora, "after the run")
    edges = eng.score_stats_edges()
    want = ssc.reference(scores, st["pair_flags"], st["rec_flags"], ov.row_ptr, ov.col, ov.n, edges, "mesh", topic)
    got = eng.score_stats(select="mesh", topic=topic)
    ssc.assert_equal(got, want, what=f"T={T} topic {topic}")
    E = ov.n_pairs
    sel = (st["rec_flags"].reshape(T, E)[topic] & abi.GSX_REC_IN_MESH) != 0
    sel &= st["pair_flags"] == (abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED)
    deg = np.bincount(ov.pair_observer()[sel], minlength=ov.n)
    assert np.array_equal(got.degree(), deg) and deg.sum() > 0


# ---- (c) membership, fanout, PX ------------------------------------------------------------
@pytest.mark.parametrize("T", [33, 64])
def test_membership_matches_oracle(gpu_ok, T):
    _, go, gs, gm, gp = M.member_run(gsx.Engine(T), T)
    ov, wo, ws, wm, wp = M.member_run(orc.Oracle(T), T)
    assert len(go) == len(wo)
    for k, (a, b) in enumerate(zip(go, wo)):
        diff = {x: (a[1][x], b[1][x]) for x in a[1] if a[1][x] != b[1][x]}
        assert a[0] == b[0] and not diff, f"step {k} ({a[0]}): {diff}"
    for k in range(len(ws)):
        M.same_snapshot(gs[k], ws[k], f"tick {k}")
        for name, x, y in zip(("joined", "fanout", "lastpub"), gm[k], wm[k]):
            assert np.array_equal(x, y), (k, name, np.argwhere(x != y)[:5].tolist())
        assert gp[k][0] == wp[k][0], k
        assert np.array_equal(gp[k][1], wp[k][1]), k
    M.member_reach(T, ov, wo, wm)


@pytest.mark.parametrize("T", [33, 64])
def test_px_member_rounds_match_oracle(gpu_ok, T):
    g = M.px_member_run(gsx.Engine(T), T)
    w = M.px_member_run(orc.Oracle(T), T)
    for (go, gr), (wo, wr) in zip(g, w):
        assert go == wo
        assert np.array_equal(gr, wr)
    M.px_member_reach(T, w)


# ---- (d) gossip exchange -------------------------------------------------------------------
@pytest.mark.parametrize("T", sorted(M.GX_CASES))
def test_gossip_exchange_matches_oracle(gpu_ok, T):
    """IWANTs, served, recovered, forwarded (k_gxf's per-topic kc[3][64] rows up to
    t = 63), broken promises and the IHAVEs, on the last topic (and topic 0 at T = 9)."""
    kw = M.GX_CASES[T]
    _, go, gs, gcache = gc.exchange_run(gsx.Engine(T), **kw)
    _, wo, ws, wcache = gc.exchange_run(orc.Oracle(T), **kw)
    for k in range(len(wo)):
        diff = {x: (go[k][x], wo[k][x]) for x in go[k] if go[k][x] != wo[k][x]}
        assert not diff, f"tick {k}: {diff}"
        M.same_snapshot(gs[k], ws[k], f"tick {k}")
    for v, (a, b) in enumerate(zip(gcache, wcache)):
        assert sorted(a.tolist()) == sorted(b.tolist()), v
    M.gx_reach(T, wo, ws)


# ---- (e) propagation credits ---------------------------------------------------------------
@pytest.mark.parametrize("topic", [8, 32])
@pytest.mark.parametrize("mode", ["now", "defer"])
def test_propagation_credits_on_one_of_33_topics(gpu_ok, mode, topic):
    """fold_pair (GSX_CREDIT_NOW) and gsx_prop_fold_credits + settle_scores (GSX_CREDIT_DEFER,
    through the stepped calls) on topic 8 / 32 of 33, batches of 1 and 65 messages."""
    T = M.CREDIT_T
    eng, ora = gsx.Engine(T), orc.Oracle(T)
    ov = M.credit_world(eng)
    M.credit_world(ora)
    E = ov.n_pairs
    for i, (m, ms) in enumerate(M.credit_batches(ov.n)):
        now = T0 + (3 + i) * S
        before = ora.export_state()
        same_state(eng.export_state(), before, f"batch {i}: before")
        want = ora.propagate(ms, M.credit_config(topic, abi.GSX_CREDIT_NOW, now))[0].as_dict()
        if mode == "defer":
            cfg = M.credit_config(topic, abi.GSX_CREDIT_DEFER, now)
            eng.prop_begin(ms, cfg)
            for _ in range(cfg.max_hops):
                eng.prop_step(0)
            got = eng.prop_end().as_dict()
            eng.fold_credits()
            eng.settle_scores()
        else:
            got = eng.propagate(ms, M.credit_config(topic, abi.GSX_CREDIT_NOW, now))[0].as_dict()
        assert got == want, (i, m)
        after = eng.export_state()
        same_state(after, ora.export_state(), f"batch {i} (m = {m})")
        same_scores(eng, ora, f"batch {i} (m = {m})")
        M.credit_reach(T, topic, E, ms, want, before, after)
        for be in (eng, ora):
            be.refresh(now + S // 2)
        same_state(eng.export_state(), ora.export_state(), f"batch {i}: after the refresh")
        same_scores(eng, ora, f"batch {i}: after the refresh")


# ---- (f) gater -----------------------------------------------------------------------------
def test_gater_fold_prop_with_topic_63_weighted(gpu_ok):
    """test_fold_prop_equals_the_model_fed_from_the_oracle's scheme at T = 64:
    topic_delivery_weight[63] = 0.3, a batch on topic 63."""
    import gater_model as gm
    import test_gpu_gater as tg

    T, topic, m, n = 64, 63, 65, tg.N_FOLD
    ov = pc.overlay(n, 6, seed=31, mix_protocols=True)
    rng = np.random.default_rng(5)
    ov.node_ips = np.asarray(ov.node_ips, dtype=np.uint32).reshape(-1, 2).copy()
    ov.node_ips[:, 0] = rng.integers(0, 60, n)
    ov.node_ips[rng.random(n) < 0.1] = tg.NO_IP
    eng, ora = gsx.Engine(T, device=0), orc.Oracle(T)
    for be in (eng, ora):
        pc.setup(be, ov, T, seed=31)
    ora.set_dup_tracking(True)
    E = ov.n_pairs
    ef = np.asarray(ov.edge_flags)
    gp, mp = tg.gater_params(weights={63: 0.3})
    assert gp.topic_delivery_weight[63] == 0.3 and gp.topic_delivery_weight[62] != 0.3
    ms = tg.fold_messages(m, seed=m)
    cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=topic, credit=0)
    _, _, frm = ora.propagate(ms, cfg, want_results=True)
    dup = ora.prop_duplicates(m)
    eng.propagate(ms, cfg)
    mr = tg.Mirror(eng, ov.row_ptr, ov.col, ef, ov.node_ips, np.ones(E, dtype=bool), gp, mp, seed=3)
    rng = np.random.default_rng(9)
    new = mr.events([(abi.GATER_ADD_PEER, 0, int(p), T0, 0) for p in np.nonzero(rng.random(E) < 0.9)[0]])
    pre = [(int(rng.choice([abi.GATER_DELIVER, abi.GATER_DUPLICATE, abi.GATER_VALIDATE])), int(rng.choice([0, 63])),
            int(rng.integers(E)), T0, 0) for _ in range(600)]
    pre += [(abi.GATER_REJECT, 0, int(rng.integers(E)), T0, int(rng.choice([7, 8, 9]))) for _ in range(300)]
    mr.events(pre)
    eng.gater_decay(T0 + S)
    for mdl in mr.models:
        mdl.decay_stats(T0 + S)
    mr.check_export(new)
    eng.gater_fold_prop()
    delivered = 0
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
                delivered += 1
            else:
                mdl.reject_message(v, gm.REJECT_FAILED if val == abi.GSX_VALIDATION_REJECT else gm.REJECT_IGNORED,
                                   cfg.now_ns)
    for p in np.nonzero(dup.any(axis=1))[0]:
        if int(p) in mr.bound_key:
            for _ in range(sum(bin(int(w)).count("1") for w in dup[p])):
                mr.models[int(mr.obs[p])].duplicate_message(int(ov.col[p]))
    x = mr.check_export()
    assert delivered > 100 and x["deliver"].any()  # deliveries weighed with topic_delivery_weight[63]
    eng.close()


# ---- (g) sharded heartbeat -----------------------------------------------------------------
def test_sharded_heartbeat_with_33_topics_matches_single_engine(gpu_ok):
    """Range shards (threads in this process, the local transport), world = 2, T = 33,
    traffic on topic 32: the packed GRAFT / PRUNE control words cross the ranks with
    bit 32 set.  The ranks' states, concatenated, == the unsharded engine's, round
    by round; the unsharded engine == the oracle, whose topic-32 mesh flags show a
    cross-shard GRAFT and PRUNE.  (Join / Leave are refused on a range shard, gsx.h:
    the meshes of topic 32 come from the setup's grafts.)"""
    from test_gpu_shard import _params, _slice_state, _slice_te

    T, n, world, seed = M.SHARD_T, M.SHARD_N, M.SHARD_WORLD, M.SHARD_SEED
    full, ora = gsx.Engine(T), orc.Oracle(T)
    ov, app = M.shard_world(full)
    M.shard_world(ora)
    st0 = full.export_state()
    E = ov.n_pairs
    rank_lo = synth.shard_ranges(n, world)
    engines = []
    for k in range(world):
        lo, hi = int(rank_lo[k]), int(rank_lo[k + 1])
        sh = synth.shard_of(ov, lo, hi)
        a, b = int(ov.row_ptr[lo]), int(ov.row_ptr[hi])
        e = gsx.Engine(T)
        _params(e, T)
        e.load_overlay_shard(n, lo, sh.row_ptr, sh.col, sh.edge_flags, sh.node_ips)
        e.import_state(_slice_state(st0, T, E, a, b))
        e.set_app_scores(app[a:b])
        engines.append((e, a, b))
    runners = shard.run_local(world, "cuda:0", lambda tp, e: shard.RangeSharded(e, rank_lo, tp),
                              [(e,) for e, _, _ in engines])
    wo, wflags, wsnaps = M.shard_rounds(ora, ov)
    for k in range(M.SHARD_ROUNDS):
        tick, now, ms, cfg = M.shard_round_args(k)
        want = full.heartbeat(tick, now, seed).as_dict()
        assert want == wo[k], (k, want, wo[k])
        res = shard.run_local(world, "cuda:0", lambda tp, r: (setattr(r, "tp", tp), r.heartbeat(tick, now, seed))[1],
                              [(r,) for r in runners])
        assert res[0][1] == want, (k, res[0][1], want)
        snap = M.hc.snapshot(full)
        M.same_snapshot(snap, wsnaps[k], f"round {k}: unsharded engine vs oracle")
        for (e, a, b) in engines:
            got = M.hc.snapshot(e)
            for f in abi.STATE_FIELDS:
                w = _slice_state(snap, T, E, a, b)[f]
                assert np.array_equal(got[f].view(np.uint8), w.view(np.uint8)), (k, f)
            for f in ("backoff", "ihave_len", "ihave_digest"):
                assert np.array_equal(np.asarray(got[f]).reshape(-1), _slice_te(snap[f], T, E, a, b)), (k, f)
            assert np.array_equal(got["scores"].view(np.uint64), snap["scores"][a:b].view(np.uint64)), k
        full.propagate(ms, cfg)
        shard.run_local(world, "cuda:0", lambda tp, r: (setattr(r, "tp", tp), r.propagate(ms, cfg))[1],
                        [(r,) for r in runners])
        full.refresh(now + 500 * abi.MILLISECOND)
        for (e, _, _) in engines:
            e.refresh(now + 500 * abi.MILLISECOND)
    M.shard_reach(ov, wflags)

"""Scenarios with more than 8 topics (up to GSX_MAX_TOPICS = 64), driven
identically through any backend, and what each of them must reach: a topic in
the second group of eight (the heartbeat's scan groups, the backoff presence
chunks), bit 32 and bit 63 of the 64-bit topic masks.

The reach checks take the ORACLE's results: tests/test_many_topics_oracle.py
runs them without a GPU, tests/test_gpu_many_topics.py after comparing the
engine with the oracle bit for bit."""
from __future__ import annotations

import numpy as np

import gossip_cases as gc
import heartbeat_cases as hc
import membership_cases as mc
import propagation_cases as pc
import px_cases as xc
import randomized as R
from gsx import abi

S = abi.SECOND
T0 = pc.T0
TOPICS = (9, 16, 33, 64)
SNAP_FIELDS = list(abi.STATE_FIELDS) + ["backoff", "scores", "ihave_len", "ihave_digest"]
COUNTERS = ("first_message_deliveries", "mesh_message_deliveries", "mesh_failure_penalty",
            "invalid_message_deliveries")


def last_group(T):
    """The topics of the last group of eight (k_hb_scan's last pass, the last backoff chunk)."""
    return list(range(8 * ((T - 1) // 8), T))


def bit(words, t):
    return (np.asarray(words, dtype=np.uint64) >> np.uint64(t)) & np.uint64(1) != 0


def same_snapshot(a, b, what):
    for f in SNAP_FIELDS:
        x, y = np.asarray(a[f]), np.asarray(b[f])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, f, np.argwhere(x != y)[:5].tolist())


# ---- scoring: one topic of 64 == the one-topic run ---------------------------------------
RELABEL_TOPICS = (0, 8, 31, 32, 63)


def relabel(ops, k):
    """R.make_ops(ov, 1, ...) with every event, tracer call and parameter reset moved to topic k."""
    out = []
    for op in ops:
        if op[0] == "events":
            out.append(("events", [(kind, k, p, now, arg) for kind, _, p, now, arg in op[1]]))
        elif op[0] == "trace":
            out.append(("trace", [c[:3] + (k,) + c[4:] for c in op[1]]))
        elif op[0] == "topic_params":
            out.append(("topic_params", k, op[2]))
        else:
            out.append(op)
    return out


def one_topic_replay(be, ov, T, k, ops):
    """R.replay with topic k the only scored topic (topic 0's parameters of the two-topic scenario)."""
    return R.replay(be, ov, T, relabel(ops, k), topic_params={k: R.scenario_params(2)[1][0]})


def assert_relabelled(got, want, T, k, E):
    """got: the checks of a T-topic run on topic k; want: those of the one-topic run."""
    assert len(got) == len(want) > 5
    for i, ((gs, gst, gn), (ws, wst, wn)) in enumerate(zip(got, want)):
        assert gn == wn, (k, i)
        assert np.array_equal(gs.view(np.uint64), ws.view(np.uint64)), (k, i, "scores")
        for f in abi.STATE_FIELDS:
            g, w = np.asarray(gst[f]), np.asarray(wst[f])
            if f in abi.RECORD_FIELDS:
                g = g.reshape(T, E)
                other = np.delete(g, k, axis=0)
                assert not other.view(np.uint8).any(), (k, i, f, "another topic's records")
                g = g[k]
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (k, i, f)


def counters_seen(snaps):
    """Every counter and a mesh flag were non-zero at some check (the relabelled run is no empty one)."""
    return all(any(np.asarray(st[f]).any() for _, st, _ in snaps) for f in COUNTERS + ("rec_flags",))


# ---- propagation with credits on one topic of many ---------------------------------------
def prop_world(be, ov, T, k, seed, mesh_degree=5):
    """pc.setup's world with topic k alone scored and meshed: AddPeer, the random
    mesh of topic k, app scores and thresholds.  The draws do not depend on T or k."""
    from gsx import synth

    rng = np.random.default_rng(seed + 1)
    be.set_peer_params(synth.bench_peer_params())
    tp = synth.spam_test_topic_params()
    tp.mesh_message_deliveries_window_ns = 25 * abi.MILLISECOND
    be.set_topic_params(k, tp)
    be.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                     accept_px_threshold=0, opportunistic_graft_threshold=0))
    be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    E = ov.n_pairs
    ev = [(abi.EV_ADD_PEER, 0, p, T0, 0) for p in range(E)]
    for i in range(ov.n):
        row = np.arange(ov.row_ptr[i], ov.row_ptr[i + 1])
        row = row[(ov.edge_flags[row] & abi.GSX_EDGE_GOSSIPSUB) != 0]
        ev += [(abi.EV_GRAFT, k, int(q), T0, 0) for q in rng.permutation(row)[:mesh_degree]]
    be.apply_events(np.array(ev, dtype=abi.event_dtype()))
    be.set_app_scores(np.where(rng.random(E) < 0.08, -500.0, rng.normal(0, 2, E)))
    be.refresh(T0 + 2 * S)


def prop_relabel_run(be, T, k, router, n=250, d=5, seed=19, m=70):
    """One credited batch on topic k -> (counters, hops, first deliverers, scores, topic k's
    records, whether any other topic's record is non-zero)."""
    ov = pc.overlay(n, d, seed, mix_protocols=True, direct_frac=0.02)
    prop_world(be, ov, T, k, seed)
    ms = pc.messages(n, m, seed, invalid=0.1)
    out, hop, frm = be.propagate(ms, pc.config(router, topic=k, latency_ms=5, delay_ms=2.0), want_results=True)
    be.settle_scores()
    st = be.export_state()
    E = ov.n_pairs
    recs = {f: np.asarray(st[f]).reshape(T, E)[k].copy() for f in abi.RECORD_FIELDS}
    other = any(np.delete(np.asarray(st[f]).reshape(T, E), k, axis=0).view(np.uint8).any() for f in abi.RECORD_FIELDS)
    return out.as_dict(), hop, frm, be.scores(), recs, other


def assert_prop_relabelled(got, want, k):
    assert got[0] == want[0], k
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), k
    assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64)), k
    for f in abi.RECORD_FIELDS:
        assert np.array_equal(got[4][f].view(np.uint8), want[4][f].view(np.uint8)), (k, f)
    assert not got[5], k
    assert want[0]["deliveries"] > 0 and want[0]["rejected"] > 0
    assert want[4]["first_message_deliveries"].any() and want[4]["invalid_message_deliveries"].any()


# ---- heartbeat ---------------------------------------------------------------------------
# T, n, d, mesh_degree, seed: meshes of 2 are grafted up to D (and lose their negative-score
# peers), meshes of 14 are pruned down to it; seeds whose overlay has n_pairs % 4 == 2
HB_CASES = [(9, 300, 6, 2, 300), (9, 300, 6, 14, 300), (16, 260, 6, 2, 300), (16, 260, 6, 14, 300),
            (33, 240, 5, 2, 302), (33, 240, 5, 14, 302), (64, 200, 5, 2, 301), (64, 200, 5, 14, 301)]
HB_TICKS = 4
HB_FIRST_TICK = 58  # the third round is an opportunistic-graft tick (60)


def hb_id(case):
    return f"T{case[0]}-m{case[3]}"


def hb_case(T, md):
    return next(c for c in HB_CASES if c[0] == T and c[3] == md)


def hb_run(be, case):
    """-> (overlay, the snapshot before the first round, per-round counters, per-round snapshots)"""
    T, n, d, md, seed = case
    pre = []
    ov, outs, snaps = hc.mesh_run(be, n, d, T, seed=seed, ticks=HB_TICKS, mesh_degree=md, mix=True, direct=0.03,
                                  disconnect=0.03, prop_msgs=48, first_tick=HB_FIRST_TICK, mostly_positive=(md < 6),
                                  prop_topics=last_group(T), pre=pre)
    return ov, pre[0], outs, snaps


def hb_reach(case, ov, pre, outs, snaps):
    """What a heartbeat case is for, on topics >= 8 of the exported arrays."""
    T, md = case[0], case[3]
    E = ov.n_pairs
    assert E % 4 != 0 and E % 64 != 0, E  # a chunk-1 backoff byte off the word boundary, a ragged tile
    assert (ov.edge_flags & abi.GSX_EDGE_DIRECT).any() and (np.asarray(pre["pair_flags"]) == abi.GSX_PAIR_PRESENT).any()
    mesh = [(np.asarray(s["rec_flags"]).reshape(T, E)[8:] & abi.GSX_REC_IN_MESH) != 0 for s in [pre] + snaps]
    gained = sum((~a & b).sum(axis=1) for a, b in zip(mesh, mesh[1:]))  # per topic 8 .. T - 1
    lost = sum((a & ~b).sum(axis=1) for a, b in zip(mesh, mesh[1:]))
    # PRUNEs in every case, and on the last topic (32 at T = 33, 63 at T = 64), with their backoff
    assert lost.sum() > 0 and lost[-1] > 0, lost
    assert any(np.asarray(s["backoff"])[8:].any() for s in snaps)
    assert any(np.asarray(s["backoff"])[T - 1].any() for s in snaps), T - 1
    if md < 6:  # GRAFTs where the meshes start under Dlo
        assert gained.sum() > 0 and gained[-1] > 0, gained
    else:
        assert sum(o["prunes"] for o in outs) > sum(o["grafts"] for o in outs)
    assert any(np.asarray(s["ihave_len"])[8:].any() for s in snaps)  # gossip of the last group's traffic


def hub_overlay():
    """The overlay of test_heartbeat_hub_nodes_match_oracle: a hub of ~700 peers and one of ~200."""
    from test_gpu_propagation import _hub_overlay, _overlay_from_edges

    n = 705
    ov = _hub_overlay(n, seed=3)
    edges = set()
    for u in range(n):
        for v in ov.col[ov.row_ptr[u]:ov.row_ptr[u + 1]]:
            edges.add((min(u, int(v)), max(u, int(v))))
    edges |= {(1, k) for k in range(2, 200)}
    return _overlay_from_edges(n, sorted(edges)), n


def hub_run(be, ov, n, T=9, md=8):
    gp = hc.be_default_params()
    gp.history_gossip = 3
    pc.setup(be, ov, T, seed=11, mesh_degree=md, disconnect_frac=0.02)
    be.set_gossipsub_params(gp)
    outs, snaps = [], []
    for k in range(3):
        now = T0 + (3 + k) * S
        outs.append(be.heartbeat(59 + k, now, 1234).as_dict())
        snaps.append(hc.snapshot(be))
        cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=T - 1, latency_ms=5, seed=k)
        cfg.now_ns = now + 100 * abi.MILLISECOND
        be.propagate(pc.messages(n, 70, 100 + k), cfg)
        be.refresh(now + 500 * abi.MILLISECOND)
    return outs, snaps


def hub_reach(ov, T, outs, snaps):
    E = ov.n_pairs
    deg = np.diff(ov.row_ptr)
    assert deg[0] > 64 and deg[1] > 64  # one wave per node
    hub_pairs = np.arange(ov.row_ptr[0], ov.row_ptr[2])
    mesh = [(np.asarray(s["rec_flags"]).reshape(T, E)[T - 1, hub_pairs] & abi.GSX_REC_IN_MESH) != 0 for s in snaps]
    assert any((a != b).any() for a, b in zip(mesh, mesh[1:])), "the hubs' meshes of topic 8 never changed"
    assert any(np.asarray(s["ihave_len"])[T - 1, hub_pairs].any() for s in snaps)  # the hubs gossiped on topic 8
    assert sum(o["grafts"] + o["prunes"] for o in outs) > 0


# ---- membership, fanout, PX ----------------------------------------------------------------
def member_topics(T):
    return {9: [0, 8], 33: [8, 31, 32]}.get(T, [31, 32, T - 1])


def member_run(be, T):
    return mc.membership_run(be, n=300, d=6, T=T, seed=9 + T, ticks=9, msgs=16, fanout_ttl_s=2, join_at=4,
                             leave_at=6, topics=member_topics(T))


def member_reach(T, ov, outs, mems):
    joined = [m[0] for m in mems]
    fanout = [m[1] for m in mems]
    obs = ov.pair_observer()
    for t in (32, T - 1):
        assert any(bit(j, t).any() for j in joined), t
        assert any(bit(f, t).any() for f in fanout), t
    assert not all(bit(j, 32).all() for j in joined)  # (a partial subscription, not the default)
    assert any(name == "join" and o["grafts"] > 0 for name, o in outs)
    assert any(name == "leave" and o["prunes"] > 0 for name, o in outs)
    expired = 0
    for t in range(32, T):
        for k in range(len(mems) - 1):
            gone = bit(fanout[k], t) & ~bit(fanout[k + 1], t)
            expired += int((gone & ~bit(joined[k + 1], t)[obs]).sum())  # (not a fanout turned mesh by a Join)
    assert expired > 0


def px_member_run(be, T):
    lt, jt = (31, 32) if T == 33 else (32, T - 1)
    return xc.px_member_run(be, n=300, d=8, T=T, seed=13 + T, leave_topic=lt, join_topic=jt)


def px_member_reach(T, res):
    lt, jt = (31, 32) if T == 33 else (32, T - 1)
    (_, _), (leave, leave_recs), (join, _) = res
    assert leave["prunes"] > 0 and leave["px_prunes"] > 0 and join["grafts"] > 0
    assert len(leave_recs) and ((leave_recs[:, 3] & 0xFF) == lt).all()  # the candidates of topic lt's PRUNEs


# ---- gossip exchange -----------------------------------------------------------------------
# (rounds 0..4 only emit IHAVEs: ids asked later than the senders' caches hold them break promises)
GX_CASES = {9: dict(T=9, topics=[8, 0], n=300, ticks=10, exchange_from=5),
            64: dict(T=64, topics=[63], n=240, ticks=10, exchange_from=5)}
GX_COUNTERS = ("iwant_msgs", "iwant_ids", "iwant_served", "gossip_delivered", "fwd_delivered", "broken_promises")


def gx_reach(T, outs, snaps):
    tot = {c: sum(o[c] for o in outs) for c in GX_COUNTERS}
    assert all(tot.values()), tot
    assert any(np.asarray(s["ihave_len"])[T - 1].any() for s in snaps)
    if T == 9:
        assert any(np.asarray(s["ihave_len"])[0].any() for s in snaps)


# ---- propagation credits on one topic of 33 ------------------------------------------------
CREDIT_T = 33
CREDITED = ("first_message_deliveries", "mesh_message_deliveries", "invalid_message_deliveries")


def credit_world(be):
    ov = pc.overlay(200, 5, seed=23, mix_protocols=True)
    pc.setup(be, ov, CREDIT_T, seed=23)
    return ov


def credit_batches(n):
    """(m, messages): one accepted message, one REJECT message, 65 with one REJECT among them."""
    out = []
    for i, (m, reject) in enumerate(((1, None), (1, 0), (65, 40))):
        ms = pc.messages(n, m, seed=23 + i)
        if reject is not None:
            ms["validation"][reject] = abi.GSX_VALIDATION_REJECT
        out.append((m, ms))
    return out


def credit_config(topic, credit, now):
    cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=topic, latency_ms=5, delay_ms=2.0, credit=credit)
    cfg.now_ns = now
    return cfg


def credit_reach(T, topic, E, ms, out, before, after):
    """The batch credited its own topic and left every other topic's records as they were."""
    accepted = (ms["validation"] == abi.GSX_VALIDATION_ACCEPT).any()
    rejected = (ms["validation"] == abi.GSX_VALIDATION_REJECT).any()
    for f in abi.RECORD_FIELDS:
        a, b = np.asarray(before[f]).reshape(T, E), np.asarray(after[f]).reshape(T, E)
        assert np.array_equal(np.delete(a, topic, 0).view(np.uint8), np.delete(b, topic, 0).view(np.uint8)), (topic, f)

    def changed(f):
        return (np.asarray(before[f]).reshape(T, E)[topic] != np.asarray(after[f]).reshape(T, E)[topic]).any()

    if accepted:
        assert out["deliveries"] > 0 and changed("first_message_deliveries") and changed("mesh_message_deliveries")
    if rejected:
        assert out["rejected"] > 0 and changed("invalid_message_deliveries")


# ---- the sharded heartbeat's control words with bit 32 -------------------------------------
SHARD_T, SHARD_N, SHARD_SEED, SHARD_WORLD, SHARD_ROUNDS = 33, 500, 41, 2, 3


def shard_world(be):
    """-> (overlay, app scores): meshes of 3 on every topic (under Dlo: GRAFTs), 8 % negative
    scores (PRUNEs), some pairs disconnected."""
    ov = pc.overlay(SHARD_N, 6, SHARD_SEED, mix_protocols=True, direct_frac=0.02)
    app = pc.setup(be, ov, SHARD_T, SHARD_SEED, mesh_degree=3, disconnect_frac=0.02)
    return ov, app


def shard_round_args(k):
    """(tick, now, the batch on topic 32 that follows the round, its config)"""
    now = T0 + (3 + k) * S
    cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=32, latency_ms=5, seed=SHARD_SEED + k)
    cfg.now_ns = now + 100 * abi.MILLISECOND
    return 59 + k, now, pc.messages(SHARD_N, 60, SHARD_SEED + 1000 * k), cfg


def shard_rounds(be, ov):
    """The rounds on an unsharded backend -> (counters, topic 32's mesh flags before the
    first round and after each, snapshots)."""
    E = ov.n_pairs
    mesh32 = lambda: (be.export_state()["rec_flags"].reshape(SHARD_T, E)[32] & abi.GSX_REC_IN_MESH) != 0  # noqa: E731
    outs, flags, snaps = [], [mesh32()], []
    for k in range(SHARD_ROUNDS):
        tick, now, ms, cfg = shard_round_args(k)
        outs.append(be.heartbeat(tick, now, SHARD_SEED).as_dict())
        snaps.append(hc.snapshot(be))
        flags.append(mesh32())
        be.propagate(ms, cfg)
        be.refresh(now + 500 * abi.MILLISECOND)
    return outs, flags, snaps


def shard_reach(ov, flags):
    """A GRAFT and a PRUNE of topic 32 crossed the ranks: the mesh flag of a pair whose two
    ends live on different ranks changed in a round."""
    from gsx import synth

    rank_lo = synth.shard_ranges(ov.n, SHARD_WORLD)
    rank = lambda v: np.searchsorted(rank_lo, v, side="right") - 1  # noqa: E731
    cross = rank(ov.pair_observer()) != rank(ov.col)
    assert cross.any() and not cross.all()
    grafts = sum(int((~a & b & cross).sum()) for a, b in zip(flags, flags[1:]))
    prunes = sum(int((a & ~b & cross).sum()) for a, b in zip(flags, flags[1:]))
    assert grafts > 0 and prunes > 0, (grafts, prunes)

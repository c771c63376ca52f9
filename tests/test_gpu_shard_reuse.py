"""Range shards and message-parallel replicas kept across calls of different
shapes (gsx/shard.py on one GPU, the harness of test_gpu_shard.py): one
RangeSharded object per rank runs a sequence of calls whose word counts go up
and down, and one full engine runs the same sequence (test_gpu_engine_reuse.py
pins it to the oracle).  After every call the totals, each rank's hops and
first deliverers, the exported state slices, the scores and the summed
gsx_prop_stats table must equal the full engine's, bit for bit.

The shard engines keep the halo, hfrom, pack_tab, the replicated frontier rows
and the per-call rows between calls whenever the new call fits the old
capacity; the aimed case at the end builds the input at which a stale halo
row of a wider call would be read as a live row of a narrower one."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported on the main thread before the shard threads use it)

import gsx
import propagation_cases as pc
from gsx import abi, shard, synth

pytestmark = pytest.mark.gpu

TOTAL_KEYS = ("deliveries", "duplicates", "transmissions", "hops", "hop_deliveries", "rejected", "ignored", "graylisted")

# m, router, max_hops: the word counts are 16, 1, 4, 2, 1, 1, 2, 1
SEQ = [
    (1024, abi.GSX_ROUTER_GOSSIPSUB, 40),
    (64, abi.GSX_ROUTER_FLOODSUB, 40),
    (200, abi.GSX_ROUTER_GOSSIPSUB, 40),
    (65, abi.GSX_ROUTER_FLOODSUB, 3),  # cut short: the last hop still delivers
    (64, abi.GSX_ROUTER_GOSSIPSUB, 40),
    (1, abi.GSX_ROUTER_FLOODSUB, 40),
    (128, abi.GSX_ROUTER_GOSSIPSUB, 40),
    (40, abi.GSX_ROUTER_FLOODSUB, 40),
]


def _params(e, T, window_ms=25):
    e.set_peer_params(synth.bench_peer_params())
    for t in range(T):
        tp = synth.spam_test_topic_params()
        tp.mesh_message_deliveries_window_ns = int(window_ms * abi.MILLISECOND)
        e.set_topic_params(t, tp)
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                    accept_px_threshold=0, opportunistic_graft_threshold=0))


def _slice_state(st, T, E, a, b):
    out = {}
    for f in abi.STATE_FIELDS:
        x = st[f]
        out[f] = x.reshape(T, E)[:, a:b].reshape(-1).copy() if f in abi.RECORD_FIELDS else x[a:b].copy()
    out["last_refresh_ns"] = st["last_refresh_ns"]
    return out


def _shard_engines(ov, T, rank_lo, st0, app, window_ms, track):
    """One engine per rank holding its nodes' rows and the full engine's state slice."""
    E = ov.n_pairs
    engines = []
    for k in range(len(rank_lo) - 1):
        lo, hi = int(rank_lo[k]), int(rank_lo[k + 1])
        sh = synth.shard_of(ov, lo, hi)
        a, b = int(ov.row_ptr[lo]), int(ov.row_ptr[hi])
        e = gsx.Engine(T)
        _params(e, T, window_ms)
        e.load_overlay_shard(ov.n, lo, sh.row_ptr, sh.col, sh.edge_flags, sh.node_ips)
        e.import_state(_slice_state(st0, T, E, a, b))
        e.set_app_scores(app[a:b])
        e.set_prop_tracking(track)
        engines.append((e, a, b, lo, hi))
    return engines


def _sharded_call(runners, msgs, cfg):
    """One propagate() through every rank's kept RangeSharded -> [(totals, summed PropStats or None, last_mode)]."""
    m = len(msgs)

    def run(tp, r):
        r.tp = tp
        tot = r.propagate(msgs, cfg)[1]
        return tot, (r.prop_stats(m) if m else None), r.last_mode

    return shard.run_local(len(runners), "cuda:0", run, [(r,) for r in runners])


def _check_call(tag, full, out, hop, frm, engines, res, T, E, m, track):
    """Every rank of one sharded call against the full engine's same call."""
    results = [e.prop_results(m) for e, _, _, _, _ in engines]
    for k, ((e, a, b, lo, hi), (h, f)) in enumerate(zip(engines, results)):  # first: where a difference is
        bad = [f"rank {k} message {int(i)} node {int(j) + lo}: hop {int(h[i, j])}, one engine {int(hop[i, j + lo])}"
               for i, j in np.argwhere(h != hop[:, lo:hi])[:5]]
        assert not bad, (tag, bad)
        if track:
            assert np.array_equal(f, frm[:, lo:hi]), (tag, k, np.argwhere(f != frm[:, lo:hi])[:5])
    want = out.as_dict()
    tot = res[0][0]
    for k in TOTAL_KEYS:
        assert tot[k] == want[k], (tag, k, tot[k], want[k])
    assert tot["new_words"] == out.new_words, tag
    # edge_sends: a shard packs a row for a remote receiver that graylists the sender, one engine never gathers it
    if want["graylisted"]:
        assert tot["edge_sends"] >= out.edge_sends, tag
    else:
        assert tot["edge_sends"] == out.edge_sends, tag
    st1, sc1 = full.export_state(), full.scores()
    one = full.prop_stats(m).hop_hist
    for k, (e, a, b, lo, hi) in enumerate(engines):
        st = e.export_state()
        want_st = _slice_state(st1, T, E, a, b)
        for fld in abi.STATE_FIELDS:
            assert np.array_equal(st[fld].view(np.uint8), want_st[fld].view(np.uint8)), (tag, k, fld)
        assert np.array_equal(e.scores().view(np.uint64), sc1[a:b].view(np.uint64)), (tag, k)
        assert np.array_equal(res[k][1].hop_hist, one), (tag, k, np.argwhere(res[k][1].hop_hist != one)[:5])


MODES = {
    # compact, track, P3 window (ms), the exchange every call must take
    "compact": (True, True, 25, "compact"),              # the halo of tagged rows
    "dense": (False, True, 25, "dense"),
    "late-entries": (True, False, 300_000, "replicated"),      # lean calls: the replicated frontier as entries
    "late-rows": (False, False, 300_000, "replicated-rows"),   # ... and as dense row slices
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("world", [2, 3])
def test_range_shards_kept_across_shapes(gpu_ok, world, mode):
    compact, track, window_ms, want_mode = MODES[mode]
    n, d, T, seed = 600, 5, 1, 61 + world
    ov = pc.overlay(n, d, seed, mix_protocols=True, direct_frac=0.03)
    E = ov.n_pairs
    full = gsx.Engine(T)
    app = pc.setup(full, ov, T, seed, disconnect_frac=0.02)
    if window_ms != 25:
        _params(full, T, window_ms)
    full.set_prop_tracking(track)
    rank_lo = synth.shard_ranges(n, world)
    engines = _shard_engines(ov, T, rank_lo, full.export_state(), app, window_ms, track)
    runners = shard.run_local(world, "cuda:0", lambda tp, e: shard.RangeSharded(e, rank_lo, tp, compact=compact),
                              [(x[0],) for x in engines])
    delivered = 0
    for k, (m, router, max_hops) in enumerate(SEQ):
        msgs = pc.messages(n, m, seed + 10 * k)
        cfg = pc.config(router, max_hops=max_hops, seed=seed + k)
        cfg.now_ns = pc.T0 + (3 + k) * pc.S
        out, hop, frm = full.propagate(msgs, cfg, want_results=True)
        res = _sharded_call(runners, msgs, cfg)
        assert [r[2] for r in res] == [want_mode] * world, (k, [r[2] for r in res])
        _check_call((k, m), full, out, hop, frm, engines, res, T, E, m, track)
        delivered += out.deliveries
    assert delivered > 0


@pytest.mark.parametrize("world", [2, 3])
def test_message_parallel_replicas_kept_across_shapes(gpu_ok, world):
    """Every replica propagates its block of each call (blocks of m // world
    messages: other word counts than the full engine's) and stays equal to one
    engine: totals, state, scores and the gathered gsx_prop_stats table."""
    n, d, T, seed = 600, 5, 1, 71 + world
    ov = pc.overlay(n, d, seed, mix_protocols=True, direct_frac=0.02)
    full = gsx.Engine(T)
    pc.setup(full, ov, T, seed, disconnect_frac=0.02)
    reps = []
    for _ in range(world):
        e = gsx.Engine(T)
        pc.setup(e, ov, T, seed, disconnect_frac=0.02)
        reps.append(e)
    runners = shard.run_local(world, "cuda:0", lambda tp, e: shard.MessageParallel(e, tp), [(e,) for e in reps])
    for k, (m, router, max_hops) in enumerate(SEQ):
        msgs = pc.messages(n, m, seed + 10 * k)
        cfg = pc.config(router, max_hops=max_hops, latency_ms=4, seed=seed + k)
        cfg.now_ns = pc.T0 + (3 + k) * pc.S
        out = full.propagate(msgs, cfg)[0]
        want, st1, sc1 = out.as_dict(), full.export_state(), full.scores()
        one = full.prop_stats(m).hop_hist

        def run(tp, r):
            r.tp = tp
            return r.propagate(msgs, cfg)[1], r.prop_stats(m)

        res = shard.run_local(world, "cuda:0", run, [(r,) for r in runners])
        for key in TOTAL_KEYS:
            assert res[0][0][key] == want[key], (k, key, res[0][0][key], want[key])
        for rank, (e, (_, stats)) in enumerate(zip(reps, res)):
            st = e.export_state()
            for fld in abi.STATE_FIELDS:
                assert np.array_equal(st[fld].view(np.uint8), st1[fld].view(np.uint8)), (k, rank, fld)
            assert np.array_equal(e.scores().view(np.uint64), sc1.view(np.uint64)), (k, rank)
            assert np.array_equal(stats.hop_hist, one), (k, rank, np.argwhere(stats.hop_hist != one)[:5])


# ---- the aimed case: a stale halo row of a two-word call read by a one-word call -----------
#
# The compacted exchange stores receive slot j of a W-word call at halo words
# [(W + 1) j, (W + 1) (j + 1)) as [tag | W words]; a row is live when its
# first word is (call serial << 8) | hop.  Read at the stride of a one-word
# call, slot s = (3 j + 1) / 2 (j odd) starts on data word 0 of the two-word
# call's slot j, and its row is that slot's data word 1.  If the two-word
# call's sender of slot j sent exactly messages 1, 9 and 64, word 0 is 0x202 =
# (2 << 8) | 2, the tag of the engine's SECOND call at hop 2, and word 1 is 1:
# message 0 would arrive at slot s's receiver at hop 2 of the second call,
# from nowhere.
N_LOCAL = 10  # nodes per rank (two ranks: nodes 0..9 and 10..19)
AIMED_EDGES = [
    (0, 10), (1, 11), (2, 12), (3, 13),  # the four cross pairs: receive slots 0..3 on either rank
    (13, 14),                            # 14 publishes in call B: 13 has it after hop 1 and sends it to 3 at hop 2
    (5, 6), (15, 16),                    # publishers whose messages cross no shard boundary
]
J, H = 1, 2           # the wide call's slot, the narrow call's hop
S_SLOT = (3 * J + 1) // 2


def _edge_overlay(n, edges):
    """Symmetric overlay from undirected edges (u, v); the lower id dials."""
    rows = [[] for _ in range(n)]
    for u, v in edges:
        rows[u].append(v)
        rows[v].append(u)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    col, ef = [], []
    for i in range(n):
        nb = sorted(set(rows[i]))
        row_ptr[i + 1] = row_ptr[i] + len(nb)
        col += nb
        ef += [abi.GSX_EDGE_GOSSIPSUB | (abi.GSX_EDGE_OUTBOUND if i < j else 0) for j in nb]
    ips = np.stack([np.arange(n, dtype=np.uint32) + 1, np.full(n, 0xFFFFFFFF, dtype=np.uint32)], axis=1)
    return synth.Overlay(n=n, row_ptr=row_ptr, col=np.array(col, dtype=np.int32), edge_flags=np.array(ef, dtype=np.uint8),
                         node_ips=ips, sybil=np.zeros(n, dtype=bool))


def _aimed_messages():
    """Call A: 66 messages (two words); node 11, the remote sender of rank 0's
    slot 1, publishes exactly 1, 9 and 64, node 5 (no cross pair within one
    hop) the rest.  Call B: 8 messages (one word); message 0 from node 15 (its
    component is {15, 16}), the others from node 14."""
    a = pc.messages(2 * N_LOCAL, 66, seed=1)
    a["source"] = 5
    a["source"][[1, 9, 64]] = 11
    b = pc.messages(2 * N_LOCAL, 8, seed=2)
    b["source"] = 14
    b["source"][0] = 15
    return a, b


def _bfs(ov, src, max_hops):
    """Floodsub arrival hops from one source (0xFF: not reached within max_hops)."""
    dist = np.full(ov.n, 0xFF, dtype=np.uint8)
    dist[src] = 0
    front = [int(src)]
    for h in range(1, max_hops + 1):
        nxt = []
        for v in front:
            for u in ov.col[ov.row_ptr[v]:ov.row_ptr[v + 1]]:
                if dist[u] == 0xFF:
                    dist[u] = h
                    nxt.append(int(u))
        front = nxt
    return dist


def _flood_hops(ov, msgs, max_hops):
    return np.stack([_bfs(ov, s, max_hops) for s in msgs["source"]]) if len(msgs) else np.zeros((0, ov.n), np.uint8)


def _recv_slots(ov, rank_lo, rank):
    """The receive slots gsx_shard_recv_plan documents: rank by rank, this rank's pairs ascending."""
    lo, hi = int(rank_lo[rank]), int(rank_lo[rank + 1])
    obs = ov.pair_observer()
    slots = []
    for k in range(len(rank_lo) - 1):
        if k == rank:
            continue
        for q in range(int(ov.row_ptr[lo]), int(ov.row_ptr[hi])):
            v = int(ov.col[q])
            if int(rank_lo[k]) <= v < int(rank_lo[k + 1]):
                slots.append((int(obs[q]), v))
    return slots


def _assert_aimed_preconditions(ov, rank_lo, ms_a, ms_b, plan_u, plan_v):
    """On the host, from the receive plan and a plain BFS: call A leaves
    [tag, 0x200 | H, b != 0] in rank 0's slot J; call B scatters a real entry
    on rank 0 at hop H, none into slot S_SLOT up to hop H, and the one-engine
    run never delivers message 0 to that slot's receiver."""
    slots = _recv_slots(ov, rank_lo, 0)
    assert [u for u, _ in slots] == plan_u.tolist() and [v for _, v in slots] == plan_v.tolist()
    assert J % 2 == 1 and S_SLOT < len(slots)
    # call A (max_hops 1): what crosses at hop 1 is each publisher's own messages, to every neighbour
    sent = {}
    for j, (u, v) in enumerate(slots):
        row = [int(k) for k in np.nonzero(ms_a["source"] == v)[0]]
        if row:
            sent[j] = row
    assert list(sent) == [J], sent  # one entry: nothing else is scattered over it or beside it
    words = [sum(1 << (k % 64) for k in sent[J] if k // 64 == w) for w in range(2)]
    assert words[0] == (2 << 8) | H and words[1] != 0, words
    assert 65 <= len(ms_a) <= 128 and len(ms_b) <= 64
    # call B: a remote sender that had a message after hop H - 1 (not from its receiver) sends it at hop H
    hb = _flood_hops(ov, ms_b, 40)
    real = [(j, u, v) for j, (u, v) in enumerate(slots) if ((hb[:, v] == H - 1) & (hb[:, u] != H - 2)).any()]
    assert real and all(j != S_SLOT for j, _, _ in real), real
    su, sv = slots[S_SLOT]
    assert (hb[:, sv] >= H).all(), hb[:, sv]  # slot S_SLOT's sender holds nothing before hop H: no entry up to hop H
    assert hb[0, su] == 0xFF                  # message 0 never reaches the slot's receiver
    assert words[1] == 1                      # ... and it is the message the stale row would deliver
    return su


@pytest.mark.parametrize("order", ["wide-narrow", "narrow-wide"])
def test_halo_row_of_a_wider_call_is_not_read_by_a_narrower_one(gpu_ok, order):
    """Two calls on the same two shard engines, compacted exchange, floodsub:
    A (66 messages, max_hops 1) then B (8 messages), and the same pair in the
    other order on fresh engines.  After each call the shards equal one engine,
    and one engine's hops are the BFS distances."""
    T, world = 1, 2
    ov = _edge_overlay(2 * N_LOCAL, AIMED_EDGES)
    E = ov.n_pairs
    rank_lo = np.array([0, N_LOCAL, 2 * N_LOCAL], dtype=np.uint32)
    ms_a, ms_b = _aimed_messages()
    full = gsx.Engine(T)
    app = pc.setup(full, ov, T, seed=3, score_spread=False)
    engines = _shard_engines(ov, T, rank_lo, full.export_state(), app, 25, True)
    _, plan_u, plan_v = engines[0][0].shard_recv_plan(rank_lo)
    receiver = _assert_aimed_preconditions(ov, rank_lo, ms_a, ms_b, plan_u, plan_v)
    runners = shard.run_local(world, "cuda:0", lambda tp, e: shard.RangeSharded(e, rank_lo, tp, compact=True),
                              [(x[0],) for x in engines])
    calls = [("A", ms_a, 1), ("B", ms_b, 40)]
    for k, (name, msgs, max_hops) in enumerate(calls if order == "wide-narrow" else calls[::-1]):
        cfg = pc.config(abi.GSX_ROUTER_FLOODSUB, max_hops=max_hops)
        cfg.now_ns = pc.T0 + (3 + k) * pc.S
        out, hop, frm = full.propagate(msgs, cfg, want_results=True)
        assert np.array_equal(hop, _flood_hops(ov, msgs, max_hops)), name
        if name == "B":
            assert hop[0, receiver] == 0xFF
        res = _sharded_call(runners, msgs, cfg)
        assert [r[2] for r in res] == ["compact"] * world
        _check_call(name, full, out, hop, frm, engines, res, T, E, len(msgs), True)

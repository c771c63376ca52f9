"""Scenarios whose runs take the redraw branch of Go's Int31n (`for v > max`,
math/rand) on a chosen draw stream, driven identically through any backend.

A draw for a list of n entries is redrawn with probability (2^31 % n) / 2^31,
so a run takes the branch only for a seed that was searched for:
tools/find_rejection_seeds.py finds the seeds below from the oracle alone and
prints the table SEEDS is copied from.  `rej` is the oracle's count of
rejected draws per tag over the whole run (oracle.rng_rejections); a test
asserts the count of its tag is still at least that before it compares the
engine, so a shifted stream fails loudly instead of going vacuous."""
from __future__ import annotations

import numpy as np

import gossip_cases as gc
import heartbeat_cases as hc
import promise_cases as prc
import propagation_cases as pc
from gsx import abi, synth

TAG_SHUFFLE, TAG_IWANT, TAG_IHAVE_SUB = 8, 9, 13
TWO31 = 1 << 31


def rejected(v, n):
    """Int31n(n) redraws the 31-bit draw v (arrays allowed): v > max."""
    n = np.asarray(n, dtype=np.int64)
    return (np.asarray(v, dtype=np.int64) > TWO31 - 1 - TWO31 % n) & ((n & (n - 1)) != 0)


# ---- hub shuffle: a star whose hub runs one wave per topic ------------------
HUB_PEERS = 10_000  # within 8,000 .. HB_HUB_MAX = 12,000


def star_overlay(n_peers):
    """Node 0 peers with nodes 1..n_peers (it dialled them); the leaves have
    one peer each, whose Int31n(1) never redraws: every rejected tag-8 draw
    of a run on this overlay is in the hub's stream."""
    row_ptr, col = prc.star(n_peers)
    n = n_peers + 1
    ef = np.full(len(col), abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8)
    ef[:n_peers] |= abi.GSX_EDGE_OUTBOUND
    ips = np.stack([np.arange(n, dtype=np.uint32) + 1, np.full(n, abi.GSX_NO_IP, dtype=np.uint32)], axis=1)
    return synth.Overlay(n=n, row_ptr=row_ptr, col=col, edge_flags=ef, node_ips=ips, sybil=np.zeros(n, dtype=bool))


_star = {}


def hub_run(be, seed, ticks=3, T=2, pre=None):
    """The star's hub starts with every leaf in its mesh (each leaf grafts its
    one peer): rounds of heartbeat, a small batch, refresh.  The hub prunes
    ~10,000 mesh peers down (shuffles of thousands of entries) and gossips
    to the rest (a shuffle of its eligible peers).  pre: a list that gets
    hub_mesh_sizes before the first round."""
    if HUB_PEERS not in _star:
        _star[HUB_PEERS] = star_overlay(HUB_PEERS)
    ov = _star[HUB_PEERS]
    pc.setup(be, ov, T, 3, mesh_degree=6)
    if pre is not None:
        pre.append(hub_mesh_sizes(be, T))
    outs, snaps = [], []
    for k in range(ticks):
        now = hc.T0 + (3 + k) * abi.SECOND
        outs.append(be.heartbeat(59 + k, now, seed).as_dict())
        snaps.append(hc.snapshot(be))
        cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=k % T, latency_ms=5, seed=k)
        cfg.now_ns = now + 100 * abi.MILLISECOND
        be.propagate(pc.messages(ov.n, 40, 100 + k), cfg)
        be.refresh(now + 500 * abi.MILLISECOND)
    return outs, snaps


# ---- lane-path shuffle: every node has at most HB_LANE_DEG peers ------------
LANE = dict(n=500, d=25, T=1, ticks=3, mesh_degree=40, first_tick=59)
LANE_NMAX = 64  # no list of a lane unit is longer than HB_LANE_DEG


def lane_run(be, seed):
    """heartbeat_cases.mesh_run's n500-T1-m40 shape (about 50 peers per node,
    meshes of ~40 pruned through the merge sort) on one fixed overlay; only
    the heartbeats' seed varies."""
    c = LANE
    ov = pc.overlay(c["n"], c["d"], 525, direct_frac=0.02)
    pc.setup(be, ov, c["T"], 525, mesh_degree=c["mesh_degree"])
    outs, snaps = [], []
    for k in range(c["ticks"]):
        now = hc.T0 + (3 + k) * abi.SECOND
        outs.append(be.heartbeat(c["first_tick"] + k, now, seed).as_dict())
        snaps.append(hc.snapshot(be))
        cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=0, latency_ms=5, seed=k)
        cfg.now_ns = now + 100 * abi.MILLISECOND
        be.propagate(pc.messages(c["n"], 64, 525 + 1000 * k), cfg)
        be.refresh(now + 500 * abi.MILLISECOND)
    return ov, outs, snaps


def lane_prefilter(seeds, n_draws=64):
    """The seeds for which some draw k < n_draws of some node's tag-8 stream of
    some round lies in the top LANE_NMAX values below 2^31: only those can be
    redrawn for a list of at most LANE_NMAX entries (mesh and gossip streams:
    bit 23 of the base clear and set)."""
    c = LANE
    v = np.arange(c["n"], dtype=np.uint64)[:, None, None, None]
    tick = (np.arange(c["ticks"], dtype=np.uint64) + np.uint64(c["first_tick"]))[None, :, None, None]
    fan = (np.arange(2, dtype=np.uint64) << np.uint64(23))[None, None, :, None]
    k = np.arange(n_draws, dtype=np.uint64)[None, None, None, :]
    base = (tick << np.uint64(32)) | fan | k
    keep = []
    for s in seeds:
        if ((synth.h(int(s), TAG_SHUFFLE, v, base) >> np.uint64(33)) >= np.uint64(TWO31 - LANE_NMAX)).any():
            keep.append(int(s))
    return keep


# ---- truncated IHAVE lists (tag 13) and the IWANT sampling (tag 9) ----------
# One batch per round of tens of thousands of messages that travel one hop on
# a small overlay: every node caches the messages of its own and its mesh
# peers' publishing, lists of tens of thousands of ids.
TRUNC = dict(n=14, d=3, T=1, ticks=3, hops=1, msgs=24_000, max_ihave_length=7_000, history_gossip=3)
# T = 2: from the third round on a sender advertises two topics' truncated
# lists in one RPC, so |iwant| is up to twice the budget MaxIHaveLength and
# the asker samples (kk < n).  Batches of 9,000 messages are 141 words, more
# than GX_MW = 128 unseen words: pass 1 of every asker runs in k_gx_node.
IWANT_HEAVY = dict(n=14, d=3, T=2, ticks=4, hops=1, msgs=9_000, max_ihave_length=2_000, history_gossip=3)
# two advertised batches of 3,400 messages (54 words each, 108 <= GX_MW): the
# asker's own lane walks them (k_gx_ask's light path)
IWANT_LIGHT = dict(n=24, d=4, T=2, ticks=4, hops=1, msgs=3_400, max_ihave_length=1_500, history_gossip=2)


class ListLengths:
    """A backend that notes every node's GetGossipIDs length per topic before
    each heartbeat (emitGossip reads the cache before the round's Shift)."""

    def __init__(self, be, n, T, history_gossip):
        self.be, self.n, self.T, self.hg, self.L = be, n, T, history_gossip, []

    def __getattr__(self, k):
        return getattr(self.be, k)

    def heartbeat(self, tick, now, seed):
        self.L.append([[len(self.be.mcache_ids(v, t, self.hg)) for v in range(self.n)] for t in range(self.T)])
        return self.be.heartbeat(tick, now, seed)


def floyd_replay(seed, node, peer, tick, topic, L, kk):
    """The steps of wave_floyd's / floyd_select's draw stream of one target at
    which a draw is rejected, replayed from the hash alone: step s draws
    Int31n(L - kk + s + 1) at the next unused counter.  -> [(step, lane,
    rejecting lanes)]: the step, its lane in the 64-step batch the engine
    evaluates it in (a batch starts at step 0, 64 steps after the last start,
    or at a rejected step, whose redraw is lane 0 of the next batch), and how
    many lanes of that batch's ballot reject (the first one is resolved, the
    later lanes are drawn again with their counters moved by one)."""
    vertex = (node << 32) | peer
    base = (tick << 32) | (topic << 24)
    out = []
    s, off, start = 0, 0, 0
    while s < kk:
        steps = np.arange(s, kk, dtype=np.uint64)
        v = synth.h(seed, TAG_IHAVE_SUB, vertex, np.uint64(base) | (steps + np.uint64(off))) >> np.uint64(33)
        idx = np.flatnonzero(rejected(v, L - kk + steps.astype(np.int64) + 1))
        if len(idx) == 0:
            break
        s0 = s
        s += int(idx[0])
        start += (s - start) // 64 * 64
        # the ballot of that batch, taken before the redraw shifts the later lanes' counters
        out.append((s, s - start, int((idx + s0 < start + 64).sum())))
        start = s
        off += 1
    return out


def trunc_targets(ov, lengths, snaps, maxl):
    """(round, node, peer, L) of every truncated list a run sent (T = 1)."""
    obs = ov.pair_observer()
    out = []
    for k, st in enumerate(snaps):
        il = np.asarray(st["ihave_len"]).reshape(-1)
        for r in np.flatnonzero(il == maxl):
            L = lengths[k][0][int(obs[r])]
            if L > maxl:
                out.append((k, int(obs[r]), int(ov.col[r]), L))
    return out


def trunc_placements(seed, ov, lengths, snaps, maxl):
    """-> (rejected draws in all, [(round, node, peer, L, kk, [(step, lane, rejecting lanes)])] of the targets that have any)"""
    tot, hits = 0, []
    for k, v, p, L in trunc_targets(ov, lengths, snaps, maxl):
        kk = min(maxl, L - maxl)
        rj = floyd_replay(seed * 31 + 7, v, p, 1 + k, 0, L, kk)
        tot += len(rj)
        if rj:
            hits.append((k, v, p, L, kk, rj))
    return tot, hits


def placements_of(hits):
    """Which of the three placements a run's rejections cover."""
    got = set()
    for _, _, _, _, kk, rj in hits:
        for s, lane, nrej in rj:
            if lane == 0:
                got.add("lane0")
            if s == kk - 1:
                got.add("last_step")
            if nrej >= 2:
                got.add("two_in_batch")
    return got


# ---- gsx_promise_add's pick (host_int31n) ----------------------------------
PROMISE_N = 1000  # handles: 2^31 % 1000 = 648 values of 2^31 are redrawn


def promise_seed_rejects(seed, pair=0, n=PROMISE_N):
    """How many draws AddPromise's Int31n(n) rejects for (seed, pair)."""
    c = 0
    while rejected(synth.h(seed, TAG_IWANT, pair, c) >> np.uint64(33), n):
        c += 1
    return c


def promise_run(be, seeds, n=PROMISE_N):
    """One promise per seed on pair 0, each picked among n handles; the kept
    handle is the one GetBrokenPromises / fulfill see: returns which handles
    were kept (fulfilling the kept one empties the pair's count)."""
    row_ptr, col = prc.star(3)
    be.set_peer_params(synth.bench_peer_params())
    be.load_overlay(row_ptr, col)
    handles = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(11)
    kept = []
    for s in seeds:
        be.promise_add(0, handles, prc.T0 + 1, seed=int(s))
        want = int(handles[_int31n(int(s), 0, n)])
        before = be.promise_count()
        be.promise_fulfill(0, want)
        kept.append((want, before, be.promise_count()))
    return kept


def _int31n(seed, pair, n):
    c = 0
    while True:
        v = int(synth.h(seed, TAG_IWANT, pair, c) >> np.uint64(33))
        if not rejected(v, n):
            return v % n
        c += 1


# ---- a draw that equals max exactly: kept by `v > max`, redrawn by `v >= max`
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def hash_inner(tag, a, b):
    """The seed-independent part of synth.h: h = mix(seed + golden * (1 + inner))."""
    return synth._mix(np.uint64(tag) ^ synth._mix(np.asarray(a, dtype=np.uint64) ^ synth._mix(np.asarray(b, dtype=np.uint64))))


def draws_of_seeds(seeds, inner):
    """[seed, draw] 31-bit draws of many seeds over fixed (tag, a, b) positions."""
    with np.errstate(over="ignore"):
        z = np.asarray(seeds, dtype=np.uint64)[:, None] + _GOLD * (np.uint64(1) + np.atleast_1d(inner))[None, :]
    return (synth._mix(z) >> np.uint64(33)).astype(np.int64)


def int31n_max(n):
    n = np.asarray(n, dtype=np.int64)
    return TWO31 - 1 - TWO31 % n


# The hub's first draws of round 59: its mesh (every leaf with a score >= 0,
# about 4,560, more than HUB_EQ_K of them) is above Dhi, so maintenance starts with
# shufflePeers over it: step k draws Int31n(k + 1) at counter k of
# h(seed, 8, 0, 59 << 32 | topic << 24 | k), as long as no earlier draw of the
# stream was redrawn.
HUB_EQ_K = 4000


def hub_eq_positions():
    """-> (inner [2 * HUB_EQ_K], max [2 * HUB_EQ_K], usable mask): topic-major."""
    k = np.arange(HUB_EQ_K, dtype=np.uint64)
    base = np.concatenate([(np.uint64(59) << np.uint64(32)) | (np.uint64(t) << np.uint64(24)) | k for t in (0, 1)])
    n = np.concatenate([k, k]).astype(np.int64) + 1
    return hash_inner(TAG_SHUFFLE, 0, base), int31n_max(n), (n & (n - 1)) != 0


def hub_eq_hits(seed):
    """[(topic, counter)] of the hub's first shuffle whose draw equals max."""
    inner, mx, ok = hub_eq_positions()
    v = draws_of_seeds([seed], inner)[0]
    return [(int(i) // HUB_EQ_K, int(i) % HUB_EQ_K) for i in np.flatnonzero((v == mx) & ok)]


def hub_mesh_sizes(be, T=2):
    """The hub's mesh peers with a score >= 0 per topic (what the first shuffle runs over)."""
    rf = np.asarray(be.export_state()["rec_flags"]).reshape(T, -1)[:, :HUB_PEERS]
    ok = np.asarray(be.scores())[:HUB_PEERS] >= 0
    return [int((((rf[t] & abi.GSX_REC_IN_MESH) != 0) & ok).sum()) for t in range(T)]


def promise_eq(seed, pair=0, n=PROMISE_N):
    """AddPromise's first draw for (seed, pair) equals max."""
    return int(synth.h(seed, TAG_IWANT, pair, 0) >> np.uint64(33)) == int(int31n_max(n))


# Copied from the output of tools/find_rejection_seeds.py.  trunc: the
# placements "last_step" and "two_in_batch" were not met by seeds 0..2353.
SEEDS = {
    'promise': {'seeds': [517557, 3827691, 4182744], 'rej': {9: 3}},
    'hub': {'seed': 24, 'rej': {8: 2}},
    'lane': {'seed': 14232, 'rej': {8: 1}, 'prefiltered_up_to': 14400},
    'iwant_heavy': {'seed': 126, 'rej': {9: 1}, 'iwant_ids': 172624},
    'promise_eq': {'seed': 4268161621, 'rej': {}},
    'hub_eq': {'seed': 946622, 'hits': [(0, 2527)], 'mesh': [4562, 4562], 'rej': {}},
    'iwant_light': {'seed': 440, 'rej': {9: 1}, 'iwant_ids': 154763},
    'trunc': {'any': {'seed': 0, 'rej': {13: 2}}, 'lane0': {'seed': 84, 'rej': {13: 5}}, 'searched_up_to': 2354},
}

"""gsx_gossipsub_params away from DefaultGossipSubParams: one table of cases,
run identically through any backend.  Every case names the parameter values
it moves and a check of the round counters that proves the branch it is
about ran; the checks read the oracle's run (test_gossipsub_params_oracle.py
runs the table through the oracle alone, test_gpu_gossipsub_params.py
compares the engine with it field by field)."""
from __future__ import annotations

import numpy as np

import gossip_cases as gc
import heartbeat_cases as hc
from gsx import abi

S, MS = abi.SECOND, abi.MILLISECOND


def _sum(outs, f):
    return sum(o[f] for o in outs)


def _first(outs, f):
    """The first round whose counter f is positive (None: never)."""
    return next((k for k, o in enumerate(outs) if o[f] > 0), None)


# ---- the exchange: gc.exchange_run at n = 300, d = 6, T = 2 -----------------
# GossipRetransmission 0: GetForPeer's count is over the limit at the first
# request, so nothing is ever served and every promise breaks, one heartbeat
# after it expires (heartbeats are 1 s apart, a promise made at round k with
# IWantFollowupTime f expires at round k + f: broken at the first round after)
def _broken_after(rounds):
    def chk(outs):
        k = _first(outs, "iwant_msgs")
        assert k is not None and _sum(outs, "iwant_served") == 0, outs
        assert _first(outs, "broken_promises") == (None if rounds is None else k + rounds), \
            [o["broken_promises"] for o in outs]
    return chk


def _gossips(outs):
    assert _sum(outs, "ihave_msgs") > 0 and _sum(outs, "iwant_msgs") > 0 and _sum(outs, "iwant_served") > 0, outs


def _no_gossip(outs):
    assert _sum(outs, "ihave_msgs") == 0 and _sum(outs, "iwant_msgs") == 0, outs
    assert _sum(outs, "mesh_links") > 0


def _ihaves(outs):
    assert _sum(outs, "ihave_msgs") > 0, outs


def _maxl0(outs):  # every emitted list is empty, and every IHAVE RPC is ignored (iasked 0 >= MaxIHaveLength 0, :630-633)
    assert _sum(outs, "ihave_msgs") > 0 and _sum(outs, "ihave_ids") == 0 and _sum(outs, "iwant_msgs") == 0, outs
    assert outs[1]["ihave_ignored"] == outs[1]["ihave_msgs"] > 0, outs[1]  # (one topic's lists yet: one IHAVE per RPC)


def _maxl1(outs):  # every list is cut to one id, and ids are asked one at a time
    assert _sum(outs, "ihave_msgs") > 0 and _sum(outs, "ihave_ids") == _sum(outs, "ihave_msgs"), outs
    assert _sum(outs, "iwant_msgs") > 0 and _sum(outs, "iwant_ids") == _sum(outs, "iwant_msgs"), outs


def _factor_beats_dlazy(outs):  # ~44 eligible peers per node: 22 targets, not Dlazy = 6, per node and topic
    assert max(o["ihave_msgs"] for o in outs) > 2 * 6 * 300, [o["ihave_msgs"] for o in outs]
    _gossips(outs)


EXCHANGE = {
    "retransmission0": (dict(gossip_retransmission=0, ticks=8), _broken_after(4)),
    # (a receiver asks for a message once, so one transmission serves everything asked)
    "retransmission1": (dict(gossip_retransmission=1, ticks=6), _gossips),
    "followup0": (dict(gossip_retransmission=0, iwant_followup_ns=0, ticks=6), _broken_after(1)),
    "followup500ms": (dict(gossip_retransmission=0, iwant_followup_ns=500 * MS, ticks=6), _broken_after(1)),
    "followup10s": (dict(gossip_retransmission=0, iwant_followup_ns=10 * S, ticks=13), _broken_after(11)),
    "max_ihave_messages1": (dict(max_ihave_messages=1, ticks=5), _gossips),
    "max_ihave_length0": (dict(max_ihave_length=0, ticks=4), _maxl0),
    "max_ihave_length1": (dict(max_ihave_length=1, ticks=5), _maxl1),
    "no_targets": (dict(d_lazy=0, gossip_factor=0.0, ticks=4), _no_gossip),
    "factor_only": (dict(d_lazy=0, gossip_factor=1.0, ticks=4), _gossips),
    "dlazy1": (dict(d_lazy=1, ticks=5), _gossips),
    "dlazy64": (dict(d_lazy=64, ticks=4), _gossips),
    "factor_half_d25": (dict(d=25, gossip_factor=0.5, ticks=4), _factor_beats_dlazy),
    "history1_1": (dict(history_length=1, history_gossip=1, ticks=5),
                   _ihaves),
    "history7_2": (dict(history_length=7, history_gossip=2, ticks=8), _gossips),
    "history5_0": (dict(history_length=5, history_gossip=0, ticks=4), _no_gossip),
}


def exchange_case(be, name):
    kw = dict(EXCHANGE[name][0])
    return gc.exchange_run(be, **kw)


def grow_run(be, n=300, d=6, T=2, seed=5, ticks=9):
    """One engine whose Dlazy / GossipFactor rise between rounds while every
    list is truncated (MaxIHaveLength 5): the truncated lists' targets per
    round grow, 2 -> 6 -> 12 and more per node.  Before round 5, 25 nodes
    leave topic 0 (membership on); three of them publish six messages each on
    topic 0 in round 5's batch (to a fanout picked then), so in round 6 their
    fanout pass gossips the left topic beside the other topic's mesh pass.
    Before round 7 ten of the 25, publishers included, join topic 0 again
    (their mesh starts from the fanout).  Returns (overlay, counters,
    snapshots, the nodes that left)."""
    import propagation_cases as pc

    ov = pc.overlay(n, d, seed)
    pc.setup(be, ov, T, seed, mesh_degree=6)
    steps = {0: (2, 0.0), 2: (6, 0.25), 4: (12, 0.9)}
    left = np.random.default_rng(seed).choice(n, 25, replace=False).astype(np.uint32)
    outs, snaps = [], []
    for k in range(ticks):
        if k in steps:
            be.set_gossipsub_params(gc.params(max_ihave_length=5, d_lazy=steps[k][0], gossip_factor=steps[k][1]))
        now = hc.T0 + (3 + k) * S
        if k == 5:
            be.set_subscriptions(np.full(n, (1 << T) - 1, dtype=np.uint64))
            be.leave(left, np.zeros(len(left), dtype=np.uint32), now - 200 * MS)
        if k == 7:
            be.join(left[:10], np.zeros(10, dtype=np.uint32), now - 100 * MS, seed + 1)
        outs.append(be.heartbeat(1 + k, now, seed * 31 + 7).as_dict())
        snaps.append(hc.snapshot(be))
        topic = 0 if k in (5, 6) else k % T
        cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=topic, max_hops=2, latency_ms=5, seed=seed + k)
        cfg.now_ns = now + 100 * MS
        ms = pc.messages(n, 24, seed + 1000 * k)
        if k == 5:
            ms["source"][:18] = np.repeat(left[:3], 6)
        be.propagate(ms, cfg)
        be.refresh(now + 500 * MS)
    return ov, outs, snaps, left


def grow_check(run):
    ov, outs, snaps, left = run
    m = [o["ihave_msgs"] for o in outs]
    assert 0 < m[1] < m[3] < m[4], m  # the targets per round grow with Dlazy / GossipFactor
    assert all(o["ihave_ids"] == 5 * o["ihave_msgs"] for o in outs[4:]), outs  # every list truncated by then
    assert _sum(outs, "iwant_msgs") > 0
    # round 6: a node that left topic 0 runs no mesh pass for it, so its IHAVEs
    # on topic 0 are its fanout pass's: some went out, each cut to 5 ids
    from_left = np.isin(ov.pair_observer(), left)
    il = np.asarray(snaps[6]["ihave_len"]).reshape(2, -1)[0][from_left]
    assert (il == 5).sum() > 0 and set(il.tolist()) <= {0, 5}, sorted(set(il.tolist()))
    # the join was real: the joined nodes' topic-0 meshes were built (grafts of the join call are not a
    # round's, but round 7 runs their mesh pass: they hold mesh peers on topic 0 afterwards)
    joined_rows = np.isin(ov.pair_observer(), left[:10])
    rf = np.asarray(snaps[7]["rec_flags"]).reshape(2, -1)[0]
    assert ((rf[joined_rows] & abi.GSX_REC_IN_MESH) != 0).sum() > 0
    rf6 = np.asarray(snaps[6]["rec_flags"]).reshape(2, -1)[0]
    assert ((rf6[from_left] & abi.GSX_REC_IN_MESH) != 0).sum() == 0  # (they had left it)


# ---- maintenance: hc.mesh_run at n = 400, d = 9, T = 2 ----------------------
def _gp(**kw):
    gp = hc.be_default_params()
    gp.history_gossip = 3
    for k, v in kw.items():
        setattr(gp, k, v)
    return gp


OG_TH = abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300, accept_px_threshold=0,
                       opportunistic_graft_threshold=1.0)  # most meshes' median app score (N(0, 2)) is below 1


def _maintains(outs):
    assert _sum(outs, "grafts") > 0 and _sum(outs, "prunes") > 0 and _sum(outs, "prunes_handled") > 0, outs


def _grafts(outs):
    assert _sum(outs, "grafts") > 0 and _sum(outs, "graft_accepted") > 0, outs


MESH = {
    # name: (mesh_run keywords, gossipsub params, thresholds, check)
    "d_all_equal": (dict(mesh_degree=9), dict(d=6, d_lo=6, d_hi=6, d_score=4, d_out=2), None, _maintains),
    "d_lo0": (dict(mesh_degree=2), dict(d_lo=0), None, _grafts),
    "d_score0": (dict(mesh_degree=14), dict(d_score=0), None, _maintains),
    "d_score_d_hi": (dict(mesh_degree=14), dict(d_score=12), None, _maintains),
    "d_out0": (dict(mesh_degree=14), dict(d_out=0), None, _maintains),
    "d_out_d": (dict(mesh_degree=14), dict(d_out=6), None, _maintains),
    "backoff0": (dict(mesh_degree=14), dict(prune_backoff_ns=0), None, _maintains),
    "backoff999ms": (dict(mesh_degree=14), dict(prune_backoff_ns=999 * MS), None, _maintains),
}
for _t in (0, 1):
    for _p in (0, 1, 5):
        MESH[f"og_ticks{_t}_peers{_p}"] = (dict(mesh_degree=6), dict(opportunistic_graft_ticks=_t,
                                                                     opportunistic_graft_peers=_p), OG_TH, _grafts)


def mesh_case(be, name):
    kw, gpkw, th, _ = MESH[name]
    return hc.mesh_run(be, 400, 9, 2, seed=77, ticks=4, gp=_gp(**gpkw), first_tick=14, prop_msgs=32,
                       thresholds=th, **kw)


def og_cross_check(grafts):
    """grafts: {case name: total grafts}.  With OpportunisticGraftTicks 1 the
    pass fires every round (0: never), and it grafts more the more peers it
    may take; 0 peers means every candidate (Go's getPeers)."""
    for p in (0, 1, 5):
        assert grafts[f"og_ticks1_peers{p}"] > grafts[f"og_ticks0_peers{p}"], (p, grafts)
    assert grafts["og_ticks1_peers0"] >= grafts["og_ticks1_peers5"] > grafts["og_ticks1_peers1"], grafts


def hub_sort_run(be):
    """test_gpu_heartbeat's md=300 hub (a mesh of ~300 at a node with 700
    peers) with Dhi 40, D = Dscore = 33: the prune keeps the 33 best of a
    merge sort above 32 entries, and the shuffle of the rest is empty."""
    from test_gpu_propagation import _hub_overlay, _overlay_from_edges

    n, T = 705, 2
    ov = _hub_overlay(n, seed=3)
    edges = set()
    for u in range(n):
        for v in ov.col[ov.row_ptr[u]:ov.row_ptr[u + 1]]:
            edges.add((min(u, int(v)), max(u, int(v))))
    ov = _overlay_from_edges(n, sorted(edges))
    hc.pc.setup(be, ov, T, seed=11, mesh_degree=300, disconnect_frac=0.02)
    be.set_gossipsub_params(_gp(d_hi=40, d=33, d_score=33, d_lo=5, d_out=2))
    outs, snaps = [], []
    for k in range(3):
        now = hc.T0 + (3 + k) * S
        outs.append(be.heartbeat(59 + k, now, 1234).as_dict())
        snaps.append(hc.snapshot(be))
        cfg = hc.pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=k % T, latency_ms=5, seed=k)
        cfg.now_ns = now + 100 * MS
        be.propagate(hc.pc.messages(n, 70, 100 + k), cfg)
        be.refresh(now + 500 * MS)
    return ov, outs, snaps


def hub_sort_check(outs):
    assert outs[0]["prunes"] > 2 * (300 - 40), outs[0]  # the hub's ~300 mesh peers per topic went down to 33

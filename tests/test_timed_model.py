"""The timed-propagation model (timed_model.py) against the propagation oracle
where they must agree (every link the same latency), against Dijkstra where
the arrival time is a shortest path (floodsub), and on a case small enough to
work out by hand.  CPU only: these are the equalities the GPU tests of
gsx_propagate_timed rely on (test_gpu_timed_prop.py)."""
import heapq

import numpy as np
import pytest

import oracle as orc
import propagation_cases as pc
import timed_model as tm
from gsx import abi, synth

TICK = 5 * abi.MILLISECOND
FS, GS = abi.GSX_ROUTER_FLOODSUB, abi.GSX_ROUTER_GOSSIPSUB


def ticks_of_hops(hop, l, vd):
    h = hop.astype(np.int64)
    return np.where(hop == 0xFF, 0xFFFF, np.where(h == 0, 0, h * l + (h - 1) * vd)).astype(np.uint16)


UNIFORM = [  # (name, router, n, m, overlay kw, setup kw, invalid, flood_publish)
    ("floodsub", FS, 300, 64, {}, {}, 0.0, 0),
    ("gossipsub", GS, 500, 100, dict(mix_protocols=True, direct_frac=0.05), dict(disconnect_frac=0.05), 0.0, 0),
    ("gossipsub-invalid", GS, 500, 100, dict(mix_protocols=True, direct_frac=0.05), dict(disconnect_frac=0.05), 0.25, 0),
    ("gossipsub-floodpub", GS, 500, 130, dict(mix_protocols=True), {}, 0.0, 1),
]


@pytest.mark.parametrize("l,vd", [(1, 0), (3, 0), (1, 2), (3, 2)])
@pytest.mark.parametrize("case", UNIFORM, ids=[c[0] for c in UNIFORM])
def test_model_equals_oracle_at_uniform_latency(case, l, vd):
    _, router, n, m, okw, skw, invalid, fp = case
    ov = pc.overlay(n, 6, seed=11, **okw)
    o = orc.Oracle(1)
    pc.setup(o, ov, 1, seed=11, **skw)
    ms = pc.messages(n, m, seed=11, invalid=invalid)
    tcfg = pc.config(router, flood_publish=fp, latency_ms=5, delay_ms=5.0 * vd)
    lat = np.full(ov.n_pairs, l, dtype=np.uint8)
    st0 = o.export_state()
    r = tm.run_on(o, ov, lat, ms, tcfg, 65534)
    out, hop, frm = o.propagate(ms, pc.config(router, flood_publish=fp, latency_ms=5 * l, delay_ms=5.0 * vd),
                                want_results=True)
    assert out.hops < 40  # the oracle's hop bound did not cut the call
    assert np.array_equal(r.tick, ticks_of_hops(hop, l, vd))
    assert np.array_equal(r.first_from, frm)
    want = out.as_dict()
    got = tm.counters(r)
    for k in ("deliveries", "duplicates", "transmissions", "rejected", "ignored", "graylisted"):
        assert got[k] == want[k], k
    assert got["last_tick"] == (out.hops * l + (out.hops - 1) * vd if out.hops else 0)
    # the per-pair counts: folded with "+1 then cap" they give the oracle's state after GSX_CREDIT_NOW
    tp = synth.spam_test_topic_params()
    st1 = o.export_state()
    mine = tm.fold(st0, 1, 0, r.first, r.dup_in, r.inv, tp.first_message_deliveries_cap, tp.mesh_message_deliveries_cap)
    for f in abi.STATE_FIELDS:
        assert np.array_equal(np.asarray(mine[f]).view(np.uint8), np.asarray(st1[f]).view(np.uint8)), f
    if router == GS and l == 3:  # 15 ms hops against a 25 ms window: the window does split the copies
        assert 0 < got["dup_in_window"] < got["duplicates"]


def dijkstra(ov, w, src):
    """Shortest arrival over weights w[(u -> v)] of a copy v sends to u."""
    dist = np.full(ov.n, np.iinfo(np.int64).max, dtype=np.int64)
    dist[src] = 0
    obs = ov.pair_observer()
    # pairs by sender: pair q = (u -> v) is an edge v -> u
    by_sender = [[] for _ in range(ov.n)]
    for q in range(ov.n_pairs):
        by_sender[int(ov.col[q])].append((int(obs[q]), int(w[q])))
    heap = [(0, src)]
    while heap:
        d, v = heapq.heappop(heap)
        if d > dist[v]:
            continue
        for u, c in by_sender[v]:
            if d + c < dist[u]:
                dist[u] = d + c
                heapq.heappush(heap, (d + c, u))
    return dist


@pytest.mark.parametrize("vd", [0, 2])
@pytest.mark.parametrize("symmetric", [True, False])
def test_floodsub_arrival_is_the_shortest_path(vd, symmetric):
    ov = pc.overlay(300, 3, seed=4)
    lat = synth.link_latency(ov, 4, 1, 7, symmetric=symmetric)
    assert lat.min() == 1 and lat.max() == 7
    ms = pc.messages(ov.n, 24, seed=4)
    E = ov.n_pairs
    r = tm.run(ov.row_ptr, ov.col, ov.edge_flags, np.full(E, 3, np.uint8), np.zeros(E, np.uint8), np.zeros(E), -200.0,
               -300.0, lat, ms, FS, 0, TICK, vd * TICK, 25 * abi.MILLISECOND, 65534)
    for k, src in enumerate(ms["source"]):
        d = dijkstra(ov, lat.astype(np.int64) + vd, int(src))
        reach = d < np.iinfo(np.int64).max
        want = np.where(np.arange(ov.n) == src, 0, d - vd)
        assert np.array_equal(r.tick[k][reach].astype(np.int64), want[reach])
        assert np.all(r.tick[k][~reach] == 0xFFFF)
    assert r.deliveries == int(((r.tick != 0xFFFF) & (r.tick != 0)).sum())


def five_nodes(slow):
    """Links 0-1, 1-4 (1 tick each), 0-2, 2-4 (`slow` ticks each), 3-4 (1 tick)."""
    links = {(0, 1): 1, (1, 4): 1, (0, 2): slow, (2, 4): slow, (3, 4): 1}
    pairs = sorted([(a, b) for a, b in links] + [(b, a) for a, b in links])
    row_ptr = np.zeros(6, dtype=np.int64)
    for u, _ in pairs:
        row_ptr[u + 1] += 1
    col = np.array([v for _, v in pairs], dtype=np.int32)
    lat = np.array([links.get((u, v), links.get((v, u))) for u, v in pairs], dtype=np.uint8)
    return np.cumsum(row_ptr), col, lat, {p: i for i, p in enumerate(pairs)}


def test_five_nodes_by_hand():
    """Node 0 publishes one message at tick 0; floodsub, no validation delay, a window of 2 ticks.

    Slow side of 3 ticks a link:
      tick 1: 1 gets it from 0.                  tick 2: 4 gets it from 1 (first copy of 4).
      tick 3: 2 gets it from 0, 3 gets it from 4.
      tick 5: 4's copy reaches 2 (sent at 2, 3 ticks): a duplicate 5 - 3 = 2 ticks after 2's
              first copy: inside the window.
      tick 6: 2's copy reaches 4 (sent at 3): a duplicate 6 - 2 = 4 ticks after: outside.
      -> 4 deliveries, 2 duplicates, 1 inside; pair (2 -> 4) has the in-window one, (4 -> 2) none.
    Every link 1 tick:
      tick 1: 1 and 2 get it.  tick 2: 4 gets it from 1 (the lower sender) and, a duplicate of
      the same tick, from 2: inside.  tick 3: 3 gets it from 4; 4's copy reaches 2 (4 did not
      get it from 2), 3 - 1 = 2 ticks after: inside.
      -> 4 deliveries, 2 duplicates, 2 inside."""
    ms = np.zeros(1, dtype=abi.msg_dtype())
    for slow, ticks, n_in, in42 in ((3, [0, 1, 3, 3, 2], 1, 0), (1, [0, 1, 1, 3, 2], 2, 1)):
        row_ptr, col, lat, idx = five_nodes(slow)
        E = len(col)
        r = tm.run(row_ptr, col, np.full(E, abi.GSX_EDGE_GOSSIPSUB, np.uint8), np.full(E, 3, np.uint8),
                   np.zeros(E, np.uint8), np.zeros(E), -200.0, -300.0, lat, ms, FS, 0, TICK, 0, 2 * TICK, 65534)
        assert r.tick[0].tolist() == ticks
        assert r.first_from[0].tolist() == [-1, 0, 0, 4, 1]
        assert (r.deliveries, r.duplicates, r.dup_in_window) == (4, 2, n_in)
        assert r.dup_in[idx[(2, 4)]] == 1 and r.dup_in[idx[(4, 2)]] == in42
        assert int(r.dup_in.sum()) == n_in and int(r.first.sum()) == 4
        assert r.first[idx[(4, 1)]] == 1 and r.first[idx[(4, 2)]] == 0
        assert r.last_tick == 3 and r.ticks_run == (6 if slow == 3 else 3)

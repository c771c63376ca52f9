"""One engine reused across propagation calls of different shapes, against the
CPU oracle running the same sequence.  gsx_prop_begin keeps hist, occ,
origin, vmask, seen, from, sel and the staging between calls whenever the new
call fits the old capacity, and most of them are strided by the capacity
(words_cap, msgs_cap, rows_cap) rather than by the call's own word count, so
the sequences here move the message count, the hop limit, the router, the
topic, the validation outcomes and the tracking mode up and down on ONE
engine.  After every call the counters, arrival hops, first deliverers,
gsx_prop_stats, every exported state array and the scores must equal the
oracle's, bit for bit.

A second, order-free reference separates "the reused engine differs" from
"the engine and the oracle share a bug": before some narrow calls that follow
a wide one the engine's state is exported and imported into a fresh engine,
which runs that single call; both engines must agree."""
import numpy as np
import pytest

import gsx
import oracle as orc
import propagation_cases as pc
from gsx import abi, synth

pytestmark = pytest.mark.gpu

H = abi.GSX_MAX_HOPS + 1
N, D, T = 300, 5, 2

# the word counts go up and down: 1, 1, 2, 16, 1, 4, 1, 0, 4, 1
MSGS = [1, 64, 65, 1024, 3, 200, 64, 0, 129, 1]
# both sides of prop_begin's GSX_MAX_HOPS / 2 + 1 row floor
MAX_HOPS = [40, 2, 33, 1, 40]
# RandomSub's `sel` rows are strided by the capacity words too
ROUTERS = [abi.GSX_ROUTER_GOSSIPSUB, abi.GSX_ROUTER_FLOODSUB, abi.GSX_ROUTER_RANDOMSUB, abi.GSX_ROUTER_GOSSIPSUB]
# narrow calls right after a wide one: 3 after 1024, 64 after 200, 1 after 129
FRESH_AT = (4, 6, 9)


def call(k, seed, latency_ms, n=N):
    """Call k of the sequence on an overlay of n nodes -> (messages, config).  Every third call carries
    messages validation does not accept, and a validation delay."""
    m = MSGS[k % len(MSGS)]
    bad = k % 3 == 2
    ms = pc.messages(n, m, seed + 10 * k, invalid=0.25 if bad else 0.0)
    cfg = pc.config(ROUTERS[k % len(ROUTERS)], topic=k % T, max_hops=MAX_HOPS[k % len(MAX_HOPS)], latency_ms=latency_ms,
                    size=50, seed=seed + k, delay_ms=3.0 if bad else 0.0)
    cfg.now_ns = pc.T0 + 3 * pc.S + k * 100 * abi.MILLISECOND
    return ms, cfg


def expected_stats(hop, n):
    """gsx_prop_stats in numpy from a hop matrix [m, n]."""
    hist = np.zeros((hop.shape[0], H), dtype=np.uint32)
    for k, row in enumerate(hop):
        hist[k] = np.bincount(row, minlength=256)[:H]
    got = (hop >= 1) & (hop <= abi.GSX_MAX_HOPS)
    if hop.shape[0] == 0:
        return hist, np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    return hist, got.sum(0).astype(np.uint32), (hop.astype(np.uint64) * got).sum(0).astype(np.uint64)


def window(be, window_ms):
    for t in range(T):
        tp = synth.spam_test_topic_params()
        tp.mesh_message_deliveries_window_ns = int(window_ms * abi.MILLISECOND)
        be.set_topic_params(t, tp)


def same_state(tag, a, b):
    sa, sb = a.export_state(), b.export_state()
    for f in abi.STATE_FIELDS:
        assert np.array_equal(sa[f].view(np.uint8), sb[f].view(np.uint8)), (tag, f)
    assert sa["last_refresh_ns"] == sb["last_refresh_ns"], tag
    assert np.array_equal(a.scores().view(np.uint64), b.scores().view(np.uint64)), tag
    return sa


def same_call(tag, eng, got, want, tracked, n):
    """The engine's call against a reference's: counters, hops, first deliverers, gsx_prop_stats."""
    (go, gh, gf), (wo, wh, wf) = got, want
    assert go.as_dict() == wo.as_dict(), (tag, go.as_dict(), wo.as_dict())
    assert gh.shape == wh.shape and np.array_equal(gh, wh), (tag, np.argwhere(gh != wh)[:5])
    if tracked:
        assert np.array_equal(gf, wf), (tag, np.argwhere(gf != wf)[:5])
    else:
        assert gf is None, tag
    hist, recv, hsum = expected_stats(wh, n)
    st = eng.prop_stats(len(wh), per_node=True)
    assert np.array_equal(st.hop_hist, hist), (tag, np.argwhere(st.hop_hist != hist)[:5])
    assert np.array_equal(st.node_received, recv) and np.array_equal(st.node_hop_sum, hsum), tag


def fresh_engine(ov, app, state, window_ms, tracked):
    """A new engine with the same parameters, overlay and app scores, holding `state`."""
    e = gsx.Engine(T)
    e.set_peer_params(synth.bench_peer_params())
    window(e, window_ms)
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                    accept_px_threshold=0, opportunistic_graft_threshold=0))
    e.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    e.import_state(state)
    e.set_app_scores(app)
    e.set_prop_tracking(tracked)
    return e


@pytest.mark.parametrize("lean", [False, True], ids=["lat10", "lat0-window5min"])
@pytest.mark.parametrize("track", [True, False, "toggled"], ids=["rows", "counts", "toggled"])
def test_engine_reused_across_shapes_matches_oracle(gpu_ok, track, lean):
    """lat10: 10 ms hops against a 25 ms P3 window (the per-hop folds).
    lat0-window5min: every duplicate inside the window (the lean hop kernels
    where nothing is tracked).  toggled: gsx_prop_set_tracking flips between
    calls (P.from is sized by the capacity words x pairs)."""
    seed = 211 + (3 if lean else 0) + {True: 0, False: 1, "toggled": 2}[track]
    latency_ms, window_ms = (0, 300_000) if lean else (10, 25)
    ov = pc.overlay(N, D, seed, mix_protocols=True)
    eng, ref = gsx.Engine(T), orc.Oracle(T)
    for be in (eng, ref):
        app = pc.setup(be, ov, T, seed, disconnect_frac=0.02)
        window(be, window_ms)
    same_state("setup", eng, ref)
    delivered = rejected = 0
    for k in range(len(MSGS)):
        tracked = (k % 2 == 0) if track == "toggled" else track
        eng.set_prop_tracking(tracked)
        ms, cfg = call(k, seed, latency_ms)
        tag = (k, len(ms), cfg.router, cfg.max_hops)
        fresh = fresh_engine(ov, app, eng.export_state(), window_ms, tracked) if k in FRESH_AT else None
        got = eng.propagate(ms, cfg, want_results=True)
        want = ref.propagate(ms, cfg, want_results=True)
        same_call(tag, eng, got, want, tracked, N)
        same_state(tag, eng, ref)
        if fresh is not None:  # the same call on an engine that never saw the calls before it
            one = fresh.propagate(ms, cfg, want_results=True)
            same_call(tag + ("fresh",), fresh, one, got, tracked, N)
            same_state(tag + ("fresh",), fresh, eng)
            fresh.close()
        delivered += got[0].deliveries
        rejected += got[0].rejected
    assert delivered > 0 and rejected > 0


def test_engine_reloaded_overlays_match_oracle(gpu_ok):
    """gsx_load_overlay on a used engine: 600 nodes and two calls, then 150
    nodes with new parameters and state and the sequence's first four calls."""
    eng, ref = gsx.Engine(T), orc.Oracle(T)
    big = pc.overlay(600, D, 307, mix_protocols=True)
    small = pc.overlay(150, 4, 311, mix_protocols=True)
    for be in (eng, ref):
        pc.setup(be, big, T, 307, disconnect_frac=0.02)
    for k in (3, 1):  # 1024 messages (16 words), then 64
        ms, cfg = call(k, 307, 10, 600)
        got, want = eng.propagate(ms, cfg, want_results=True), ref.propagate(ms, cfg, want_results=True)
        same_call(("big", k), eng, got, want, True, 600)
        same_state(("big", k), eng, ref)
    for be in (eng, ref):
        pc.setup(be, small, T, 311, mesh_degree=4, disconnect_frac=0.05)
        window(be, 40)
        be.set_thresholds(abi.Thresholds(gossip_threshold=-10, publish_threshold=-20, graylist_threshold=-30,
                                         accept_px_threshold=0, opportunistic_graft_threshold=0))
    same_state("reloaded", eng, ref)
    delivered = 0
    for k in range(4):
        ms, cfg = call(k, 311, 10, 150)
        got, want = eng.propagate(ms, cfg, want_results=True), ref.propagate(ms, cfg, want_results=True)
        same_call(("small", k), eng, got, want, True, 150)
        same_state(("small", k), eng, ref)
        delivered += got[0].deliveries
    assert delivered > 0

"""gsx_prop_stats through the multi-GPU drivers (gsx/shard.py) on one GPU, in
the pattern of test_gpu_shard.py: the range shards' summed histogram and the
message-parallel replicas' gathered table equal the one-engine histogram, which
numpy computes from the one-engine gsx_prop_results hop matrix.  Exact."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported on the main thread before the shard threads use it)

import gsx
import propagation_cases as pc
from gsx import abi, shard, synth

pytestmark = pytest.mark.gpu

H = abi.GSX_MAX_HOPS + 1


def expected(hop):
    hist = np.zeros((hop.shape[0], H), dtype=np.uint32)
    for k, row in enumerate(hop):
        hist[k] = np.bincount(row, minlength=256)[:H]
    got = (hop >= 1) & (hop <= abi.GSX_MAX_HOPS)
    return hist, got.sum(0).astype(np.uint32), (hop.astype(np.uint64) * got).sum(0).astype(np.uint64)


def _params(e, T):
    e.set_peer_params(synth.bench_peer_params())
    for t in range(T):
        tp = synth.spam_test_topic_params()
        tp.mesh_message_deliveries_window_ns = 25 * abi.MILLISECOND
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


CASES = [
    # world, n, router, m, compact, track, invalid
    (2, 700, abi.GSX_ROUTER_GOSSIPSUB, 130, True, True, 0.0),
    (2, 700, abi.GSX_ROUTER_GOSSIPSUB, 130, False, True, 0.0),
    (3, 650, abi.GSX_ROUTER_FLOODSUB, 70, True, False, 0.0),
    (3, 650, abi.GSX_ROUTER_GOSSIPSUB, 200, True, True, 0.25),
]


@pytest.mark.parametrize("case", CASES, ids=["w2-compact", "w2-dense", "w3-counts", "w3-invalid"])
def test_range_sharded_stats(gpu_ok, case):
    world, n, router, m, compact, track, invalid = case
    T, seed = 1, 5 * n + m
    ov = pc.overlay(n, 2, seed, mix_protocols=True, direct_frac=0.03)
    msgs = pc.messages(n, m, seed, invalid=invalid)
    cfg = pc.config(router, size=60, delay_ms=3.0 if invalid else 0.0)
    full = gsx.Engine(T)
    app = pc.setup(full, ov, T, seed, disconnect_frac=0.4)
    st0 = full.export_state()
    out = full.propagate(msgs, cfg)[0]
    hop, _ = full.prop_results(m)
    hist, recv, hsum = expected(hop)
    one = full.prop_stats(m, per_node=True)
    assert np.array_equal(one.hop_hist, hist)

    rank_lo = synth.shard_ranges(n, world)
    E = ov.n_pairs
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
        e.set_prop_tracking(track)
        engines.append(e)

    def run(tp, e):
        rs = shard.RangeSharded(e, rank_lo, tp, compact=compact)
        tot = rs.propagate(msgs, cfg)[1]
        return tot, rs.prop_stats(m, per_node=True), e.prop_stats(m)

    res = shard.run_local(world, "cuda:0", run, [(e,) for e in engines])
    assert res[0][0]["deliveries"] == out.deliveries > 0
    local = None
    for k, (_, st, mine) in enumerate(res):
        lo, hi = int(rank_lo[k]), int(rank_lo[k + 1])
        assert np.array_equal(st.hop_hist, hist), (k, np.argwhere(st.hop_hist != hist)[:5])  # the summed table, on every rank
        assert np.array_equal(st.node_received, recv[lo:hi]), k  # the per-node arrays stay per rank
        assert np.array_equal(st.node_hop_sum, hsum[lo:hi]), k
        assert np.array_equal(mine.hop_hist, expected(hop[:, lo:hi])[0]), k  # this rank's nodes alone
        local = mine if local is None else local + mine
    assert np.array_equal(local.hop_hist, hist)  # PropStats.__add__ over the ranks
    if invalid:
        bad = msgs["validation"] != abi.GSX_VALIDATION_ACCEPT
        assert (hist[bad, 1] > 0).any() and not hist[bad, 2:].any()
    assert (hop == 0xFF).any()


def test_message_parallel_stats(gpu_ok):
    world, n, m, T, seed = 3, 600, 300, 1, 23
    ov = pc.overlay(n, 5, seed, mix_protocols=True, direct_frac=0.02)
    msgs = pc.messages(n, m, seed)
    cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, latency_ms=4)
    full = gsx.Engine(T)
    pc.setup(full, ov, T, seed, disconnect_frac=0.05)
    out = full.propagate(msgs, cfg)[0]
    hop, _ = full.prop_results(m)
    hist, recv, hsum = expected(hop)
    assert np.array_equal(full.prop_stats(m).hop_hist, hist)
    reps = []
    for _ in range(world):
        e = gsx.Engine(T)
        pc.setup(e, ov, T, seed, disconnect_frac=0.05)
        reps.append(e)

    def run(tp, e):
        mp = shard.MessageParallel(e, tp)
        tot = mp.propagate(msgs, cfg)[1]
        return tot, mp.prop_stats(m, per_node=True)

    res = shard.run_local(world, "cuda:0", run, [(e,) for e in reps])
    assert res[0][0]["deliveries"] == out.deliveries > 0
    for _, st in res:
        assert np.array_equal(st.hop_hist, hist), np.argwhere(st.hop_hist != hist)[:5]
        assert np.array_equal(st.node_received, recv)
        assert np.array_equal(st.node_hop_sum, hsum)

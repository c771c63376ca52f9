"""gsx_score_stats through RangeSharded (gsx/shard.py) on one GPU, in the pattern
of test_gpu_prop_stats_shard.py: every rank gets the full engine's hist,
peer_bins and peer_min (one all-reduce of the sums, one of the minima) and its
own rows of obs_bins / obs_min; the ranks' local tables add up to the full
table (ScoreStats.__add__).  Exact."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported on the main thread before the shard threads use it)

import gsx
import propagation_cases as pc
import score_stats_cases as sc
from gsx import abi, shard, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND


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
    # world, n, T, select, topic
    (2, 700, 1, "present", 0),
    (3, 650, 2, "mesh", 1),
    (3, 650, 1, "connected", 0),
]


@pytest.mark.parametrize("case", CASES, ids=["w2-present", "w3-mesh", "w3-connected"])
def test_range_sharded_score_stats(gpu_ok, case):
    world, n, T, select, topic = case
    seed = 3 * n + world
    ov = pc.overlay(n, 2, seed, mix_protocols=True, direct_frac=0.03)
    full = gsx.Engine(T)
    app = pc.setup(full, ov, T, seed, disconnect_frac=0.3)
    full.propagate(pc.messages(n, 60, seed), pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=T - 1))  # credits spread the scores
    st0 = full.export_state()
    now = pc.T0 + 5 * S
    full.refresh(now)
    scores, st1 = full.scores(), full.export_state()
    edges = sc.edges_from(scores[st1["pair_flags"] != 0], 5)
    one = full.score_stats(edges, select, topic)
    sc.assert_equal(one, sc.reference(scores, st1["pair_flags"], st1["rec_flags"], ov.row_ptr, ov.col, n, edges,
                                      select, topic))
    assert int(one.hist.sum()) > 0 and (st1["pair_flags"] == 0).any()

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
        e.refresh(now)  # the same refresh on every rank
        engines.append(e)

    def run(tp, e):
        rs = shard.RangeSharded(e, rank_lo, tp)
        return rs.score_stats(edges, select, topic), e.score_stats(edges, select, topic)

    res = shard.run_local(world, "cuda:0", run, [(e,) for e in engines])
    local = None
    for k, (st, mine) in enumerate(res):
        lo, hi = int(rank_lo[k]), int(rank_lo[k + 1])
        want = {"hist": one.hist, "peer_bins": one.peer_bins, "peer_min": one.peer_min,
                "obs_bins": one.obs_bins[lo:hi], "obs_min": one.obs_min[lo:hi]}
        sc.assert_equal(st, want, what=("rank", k))  # the whole overlay's table, this rank's rows
        assert mine.peer_bins.shape == (n, len(edges) + 1) and mine.obs_bins.shape == (hi - lo, len(edges) + 1)
        sc.assert_equal(mine, {"obs_bins": one.obs_bins[lo:hi], "obs_min": one.obs_min[lo:hi]},
                        fields=("obs_bins", "obs_min"), what=("local", k))
        local = mine if local is None else local + mine
    sc.assert_equal(local, {f: getattr(one, f) for f in sc.FIELDS}, what="sum of the local tables")

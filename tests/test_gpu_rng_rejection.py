"""Go's Int31n redraw (`for v > max`) on the GPU: Rng::int31n in the shuffles,
wave_floyd's ballot, the IWANT selection sampling's lane-parallel forms and
host_int31n, on runs whose seeds were searched so that the oracle's run
takes the branch (rejection_cases.SEEDS, found by
tools/find_rejection_seeds.py).  Every case first asserts that the oracle
rejected at least the recorded number of draws of its tag, then that the
engine equals the oracle bit for bit."""
import numpy as np
import pytest

import gossip_cases as gc
import gsx
import oracle as orc
import rejection_cases as rc
from test_gpu_gossip import _same as _same_exchange
from test_gpu_heartbeat import _same as _same_state

pytestmark = pytest.mark.gpu


def _oracle(fn, tag, recorded):
    """fn's result on the oracle, after asserting its run redrew at least
    `recorded` draws of `tag`."""
    orc.rng_rejections_reset()
    res = fn()
    got = orc.rng_rejections().get(tag, 0)
    assert got >= recorded > 0, f"tag {tag}: the oracle rejected {got} draws, {recorded} recorded: search the seed again"
    return res


def _rounds_equal(go, gs, wo, ws):
    for k in range(len(wo)):
        assert go[k] == wo[k], (k, go[k], wo[k])
        _same_state(gs[k], ws[k], f"tick {k}")


def test_hub_shuffle_redraws(gpu_ok):
    """A hub with 10,000 peers (one wave): its shuffles of thousands of
    entries; the star's leaves never redraw, so the hub's stream did."""
    c = rc.SEEDS["hub"]
    wo, ws = _oracle(lambda: rc.hub_run(orc.Oracle(2), c["seed"]), rc.TAG_SHUFFLE, c["rej"][rc.TAG_SHUFFLE])
    go, gs = rc.hub_run(gsx.Engine(2), c["seed"])
    _rounds_equal(go, gs, wo, ws)
    assert wo[0]["prunes"] > rc.HUB_PEERS


def test_lane_shuffle_redraws(gpu_ok):
    """Nodes of about 50 peers (one lane each, lists of at most 64)."""
    c = rc.SEEDS["lane"]
    T = rc.LANE["T"]
    _, wo, ws = _oracle(lambda: rc.lane_run(orc.Oracle(T), c["seed"]), rc.TAG_SHUFFLE, c["rej"][rc.TAG_SHUFFLE])
    _, go, gs = rc.lane_run(gsx.Engine(T), c["seed"])
    _rounds_equal(go, gs, wo, ws)
    assert sum(o["grafts"] + o["prunes"] for o in wo) > 0


@pytest.mark.parametrize("placement", [p for p in ("any", "lane0", "last_step", "two_in_batch") if p in rc.SEEDS["trunc"]])
def test_truncated_lists_redraw(gpu_ok, placement):
    """wave_floyd: lists of tens of thousands of ids cut to 7,000 per target.
    The placement of a redraw in its 64-step batch (lane 0; the last step
    kk - 1; two rejecting lanes in one ballot) is replayed from the hash of
    the target's stream and asserted before the engine runs."""
    c = rc.SEEDS["trunc"][placement]
    kw = rc.TRUNC
    be = rc.ListLengths(orc.Oracle(kw["T"]), kw["n"], kw["T"], kw["history_gossip"])
    w = _oracle(lambda: gc.exchange_run(be, seed=c["seed"], **kw), rc.TAG_IHAVE_SUB, c["rej"][rc.TAG_IHAVE_SUB])
    tot, hits = rc.trunc_placements(c["seed"], w[0], be.L, w[2], kw["max_ihave_length"])
    assert tot == orc.rng_rejections()[rc.TAG_IHAVE_SUB]  # the replay sees the oracle's redraws, all of them
    if placement != "any":
        assert placement in rc.placements_of(hits), hits
    g = gc.exchange_run(gsx.Engine(kw["T"]), seed=c["seed"], **kw)
    _same_exchange(g, w)


@pytest.mark.parametrize("path", ["heavy", "light"])
def test_iwant_sampling_redraws(gpu_ok, path):
    """The IWANT selection sampling (kk < n: two topics' lists in one RPC
    against one budget) and AddPromise's pick.  heavy: batches of 141 words,
    every asker's pass 1 in k_gx_node; light: 108 unseen words at most, the
    asker's own lane (GX_MW = 128)."""
    c = rc.SEEDS["iwant_" + path]
    kw = rc.IWANT_HEAVY if path == "heavy" else rc.IWANT_LIGHT
    w = _oracle(lambda: gc.exchange_run(orc.Oracle(kw["T"]), seed=c["seed"], **kw), rc.TAG_IWANT, c["rej"][rc.TAG_IWANT])
    assert sum(o["iwant_msgs"] for o in w[1]) > 0
    g = gc.exchange_run(gsx.Engine(kw["T"]), seed=c["seed"], **kw)
    _same_exchange(g, w)


def test_promise_add_redraws(gpu_ok):
    """host_int31n: gsx_promise_add's pick among 1000 handles with seeds whose
    first draw is rejected; the kept promise is the oracle's (and the one the
    hash predicts: fulfilling that handle leaves none)."""
    c = rc.SEEDS["promise"]
    w = _oracle(lambda: rc.promise_run(orc.Oracle(1), c["seeds"]), rc.TAG_IWANT, c["rej"][rc.TAG_IWANT])
    g = rc.promise_run(gsx.Engine(1), c["seeds"])
    assert g == w
    assert all(before == 1 and after == 0 for _, before, after in g), g


def test_promise_add_draw_equals_max(gpu_ok):
    """host_int31n at the boundary: the first draw of this seed equals max of
    Int31n(1000) exactly (asserted from the hash), so `v > max` keeps it
    (handle 999, no redraw on the oracle) where `v >= max` would redraw."""
    s = rc.SEEDS["promise_eq"]["seed"]
    assert rc.promise_eq(s)
    orc.rng_rejections_reset()
    w = rc.promise_run(orc.Oracle(1), [s])
    assert orc.rng_rejections() == {}
    g = rc.promise_run(gsx.Engine(1), [s])
    assert g == w and g[0][1:] == (1, 0), (g, w)
    assert g[0][0] == 999 * 7 + 11  # max % 1000 = 999


def test_hub_shuffle_draw_equals_max(gpu_ok):
    """Rng::int31n at the boundary, on the device: a step k of the hub's first
    shuffle of round 59 draws exactly max of Int31n(k + 1) (from the hash; the
    mesh is longer than k and the oracle's round redraws nothing, so counter k
    is step k).  `v > max` keeps the draw, `v >= max` would redraw it and
    shift every later draw of the stream."""
    c = rc.SEEDS["hub_eq"]
    hits = rc.hub_eq_hits(c["seed"])
    assert hits and hits == c["hits"]
    pre = []
    orc.rng_rejections_reset()
    wo, ws = rc.hub_run(orc.Oracle(2), c["seed"], ticks=1, pre=pre)
    assert orc.rng_rejections().get(rc.TAG_SHUFFLE, 0) == 0
    assert all(pre[0][t] > k for t, k in hits) and min(pre[0]) > 12  # above Dhi: the shuffle runs
    go, gs = rc.hub_run(gsx.Engine(2), c["seed"], ticks=1)
    _rounds_equal(go, gs, wo, ws)
    assert wo[0]["prunes"] > rc.HUB_EQ_K

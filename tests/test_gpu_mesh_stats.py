"""gsx_mesh_stats on the GPU: every table against the model of the contract
(mesh_stats_model.py) fed from the engine's own exports.  Everything is an
integer count: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library loads: both then share one HIP runtime)

import gsx
import heartbeat_cases as hc
import mesh_stats_model as msm
import nonfinite_cases as nf
import oracle as orc
import propagation_cases as pc
import test_mesh_stats_model as cpu
from gsx import abi

pytestmark = pytest.mark.gpu

S = abi.SECOND
COL = cpu.COL
AGES = [0, S, 2 * S + S // 2]


def call(e, now, **kw):
    kw.setdefault("age_edges_ns", AGES)
    return e.mesh_stats(now, **kw)


def model(e, ov, now, gp=None, **kw):
    kw.setdefault("age_edges_ns", AGES)
    return msm.of_backend(e, ov.row_ptr, ov.col, ov.edge_flags, gp or orc.default_gossipsub_params(), now, **kw)


def assert_same(got, ref, what=""):
    for f in msm.FIELDS:
        g = getattr(got, f)
        if g is None:
            assert ref[f].size == 0, (what, f)
            continue
        r = ref[f].reshape(g.shape)
        assert g.dtype == r.dtype, (what, f, g.dtype)
        if not np.array_equal(g, r):
            bad = np.argwhere(g != r)[:5]
            raise AssertionError(f"{what} {f}: differs at {bad.tolist()}: got {[int(g[tuple(i)]) for i in bad]} "
                                 f"want {[int(r[tuple(i)]) for i in bad]}")


def check(e, ov, now, what="", gp=None, **kw):
    got = call(e, now, **kw)
    ref = model(e, ov, now, gp, **kw)
    assert_same(got, ref, what)
    return got


# ---- 1. sizes: a partial wave; rows cut by tile edges, three node tiles, T above the kernel-argument path ----
def test_a_single_partial_wave(gpu_ok):
    ov = pc.overlay(20, 3, 3)
    assert 0 < ov.n_pairs < 64 or ov.n_pairs % 64
    e = gsx.Engine(1)
    pc.setup(e, ov, 1, 3, mesh_degree=3)
    got = check(e, ov, pc.T0 + 3 * S, "n = 20")
    assert got.total("links") > 0


@pytest.mark.parametrize("T", [1, 3, 9])
def test_random_mesh_before_any_heartbeat(gpu_ok, T):
    ov = pc.overlay(130, 3, 7 + T)
    e = gsx.Engine(T)
    pc.setup(e, ov, T, 7 + T, mesh_degree=4, disconnect_frac=0.1)
    got = check(e, ov, pc.T0 + 3 * S, T)
    assert got.total("one_sided") > 0 and got.total("backoff") == got.total("backoff_expired") == 0
    assert got.total("negative") > 0 and (got.topic_tot[:, COL["links"]] > 0).all()


@pytest.mark.parametrize("T", [1, 3, 9])
def test_after_three_heartbeats(gpu_ok, T):
    e = gsx.Engine(T)
    ov, outs, snaps = hc.mesh_run(e, 130, 3, T, seed=11 + T, ticks=3, mesh_degree=4, disconnect=0.1)
    b = e.export_backoff()
    tt, pp = np.nonzero(b)
    assert len(tt) >= 4
    b[tt[::3], pp[::3]] = pc.T0 + S  # every third entry has run out and waits for clearBackoff
    e.import_backoff(b)
    now = pc.T0 + 10 * S  # splits the entries into live and expired
    pf = snaps[-1]["pair_flags"]
    assert (pf == abi.GSX_PAIR_PRESENT).any()  # retained pairs
    got = check(e, ov, now, T)
    assert got.total("backoff") > 0 and got.total("backoff_expired") > 0
    assert got.total("links") == outs[-1]["mesh_links"]
    assert int(got.node_deg.sum()) == int(got.node_in.sum()) == got.total("links")
    for h in (got.deg_hist, got.out_hist, got.in_hist):
        assert np.array_equal(h.sum(1), got.topic_tot[:, COL["units"]])
    # a now_ns below some graft times: negative ages land in bin 0
    early = check(e, ov, pc.T0 + 2 * S, (T, "early"))
    assert early.age_hist[:, 0].sum() > 0 and early.age_hist[:, 1:].sum() > 0


# ---- 2. a hub: its row spans seven waves, every segment adds with an atomic --------------------------------
def test_a_hub_row(gpu_ok):
    n, hub = 400, 5
    ov = pc.with_hub(pc.overlay(n, 3, 21), hub, n - 1, 21)
    assert np.diff(ov.row_ptr)[hub] == n - 1
    e = gsx.Engine(2)
    pc.setup(e, ov, 2, 21, mesh_degree=500)  # the hub grafts its whole row
    got = check(e, ov, pc.T0 + 3 * S, "hub", n_bins=64)
    assert got.degree(0)[hub] > 300 and got.deg_hist[0, 63] >= 1 and got.total("above_dhi", 0) >= 1


# ---- 3. partial subscriptions and fanout -------------------------------------------------------------------
def test_partial_subscriptions_and_fanout(gpu_ok):
    n, T, seed = 130, 3, 31
    ov = pc.overlay(n, 3, seed)
    e = gsx.Engine(T)
    pc.setup(e, ov, T, seed, mesh_degree=4)
    rng = np.random.default_rng(seed)
    joined = np.zeros(n, dtype=np.uint64)
    for t in range(T):
        joined |= (rng.random(n) >= 1 / 3).astype(np.uint64) << np.uint64(t)
    e.set_subscriptions(joined)
    ms = pc.messages(n, 30, seed)
    unjoined = np.nonzero((joined & np.uint64(1)) == 0)[0]
    ms["source"] = unjoined[np.arange(len(ms)) % len(unjoined)].astype(np.uint32)
    e.propagate(ms, pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=0, latency_ms=5))
    got = check(e, ov, pc.T0 + 3 * S, "before the heartbeat")
    assert got.total("fanout_units", 0) > 0 and got.total("fanout_links", 0) >= got.total("fanout_units", 0)
    e.heartbeat(1, pc.T0 + 4 * S, 9)
    got = check(e, ov, pc.T0 + 5 * S, "after the heartbeat")
    assert got.total("fanout_units", 0) > 0
    units = [int(((joined >> np.uint64(t)) & np.uint64(1)).sum()) for t in range(T)]
    assert got.topic_tot[:, COL["units"]].tolist() == units and max(units) < n


# ---- 4. classes, symmetry off ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grown(gpu_ok):
    """One engine after two heartbeats, shared by the tests below: the call is read-only."""
    T = 2
    e = gsx.Engine(T)
    ov, outs, snaps = hc.mesh_run(e, 130, 3, T, seed=41, ticks=2, mesh_degree=3, disconnect=0.05)
    return e, ov, pc.T0 + 6 * S


@pytest.mark.parametrize("hostile_mask", [0b100, 0b011])
@pytest.mark.parametrize("min_honest", [0, 1, 3])
def test_classes(gpu_ok, grown, hostile_mask, min_honest):
    e, ov, now = grown
    cls = np.random.default_rng(5).integers(0, 3, ov.n).astype(np.uint8)
    got = check(e, ov, now, (hostile_mask, min_honest), node_class=cls, n_classes=3, hostile_mask=hostile_mask,
                min_honest=min_honest)
    assert int(got.class_links.sum()) == got.total("links") == int(got.node_class_deg.sum())
    assert (got.below_honest() == 0) == (min_honest == 0)
    if min_honest == 3:
        assert got.below_honest() > got.eclipsed()
    assert np.allclose(np.nansum(got.class_share(0), 1), 1.0)


def test_symmetry_off(gpu_ok, grown):
    e, ov, now = grown
    on, off = call(e, now), check(e, ov, now, "symmetry off", symmetry=False)
    assert on.total("one_sided") > 0 and off.total("one_sided") == 0
    on.topic_tot[:, COL["one_sided"]] = 0
    for f in msm.FIELDS:
        a, b = getattr(on, f), getattr(off, f)
        assert (a is None and b is None) or np.array_equal(a, b), f


# ---- 5. non-finite scores on mesh links ----------------------------------------------------------------------
def test_nan_and_inf_scores_on_mesh_links(gpu_ok):
    ov = pc.overlay(130, 3, 51)
    e = gsx.Engine(1)
    app = pc.setup(e, ov, 1, 51, mesh_degree=4).copy()
    st = e.export_state()
    links = np.nonzero((st["rec_flags"] & abi.GSX_REC_IN_MESH) != 0)[0]
    app[links[0]], app[links[1]], app[links[2]] = np.nan, -np.inf, np.inf
    e.set_app_scores(app)
    e.refresh(pc.T0 + 3 * S)
    sc = e.scores()
    assert np.isnan(sc[links[0]]) and sc[links[1]] == -np.inf
    got = check(e, ov, pc.T0 + 3 * S, "non-finite")
    assert got.total("negative") == int((sc[links] < 0).sum())


@pytest.mark.parametrize("T,variant", nf.CASES[:2])
def test_nonfinite_cases(gpu_ok, T, variant):
    ov = nf.overlay()
    e = gsx.Engine(T)
    nf.load(e, ov, T, variant)
    check(e, ov, pc.T0 + 3 * S, (T, variant))


# ---- 6. the reference's assertion ----------------------------------------------------------------------------
def test_opportunistic_grafting_keeps_honest_peers(gpu_ok):
    e = gsx.Engine(1)
    out, pair, row_ptr, col, ef = cpu.opportunistic(e)
    node0, back = cpu.hand_count(e, pair)
    now = hc.T0 + 2 * S
    cls = cpu.classes_of_case()
    for mh, below in ((3, 5), (2, 4)):
        got = e.mesh_stats(now, node_class=cls, n_classes=2, hostile_mask=0b10, min_honest=mh)
        ref = {f: getattr(got, f) for f in msm.FIELDS}
        cpu.check_opportunistic(ref, node0, back)
        assert got.eclipsed(0) == 0 and got.below_honest(0) == below
        assert got.class_links[0].tolist() == [[4, 6], [6, 0]]
        want = msm.reference(msm.backend_inputs(e), row_ptr, col, ef, 1, orc.default_gossipsub_params(), now,
                             node_class=cls, n_classes=2, hostile_mask=0b10, min_honest=mh)
        assert_same(got, want, mh)


# ---- 7. read-only, deterministic, device outputs ---------------------------------------------------------------
def test_read_only_and_deterministic(gpu_ok):
    T, seed = 2, 61
    e, o = gsx.Engine(T), orc.Oracle(T)
    for be in (e, o):
        ov, outs, snaps = hc.mesh_run(be, 130, 3, T, seed=seed, ticks=2, mesh_degree=3, disconnect=0.05,
                                     gp=orc.default_gossipsub_params())
    now = pc.T0 + 6 * S
    before = hc.snapshot(e)
    a, b = call(e, now), call(e, now)
    for f in msm.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None and y is None and f in ("class_links", "node_class_deg")) or x.tobytes() == y.tobytes(), f
    after = hc.snapshot(e)
    for f in before:
        x, y = np.asarray(before[f]), np.asarray(after[f])
        assert bool(nf.same_mask(x, y).all()) if x.dtype.kind == "f" else np.array_equal(x, y), f
    he, ho = e.heartbeat(3, now, seed * 31 + 7).as_dict(), o.heartbeat(3, now, seed * 31 + 7).as_dict()
    assert he == ho
    se, so = e.export_state(), o.export_state()
    assert np.array_equal(se["rec_flags"] & 3, so["rec_flags"] & 3) and np.array_equal(e.export_backoff(), o.export_backoff())
    e.timing_begin(3)
    for _ in range(2):
        call(e, now)
    tot, lo, hi, k = e.timing_end()
    assert k == 2 and tot > 0  # each call is one timed launch


def test_device_pointer_outputs(gpu_ok, grown):
    import torch

    e, ov, now = grown
    cls = (np.arange(ov.n) % 3).astype(np.uint8)
    kw = dict(node_class=cls, n_classes=3, hostile_mask=0b100, min_honest=2, n_bins=17)
    ref = call(e, now, **kw)
    T, n, B, A, NC = e.n_topics, ov.n, 17, len(AGES) + 1, 3
    shapes = {"topic_tot": (T, 16), "deg_hist": (T, B), "out_hist": (T, B), "in_hist": (T, B), "age_hist": (T, A),
              "class_links": (T, NC, NC), "node_deg": (T, n), "node_out": (T, n), "node_in": (T, n),
              "node_class_deg": (T, n, NC)}
    t = [torch.full(shapes[f], -1, dtype=torch.int32 if f.startswith("node_") else torch.int64, device="cuda:0")
         for f in msm.FIELDS]
    dcls = torch.from_numpy(cls).to("cuda:0")
    torch.cuda.synchronize()
    kw["node_class"] = dcls
    assert call(e, now, out_ptrs=t, **kw) is None
    e.sync()
    for f, x in zip(msm.FIELDS, t):
        assert np.array_equal(x.cpu().numpy().view(msm.DTYPES[f]), getattr(ref, f)), f
    # totals alone, on the device: pass 2 reads the engine's own node tables
    t[0].fill_(-1)
    torch.cuda.synchronize()
    assert call(e, now, out_ptrs=[t[0]] + [None] * 9, **kw) is None
    e.sync()
    assert np.array_equal(t[0].cpu().numpy().view(np.uint64), ref.topic_tot)
    assert_same(call(e, now, per_node=False, **kw), {f: (getattr(ref, f) if not f.startswith("node_") else np.zeros(0, np.uint32))
                                                      for f in msm.FIELDS}, "per_node off")


# ---- 8. errors: all refused on the host before any launch ---------------------------------------------------------
def raw(e, arrays, **spec):
    spec.setdefault("n_bins", 33)
    spec.setdefault("symmetry", 1)
    edges = spec.pop("edges", ())
    sp = abi.MeshStatsSpec(n_age_edges=len(edges), **spec)
    for k, x in enumerate(edges[: abi.GSX_MS_MAX_AGE_EDGES]):
        sp.age_edges_ns[k] = x
    out = abi.MeshStatsOut(**{f: a.ctypes.data for f, a in arrays.items()})
    return e.lib.gsx_mesh_stats(e.h, C.byref(sp), C.byref(out))


def test_errors_and_empty_engines(gpu_ok, grown):
    e, ov, now = grown
    T, n = e.n_topics, ov.n
    tot = {"topic_tot": np.zeros((T, 16), dtype=np.uint64)}
    cls = np.zeros(n, dtype=np.uint8)
    assert raw(e, tot, now_ns=now) == 0 and tot["topic_tot"][:, COL["links"]].sum() > 0
    for nb in (0, 1, 65):
        assert raw(e, tot, now_ns=now, n_bins=nb) == abi.GSX_EINVAL, nb
    assert raw(e, tot, now_ns=now, n_bins=2) == 0 and raw(e, tot, now_ns=now, n_bins=64) == 0
    assert raw(e, tot, now_ns=now, edges=list(range(9))) == abi.GSX_EINVAL
    assert raw(e, tot, now_ns=now, edges=[5, 5]) == abi.GSX_EINVAL and raw(e, tot, now_ns=now, edges=[5, 4]) == abi.GSX_EINVAL
    assert raw(e, tot, now_ns=now, edges=list(range(8))) == 0
    assert raw(e, tot, now_ns=now, node_class=cls.ctypes.data, n_classes=0) == abi.GSX_EINVAL
    assert raw(e, tot, now_ns=now, node_class=cls.ctypes.data, n_classes=9) == abi.GSX_EINVAL
    cls[n // 2] = 2
    assert raw(e, tot, now_ns=now, node_class=cls.ctypes.data, n_classes=2) == abi.GSX_EINVAL  # a class id out of range
    assert raw(e, tot, now_ns=now, node_class=cls.ctypes.data, n_classes=3) == 0
    cl = {"class_links": np.zeros((T, 3, 3), dtype=np.uint64)}
    ncd = {"node_class_deg": np.zeros((T, n, 3), dtype=np.uint32)}
    assert raw(e, cl, now_ns=now, n_classes=3) == abi.GSX_EINVAL and raw(e, ncd, now_ns=now, n_classes=3) == abi.GSX_EINVAL
    ok = abi.MeshStatsSpec(n_bins=33)
    out = abi.MeshStatsOut(topic_tot=tot["topic_tot"].ctypes.data)
    assert e.lib.gsx_mesh_stats(None, C.byref(ok), C.byref(out)) == abi.GSX_EINVAL
    assert e.lib.gsx_mesh_stats(e.h, None, C.byref(out)) == abi.GSX_EINVAL
    assert e.lib.gsx_mesh_stats(e.h, C.byref(ok), None) == abi.GSX_EINVAL
    assert e.lib.gsx_mesh_stats(e.h, C.byref(ok), C.byref(abi.MeshStatsOut())) == 0  # all NULL: nothing to do
    with pytest.raises(gsx.GsxError) as ei:
        e.mesh_stats(now, n_bins=1)
    assert ei.value.code == abi.GSX_EINVAL
    check(e, ov, now, "the engine is as it was")
    fresh = gsx.Engine(1)
    assert fresh.lib.gsx_mesh_stats(fresh.h, C.byref(ok), C.byref(out)) == abi.GSX_ESTATE  # no overlay loaded
    shard = gsx.Engine(1)  # a range shard: not offered
    half = ov.n // 2
    rp = ov.row_ptr[: half + 1]
    shard.load_overlay_shard(ov.n, 0, rp, ov.col[: rp[-1]], ov.edge_flags[: rp[-1]], ov.node_ips)
    assert shard.lib.gsx_mesh_stats(shard.h, C.byref(ok), C.byref(out)) == abi.GSX_EINVAL
    # an engine of no nodes writes nothing; nodes without pairs: units and nothing else
    from gsx import synth
    for nn in (0, 3):
        empty = gsx.Engine(2)
        empty.set_peer_params(synth.bench_peer_params())
        empty.load_overlay(np.zeros(nn + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
        t2 = np.full((2, 16), 0xAB, dtype=np.uint64)
        assert raw(empty, {"topic_tot": t2}, now_ns=now) == 0
        if nn == 0:
            assert (t2 == 0xAB).all()
        else:
            assert t2[:, COL["units"]].tolist() == [3, 3] and t2[:, COL["empty"]].tolist() == [3, 3] and not t2[:, 5:].any()


def test_refused_while_a_sharded_exchange_is_in_flight(gpu_ok):
    """test_gpu_score_parts.py's probe: between gsx_hb_end and gsx_gx_end the call is refused with
    GSX_ESTATE, and on the same range shard with nothing in flight with GSX_EINVAL."""
    import gossip_cases as gc
    from gsx import shard, synth

    n, d, seed, T, world = 600, 6, 53, 1, 2
    ov = pc.overlay(n, d, seed)
    full = gsx.Engine(T)
    app = pc.setup(full, ov, T, seed, mesh_degree=6)
    st0 = full.export_state()
    E = ov.n_pairs
    rank_lo = synth.shard_ranges(n, world)
    engines = []
    for k in range(world):
        lo, hi = int(rank_lo[k]), int(rank_lo[k + 1])
        sh = synth.shard_of(ov, lo, hi)
        a, b = int(ov.row_ptr[lo]), int(ov.row_ptr[hi])
        e = gsx.Engine(T)
        e.set_peer_params(synth.bench_peer_params())
        tp = synth.spam_test_topic_params()
        tp.mesh_message_deliveries_window_ns = 25 * abi.MILLISECOND
        e.set_topic_params(0, tp)
        e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                        accept_px_threshold=0, opportunistic_graft_threshold=0))
        e.load_overlay_shard(n, lo, sh.row_ptr, sh.col, sh.edge_flags, sh.node_ips)
        st = {f: (st0[f].reshape(T, E)[:, a:b].reshape(-1).copy() if f in abi.RECORD_FIELDS else st0[f][a:b].copy())
              for f in abi.STATE_FIELDS}
        st["last_refresh_ns"] = st0["last_refresh_ns"]
        e.import_state(st)
        e.set_app_scores(app[a:b])
        e.set_gossipsub_params(gc.params())
        engines.append(e)

    def probe(be):
        return raw(be, {"topic_tot": np.zeros((T, 16), dtype=np.uint64)}, now_ns=pc.T0 + S)

    codes = []

    class Probe(shard.RangeSharded):
        def _gx_exchange(self, n_sets):
            assert self.be.gx_pending() is not None
            codes.append(probe(self.be))
            return super()._gx_exchange(n_sets)

    runners = shard.run_local(world, "cuda:0", lambda tp, e: Probe(e, rank_lo, tp), [(e,) for e in engines])
    cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=0, max_hops=2, latency_ms=5, seed=seed)
    ms = pc.messages(n, 40, seed)
    shard.run_local(world, "cuda:0", lambda tp, r: (setattr(r, "tp", tp), r.propagate(ms, cfg))[1], [(r,) for r in runners])
    shard.run_local(world, "cuda:0", lambda tp, r: (setattr(r, "tp", tp), r.heartbeat(1, pc.T0 + S, 5))[1],
                    [(r,) for r in runners])
    assert codes and all(c == abi.GSX_ESTATE for c in codes), codes
    assert all(e.gx_pending() is None for e in engines)
    assert [probe(e) for e in engines] == [abi.GSX_EINVAL] * world  # a range shard, nothing in flight

"""The output-pointer rule of the stats entry points (NULL is skipped, device
memory is written in place, host memory gets a copy of an engine staging buffer) where the
per-call tests do not look: outputs of one call in host memory, device memory and NULL at
once; staging buffers that must grow with the call or with a reloaded overlay; the
one-launch timing bracket of the calls no other test brackets; calls with no output at all.

Every comparison is between two runs of the same integer (or bit-copied f64) tables, so
equality is exact.  gsx_conn_trim needs its trim bytes and gsx_accept_from its out (NULL is
GSX_EINVAL), so the all-NULL cases leave those two out."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library loads: both then share one HIP runtime)

import gsx
import propagation_cases as pc
from gsx import abi, synth
from test_gpu_timed_prop import DevBuf

pytestmark = pytest.mark.gpu

S = abi.SECOND
T = 2
GS = abi.GSX_ROUTER_GOSSIPSUB
SEED = 31
EDGES2 = [-100.0, 0.0]
EDGES7 = [-300.0, -200.0, -100.0, -5.0, 0.0, 5.0, 10.0]  # GSX_SS_MAX_EDGES of them
N_CLASSES = 3


@functools.lru_cache(maxsize=None)
def overlay(n):
    return pc.overlay(n, 6, seed=SEED, mix_protocols=True)


def sizes(m):
    return ((np.arange(m, dtype=np.uint64) * 977 + 13) % 1500).astype(np.uint32)


class World:
    """One engine on an overlay of n nodes, with everything the stats calls read: scores, a
    mesh, a gater with some rejections, a tag tracer with some tags.  plain(m) / timed(m) run
    a propagation of m messages (credits off: the state stays what load() made it)."""

    def __init__(self, n, e=None):
        self.e = e if e is not None else gsx.Engine(T)
        self.load(n)

    def load(self, n):
        e, ov = self.e, overlay(n)
        self.ov, self.n, self.E = ov, ov.n, ov.n_pairs
        pc.setup(e, ov, T, seed=SEED)
        # (the gater and the tag tracer belong to the overlay: set again after every load)
        gp = abi.GaterParams()
        assert e.lib.gsx_default_gater_params(C.byref(gp)) == 0
        gp.threshold, gp.quiet_ns = 0.1, abi.HOUR
        e.set_gater_params(gp)
        ev = [(abi.GATER_ADD_PEER, 0, p, pc.T0, 0, 0) for p in range(self.E)]
        ev += [(abi.GATER_REJECT, 0, p, pc.T0, 7, 0) for p in range(0, self.E, 4)]
        e.gater_events(np.array(ev, dtype=abi.gater_event_dtype()))
        e.set_tag_params(abi.TagParams(bump=1, decay_amount=1, cap=15, decay_interval_ns=600 * S))
        e.tag_events(np.array([(p, p % T, 1 + p % 5) for p in range(0, self.E, 3)], dtype=abi.tag_event_dtype()))
        self.node_class = (np.arange(self.n) % N_CLASSES).astype(np.uint8)
        self.m, self.edges, self.n_bins = 0, EDGES2, 4

    def plain(self, m):
        self.m = m
        self.e.propagate(pc.messages(self.n, m, seed=SEED + m, invalid=0.1), pc.config(GS, credit=0, delay_ms=1.0))

    def timed(self, m):
        self.m = m
        self.e.set_link_latency(synth.link_latency(self.ov, SEED, 1, 9))
        self.e.propagate_timed(pc.messages(self.n, m, seed=SEED + m, invalid=0.1),
                               pc.config(GS, latency_ms=5, credit=0), 65534)

    def close(self):
        self.e.close()


# name -> (the outputs of the call as (shape, dtype) given the world, the call with one address or None per output)
def _prop_stats(w):
    return [((w.m, abi.GSX_MAX_HOPS + 1), np.uint32), ((w.n,), np.uint32), ((w.n,), np.uint64)]


def _prop_traffic(w):
    K = abi.GSX_TRAFFIC_COLS
    return [((w.m, K), np.uint32), ((w.n, K), np.uint32), ((w.n, 2), np.uint64), ((w.E,), np.uint32), ((w.E,), np.uint64)]


def _timed_stats(w):
    return [((w.m, w.n_bins), np.uint32), ((w.n,), np.uint32), ((w.n,), np.uint64)]


def _timed_traffic(w):
    K, B = abi.GSX_TT_COLS, w.n_bins
    return [((w.m, K), np.uint32), ((w.n, K), np.uint32), ((w.n, 2), np.uint64), ((w.E,), np.uint32), ((w.E,), np.uint64),
            ((B, K), np.uint64), ((B, 2), np.uint64), ((w.n, 2), np.uint64), ((w.n, 2), np.uint32)]


def _score_stats(w):
    B = len(w.edges) + 1
    return [((B,), np.uint64), ((w.n, B), np.uint32), ((w.n,), np.float64), ((w.n, B), np.uint32), ((w.n,), np.float64)]


def _score_parts(w):
    B, NC = len(w.edges) + 1, abi.GSX_CAUSES
    return [((w.E, abi.GSX_PARTS), np.float64), ((w.E,), np.uint8), ((w.E,), np.uint8), ((B, NC), np.uint64),
            ((B, T + 1), np.uint64), ((w.n, NC), np.uint32), ((w.n, NC), np.uint32)]


def _mesh_stats(w):
    B, A, NC = 9, 3, N_CLASSES
    return [((T, abi.GSX_MS_COLS), np.uint64), ((T, B), np.uint64), ((T, B), np.uint64), ((T, B), np.uint64),
            ((T, A), np.uint64), ((T, NC, NC), np.uint64), ((T, w.n), np.uint32), ((T, w.n), np.uint32),
            ((T, w.n), np.uint32), ((T, w.n, NC), np.uint32)]


def _conn_values(w):
    return [((w.E,), np.uint32), ((w.E,), np.uint8)]


def _conn_trim(w):
    return [((w.E,), np.uint8), ((w.n,), np.uint32)]


def _raw(w, fn, *args):
    w.e._chk(fn(w.e.h, *args), fn.__name__)


CALLS = {
    "prop_stats": (_prop_stats, lambda w, p: w.e.prop_stats(w.m, out_ptrs=p)),
    "prop_traffic": (_prop_traffic, lambda w, p: w.e.prop_traffic(w.m, sizes(w.m), out_ptrs=p)),
    "timed_stats": (_timed_stats, lambda w, p: w.e.timed_stats(w.m, 2, w.n_bins, out_ptrs=p)),
    "timed_traffic": (_timed_traffic, lambda w, p: w.e.timed_traffic(w.m, sizes(w.m), 2, w.n_bins, out_ptrs=p)),
    "score_stats": (_score_stats, lambda w, p: w.e.score_stats(w.edges, out_ptrs=p)),
    "score_parts": (_score_parts, lambda w, p: w.e.score_parts(w.edges, out_ptrs=p)),
    "mesh_stats": (_mesh_stats, lambda w, p: w.e.mesh_stats(pc.T0 + 3 * S, n_bins=9, age_edges_ns=[0, S],
                                                            node_class=w.node_class, n_classes=N_CLASSES,
                                                            hostile_mask=0b100, min_honest=1, out_ptrs=p)),
    "conn_values": (_conn_values, lambda w, p: _raw(w, w.e.lib.gsx_conn_values, *[C.c_void_p(x) for x in p])),
    "conn_trim": (_conn_trim, lambda w, p: _raw(w, w.e.lib.gsx_conn_trim, 5, *[C.c_void_p(x) for x in p])),
}
PLAIN = ("prop_stats", "prop_traffic", "score_stats", "score_parts", "mesh_stats", "conn_values", "conn_trim")
TIMED = ("timed_stats", "timed_traffic")
NEEDS_FIRST = ("conn_trim",)  # (its first output may not be NULL)


def call(w, name, kinds, fill=0x07):
    """One call with output i in host memory ("h"), device memory ("d", preset to `fill`
    bytes) or NULL ("n") -> the tables written, as bytes (None where NULL)."""
    outs, run = CALLS[name]
    bufs, ptrs = [], []
    for (shape, dt), k in zip(outs(w), kinds):
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        assert nbytes > 0, (name, shape)
        if k == "h":
            b = np.full(nbytes, 0xEE, dtype=np.uint8)
            ptrs.append(b.ctypes.data)
        elif k == "d":
            b = DevBuf(nbytes)
            b.fill(fill)
            ptrs.append(b.ptr)
        else:
            b = None
            ptrs.append(None)
        bufs.append(b)
    run(w, ptrs)
    w.e.sync()
    got = []
    for b in bufs:
        got.append(None if b is None else b.tobytes() if isinstance(b, np.ndarray) else b.read(np.uint8).tobytes())
        if isinstance(b, DevBuf):
            b.free()
    return got


def all_host(w, name):
    return call(w, name, "h" * len(CALLS[name][0](w)))


def every_call(w, m):
    """Every stats call of the ABI with host outputs, over a plain and then a timed propagation
    of m messages -> {call: tables}; plus both forms of gsx_accept_from and gsx_tag_export."""
    w.plain(m)
    res = {name: all_host(w, name) for name in PLAIN}
    res["accept_all"] = w.e.accept_from(pc.T0 + 3 * S, 9, 0).tobytes()
    res["accept_listed"] = w.e.accept_from(pc.T0 + 3 * S, 9, 0, pairs=np.arange(0, w.E, 2)).tobytes()
    res["tag_export"] = w.e.tag_export().tobytes()
    w.timed(m)
    res.update({name: all_host(w, name) for name in TIMED})
    return res


def assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for name in want:
        if isinstance(want[name], bytes):
            assert got[name] == want[name], (what, name)
            continue
        for i, (a, b) in enumerate(zip(got[name], want[name])):
            assert a == b, (what, name, i)


@pytest.fixture(scope="module")
def world(gpu_ok):
    w = World(150)
    yield w
    w.close()


@pytest.fixture(scope="module")
def fresh600(gpu_ok):
    """What a fresh engine answers on the 600-node overlay, with the most edges gsx_score_stats takes."""
    w = World(600)
    w.edges, w.n_bins = EDGES7, 64
    res = every_call(w, 192)
    w.close()
    return res


SPLITS = ("hdn", "dnh", "nhd")  # output i of a call takes letter i mod 3: each is host, device and NULL once


@pytest.mark.parametrize("name", list(CALLS))
def test_mixed_outputs(world, name):
    w = world
    (w.timed if name in TIMED else w.plain)(64)
    want = all_host(w, name)
    for k, split in enumerate(SPLITS):
        kinds = "".join(split[i % 3] for i in range(len(want)))
        if name in NEEDS_FIRST and kinds[0] == "n":
            continue
        got = call(w, name, kinds, fill=(0x07, 0xA5, 0x5A)[k])
        for i, kind in enumerate(kinds):
            # (a device buffer equal to the host table holds no byte of its preset left where one had to change)
            assert got[i] == (None if kind == "n" else want[i]), (name, kinds, i)
    assert all_host(w, name) == want  # the staging buffers serve the next all-host call as before


def test_growth(gpu_ok):
    """One engine through calls of 64 (W = 1), 192 (W = 4) and 64 messages, n_bins 4, 64, 4: the
    staging of a larger call replaces a smaller one's, and a smaller call after it reads only its part."""
    names = ("prop_stats", "prop_traffic", "timed_stats", "timed_traffic")
    fresh = {}
    for m, n_bins in ((64, 4), (192, 64)):
        f = World(150)
        f.n_bins = n_bins
        f.plain(m)
        fresh[m] = {name: all_host(f, name) for name in names[:2]}
        f.timed(m)
        fresh[m].update({name: all_host(f, name) for name in names[2:]})
        f.close()
    w = World(150)
    for m, n_bins in ((64, 4), (192, 64), (64, 4)):
        w.n_bins = n_bins
        w.plain(m)
        got = {name: all_host(w, name) for name in names[:2]}
        w.timed(m)
        got.update({name: all_host(w, name) for name in names[2:]})
        assert_same(got, fresh[m], f"m={m}")
    w.close()


def test_reload(gpu_ok, fresh600):
    """One engine from 150 nodes to 600 and back: no staging buffer of the smaller overlay
    survives into the larger one, and none of the larger one's tables shows through afterwards."""
    w = World(150)
    first = every_call(w, 64)
    w.load(600)
    w.edges, w.n_bins = EDGES7, 64
    assert_same(every_call(w, 192), fresh600, "150 -> 600")
    w.load(150)
    assert_same(every_call(w, 64), first, "600 -> 150")
    w.close()


def test_timing_bracket(world):
    """Each call is one timed launch of gsx_timing_begin, whatever it launches."""
    w, e = world, world.e
    now = pc.T0 + 3 * S

    def one(fn):
        e.timing_begin(2)
        fn()
        tot, lo, hi, n = e.timing_end()
        assert n == 1 and tot > 0, fn

    w.plain(64)
    one(lambda: all_host(w, "prop_stats"))
    one(lambda: all_host(w, "prop_traffic"))
    one(lambda: e.accept_from(now, 9, 0))
    one(lambda: e.accept_from(now, 9, 0, pairs=np.arange(0, w.E, 2)))
    one(lambda: all_host(w, "conn_values"))
    one(lambda: all_host(w, "conn_trim"))
    w.timed(64)
    one(lambda: all_host(w, "timed_stats"))
    one(lambda: all_host(w, "timed_traffic"))
    e.timing_begin(2)
    for _ in range(3):
        all_host(w, "conn_values")
    assert e.timing_end()[3] == 2  # the third call found no event pair left: it is not timed


@pytest.mark.parametrize("name", [c for c in CALLS if c not in NEEDS_FIRST])
def test_no_output_at_all(world, name):
    w, e = world, world.e
    (w.timed if name in TIMED else w.plain)(64)
    e.timing_begin(1)
    assert call(w, name, "n" * len(CALLS[name][0](w))) == [None] * len(CALLS[name][0](w))
    assert e.timing_end()[3] == 0  # no launch was bracketed

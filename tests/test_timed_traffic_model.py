"""timed_traffic_model.py against what it must agree with: timed_model.run's counters and
arrival ticks over links of different latencies, the column identities of gsx.h, and, with
every link 1 tick, no validation delay and a generous max_ticks, traffic_model's tables of
the same call.  CPU only, on the oracle's exported state: these are the facts the GPU tests
of gsx_timed_traffic rely on (test_gpu_timed_traffic.py)."""
import functools

import numpy as np
import pytest

import oracle as orc
import propagation_cases as pc
import timed_model as tm
import timed_traffic_model as ttm
import traffic_model as trm
from gsx import abi, synth

FS, GS = abi.GSX_ROUTER_FLOODSUB, abi.GSX_ROUTER_GOSSIPSUB

# name -> router, n, d, T, m, overlay kw, setup kw, invalid, flood publish, tick (ms), vd (ticks):
# the shapes of test_gpu_timed_prop.py
SHAPES = {
    "floodsub": (FS, 300, 6, 1, 64, {}, {}, 0.0, 0, 5, 0),
    "gossipsub": (GS, 500, 6, 2, 100, dict(mix_protocols=True, direct_frac=0.05), dict(disconnect_frac=0.05), 0.0, 0, 5, 0),
    "floodpub": (GS, 500, 6, 1, 130, dict(mix_protocols=True), {}, 0.0, 1, 5, 0),
    "delay-invalid": (GS, 500, 6, 1, 100, dict(mix_protocols=True, direct_frac=0.05), dict(disconnect_frac=0.05), 0.25, 0,
                      1, 7),
    "one-word": (GS, 1500, 7, 1, 50, dict(mix_protocols=True), {}, 0.0, 0, 5, 0),
}


@functools.lru_cache(maxsize=None)
def backend(name):
    router, n, d, T, m, okw, skw, invalid, fp, tick_ms, vd = SHAPES[name]
    ov = pc.overlay(n, d, seed=11, **okw)
    ms = pc.messages(n, m, seed=11, invalid=invalid)
    o = orc.Oracle(T)
    pc.setup(o, ov, T, seed=11, **skw)
    return o, ov, ms


def tcfg(name, vd=None):
    router, n, d, T, m, okw, skw, invalid, fp, tick_ms, vd0 = SHAPES[name]
    vd = vd0 if vd is None else vd
    return pc.config(router, flood_publish=fp, latency_ms=tick_ms, delay_ms=float(tick_ms * vd))


def identities(t):
    for tab in (t.msg, t.node, t.bins):
        s = tab.astype(np.int64).sum(0)
        assert s[ttm.SENT] == s[ttm.FIRST:ttm.IN_FLIGHT + 1].sum()
        assert s[ttm.DUP_IN_WINDOW] <= s[ttm.DUP]
    assert t.msg.astype(np.int64).sum(0).tolist() == t.node.astype(np.int64).sum(0).tolist() == \
        t.bins.astype(np.int64).sum(0).tolist()
    assert t.node_bytes.sum(0).tolist() == t.bin_bytes.sum(0).tolist()
    assert t.pair.sum() == t.msg[:, ttm.FIRST:ttm.GRAYLISTED + 1].sum() and t.pair_bytes.sum() == t.node_bytes[:, 1].sum()


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_column_sums_are_the_timed_models_counters(name, symmetric):
    o, ov, ms = backend(name)
    T = SHAPES[name][3]
    lat = synth.link_latency(ov, 11, 1, 9, symmetric=symmetric)
    want = tm.run_on(o, ov, lat, ms, tcfg(name), 65534, T=T)
    R = ttm.run_on(o, ov, lat, ms, tcfg(name), 65534, T=T)
    assert np.array_equal(R.tick, want.tick)
    c = ttm.counters(R)
    assert (c["deliveries"], c["duplicates"], c["invalid"], c["graylisted"], c["dup_in_window"], c["transmissions"]) == \
        (want.deliveries, want.duplicates, want.rejected + want.ignored, want.graylisted, want.dup_in_window,
         want.transmissions)
    assert c["in_flight"] == 0
    t = ttm.tables(R, None, 1, 64)
    s = t.msg.astype(np.int64).sum(0)
    assert s.tolist() == [want.transmissions, want.deliveries, want.duplicates, want.rejected + want.ignored,
                          want.graylisted, 0, want.dup_in_window]
    identities(t)
    if name == "gossipsub":  # a late duplicate outside the window exists: the window column is no copy of DUP
        assert 0 < s[ttm.DUP_IN_WINDOW] < s[ttm.DUP]
    if name == "delay-invalid":
        assert s[ttm.INVALID] > 0 and s[ttm.GRAYLISTED] > 0


def test_the_cut_case_has_copies_in_flight():
    name = "gossipsub"
    o, ov, ms = backend(name)
    lat = synth.link_latency(ov, 11, 1, 9)
    full = tm.run_on(o, ov, lat, ms, tcfg(name), 65534, T=2)
    cut = max(full.last_tick // 2, 1)
    want = tm.run_on(o, ov, lat, ms, tcfg(name), cut, T=2)
    R = ttm.run_on(o, ov, lat, ms, tcfg(name), cut, T=2)
    assert np.array_equal(R.tick, want.tick)
    c = ttm.counters(R)
    assert c["in_flight"] > 0 and c["transmissions"] == want.transmissions and c["dup_in_window"] == want.dup_in_window
    assert (c["deliveries"], c["duplicates"], c["graylisted"]) == (want.deliveries, want.duplicates, want.graylisted)
    t = ttm.tables(R, None, 1, 64)
    identities(t)
    s = t.msg.astype(np.int64).sum(0)
    assert s[ttm.SENT] - s[ttm.IN_FLIGHT] == want.transmissions
    # a node whose send tick is past the cut sent nothing (vd = 0: those that first got a message at the cut
    # still send at it; none later exists, so delay the validation by 3 ticks and look again)
    Rd = ttm.run_on(o, ov, lat, ms, tcfg(name, vd=3), cut, T=2)
    late = [(k, u) for k in range(len(ms)) for u in range(ov.n) if Rd.tick[k, u] != 0xFFFF and 0 < Rd.tick[k, u] and
            Rd.tick[k, u] + 3 > cut]
    sent = {(k, v) for k, v, *_ in Rd.copies}
    assert late and not sent & set(late)
    assert all(f <= cut for _, _, _, f, *_ in Rd.copies)


@pytest.mark.parametrize("name", ["floodsub", "gossipsub", "floodpub", "delay-invalid"])
def test_one_tick_links_give_the_hop_models_tables(name):
    o, ov, ms = backend(name)
    T = SHAPES[name][3]
    m = len(ms)
    cfg = tcfg(name, vd=0)
    R = ttm.run_on(o, ov, np.ones(ov.n_pairs, dtype=np.uint8), ms, cfg, 65534, T=T)
    H = trm.run_on(o, ov, ms, cfg, T=T)
    assert H.hops < 40
    B = np.stack([trm.bits_of_ints(H.rows[c], m) for c in range(trm.COLS)])
    sizes = (np.arange(m, dtype=np.uint64) * 977 + 13) % 1500
    for sz in (None, sizes):
        msg, node, nbytes, pair, pbytes = trm.tables(B, ov.row_ptr, ov.col, sz)
        t = ttm.tables(R, sz, 1, 64)
        assert np.array_equal(t.msg[:, :5], msg) and np.array_equal(t.node[:, :5], node)
        assert np.array_equal(t.node_bytes, nbytes) and np.array_equal(t.pair, pair) and np.array_equal(t.pair_bytes, pbytes)
        assert not t.msg[:, ttm.IN_FLIGHT].any() and not t.node[:, ttm.IN_FLIGHT].any()


def test_vectorised_tables_equal_the_loop_and_the_peaks_the_node_bins():
    name = "floodsub"
    o, ov, ms = backend(name)
    lat = synth.link_latency(ov, 11, 1, 9, symmetric=False)
    R = ttm.run_on(o, ov, lat, ms, tcfg(name), 12)
    sizes = (np.arange(len(ms), dtype=np.uint64) * 977 + 13) % 1500
    for bin_ticks, n_bins in ((1, 5), (3, 64), (1, 1)):
        a, b = ttm.tables(R, sizes, bin_ticks, n_bins), ttm.tables_loop(R, sizes, bin_ticks, n_bins)
        for f in ttm.Tables.NAMES[:7]:
            assert getattr(a, f).dtype == getattr(b, f).dtype and np.array_equal(getattr(a, f), getattr(b, f)), f
        assert np.array_equal(a.node_bin.sum(1), a.node_bytes) and np.array_equal(a.node_bin.sum(0), a.bin_bytes)
        for u in range(ov.n):
            for d in range(2):
                row = a.node_bin[u, :, d].tolist()
                assert a.node_peak[u, d] == max(row) and a.node_peak_bin[u, d] == (row.index(max(row)) if max(row) else 0)

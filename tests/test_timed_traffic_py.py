"""TimedTraffic's helpers on hand-made tables (numpy only; the entry point's
declaration is checked against the library).  No device work here (CPU suite)."""
import ctypes as C

import numpy as np
import pytest

import gsx
from gsx import abi

SENT, FIRST, DUP, INVALID, GRAY, FLIGHT, DUPWIN = range(7)


def table():
    msg = np.array([[12, 4, 5, 0, 1, 2, 3],   # amplification 12 / 4
                    [6, 0, 0, 3, 3, 0, 0],    # only invalid first receipts: 6 / 3
                    [0, 0, 0, 0, 0, 0, 0],    # never sent: 0 / max(0, 1)
                    [5, 0, 0, 0, 4, 1, 0]], dtype=np.uint32)
    node = np.array([[7, 2, 2, 0, 0, 1, 1],
                     [0, 0, 0, 0, 0, 0, 0],   # nothing reached it: ratio 0, not nan
                     [9, 1, 3, 2, 2, 0, 2],
                     [7, 1, 0, 1, 6, 2, 0]], dtype=np.uint32)
    nbytes = np.array([[700, 40], [0, 0], [700, 90], [2 ** 63 + 5, 90]], dtype=np.uint64)
    bins = np.array([[20, 3, 1, 3, 6, 0, 1], [3, 1, 4, 0, 2, 3, 2]], dtype=np.uint64)
    bbytes = np.array([[2000, 130], [2 ** 63 + 105, 90]], dtype=np.uint64)
    peak = np.array([[400, 40], [0, 0], [700, 50], [2 ** 63, 50]], dtype=np.uint64)
    pbin = np.array([[0, 1], [0, 0], [1, 0], [1, 1]], dtype=np.uint32)
    return gsx.TimedTraffic(msg, node, nbytes, np.array([3, 0, 17], np.uint32), np.array([30, 0, 2 ** 40], np.uint64),
                            bins, bbytes, peak, pbin, bin_ticks=4, tick_ns=5 * abi.MILLISECOND)


def test_the_entry_point_is_declared():
    assert "gsx_timed_traffic" in abi.SIGNATURES
    lib = gsx.load_library()
    assert hasattr(lib, "gsx_timed_traffic")
    o = abi.TimedTrafficOut()
    assert lib.gsx_timed_traffic(None, None, 1, 64, C.byref(o)) == abi.GSX_EINVAL
    assert C.sizeof(abi.TimedTrafficOut) == 9 * C.sizeof(C.c_void_p)
    assert (gsx.TimedTraffic.SENT, gsx.TimedTraffic.IN_FLIGHT, gsx.TimedTraffic.DUP_IN_WINDOW, gsx.TimedTraffic.COLS) == \
        (0, 5, 6, 7)
    assert (abi.GSX_TT_FIRST, abi.GSX_TT_DUP, abi.GSX_TT_INVALID, abi.GSX_TT_GRAYLISTED, abi.GSX_TT_COLS) == (1, 2, 3, 4, 7)


def test_totals_and_ratios():
    t = table()
    assert t.sent() == 23 == t.total(SENT) and t.total(DUP) == 5 and t.total(GRAY) == 8 and t.in_flight() == 3
    assert t.total(SENT) == sum(t.total(c) for c in (FIRST, DUP, INVALID, GRAY, FLIGHT))
    assert np.array_equal(t.amplification(), [3.0, 2.0, 0.0, 5.0])
    assert np.array_equal(t.duplicate_ratio(), [0.5, 0.0, 3 / 8, 0.0])  # (IN_FLIGHT and DUP_IN_WINDOW are no receipts)
    assert np.isfinite(t.amplification()).all() and np.isfinite(t.duplicate_ratio()).all()
    assert np.array_equal(t.upload_bytes(), t.node_bytes[:, 0]) and np.array_equal(t.download_bytes(), [40, 0, 90, 90])
    only_bins = gsx.TimedTraffic(bins=t.bins)
    assert only_bins.sent() == 23 and only_bins.in_flight() == 3 and only_bins.msg is None
    only_nodes = gsx.TimedTraffic(node=t.node)
    assert only_nodes.sent() == 23 and only_nodes.bins is None


def test_load_and_peaks():
    t = table()
    assert np.array_equal(t.load(), t.bin_bytes) and t.load().dtype == np.uint64
    assert np.array_equal(t.load("copies"), [[20, 13], [3, 7]])
    assert np.array_equal(t.peak_upload(), [400, 0, 700, 2 ** 63]) and np.array_equal(t.peak_download(), [40, 0, 50, 50])
    with pytest.raises(ValueError):
        t.load("packets")
    # a bin is 4 ticks of 5 ms = 20 ms: 130 bytes in it are 6500 bytes per second
    assert np.array_equal(t.bytes_per_second(t.load()[:, 1]), [6500.0, 4500.0])
    assert np.array_equal(t.bytes_per_second([40], tick_ns=abi.MILLISECOND), [10000.0])
    with pytest.raises(ValueError):
        gsx.TimedTraffic(bins=t.bins).bytes_per_second([1])
    with pytest.raises(ValueError):
        gsx.TimedTraffic(bins=t.bins, bin_ticks=0)


def test_busiest_breaks_ties_by_ascending_id():
    t = table()
    assert t.busiest(4).tolist() == [3, 0, 2, 1]  # (2^63 + 5 sorts as an integer; 700 twice: node 0 first)
    assert t.busiest(2, by="download_bytes").tolist() == [2, 3]
    assert t.busiest(3, by="sent").tolist() == [2, 0, 3]
    assert t.busiest(9, by="received").tolist() == [2, 3, 0, 1] and t.busiest(0).tolist() == []
    assert t.busiest(2, by="peak_upload").tolist() == [3, 2] and t.busiest(3, by="peak_download").tolist() == [2, 3, 0]
    with pytest.raises(ValueError):
        t.busiest(1, by="hops")

"""PropTraffic's helpers on hand-made tables (numpy only; the entry point's
declaration is checked against the library).  No device work here (CPU suite)."""
import numpy as np
import pytest

import gsx
from gsx import abi

SENT, FIRST, DUP, INVALID, GRAY = range(5)


def table():
    msg = np.array([[10, 4, 5, 0, 1],   # amplification 10 / 4
                    [6, 0, 0, 3, 3],    # only invalid first receipts: 6 / 3
                    [0, 0, 0, 0, 0],    # never sent: 0 / max(0, 1)
                    [5, 0, 0, 0, 5]], dtype=np.uint32)  # every copy graylisted: 5 / 1
    node = np.array([[7, 2, 2, 0, 0],
                     [0, 0, 0, 0, 0],   # nothing reached it: ratio 0, not nan
                     [9, 1, 3, 2, 2],
                     [5, 1, 0, 1, 7]], dtype=np.uint32)
    nbytes = np.array([[700, 40], [0, 0], [700, 90], [2 ** 63 + 5, 90]], dtype=np.uint64)
    return gsx.PropTraffic(msg, node, nbytes, np.array([3, 0, 18], np.uint32), np.array([30, 0, 2 ** 40], np.uint64))


def test_the_entry_point_is_declared():
    assert "gsx_prop_traffic" in abi.SIGNATURES
    assert hasattr(gsx.load_library(), "gsx_prop_traffic")
    assert gsx.load_library().gsx_prop_traffic(None, None, None, None, None, None, None) == abi.GSX_EINVAL
    assert (gsx.PropTraffic.SENT, gsx.PropTraffic.GRAYLISTED, gsx.PropTraffic.COLS) == (0, 4, 5)
    assert (abi.GSX_TRAFFIC_FIRST, abi.GSX_TRAFFIC_DUP, abi.GSX_TRAFFIC_INVALID) == (1, 2, 3)


def test_totals_and_ratios():
    t = table()
    assert t.sent() == 21 == t.total(SENT) and t.total(DUP) == 5 and t.total(GRAY) == 9
    assert np.array_equal(t.amplification(), [2.5, 2.0, 0.0, 5.0])
    assert np.array_equal(t.duplicate_ratio(), [0.5, 0.0, 3 / 8, 0.0])
    assert np.isfinite(t.amplification()).all() and np.isfinite(t.duplicate_ratio()).all()
    assert np.array_equal(t.upload_bytes(), t.node_bytes[:, 0]) and np.array_equal(t.download_bytes(), [40, 0, 90, 90])
    only_nodes = gsx.PropTraffic(None, t.node)
    assert only_nodes.sent() == 21 and only_nodes.msg is None and only_nodes.pair is None


def test_busiest_breaks_ties_by_ascending_id():
    t = table()
    assert t.busiest(4).tolist() == [3, 0, 2, 1]  # (2^63 + 5 sorts as an integer; 700 twice: node 0 first)
    assert t.busiest(2, by="download_bytes").tolist() == [2, 3]
    assert t.busiest(3, by="sent").tolist() == [2, 0, 3]
    assert t.busiest(9, by="received").tolist() == [3, 2, 0, 1] and t.busiest(0).tolist() == []
    with pytest.raises(ValueError):
        t.busiest(1, by="hops")


def test_concat_of_replicas():
    t = table()
    both = gsx.PropTraffic.concat([t, t])
    assert both.msg.shape == (8, 5) and np.array_equal(both.node, 2 * t.node)
    assert both.node_bytes[3, 0] == np.uint64((2 * (2 ** 63 + 5)) % 2 ** 64) and np.array_equal(both.pair, [6, 0, 36])
    assert gsx.PropTraffic.concat([t, gsx.PropTraffic(t.msg)]).node is None

"""PropStats (gsx/engine.py): the derived per-message quantities are plain numpy
on the integer histogram gsx_prop_stats returns; checked on hand-made tables.
No device work here (CPU suite)."""
import ctypes as C

import numpy as np
import pytest

import gsx
from gsx import abi

H = abi.GSX_MAX_HOPS + 1


def table(rows):
    """rows: per message {hop: count} -> [m, 65] u32"""
    t = np.zeros((len(rows), H), dtype=np.uint32)
    for k, r in enumerate(rows):
        for h, c in r.items():
            t[k, h] = c
    return t


# 10 receivers: message 0 reaches all by hop 3, message 1 half of them, message 2 nobody,
# message 3 reaches 9 at the last hop the history holds
ROWS = [{0: 1, 1: 2, 2: 3, 3: 5}, {0: 1, 1: 1, 4: 4}, {0: 1}, {0: 1, 1: 4, 64: 5}]


def test_reached_ratio_last_and_mean_hop():
    st = gsx.PropStats(table(ROWS))
    assert st.n_msgs == 4 and st.hop_hist.dtype == np.uint32
    assert st.reached().tolist() == [10, 5, 0, 9]
    assert np.array_equal(st.delivery_ratio(10), np.array([1.0, 0.5, 0.0, 0.9]))
    assert np.array_equal(st.delivery_ratio([10, 5, 1, 18]), np.array([1.0, 1.0, 0.0, 0.5]))
    assert st.last_hop().tolist() == [3, 4, 0, 64]
    assert gsx.PropStats(np.zeros((2, H), dtype=np.uint32)).last_hop().tolist() == [-1, -1]
    mh = st.mean_hop()
    assert mh[0] == (2 * 1 + 3 * 2 + 5 * 3) / 10 and mh[1] == (1 + 16) / 5 and np.isnan(mh[2])
    assert mh[3] == (4 + 5 * 64) / 9


@pytest.mark.parametrize("q,want", [(0.5, [2, 4, -1, 64]), (0.9, [3, -1, -1, 64]), (1.0, [3, -1, -1, -1])])
def test_hops_to_fraction(q, want):
    st = gsx.PropStats(table(ROWS))
    assert st.hops_to_fraction(q, 10).tolist() == want


def test_hops_to_fraction_per_message_receivers():
    st = gsx.PropStats(table(ROWS))
    assert st.hops_to_fraction(1.0, [10, 5, 1, 9]).tolist() == [3, 4, -1, 64]
    assert st.hops_to_fraction(0.7, 10).tolist() == [3, -1, -1, 64]  # 7 of 10 is 0.7, not 0.7000000000000001


def test_add_sums_range_shards():
    a = gsx.PropStats(table([{0: 1, 1: 2}, {1: 3}]), np.array([1, 2], np.uint32), np.array([1, 3], np.uint64))
    b = gsx.PropStats(table([{1: 1, 2: 4}, {0: 1, 2: 2}]), np.array([2], np.uint32), np.array([4], np.uint64))
    s = a + b
    assert np.array_equal(s.hop_hist, table([{0: 1, 1: 3, 2: 4}, {0: 1, 1: 3, 2: 2}]))
    assert s.hop_hist.dtype == np.uint32
    assert s.node_received.tolist() == [1, 2, 2] and s.node_hop_sum.tolist() == [1, 3, 4]
    assert s.node_mean_hop().tolist() == [1.0, 1.5, 2.0]
    assert (a + gsx.PropStats(b.hop_hist)).node_received is None
    with pytest.raises(ValueError):
        a + gsx.PropStats(table([{0: 1}]))


def test_concat_joins_message_slices():
    a = gsx.PropStats(table([{0: 1, 1: 2}]), np.array([1, 1, 0], np.uint32), np.array([1, 1, 0], np.uint64))
    b = gsx.PropStats(table([{0: 1, 2: 1}, {0: 1}]), np.array([0, 0, 1], np.uint32), np.array([0, 0, 2], np.uint64))
    c = gsx.PropStats.concat([a, b])
    assert np.array_equal(c.hop_hist, table([{0: 1, 1: 2}, {0: 1, 2: 1}, {0: 1}]))
    assert c.node_received.tolist() == [1, 1, 1] and c.node_hop_sum.tolist() == [1, 1, 2]
    assert c.node_received.dtype == np.uint32 and c.node_hop_sum.dtype == np.uint64
    assert gsx.PropStats.concat([a, gsx.PropStats(b.hop_hist)]).node_received is None
    assert gsx.PropStats.concat([]).hop_hist.shape == (0, H)


def test_abi_signature_and_symbol():
    assert abi.SIGNATURES["gsx_prop_stats"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    lib = gsx.load_library()
    assert lib.gsx_prop_stats(None, None, None, None) == abi.GSX_EINVAL  # a NULL engine, before any device work
    assert callable(gsx.Engine.prop_stats)

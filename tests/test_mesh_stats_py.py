"""MeshStats (gsx/engine.py): the readers on hand-made tables.  No device work
(CPU suite)."""
import math

import numpy as np
import pytest

import gsx
from gsx import abi

COL = {name: k for k, name in enumerate(abi.MS_COL_NAMES)}


def hand_made():
    T, n, B, NC = 2, 4, 5, 2
    tot = np.zeros((T, abi.GSX_MS_COLS), dtype=np.uint64)
    tot[0, [COL["units"], COL["below_dlo"], COL["above_dhi"], COL["links"], COL["one_sided"]]] = [4, 1, 1, 10, 2]
    tot[0, [COL["eclipsed"], COL["below_honest"]]] = [1, 3]
    tot[1, [COL["units"], COL["links"], COL["one_sided"], COL["below_honest"]]] = [2, 6, 3, 1]
    deg = np.array([[3, 0, 5, 2], [1, 1, 4, 0]], dtype=np.uint32)
    cl = np.array([[[6, 2], [0, 0]], [[1, 1], [3, 1]]], dtype=np.uint64)
    return gsx.MeshStats(T, B, age_edges_ns=[0, 10], n_classes=NC, topic_tot=tot.reshape(-1),
                         deg_hist=np.arange(T * B), out_hist=np.zeros((T, B)), in_hist=np.ones((T, B)),
                         age_hist=np.arange(T * 3), class_links=cl, node_deg=deg, node_out=deg // 2,
                         node_in=deg[:, ::-1], node_class_deg=np.arange(T * n * NC))


def test_shapes_and_dtypes():
    m = hand_made()
    assert m.topic_tot.shape == (2, 16) and m.topic_tot.dtype == np.uint64
    assert m.deg_hist.shape == m.out_hist.shape == m.in_hist.shape == (2, 5) and m.in_hist.dtype == np.uint64
    assert m.age_hist.shape == (2, 3) and m.class_links.shape == (2, 2, 2)
    assert m.node_deg.shape == (2, 4) and m.node_deg.dtype == np.uint32 and m.node_class_deg.shape == (2, 4, 2)
    assert m.age_edges_ns.tolist() == [0, 10] and m.age_edges_ns.dtype == np.int64
    bare = gsx.MeshStats(3, 33)
    assert all(getattr(bare, f) is None for f in abi.MS_OUT_FIELDS)
    assert len(abi.MS_COL_NAMES) == abi.GSX_MS_COLS == 16 and abi.MS_COL_NAMES[abi.GSX_MS_BELOW_HONEST] == "below_honest"
    assert abi.MS_COL_NAMES[abi.GSX_MS_LINKS] == "links" and abi.MS_COL_NAMES[abi.GSX_MS_FANOUT_UNITS] == "fanout_units"


def test_totals():
    m = hand_made()
    assert m.total("links") == 16 and m.total("links", 0) == 10 and m.total(abi.GSX_MS_LINKS, 1) == 6
    assert m.total("units") == 6 and m.total("backoff") == 0
    with pytest.raises(ValueError):
        m.total("no such column")


def test_node_readers():
    m = hand_made()
    assert m.degree(0).tolist() == [3, 0, 5, 2] and m.outbound(0).tolist() == [1, 0, 2, 1]
    assert m.indegree(1).tolist() == [0, 4, 1, 1]


def test_ratios():
    m = hand_made()
    assert m.within_bounds(0) == 0.5 and m.within_bounds(1) == 1.0
    assert m.one_sided_ratio(0) == 0.2 and m.one_sided_ratio(1) == 0.5 and m.one_sided_ratio() == 5 / 16
    assert m.eclipsed() == 1 and m.eclipsed(1) == 0 and m.below_honest() == 4 and m.below_honest(0) == 3
    empty = gsx.MeshStats(1, 2, topic_tot=np.zeros(16))
    assert math.isnan(empty.within_bounds(0)) and math.isnan(empty.one_sided_ratio())


def test_class_share():
    m = hand_made()
    s0, s1 = m.class_share(0), m.class_share(1)
    assert s0[0].tolist() == [0.75, 0.25] and np.isnan(s0[1]).all()
    assert s1.tolist() == [[0.5, 0.5], [0.75, 0.25]]

"""gsx_score_stats without a device: the ABI's bookkeeping, the ctypes structs
against the header, the ScoreStats helpers on hand-made tables, and the numpy
reference (score_stats_cases.reference) on a 5-node overlay worked by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gsx
import score_stats_cases as sc
from gsx import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gsx.h")).read()
INF = np.inf


def test_abi_entries():
    assert abi.SIGNATURES["gsx_score_stats"] == (C.c_int, [C.c_void_p, C.POINTER(abi.ScoreStatsSpec),
                                                           C.POINTER(abi.ScoreStatsOut)])
    assert abi.SIGNATURES["gsx_score_stats_edges"] == (C.c_int, [C.c_void_p, C.POINTER(abi.ScoreStatsSpec)])
    lib = gsx.load_library()
    assert lib.gsx_score_stats(None, None, None) == abi.GSX_EINVAL  # a NULL engine, before any device work
    assert lib.gsx_score_stats_edges(None, None) == abi.GSX_EINVAL
    assert callable(gsx.Engine.score_stats) and gsx.ScoreStats is not None


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*\]", "", d.split()[-1]).lstrip("*") for d in body.split(";") if d.strip()]


def test_structs_match_the_header():
    for k in ("GSX_SS_MAX_EDGES", "GSX_SS_PRESENT", "GSX_SS_CONNECTED", "GSX_SS_MESH"):
        assert int(re.search(r"#define %s (\d+)" % k, HEADER).group(1)) == getattr(abi, k)
    S, O = abi.ScoreStatsSpec, abi.ScoreStatsOut
    assert [f for f, _ in S._fields_] == _struct_fields("gsx_score_stats_spec")
    assert [f for f, _ in O._fields_] == _struct_fields("gsx_score_stats_out")
    assert C.sizeof(S) == 16 + 56 and S.edges.offset == 16 and S.edges.size == 8 * abi.GSX_SS_MAX_EDGES
    assert [getattr(S, f).offset for f in ("select", "topic", "n_edges", "reserved")] == [0, 4, 8, 12]
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(O) == 5 * p
    assert [getattr(O, f).offset for f in ("hist", "obs_bins", "obs_min", "peer_bins", "peer_min")] == \
        [0, p, 2 * p, 3 * p, 4 * p]


# edges (-10, 0, 5): bins  s < -10 | -10 <= s < 0 | 0 <= s < 5 | 5 <= s
EDGES = [-10.0, 0.0, 5.0]


def table():
    return gsx.ScoreStats(EDGES, hist=[3, 2, 4, 1],
                          obs_bins=[[2, 0, 1, 0], [1, 2, 0, 1], [0, 0, 3, 0], [0, 0, 0, 0]],
                          obs_min=[-50.0, -11.0, 0.0, INF],
                          peer_bins=[[0, 1, 2, 0], [3, 0, 0, 0], [0, 1, 2, 1], [0, 0, 0, 0]],
                          peer_min=[-3.0, -50.0, -1.0, INF])


def test_helpers_below_and_degrees():
    st = table()
    assert st.hist.dtype == np.uint64 and st.obs_bins.dtype == np.uint32 and st.obs_bins.shape == (4, 4)
    h, o, p = st.below(-10.0)
    assert h == 3 and o.tolist() == [2, 1, 0, 0] and p.tolist() == [0, 3, 0, 0]
    h, o, p = st.below(0.0)
    assert h == 5 and o.tolist() == [2, 3, 0, 0] and p.tolist() == [1, 3, 1, 0]
    h, o, p = st.below(5.0)
    assert h == 9 and o.tolist() == [3, 3, 3, 0] and p.tolist() == [3, 3, 3, 0]
    with pytest.raises(ValueError):
        st.below(1.0)  # not an edge
    assert st.degree().tolist() == [3, 4, 3, 0] and st.degree().dtype == np.int64
    assert st.indegree().tolist() == [3, 3, 4, 0]
    assert int(st.hist.sum()) == st.degree().sum() == st.indegree().sum() == 10


def test_helpers_fraction_below():
    st = table()
    h, o, p = st.fraction_below(0.0)
    assert h == 0.5
    assert o[:3].tolist() == [2 / 3, 3 / 4, 0.0] and np.isnan(o[3])
    assert p[:3].tolist() == [1 / 3, 1.0, 1 / 4] and np.isnan(p[3])
    hist_only = gsx.ScoreStats(EDGES, hist=[1, 0, 0, 3])
    assert hist_only.below(-10.0) == (1, None, None) and hist_only.fraction_below(5.0) == (0.25, None, None)
    none = gsx.ScoreStats([], hist=[0], obs_bins=[[0], [0]])  # no edges: one bin
    assert none.hist.shape == (1,) and none.degree().tolist() == [0, 0]


def test_helpers_add():
    a = gsx.ScoreStats(EDGES, [1, 0, 2, 0], [[1, 0, 0, 0], [0, 0, 2, 0]], [-20.0, 1.0],
                       [[0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 1, 0]], [2.0, -20.0, 1.0])
    b = gsx.ScoreStats(EDGES, [0, 1, 0, 1], [[0, 1, 0, 1]], [-5.0],
                       [[0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], [-5.0, 7.0, INF])
    c = a + b
    assert c.hist.tolist() == [1, 1, 2, 1]
    assert c.obs_bins.tolist() == [[1, 0, 0, 0], [0, 0, 2, 0], [0, 1, 0, 1]]  # rank order
    assert c.obs_min.tolist() == [-20.0, 1.0, -5.0]
    assert c.peer_bins.tolist() == [[0, 1, 1, 0], [1, 0, 0, 1], [0, 0, 1, 0]]
    assert c.peer_min.tolist() == [-5.0, -20.0, 1.0]
    assert c.edges.tolist() == EDGES
    assert (a + gsx.ScoreStats(EDGES, [0, 0, 0, 0])).obs_bins is None  # kept when both sides have them
    with pytest.raises(ValueError):
        a + gsx.ScoreStats([0.0], [0, 0])


def test_reference_on_a_hand_worked_overlay():
    """5 nodes, directed.  Nobody points at node 4; node 3 has an empty row.
        pair  obs -> peer  score  flags                mesh(t0)
         0     0  ->  1     -10.0  present+connected    yes      on the edge -10: upper bin
         1     0  ->  2     -10.5  present+connected    no
         2     1  ->  0       0.0  present+connected    yes      on the edge 0
         3     1  ->  2       3.0  present (retained)   no
         4     1  ->  3       9.0  absent               no       never counted
         5     2  ->  0      -0.5  present+connected    yes
         6     4  ->  0       5.0  present+connected    no       on the edge 5
         7     4  ->  1      -99.0 present+connected    yes
    """
    PC = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
    row_ptr = [0, 2, 5, 6, 6, 8]
    col = [1, 2, 0, 2, 3, 0, 0, 1]
    scores = [-10.0, -10.5, 0.0, 3.0, 9.0, -0.5, 5.0, -99.0]
    pf = [PC, PC, PC, abi.GSX_PAIR_PRESENT, 0, PC, PC, PC]
    M = abi.GSX_REC_IN_MESH
    rf = np.array([[M, 0, M, 0, 0, M, 0, M], [0] * 8], dtype=np.uint8)  # [T = 2, E]
    r = sc.reference(scores, pf, rf, row_ptr, col, 5, EDGES, "present")
    assert r["hist"].tolist() == [2, 2, 2, 1] and r["hist"].dtype == np.uint64
    assert r["obs_bins"].tolist() == [[1, 1, 0, 0], [0, 0, 2, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 0, 0, 1]]
    assert r["obs_min"].tolist() == [-10.5, 0.0, -0.5, INF, -99.0]
    assert r["peer_bins"].tolist() == [[0, 1, 1, 1], [1, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert r["peer_min"].tolist() == [-0.5, -99.0, -10.5, INF, INF]  # nobody points at 4; 3 only by an absent pair
    r = sc.reference(scores, pf, rf, row_ptr, col, 5, EDGES, "connected")
    assert r["hist"].tolist() == [2, 2, 1, 1]
    assert r["obs_bins"][1].tolist() == [0, 0, 1, 0] and r["peer_min"][2] == -10.5
    r = sc.reference(scores, pf, rf, row_ptr, col, 5, [], "mesh", topic=0)
    assert r["hist"].tolist() == [4]
    assert r["obs_bins"].ravel().tolist() == [1, 1, 1, 0, 1]  # the mesh degrees
    assert r["peer_bins"].ravel().tolist() == [2, 2, 0, 0, 0]
    assert r["obs_min"].tolist() == [-10.0, 0.0, -0.5, INF, -99.0]
    r = sc.reference(scores, pf, rf, row_ptr, col, 5, [0.0], "mesh", topic=1)
    assert r["hist"].tolist() == [0, 0] and not r["obs_bins"].any() and np.isinf(r["peer_min"]).all()

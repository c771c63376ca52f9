"""The model of gsx_mesh_stats (mesh_stats_model.py) on the oracle backend:
hand-counted numbers of the reference's opportunistic-grafting test in
miniature, and the identities the tables must keep on a seeded mesh run."""
import numpy as np

import heartbeat_cases as hc
import mesh_stats_model as msm
import oracle as orc
from gsx import abi

S = abi.SECOND
COL = {name: k for k, name in enumerate(abi.MS_COL_NAMES)}


def opportunistic(be):
    """heartbeat_cases.opportunistic_graft_case -> (out, pair map, row_ptr, col, edge flags) of its overlay."""
    out, pair = hc.opportunistic_graft_case(be)
    n = 11
    keys = sorted(pair, key=pair.get)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    for u, _ in keys:
        row_ptr[u + 1] += 1
    col = np.array([v for _, v in keys], dtype=np.int32)
    ef = np.array([abi.GSX_EDGE_GOSSIPSUB | abi.GSX_EDGE_OUTBOUND if u == 0 else 0 for u, _ in keys], dtype=np.uint8)
    return out, pair, np.cumsum(row_ptr), col, ef


def hand_count(be, pair):
    """The case's numbers again, from its edges and the mesh bits alone."""
    mesh = (be.export_state()["rec_flags"] & abi.GSX_REC_IN_MESH) != 0
    node0 = [k for k in range(1, 11) if mesh[pair[(0, k)]]]
    back = [k for k in range(1, 11) if mesh[pair[(k, 0)]]]
    return node0, back


def check_opportunistic(ref, node0, back):
    """What TestGossipsubOpportunisticGrafting leaves after its one heartbeat, topic 0."""
    tot = ref["topic_tot"][0]
    assert sorted(node0[:6]) == [1, 2, 3, 4, 5, 6] and len(node0) == 8 and sorted(back) == sorted(node0)
    assert len(node0) + len(back) == 16 and 11 - 1 - len(back) == 2  # links; the peers left without a mesh
    assert tot[COL["units"]] == 11 and tot[COL["links"]] == 16 and tot[COL["outbound"]] == 8
    assert tot[COL["one_sided"]] == 0 and tot[COL["empty"]] == 2
    assert ref["node_deg"][0, 0] == 8 and ref["node_out"][0, 0] == 8
    assert ref["node_in"][0, 0] == 8 and ref["node_in"][0, 1:].sum() == 8


def classes_of_case():
    cls = np.zeros(11, dtype=np.uint8)
    cls[1:7] = 1  # the six peers of the first mesh: the sybils
    return cls


def test_opportunistic_graft_case_by_hand():
    o = orc.Oracle(1)
    out, pair, row_ptr, col, ef = opportunistic(o)
    gp = orc.default_gossipsub_params()
    node0, back = hand_count(o, pair)
    now = hc.T0 + 2 * S
    ref = msm.of_backend(o, row_ptr, col, ef, gp, now)
    check_opportunistic(ref, node0, back)
    assert ref["topic_tot"][0, COL["links"]] == out.as_dict()["mesh_links"]
    # every mesh of one peer is below Dlo = 5, node 0's 8 are within [5, 12]
    assert ref["topic_tot"][0, COL["below_dlo"]] == 10 and ref["topic_tot"][0, COL["above_dhi"]] == 0
    assert ref["topic_tot"][0, COL["below_dout"]] == 10  # only node 0 has outbound links
    assert ref["deg_hist"][0, :9].tolist() == [2, 8, 0, 0, 0, 0, 0, 0, 1] and ref["deg_hist"][0].sum() == 11
    # classes: node 0 keeps the two honest peers it grafted; they have node 0; the two left out have nobody
    cls = classes_of_case()
    want_honest = {3: 5, 2: 4}
    for mh, below in want_honest.items():
        r = msm.of_backend(o, row_ptr, col, ef, gp, now, node_class=cls, n_classes=2, hostile_mask=0b10, min_honest=mh)
        assert r["topic_tot"][0, COL["eclipsed"]] == 0 and r["topic_tot"][0, COL["below_honest"]] == below, mh
        assert r["class_links"][0].tolist() == [[4, 6], [6, 0]]
        assert r["node_class_deg"][0, 0].tolist() == [2, 6]


def test_identities_on_a_mesh_run():
    n, d, T, ticks = 130, 3, 3, 3
    o = orc.Oracle(T)
    gp = orc.default_gossipsub_params()
    ov, outs, snaps = hc.mesh_run(o, n, d, T, seed=5, ticks=ticks, gp=gp)
    now = hc.T0 + (3 + ticks) * S
    cls = (np.arange(n) % 3).astype(np.uint8)
    edges = [0, S, 2 * S + S // 2]
    ref = msm.of_backend(o, ov.row_ptr, ov.col, ov.edge_flags, gp, now, age_edges_ns=edges, node_class=cls, n_classes=3,
                         hostile_mask=0b100, min_honest=1)
    tot = ref["topic_tot"]
    links = int(tot[:, COL["links"]].sum())
    assert links == outs[-1]["mesh_links"] > 0
    assert int(ref["node_deg"].sum()) == int(ref["node_in"].sum()) == links
    assert int(ref["class_links"].sum()) == int(ref["age_hist"].sum()) == int(ref["node_class_deg"].sum()) == links
    assert (ref["age_hist"] > 0).sum() >= 2  # links of the setup and links the heartbeats grafted
    for f in ("deg_hist", "out_hist", "in_hist"):
        assert np.array_equal(ref[f].sum(1), tot[:, COL["units"]]), f
    assert (tot[:, COL["units"]] == n).all()
    # the degrees as test_heartbeat_oracle.py's invariants count them
    st = snaps[-1]
    E = ov.n_pairs
    present = (st["pair_flags"] & abi.GSX_PAIR_PRESENT) != 0
    mesh = ((st["rec_flags"].reshape(T, E) & abi.GSX_REC_IN_MESH) != 0) & present
    obs = ov.pair_observer()
    deg = np.zeros((T, n), dtype=np.int64)
    for t in range(T):
        np.add.at(deg[t], obs[mesh[t]], 1)
    assert np.array_equal(deg, ref["node_deg"])
    out_of_bounds = ((deg < gp.d_lo) | (deg > gp.d_hi)).sum(1)
    assert np.array_equal(tot[:, COL["below_dlo"]] + tot[:, COL["above_dhi"]], out_of_bounds)
    assert (deg <= gp.d_hi + 3).all() and not tot[:, COL["above_dhi"]].sum() > (deg > gp.d_hi).sum()
    # no membership set, no disconnects: no fanout; backoff only from PRUNEs
    assert not tot[:, COL["fanout_units"]].any() and not tot[:, COL["fanout_links"]].any()
    assert int((tot[:, COL["backoff"]] + tot[:, COL["backoff_expired"]]).sum()) == int((st["backoff"] != 0).sum())

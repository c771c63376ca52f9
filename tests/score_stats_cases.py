"""The numpy reference of gsx_score_stats, and the overlays its tests share.

reference() knows nothing of the engine's layout: scores and pair flags per
pair, record flags topic-major [T, E] as gsx_export_state returns them, the
overlay as (row_ptr, col)."""
from __future__ import annotations

import numpy as np

from gsx import abi, synth

SELECT = {"present": abi.GSX_SS_PRESENT, "connected": abi.GSX_SS_CONNECTED, "mesh": abi.GSX_SS_MESH}


def reference(scores, pair_flags, rec_flags, row_ptr, col, n_total, edges, select="present", topic=0):
    """-> dict(hist [B] u64, obs_bins [n_local, B] u32, obs_min [n_local] f64,
    peer_bins [n_total, B] u32, peer_min [n_total] f64), B = len(edges) + 1."""
    scores = np.asarray(scores, dtype=np.float64)
    pf = np.asarray(pair_flags, dtype=np.uint8)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    E, n_local, B = len(scores), len(row_ptr) - 1, len(edges) + 1
    sel = (pf & abi.GSX_PAIR_PRESENT) != 0
    if SELECT.get(select, select) != abi.GSX_SS_PRESENT:
        sel &= (pf & abi.GSX_PAIR_CONNECTED) != 0
    if SELECT.get(select, select) == abi.GSX_SS_MESH and E:
        rf = np.asarray(rec_flags, dtype=np.uint8).reshape(-1, E)
        sel &= (rf[topic] & abi.GSX_REC_IN_MESH) != 0
    obs = np.repeat(np.arange(n_local, dtype=np.int64), np.diff(row_ptr))
    q = np.nonzero(sel)[0]
    b = np.searchsorted(edges, scores[q], side="right")
    hist = np.zeros(B, dtype=np.uint64)
    np.add.at(hist, b, np.uint64(1))
    obs_bins = np.zeros((n_local, B), dtype=np.uint32)
    np.add.at(obs_bins, (obs[q], b), np.uint32(1))
    peer_bins = np.zeros((n_total, B), dtype=np.uint32)
    np.add.at(peer_bins, (col[q], b), np.uint32(1))
    obs_min = np.full(n_local, np.inf)
    np.fmin.at(obs_min, obs[q], scores[q])  # (fmin: the minima ignore a NaN score, gsx.h)
    peer_min = np.full(n_total, np.inf)
    np.fmin.at(peer_min, col[q], scores[q])
    return {"hist": hist, "obs_bins": obs_bins, "obs_min": obs_min, "peer_bins": peer_bins, "peer_min": peer_min}


FIELDS = ("hist", "obs_bins", "obs_min", "peer_bins", "peer_min")


def assert_equal(st, want, fields=FIELDS, what=""):
    """Raw bytes: the counters as they are, the f64 minima as their u64 views."""
    for f in fields:
        got, ref = getattr(st, f), want[f]
        assert got is not None, (what, f)
        assert got.shape == ref.shape and got.dtype == ref.dtype, (what, f, got.shape, ref.shape, got.dtype)
        if got.dtype == np.float64:
            got, ref = got.view(np.uint64), ref.view(np.uint64)
        assert np.array_equal(got, ref), (what, f, np.argwhere(got != ref)[:5].tolist())


def overlay_from_rows(rows):
    """rows[u] = the peers of node u (any order, no duplicates) -> synth.Overlay of gossipsub
    pairs; directed: (u -> v) needs no (v -> u)."""
    n = len(rows)
    deg = np.array([len(r) for r in rows], dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = (np.concatenate([np.sort(np.asarray(r, dtype=np.int32)) for r in rows]) if deg.sum()
           else np.zeros(0)).astype(np.int32)
    ips, sybil = synth._ips(n, 0.0, 50)
    return synth.Overlay(n, row_ptr, col, np.full(len(col), abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8), ips,
                         sybil)


def isolate(ov, u):
    """ov without node u's pairs, both ways: u keeps its id, an empty row, and nobody points at it."""
    import dataclasses

    keep = (ov.pair_observer() != u) & (ov.col != u)
    deg = np.bincount(ov.pair_observer()[keep], minlength=ov.n)
    return dataclasses.replace(ov, row_ptr=np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), col=ov.col[keep],
                               edge_flags=ov.edge_flags[keep])


def edges_from(values, k):
    """k edges out of the values themselves, at spread quantiles of the distinct ones: ties on
    every edge are certain."""
    u = np.unique(np.asarray(values, dtype=np.float64))
    assert len(u) >= k + 2, len(u)
    idx = np.linspace(0, len(u) - 1, k + 2)[1:-1].astype(int)
    assert len(set(idx.tolist())) == k
    return u[idx]


def degrees_overlay(n, degs, seed):
    """A directed overlay of n nodes whose row u holds degs[u] peers (< n each), drawn from the seed."""
    rng = np.random.default_rng(seed)
    rows = []
    for u, d in enumerate(degs):
        others = np.concatenate([np.arange(u), np.arange(u + 1, n)])
        rows.append(rng.choice(others, size=int(d), replace=False) if d else np.zeros(0, dtype=np.int64))
    return overlay_from_rows(rows)

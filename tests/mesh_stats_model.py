"""The contract of gsx_mesh_stats (include/gsx.h) as plain per-pair loops: no
run segmentation, nothing shared with the kernel.  Inputs are what any backend
(engine or oracle) exports: export_state(), export_backoff(),
export_membership(), scores(), the overlay arrays and the gossipsub params;
the reverse map is built from (u, v) lookups."""
from __future__ import annotations

import numpy as np

from gsx import abi

FIELDS = abi.MS_OUT_FIELDS
DTYPES = {f: (np.uint32 if f.startswith("node_") else np.uint64) for f in FIELDS}
PC = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED


def backend_inputs(be):
    """-> dict of the exports the model reads, taken from `be` now."""
    st = be.export_state()
    joined, fanout, _ = be.export_membership()
    return dict(pair_flags=st["pair_flags"], rec_flags=st["rec_flags"], graft=st["graft_time_ns"],
                backoff=be.export_backoff(), joined=joined, fanout=fanout, scores=be.scores())


def wrap64(x):
    """x as a wrapping int64 (the device subtracts in 64 bits)."""
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def age_bin(age, edges):
    return sum(1 for e in edges if not age < e)


def reference(inp, row_ptr, col, edge_flags, n_topics, gp, now_ns, n_bins=33, age_edges_ns=(), node_class=None,
              n_classes=0, hostile_mask=0, min_honest=0, symmetry=True):
    """-> {field: array} for every field of abi.MS_OUT_FIELDS (class tables of C = 0 without classes)."""
    T, n, E = int(n_topics), len(row_ptr) - 1, len(col)
    C = int(n_classes) if node_class is not None else 0
    edges = [int(x) for x in age_edges_ns]
    obs = np.repeat(np.arange(n), np.diff(row_ptr))
    pair_of = {(int(obs[p]), int(col[p])): p for p in range(E)}
    pf = np.asarray(inp["pair_flags"]).reshape(E)
    rf = np.asarray(inp["rec_flags"]).reshape(T, E)
    graft = np.asarray(inp["graft"]).reshape(T, E)
    backoff = np.asarray(inp["backoff"]).reshape(T, E)
    scores = np.asarray(inp["scores"]).reshape(E)
    joined, fanout = inp["joined"], inp["fanout"]

    def link(p, t):
        return (int(pf[p]) & PC) == PC and bool(int(rf[t, p]) & abi.GSX_REC_IN_MESH)

    def hostile(c):
        return bool((hostile_mask >> int(c)) & 1)

    tot = np.zeros((T, abi.GSX_MS_COLS), dtype=np.uint64)
    hists = {f: np.zeros((T, n_bins), dtype=np.uint64) for f in ("deg_hist", "out_hist", "in_hist")}
    age_hist = np.zeros((T, len(edges) + 1), dtype=np.uint64)
    class_links = np.zeros((T, C, C), dtype=np.uint64)
    deg = np.zeros((T, n), dtype=np.uint32)
    outd = np.zeros((T, n), dtype=np.uint32)
    ind = np.zeros((T, n), dtype=np.uint32)
    cdeg = np.zeros((T, n, C), dtype=np.uint32)
    fan_units = set()
    for t in range(T):
        for p in range(E):
            u, v = int(obs[p]), int(col[p])
            if (int(fanout[p]) >> t) & 1:
                tot[t, abi.GSX_MS_FANOUT_LINKS] += 1
                fan_units.add((u, t))
            b = int(backoff[t, p])
            if b != 0:
                tot[t, abi.GSX_MS_BACKOFF if b > now_ns else abi.GSX_MS_BACKOFF_EXPIRED] += 1
            if not link(p, t):
                continue
            tot[t, abi.GSX_MS_LINKS] += 1
            deg[t, u] += 1
            ind[t, v] += 1
            if int(edge_flags[p]) & abi.GSX_EDGE_OUTBOUND:
                tot[t, abi.GSX_MS_OUTBOUND] += 1
                outd[t, u] += 1
            if symmetry:
                q = pair_of.get((v, u))
                if q is None or not link(q, t):
                    tot[t, abi.GSX_MS_ONE_SIDED] += 1
            if scores[p] < 0:  # (False for a NaN)
                tot[t, abi.GSX_MS_NEGATIVE] += 1
            if int(rf[t, p]) & abi.GSX_REC_ACTIVE:
                tot[t, abi.GSX_MS_ACTIVE] += 1
            age = wrap64(int(now_ns) - int(graft[t, p]))
            age_hist[t, age_bin(age, edges)] += 1
            if C:
                class_links[t, int(node_class[u]), int(node_class[v])] += 1
                cdeg[t, u, int(node_class[v])] += 1
        for u in range(n):
            if (u, t) in fan_units:
                tot[t, abi.GSX_MS_FANOUT_UNITS] += 1
            if not (int(joined[u]) >> t) & 1:
                continue
            d, o, i = int(deg[t, u]), int(outd[t, u]), int(ind[t, u])
            tot[t, abi.GSX_MS_UNITS] += 1
            tot[t, abi.GSX_MS_EMPTY] += d == 0
            tot[t, abi.GSX_MS_BELOW_DLO] += d < gp.d_lo
            tot[t, abi.GSX_MS_ABOVE_DHI] += d > gp.d_hi
            tot[t, abi.GSX_MS_BELOW_DOUT] += o < gp.d_out
            hists["deg_hist"][t, min(d, n_bins - 1)] += 1
            hists["out_hist"][t, min(o, n_bins - 1)] += 1
            hists["in_hist"][t, min(i, n_bins - 1)] += 1
            if C and not hostile(node_class[u]):
                honest = sum(int(cdeg[t, u, c]) for c in range(C) if not hostile(c))
                tot[t, abi.GSX_MS_ECLIPSED] += d >= 1 and honest == 0
                tot[t, abi.GSX_MS_BELOW_HONEST] += honest < min_honest
    return dict(topic_tot=tot, age_hist=age_hist, class_links=class_links, node_deg=deg, node_out=outd, node_in=ind,
                node_class_deg=cdeg, **hists)


def of_backend(be, ov_row_ptr, ov_col, ov_edge_flags, gp, now_ns, **kw):
    return reference(backend_inputs(be), ov_row_ptr, ov_col, ov_edge_flags, be.n_topics, gp, now_ns, **kw)

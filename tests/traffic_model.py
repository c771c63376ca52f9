"""A line-by-line model of what a propagation call costs (gsx.h, gsx_prop_traffic),
for the tests: the hop rule replayed copy by copy, every copy put into its class
by what the receiver's router did with it, and from that the five tables.  The
counterpart of timed_model.py (whose fwd_byte it uses) on the hop clock, with
max_hops: plain Python on the exported state, knowing nothing of the engine's
layout.  Floodsub and gossipsub with every node joined (no fanout branch); it is
the only source of the GRAYLISTED copies per pair.

A copy is message k sent by v to u; it is recorded on u's pair q = (u -> v), one
Python int per (class, pair) with bit k = message k.
"""
from __future__ import annotations

import numpy as np

from gsx import abi
from timed_model import FWD_FORWARD, FWD_GIN, FWD_PUBLISH, fwd_byte

SENT, FIRST, DUP, INVALID, GRAYLISTED = range(5)
COLS = 5


class Result:
    pass


def run(row_ptr, col, edge_flags, pair_flags, in_mesh, scores, publish_threshold, graylist_threshold, msgs, router,
        flood_publish, max_hops, gin_extra=None):
    """gin_extra: [n_pairs] bool, pairs whose observer drops the neighbour's payload whatever the
    score says (AcceptControl under gsx_gater_enforce; direct peers are never gated).
    -> Result with rows[c][q]: the copies of pair q in column c, and the gsx_prop_out counters."""
    n = len(row_ptr) - 1
    E = len(col)
    m = len(msgs)
    obs = np.repeat(np.arange(n), np.diff(row_ptr))
    key = {(int(obs[q]), int(col[q])): q for q in range(E)}
    rev = [key.get((int(col[q]), int(obs[q]))) for q in range(E)]
    fwd = [fwd_byte(router, flood_publish, int(pair_flags[q]), int(edge_flags[q]), int(in_mesh[q]), float(scores[q]),
                    publish_threshold, graylist_threshold) for q in range(E)]
    if gin_extra is not None and router == abi.GSX_ROUTER_GOSSIPSUB:
        for q in range(E):
            if gin_extra[q] and not (int(edge_flags[q]) & abi.GSX_EDGE_DIRECT):
                fwd[q] |= FWD_GIN
    drop = 0
    origin = [0] * n
    for k in range(m):
        if int(msgs["validation"][k]) != abi.GSX_VALIDATION_ACCEPT:
            drop |= 1 << k
        origin[int(msgs["source"][k])] |= 1 << k
    seen = list(origin)
    frm = [0] * E  # pair (u -> v): messages u first received from v
    rows = [[0] * E for _ in range(COLS)]
    arriving = {}  # receiver -> [(pair q = (u -> v), bits)] of the next hop

    def send(v, row, need):
        """v sends `row` to its targets: never back to the first deliverer, never to the origin"""
        for r in range(int(row_ptr[v]), int(row_ptr[v + 1])):
            if not (fwd[r] & need) or rev[r] is None:
                continue
            x = int(col[r])
            s = row & ~frm[r] & ~origin[x]
            if not s:
                continue
            q = rev[r]
            rows[SENT][q] |= s
            if fwd[q] & FWD_GIN:  # AcceptFrom at x drops the RPC before pushMsg
                rows[GRAYLISTED][q] |= s
                continue
            arriving.setdefault(x, []).append((q, s))

    if max_hops >= 1:  # hop 1 runs: the sources publish
        for v in range(n):
            if origin[v]:
                send(v, origin[v], FWD_PUBLISH)
    h = 0
    while arriving:
        h += 1
        cur, forward = arriving, []
        arriving = {}
        for u, copies in cur.items():
            before = seen[u]
            for q, c in sorted(copies):  # ascending sender: the lowest of a hop is the first deliverer
                nb = c & ~seen[u]
                seen[u] |= nb
                frm[q] |= nb
                rows[FIRST][q] |= nb & ~drop
                rows[INVALID][q] |= nb & drop
                rows[DUP][q] |= c & ~nb
            row = (seen[u] ^ before) & ~drop
            if row:
                forward.append((u, row))
        if h < max_hops:  # hop h + 1 runs: this hop's accepted first receipts are forwarded
            for u, row in forward:
                send(u, row, FWD_FORWARD)
    R = Result()
    R.rows, R.hops = rows, h
    cnt = [sum(bin(x).count("1") for x in rows[c]) for c in range(COLS)]
    R.transmissions, R.deliveries, R.duplicates, R.invalid, R.graylisted = cnt
    return R


def run_on(be, ov, msgs, cfg, T=1, thresholds=None, gin_extra=None):
    """run() on a backend's exported state (engine or oracle), before the call under test."""
    st = be.export_state()
    rf = st["rec_flags"].reshape(T, ov.n_pairs)[cfg.topic]
    pub, gray = (-200.0, -300.0) if thresholds is None else thresholds
    return run(ov.row_ptr, ov.col, ov.edge_flags, st["pair_flags"], rf & abi.GSX_REC_IN_MESH, be.scores(), pub, gray,
               msgs, cfg.router, cfg.flood_publish, cfg.max_hops, gin_extra)


# ---- class rows as bit matrices, and the tables --------------------------------------------
def bits_of_ints(rows, m) -> np.ndarray:
    """[E] Python ints -> [E, m] u8 (bit k of row q)."""
    nb = (m + 7) // 8
    raw = np.frombuffer(b"".join(int(x).to_bytes(nb, "little") for x in rows), dtype=np.uint8).reshape(len(rows), nb)
    return np.unpackbits(raw, axis=1, bitorder="little")[:, :m] if len(rows) else np.zeros((0, m), np.uint8)


def bits_of_words(words, m) -> np.ndarray:
    """[E, W] u64 rows (gsx_prop_duplicates' layout) -> [E, m] u8."""
    w = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :m]


def first_rows(first_from, row_ptr, col) -> np.ndarray:
    """first_from [m, n] i32 (-1: none) -> [E, m] u8: bit k of pair (u -> v) when u first got k from v."""
    m, n = first_from.shape
    out = np.zeros((len(col), m), dtype=np.uint8)
    for k, u in zip(*np.nonzero(first_from >= 0)):
        q0, q1 = int(row_ptr[u]), int(row_ptr[u + 1])
        q = q0 + int(np.searchsorted(col[q0:q1], first_from[k, u]))
        assert q < q1 and col[q] == first_from[k, u]
        out[q, k] = 1
    return out


def class_bits(first, dup, gray, validation) -> np.ndarray:
    """[E, m] first-deliverer, duplicate and graylisted bits -> [COLS, E, m] u8, column SENT their union."""
    bad = np.asarray(validation) != abi.GSX_VALIDATION_ACCEPT
    B = np.zeros((COLS,) + first.shape, dtype=np.uint8)
    B[FIRST] = first * ~bad
    B[INVALID] = first * bad
    B[DUP] = dup
    B[GRAYLISTED] = gray
    assert int(B[FIRST:].sum(0).max(initial=0)) <= 1  # every copy in one class
    B[SENT] = B[FIRST:].sum(0)
    return B


def tables(B, row_ptr, col, sizes=None):
    """The five tables of gsx_prop_traffic from the class bits [COLS, E, m] (vectorised):
    -> (msg [m, 5] u32, node [n, 5] u32, node_bytes [n, 2] u64, pair [E] u32, pair_bytes [E] u64)."""
    n = len(row_ptr) - 1
    E, m = B.shape[1:]
    obs = np.repeat(np.arange(n), np.diff(row_ptr))
    sz = np.ones(m, dtype=np.uint64) if sizes is None else np.asarray(sizes, dtype=np.uint64)
    msg = B.sum(1, dtype=np.uint64).T.astype(np.uint32)
    per_pair = B.sum(2, dtype=np.uint64)  # [COLS, E]
    pair_bytes = (B[SENT].astype(np.uint64) * sz[None, :]).sum(1, dtype=np.uint64)
    node = np.zeros((n, COLS), dtype=np.uint64)
    node_bytes = np.zeros((n, 2), dtype=np.uint64)
    np.add.at(node[:, SENT], np.asarray(col, dtype=np.int64), per_pair[SENT])
    np.add.at(node_bytes[:, 0], np.asarray(col, dtype=np.int64), pair_bytes)
    for c in range(FIRST, COLS):
        np.add.at(node[:, c], obs, per_pair[c])
    np.add.at(node_bytes[:, 1], obs, pair_bytes)
    return msg, node.astype(np.uint32), node_bytes, per_pair[SENT].astype(np.uint32), pair_bytes


def tables_loop(B, row_ptr, col, sizes=None):
    """tables() by brute force: one Python step per copy."""
    n = len(row_ptr) - 1
    E, m = B.shape[1:]
    msg = [[0] * COLS for _ in range(m)]
    node = [[0] * COLS for _ in range(n)]
    nbytes = [[0, 0] for _ in range(n)]
    pair, pbytes = [0] * E, [0] * E
    for u in range(n):
        for q in range(int(row_ptr[u]), int(row_ptr[u + 1])):
            v = int(col[q])
            for k in range(m):
                for c in range(FIRST, COLS):
                    if B[c, q, k]:
                        b = 1 if sizes is None else int(sizes[k])
                        msg[k][SENT] += 1
                        msg[k][c] += 1
                        node[v][SENT] += 1
                        node[u][c] += 1
                        nbytes[v][0] += b
                        nbytes[u][1] += b
                        pair[q] += 1
                        pbytes[q] += b
    return (np.array(msg, dtype=np.uint32).reshape(m, COLS), np.array(node, dtype=np.uint32).reshape(n, COLS),
            np.array(nbytes, dtype=np.uint64).reshape(n, 2), np.array(pair, dtype=np.uint32),
            np.array(pbytes, dtype=np.uint64))

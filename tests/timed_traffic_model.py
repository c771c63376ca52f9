"""A copy-by-copy model of what a timed propagation costs and when (gsx.h,
gsx_timed_traffic), for the tests: its own event loop over the rule of
gsx_propagate_timed (the style of timed_model.py, whose fwd_byte it uses; it
does not call timed_model.run), recording every copy as
(k, v, u, send tick, arrival tick, class, in-window), and the nine tables built
from that list.  Plain Python on the exported state, knowing nothing of the
engine's layout.  Floodsub and gossipsub with every node joined (no fanout).
"""
from __future__ import annotations

import numpy as np

from gsx import abi
from timed_model import FWD_FORWARD, FWD_GIN, FWD_PUBLISH, fwd_byte

SENT, FIRST, DUP, INVALID, GRAYLISTED, IN_FLIGHT, DUP_IN_WINDOW = range(7)
COLS = 7


class Result:
    pass


def run(row_ptr, col, edge_flags, pair_flags, in_mesh, scores, publish_threshold, graylist_threshold, lat, msgs,
        router, flood_publish, tick_ns, validation_delay_ns, window_ns, max_ticks):
    """-> Result with copies: a list of (k, v, u, f, at, class, in_window) for every copy sent at
    a tick f <= max_ticks (class one of FIRST, DUP, INVALID, GRAYLISTED, IN_FLIGHT), tick [m, n]
    (0xFFFF: never) and pair_of: {(u, v): q}."""
    n = len(row_ptr) - 1
    E = len(col)
    m = len(msgs)
    assert validation_delay_ns % tick_ns == 0 and np.all(np.asarray(lat) >= 1)
    vd = validation_delay_ns // tick_ns
    lim = vd + window_ns // tick_ns
    obs = np.repeat(np.arange(n), np.diff(row_ptr))
    key = {(int(obs[q]), int(col[q])): q for q in range(E)}
    rev = [key.get((int(col[q]), int(obs[q]))) for q in range(E)]
    fwd = [fwd_byte(router, flood_publish, int(pair_flags[q]), int(edge_flags[q]), int(in_mesh[q]), float(scores[q]),
                    publish_threshold, graylist_threshold) for q in range(E)]
    accept = [int(msgs["validation"][k]) == abi.GSX_VALIDATION_ACCEPT for k in range(m)]
    source = [int(msgs["source"][k]) for k in range(m)]
    held = [set() for _ in range(n)]       # messages a node has seen
    first_of = [dict() for _ in range(n)]  # message -> the peer it first came from
    tick = np.full((m, n), 0xFFFF, dtype=np.uint16)
    copies = []
    arriving = {}  # arrival tick -> receiver -> [(sender, k, f)]

    def send(v, f, ks, need):
        if f > max_ticks:  # a node whose send tick lies beyond the call's end sends nothing
            return
        for r in range(int(row_ptr[v]), int(row_ptr[v + 1])):
            if not (fwd[r] & need) or rev[r] is None:
                continue
            u = int(col[r])
            q = rev[r]
            for k in ks:
                if first_of[v].get(k) == u or source[k] == u:
                    continue
                at = f + int(lat[q])
                if at > max_ticks:
                    copies.append((k, v, u, f, at, IN_FLIGHT, False))
                elif fwd[q] & FWD_GIN:  # AcceptFrom at u drops the RPC before pushMsg
                    copies.append((k, v, u, f, at, GRAYLISTED, False))
                else:
                    arriving.setdefault(at, {}).setdefault(u, []).append((v, k, f))

    own = [[] for _ in range(n)]
    for k in range(m):
        own[source[k]].append(k)
        held[source[k]].add(k)
        tick[k, source[k]] = 0
    for v in range(n):
        if own[v]:
            send(v, 0, own[v], FWD_PUBLISH)
    while arriving:
        t = min(arriving)
        for u, got in arriving.pop(t).items():
            fresh = []
            for v, k, f in sorted(got):  # ascending sender: the lowest of a tick is the first deliverer
                if k in held[u]:
                    copies.append((k, v, u, f, t, DUP, t - int(tick[k, u]) <= lim))
                    continue
                held[u].add(k)
                first_of[u][k] = v
                tick[k, u] = t
                copies.append((k, v, u, f, t, FIRST if accept[k] else INVALID, False))
                if accept[k]:
                    fresh.append(k)
            if fresh:
                send(u, t + vd, fresh, FWD_FORWARD)
    R = Result()
    R.copies, R.tick, R.pair_of, R.n, R.m, R.E = copies, tick, key, n, m, E
    return R


def run_on(be, ov, lat, msgs, cfg, max_ticks, T=1, thresholds=None, window_ns=None):
    """run() on a backend's exported state (engine or oracle), before the call under test."""
    st = be.export_state()
    rf = st["rec_flags"].reshape(T, ov.n_pairs)[cfg.topic]
    pub, gray = (-200.0, -300.0) if thresholds is None else thresholds
    window = 25 * abi.MILLISECOND if window_ns is None else window_ns
    return run(ov.row_ptr, ov.col, ov.edge_flags, st["pair_flags"], rf & abi.GSX_REC_IN_MESH, be.scores(), pub, gray,
               lat, msgs, cfg.router, cfg.flood_publish, cfg.hop_latency_ns, cfg.validation_delay_ns, window, max_ticks)


def counters(R) -> dict:
    """The counters of timed_model.run / gsx_timed_out the copies determine."""
    c = [0] * COLS
    win = 0
    for _, _, _, _, _, cls, inw in R.copies:
        c[cls] += 1
        win += inw
    return dict(deliveries=c[FIRST], duplicates=c[DUP], invalid=c[INVALID], graylisted=c[GRAYLISTED],
                in_flight=c[IN_FLIGHT], dup_in_window=win,
                transmissions=c[FIRST] + c[DUP] + c[INVALID] + c[GRAYLISTED])


class Tables:
    NAMES = ("msg", "node", "node_bytes", "pair", "pair_bytes", "bins", "bin_bytes", "node_peak", "node_peak_bin")


def tables(R, sizes=None, bin_ticks=1, n_bins=64) -> Tables:
    """The nine tables of gsx_timed_traffic from the copy list, and node_bin [n, n_bins, 2]: the
    bytes each node sent / that reached it per bin."""
    n, m, E = R.n, R.m, R.E
    sz = np.ones(m, dtype=np.uint64) if sizes is None else np.asarray(sizes, dtype=np.uint64)
    T = Tables()
    T.msg = np.zeros((m, COLS), dtype=np.uint64)
    T.node = np.zeros((n, COLS), dtype=np.uint64)
    T.node_bytes = np.zeros((n, 2), dtype=np.uint64)
    T.pair = np.zeros(E, dtype=np.uint64)
    T.pair_bytes = np.zeros(E, dtype=np.uint64)
    T.bins = np.zeros((n_bins, COLS), dtype=np.uint64)
    T.bin_bytes = np.zeros((n_bins, 2), dtype=np.uint64)
    T.node_bin = np.zeros((n, n_bins, 2), dtype=np.uint64)
    if R.copies:
        c = np.array([(k, v, u, f, at, cls, inw, R.pair_of[(u, v)]) for k, v, u, f, at, cls, inw in R.copies],
                     dtype=np.int64)
        k, v, u, f, at, cls, inw, q = c.T
        one = np.uint64(1)
        b = sz[k]
        sb = np.minimum(f // bin_ticks, n_bins - 1)
        ab = np.minimum(at // bin_ticks, n_bins - 1)
        arrived = cls != IN_FLIGHT
        w = inw.astype(bool)
        # every copy was sent: the sender's side
        np.add.at(T.msg, (k, SENT), one)
        np.add.at(T.node, (v, SENT), one)
        np.add.at(T.bins, (sb, SENT), one)
        np.add.at(T.node_bytes, (v, 0), b)
        np.add.at(T.bin_bytes, (sb, 0), b)
        np.add.at(T.node_bin, (v, sb, 0), b)
        fl = ~arrived
        np.add.at(T.msg, (k[fl], IN_FLIGHT), one)
        np.add.at(T.node, (v[fl], IN_FLIGHT), one)
        np.add.at(T.bins, (sb[fl], IN_FLIGHT), one)
        # the arrived ones: the receiver's side
        a = arrived
        np.add.at(T.msg, (k[a], cls[a]), one)
        np.add.at(T.node, (u[a], cls[a]), one)
        np.add.at(T.bins, (ab[a], cls[a]), one)
        np.add.at(T.node_bytes, (u[a], 1), b[a])
        np.add.at(T.bin_bytes, (ab[a], 1), b[a])
        np.add.at(T.node_bin, (u[a], ab[a], 1), b[a])
        np.add.at(T.pair, q[a], one)
        np.add.at(T.pair_bytes, q[a], b[a])
        np.add.at(T.msg, (k[w], DUP_IN_WINDOW), one)
        np.add.at(T.node, (u[w], DUP_IN_WINDOW), one)
        np.add.at(T.bins, (ab[w], DUP_IN_WINDOW), one)
    T.node_peak = T.node_bin.max(1)
    T.node_peak_bin = np.where(T.node_peak > 0, T.node_bin.argmax(1), 0).astype(np.uint32)  # (argmax: the lowest)
    assert T.msg.max(initial=0) < 2 ** 32 and T.node.max(initial=0) < 2 ** 32 and T.pair.max(initial=0) < 2 ** 32
    T.msg, T.node, T.pair = T.msg.astype(np.uint32), T.node.astype(np.uint32), T.pair.astype(np.uint32)
    return T


def tables_loop(R, sizes=None, bin_ticks=1, n_bins=64) -> Tables:
    """tables() by brute force: one Python step per copy (no peaks)."""
    n, m, E = R.n, R.m, R.E
    T = Tables()
    T.msg = np.zeros((m, COLS), dtype=np.uint32)
    T.node = np.zeros((n, COLS), dtype=np.uint32)
    T.node_bytes = np.zeros((n, 2), dtype=np.uint64)
    T.pair = np.zeros(E, dtype=np.uint32)
    T.pair_bytes = np.zeros(E, dtype=np.uint64)
    T.bins = np.zeros((n_bins, COLS), dtype=np.uint64)
    T.bin_bytes = np.zeros((n_bins, 2), dtype=np.uint64)
    for k, v, u, f, at, cls, inw in R.copies:
        b = np.uint64(1 if sizes is None else int(sizes[k]))
        sb, ab = min(f // bin_ticks, n_bins - 1), min(at // bin_ticks, n_bins - 1)
        T.msg[k, SENT] += 1
        T.node[v, SENT] += 1
        T.bins[sb, SENT] += np.uint64(1)
        T.node_bytes[v, 0] += b
        T.bin_bytes[sb, 0] += b
        if cls == IN_FLIGHT:
            T.msg[k, cls] += 1
            T.node[v, cls] += 1
            T.bins[sb, cls] += np.uint64(1)
            continue
        q = R.pair_of[(u, v)]
        T.msg[k, cls] += 1
        T.node[u, cls] += 1
        T.bins[ab, cls] += np.uint64(1)
        T.node_bytes[u, 1] += b
        T.bin_bytes[ab, 1] += b
        T.pair[q] += 1
        T.pair_bytes[q] += b
        if inw:
            T.msg[k, DUP_IN_WINDOW] += 1
            T.node[u, DUP_IN_WINDOW] += 1
            T.bins[ab, DUP_IN_WINDOW] += np.uint64(1)
    return T

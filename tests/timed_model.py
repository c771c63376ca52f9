"""A line-by-line model of timed propagation (gsx.h, gsx_propagate_timed), for
the tests: what every node receives at which tick over links of different
latencies, who delivered it first, the counters, and the per-pair counts the
credits are folded from.  The counterpart of gater_model.py and tag_model.py:
plain Python on the exported state, knowing nothing of the engine's layout.

A node's message set is one Python int (bit k = message k); the copies in
flight are kept per arrival tick.  fwd_byte restates the routers' targets
(floodsub.go:76-100; gossipsub.go:943-1013: direct peers, floodsub peers above
publishThreshold, mesh peers, flood publish; AcceptFrom's graylist gate,
gossipsub.go:583-594).  Every node has joined the topic (asserted by the
caller's setup: no set_subscriptions), so there is no fanout branch.
"""
from __future__ import annotations

import numpy as np

from gsx import abi

FWD_FORWARD, FWD_PUBLISH, FWD_GIN = 1, 2, 8


def fwd_byte(router, flood_publish, pf, ef, in_mesh, score, publish_threshold, graylist_threshold):
    """Pair r = (v -> u), v's own record of u: what v sends to u (FORWARD: messages v received,
    PUBLISH: messages v published), and GIN: v drops every copy u sends it."""
    out = 0
    both = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
    if (pf & both) == both:  # in ps.topics[topic]
        if router == abi.GSX_ROUTER_FLOODSUB:
            out = FWD_FORWARD | FWD_PUBLISH
        else:
            direct = bool(ef & abi.GSX_EDGE_DIRECT)
            floodsub_peer = not (ef & abi.GSX_EDGE_GOSSIPSUB)
            above = (not direct) and (floodsub_peer or flood_publish) and score >= publish_threshold
            fwd = direct or (floodsub_peer and above) or bool(in_mesh)
            pub = (direct or above) if flood_publish else fwd
            out = (FWD_FORWARD if fwd else 0) | (FWD_PUBLISH if pub else 0)
    if router == abi.GSX_ROUTER_GOSSIPSUB and not (ef & abi.GSX_EDGE_DIRECT) and score < graylist_threshold:
        out |= FWD_GIN
    return out


class Result:
    pass


def run(row_ptr, col, edge_flags, pair_flags, in_mesh, scores, publish_threshold, graylist_threshold, lat, msgs,
        router, flood_publish, tick_ns, validation_delay_ns, window_ns, max_ticks):
    """in_mesh: [n_pairs] the topic's REC_IN_MESH flags; window_ns: the topic's
    MeshMessageDeliveriesWindow (0 for a topic that is not scored).  -> Result with tick [m, n]
    u16, first_from [m, n] i32, the counters, and first / dup_in / inv [n_pairs] counts."""
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
    drop = rej = 0
    origin = [0] * n
    for k in range(m):
        v = int(msgs["validation"][k])
        if v != abi.GSX_VALIDATION_ACCEPT:
            drop |= 1 << k
            if v == abi.GSX_VALIDATION_REJECT:
                rej |= 1 << k
        origin[int(msgs["source"][k])] |= 1 << k
    seen = list(origin)
    frm = [0] * E  # pair (u -> v): messages u first received from v
    tick = np.full((m, n), 0xFFFF, dtype=np.uint16)
    first_from = np.full((m, n), -1, dtype=np.int32)
    for k in range(m):
        tick[k, int(msgs["source"][k])] = 0
    first = np.zeros(E, dtype=np.uint32)
    dup_in = np.zeros(E, dtype=np.uint32)
    inv = np.zeros(E, dtype=np.uint32)
    R = Result()
    R.deliveries = R.duplicates = R.dup_in_window = R.rejected = R.ignored = R.graylisted = 0
    R.last_tick = R.ticks_run = 0
    arriving = {}  # arrival tick -> receiver -> [(pair q = (u -> v), bits)]

    def send(v, f, row, need):
        """v sends `row` at tick f to its targets: never back to the first deliverer, never to the origin"""
        for r in range(int(row_ptr[v]), int(row_ptr[v + 1])):
            if not (fwd[r] & need) or rev[r] is None:
                continue
            x = int(col[r])
            s = row & ~frm[r] & ~origin[x]
            if not s:
                continue
            q = rev[r]
            at = f + int(lat[q])
            if at > max_ticks:  # in flight when the call ends
                continue
            R.ticks_run = max(R.ticks_run, at)
            if fwd[q] & FWD_GIN:  # AcceptFrom at x drops the RPC before pushMsg
                R.graylisted += bin(s).count("1")
                continue
            arriving.setdefault(at, {}).setdefault(x, []).append((q, s))

    for v in range(n):
        if origin[v]:
            send(v, 0, origin[v], FWD_PUBLISH)
    t = 0
    while arriving:
        t = min(arriving)
        for u, copies in arriving.pop(t).items():
            before = seen[u]
            for q, c in sorted(copies):  # ascending sender: the lowest of a tick is the first deliverer
                nb = c & ~seen[u]
                seen[u] |= nb
                frm[q] |= nb
                b = nb
                while b:
                    k = (b & -b).bit_length() - 1
                    b &= b - 1
                    tick[k, u] = t
                    first_from[k, u] = col[q]
                    if not (drop >> k) & 1:
                        R.deliveries += 1
                        first[q] += 1
                    elif (rej >> k) & 1:
                        R.rejected += 1
                        inv[q] += 1
                    else:
                        R.ignored += 1
                if nb:
                    R.last_tick = t
                d = c & ~nb
                while d:
                    k = (d & -d).bit_length() - 1
                    d &= d - 1
                    R.duplicates += 1
                    if t - int(tick[k, u]) <= lim:  # arrival <= validated + window
                        R.dup_in_window += 1
                        dup_in[q] += 1
            row = (seen[u] ^ before) & ~drop
            if row:
                send(u, t + vd, row, FWD_FORWARD)
    R.transmissions = R.deliveries + R.duplicates + R.rejected + R.ignored + R.graylisted
    R.tick, R.first_from, R.first, R.dup_in, R.inv = tick, first_from, first, dup_in, inv
    return R


def counters(r) -> dict:
    """The fields abi.TimedOut.as_dict() has, of a Result or a TimedOut."""
    return {k: int(getattr(r, k)) for k in ("deliveries", "duplicates", "transmissions", "rejected", "ignored",
                                            "graylisted", "dup_in_window", "last_tick", "ticks_run")}


def run_on(be, ov, lat, msgs, cfg, max_ticks, T=1, thresholds=None, topic_params=None):
    """run() on a backend's exported state (engine or oracle), before the call under test."""
    st = be.export_state()
    E = ov.n_pairs
    rf = st["rec_flags"].reshape(T, E)[cfg.topic]
    pub, gray = (-200.0, -300.0) if thresholds is None else thresholds
    window = 25 * abi.MILLISECOND if topic_params is None else topic_params
    return run(ov.row_ptr, ov.col, ov.edge_flags, st["pair_flags"], rf & abi.GSX_REC_IN_MESH, be.scores(), pub, gray,
               lat, msgs, cfg.router, cfg.flood_publish, cfg.hop_latency_ns, cfg.validation_delay_ns, window, max_ticks)


def add_ones_capped(x: float, k: int, cap: float) -> float:
    """k steps of `x += 1; if x > cap: x = cap` (score.go:925-938, 970-973)."""
    for _ in range(int(k)):
        x = x + 1.0
        if x > cap:
            return cap
    return x


def fold(st, T, topic, first, dup_in, inv, fmd_cap, mmd_cap):
    """The exported state after the counts are folded: markFirstMessageDelivery (fmd, and mmd
    when in mesh), markDuplicateMessageDelivery (mmd when in mesh), markInvalidMessageDelivery
    (imd, no cap), for present pairs (score.go:894-974)."""
    out = {k: np.array(v, copy=True) for k, v in st.items() if isinstance(v, np.ndarray)}
    E = len(first)
    fmd = out["first_message_deliveries"].reshape(T, E)[topic]
    mmd = out["mesh_message_deliveries"].reshape(T, E)[topic]
    imd = out["invalid_message_deliveries"].reshape(T, E)[topic]
    rf = out["rec_flags"].reshape(T, E)[topic]
    for q in np.nonzero((first | dup_in | inv) != 0)[0]:
        if not out["pair_flags"][q] & abi.GSX_PAIR_PRESENT:
            continue
        imd[q] = add_ones_capped(float(imd[q]), inv[q], float("inf"))
        fmd[q] = add_ones_capped(float(fmd[q]), first[q], fmd_cap)
        if rf[q] & abi.GSX_REC_IN_MESH:
            mmd[q] = add_ones_capped(float(mmd[q]), int(first[q]) + int(dup_in[q]), mmd_cap)
    return out

"""Python handle on the HIP engine (libgsx.so) through the C ABI of include/gsx.h.

This is plumbing for tests and bench.py: every call goes straight to the
C ABI; nothing here computes scores.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional

import numpy as np

from . import abi
from .abi import GsxError, prop_words


def _ptr(a: Optional[np.ndarray], ctype):
    if a is None:
        return C.cast(None, C.POINTER(ctype))
    return a.ctypes.data_as(C.POINTER(ctype))


_CTYPES = {"<f8": C.c_double, "<i8": C.c_int64, "u1": C.c_uint8}


def default_gossipsub_params(**kw) -> abi.GossipSubParams:
    """DefaultGossipSubParams (gossipsub.go:230-260, gsx_default_gossipsub_params) with overrides."""
    gp = abi.GossipSubParams()
    rc = abi.load_library().gsx_default_gossipsub_params(C.byref(gp))
    if rc != 0:
        raise RuntimeError(f"gsx_default_gossipsub_params -> {rc}")
    for k, v in kw.items():
        setattr(gp, k, v)
    return gp


def make_struct(cls, **kw):
    s = cls()
    for k, v in kw.items():
        if not hasattr(s, k):
            raise AttributeError(f"{cls.__name__} has no field {k}")
        setattr(s, k, v)
    return s


class PropStats:
    """Per-message delivery and latency summary of a propagation call
    (gsx_prop_stats): hop_hist[k, h] = nodes that first got message k at hop
    h (h = 0: its source); optionally node_received[u] = messages node u got
    at hops >= 1 and node_hop_sum[u] = the sum of their hops.  Everything
    below is numpy on those integers; nothing here touches the device."""

    def __init__(self, hop_hist, node_received=None, node_hop_sum=None):
        self.hop_hist = np.ascontiguousarray(hop_hist, dtype=np.uint32).reshape(-1, abi.GSX_MAX_HOPS + 1)
        self.node_received = None if node_received is None else np.ascontiguousarray(node_received, dtype=np.uint32)
        self.node_hop_sum = None if node_hop_sum is None else np.ascontiguousarray(node_hop_sum, dtype=np.uint64)

    @property
    def n_msgs(self) -> int:
        return self.hop_hist.shape[0]

    def _h(self) -> np.ndarray:
        return self.hop_hist.astype(np.int64)

    def reached(self) -> np.ndarray:
        """[m] i64: nodes that received each message (first receipts, hops >= 1; the source is not one)."""
        return self._h()[:, 1:].sum(1)

    def delivery_ratio(self, n_receivers) -> np.ndarray:
        """[m] f64: reached() / n_receivers (a count, or one per message: e.g. the topic's subscribers - 1)."""
        return self.reached() / np.asarray(n_receivers, dtype=np.float64)

    def last_hop(self) -> np.ndarray:
        """[m] i64: the last hop at which a node got the message (0: only its source holds it; -1: an
        empty row, e.g. a shard that holds neither the source nor a receiver)."""
        nz = self.hop_hist != 0
        last = nz.shape[1] - 1 - np.argmax(nz[:, ::-1], axis=1)
        return np.where(nz.any(1), last, -1).astype(np.int64)

    def mean_hop(self) -> np.ndarray:
        """[m] f64: mean arrival hop over the message's receivers (nan: nobody received it)."""
        h = self._h()
        tot = (h[:, 1:] * np.arange(1, h.shape[1])).sum(1)
        r = h[:, 1:].sum(1)
        return np.where(r > 0, tot / np.maximum(r, 1), np.nan)

    def hops_to_fraction(self, q: float, n_receivers) -> np.ndarray:
        """[m] i64: the smallest hop h after which at least a fraction q of n_receivers holds the
        message (receipts of hops 1 .. h over n_receivers >= q); -1 if the call never got there."""
        cum = np.cumsum(self._h(), axis=1)
        cum -= cum[:, :1]  # hop 0 is the source, not a receipt
        ok = cum / np.asarray(n_receivers, dtype=np.float64).reshape(-1, 1) >= q
        return np.where(ok.any(1), np.argmax(ok, axis=1), -1).astype(np.int64)

    def node_mean_hop(self) -> np.ndarray:
        """[n] f64: mean arrival hop per node (nan: the node received nothing); needs per_node."""
        r = self.node_received.astype(np.float64)
        return np.where(r > 0, self.node_hop_sum.astype(np.float64) / np.maximum(r, 1), np.nan)

    def __add__(self, other: "PropStats") -> "PropStats":
        """Range shards of one call, in rank order: the histograms add up (each node is on one
        shard), the per-node arrays (kept when both sides have them) follow one another."""
        if self.hop_hist.shape != other.hop_hist.shape:
            raise ValueError("histograms of different calls")
        tot = self._h() + other._h()
        both = self.node_received is not None and other.node_received is not None
        return PropStats(tot, np.concatenate([self.node_received, other.node_received]) if both else None,
                         np.concatenate([self.node_hop_sum, other.node_hop_sum]) if both else None)

    @staticmethod
    def concat(parts) -> "PropStats":
        """Message-parallel replicas, in rank order: each holds the rows of its message slice over
        every node, so the rows follow one another and the per-node arrays add up."""
        parts = list(parts)
        per_node = bool(parts) and all(p.node_received is not None for p in parts)
        return PropStats(np.concatenate([p.hop_hist for p in parts], 0) if parts else np.zeros((0, 65), np.uint32),
                         sum(p.node_received.astype(np.uint64) for p in parts) if per_node else None,
                         sum(p.node_hop_sum for p in parts) if per_node else None)


class PropTraffic:
    """What a propagation call cost (gsx_prop_traffic).  A copy is message k sent by v to u;
    the columns are SENT (every copy) and the four classes FIRST, DUP, INVALID, GRAYLISTED by
    what u's router did with it.  msg[k, c]: copies of message k; node[u, SENT]: copies u sent,
    node[u, c] otherwise: copies of class c that reached u; node_bytes[u] = (bytes u sent, bytes
    that reached u); pair[q] / pair_bytes[q]: the copies pair q's neighbour sent its observer.
    Any table may be None (not asked for).  Numpy on those integers; nothing here touches the
    device."""

    SENT, FIRST, DUP, INVALID, GRAYLISTED = range(abi.GSX_TRAFFIC_COLS)
    COLS = abi.GSX_TRAFFIC_COLS

    def __init__(self, msg=None, node=None, node_bytes=None, pair=None, pair_bytes=None):
        def arr(x, dt, shape):
            return None if x is None else np.ascontiguousarray(x, dtype=dt).reshape(shape)

        self.msg = arr(msg, np.uint32, (-1, self.COLS))
        self.node = arr(node, np.uint32, (-1, self.COLS))
        self.node_bytes = arr(node_bytes, np.uint64, (-1, 2))
        self.pair = arr(pair, np.uint32, (-1,))
        self.pair_bytes = arr(pair_bytes, np.uint64, (-1,))

    def total(self, col: int) -> int:
        """Copies of a column over the whole call (from the per-message table, else the per-node one)."""
        t = self.msg if self.msg is not None else self.node
        return int(t[:, col].astype(np.int64).sum())

    def sent(self) -> int:
        """Every copy of the call: gsx_prop_out.transmissions."""
        return self.total(self.SENT)

    def amplification(self) -> np.ndarray:
        """[m] f64: copies sent per first receipt of the message, SENT / max(FIRST + INVALID, 1)."""
        t = self.msg.astype(np.int64)
        return t[:, self.SENT] / np.maximum(t[:, self.FIRST] + t[:, self.INVALID], 1)

    def duplicate_ratio(self) -> np.ndarray:
        """[n] f64: the share of the copies that reached a node which it had already seen (0 where none did)."""
        t = self.node.astype(np.int64)
        got = t[:, self.FIRST:].sum(1)
        return np.where(got > 0, t[:, self.DUP] / np.maximum(got, 1), 0.0)

    def upload_bytes(self) -> np.ndarray:
        return self.node_bytes[:, 0]

    def download_bytes(self) -> np.ndarray:
        return self.node_bytes[:, 1]

    def busiest(self, k: int, by: str = "upload_bytes") -> np.ndarray:
        """The k node ids with the largest `by` ("upload_bytes", "download_bytes", "sent" or
        "received" copies), largest first, ties broken by ascending id."""
        if by in ("upload_bytes", "download_bytes"):
            key = getattr(self, by)()
        elif by == "sent":
            key = self.node[:, self.SENT]
        elif by == "received":
            key = self.node[:, self.FIRST:].astype(np.int64).sum(1)
        else:
            raise ValueError(f"busiest by {by!r}")
        # ascending by (key, -id), reversed: key descending, equal keys by ascending id
        order = np.lexsort((-np.arange(len(key), dtype=np.int64), key))[::-1]
        return order[: max(int(k), 0)].astype(np.int64)

    @staticmethod
    def concat(parts) -> "PropTraffic":
        """Message-parallel replicas, in rank order: the message rows follow one another, the node and
        pair tables (kept when every part has them) add up."""
        parts = list(parts)

        def add(name, dt):
            xs = [getattr(p, name) for p in parts]
            if not xs or any(x is None for x in xs):
                return None
            return sum(x.astype(np.uint64) for x in xs).astype(dt)

        msgs = [p.msg for p in parts]
        msg = None if not msgs or any(x is None for x in msgs) else np.concatenate(msgs, 0)
        return PropTraffic(msg, add("node", np.uint32), add("node_bytes", np.uint64), add("pair", np.uint32),
                           add("pair_bytes", np.uint64))


class TimedTraffic:
    """What a timed propagation cost, and when (gsx_timed_traffic).  A copy is message k sent by
    v to u at a tick <= max_ticks.  The columns are SENT (every copy), the classes FIRST, DUP,
    INVALID, GRAYLISTED (arrived: what u's router did with it) and IN_FLIGHT (not arrived when the
    call ended), and DUP_IN_WINDOW (the DUP copies inside the P3 window; not a class).
    msg[k, c]: copies of message k; node[u, SENT / IN_FLIGHT]: copies u sent, node[u, c]
    otherwise: copies that reached u; node_bytes[u] = (bytes u sent, bytes that reached u);
    pair[q] / pair_bytes[q]: the arrived copies pair q's neighbour sent its observer;
    bins[b, c] / bin_bytes[b] = (sent, arrived): the same per tick bin (SENT and IN_FLIGHT by
    send tick, the rest by arrival tick; bin of tick t: min(t // bin_ticks, n_bins - 1));
    node_peak[u] = (largest bytes u sent in one bin, largest bytes that reached u in one bin),
    node_peak_bin[u]: the lowest bins that hold them.  Any table may be None (not asked for).
    Numpy on those integers; nothing here touches the device."""

    SENT, FIRST, DUP, INVALID, GRAYLISTED, IN_FLIGHT, DUP_IN_WINDOW = range(abi.GSX_TT_COLS)
    COLS = abi.GSX_TT_COLS

    def __init__(self, msg=None, node=None, node_bytes=None, pair=None, pair_bytes=None, bins=None, bin_bytes=None,
                 node_peak=None, node_peak_bin=None, bin_ticks=1, tick_ns=None):
        def arr(x, dt, shape):
            return None if x is None else np.ascontiguousarray(x, dtype=dt).reshape(shape)

        self.msg = arr(msg, np.uint32, (-1, self.COLS))
        self.node = arr(node, np.uint32, (-1, self.COLS))
        self.node_bytes = arr(node_bytes, np.uint64, (-1, 2))
        self.pair = arr(pair, np.uint32, (-1,))
        self.pair_bytes = arr(pair_bytes, np.uint64, (-1,))
        self.bins = arr(bins, np.uint64, (-1, self.COLS))
        self.bin_bytes = arr(bin_bytes, np.uint64, (-1, 2))
        self.node_peak = arr(node_peak, np.uint64, (-1, 2))
        self.node_peak_bin = arr(node_peak_bin, np.uint32, (-1, 2))
        self.bin_ticks = int(bin_ticks)
        if self.bin_ticks < 1:
            raise ValueError("bin_ticks >= 1")
        self.tick_ns = tick_ns

    def total(self, col: int) -> int:
        """Copies of a column over the whole call (from the per-message table, else the per-bin
        one, else the per-node one)."""
        t = self.msg if self.msg is not None else self.bins if self.bins is not None else self.node
        return int(t[:, col].astype(np.int64).sum())

    def sent(self) -> int:
        """Every copy of the call: gsx_timed_out.transmissions + in_flight()."""
        return self.total(self.SENT)

    def in_flight(self) -> int:
        """Copies sent and not arrived when the call ended."""
        return self.total(self.IN_FLIGHT)

    def amplification(self) -> np.ndarray:
        """[m] f64: copies sent per first receipt of the message, SENT / max(FIRST + INVALID, 1)."""
        t = self.msg.astype(np.int64)
        return t[:, self.SENT] / np.maximum(t[:, self.FIRST] + t[:, self.INVALID], 1)

    def duplicate_ratio(self) -> np.ndarray:
        """[n] f64: the share of the copies that reached a node which it had already seen (0 where none did)."""
        t = self.node.astype(np.int64)
        got = t[:, self.FIRST:self.GRAYLISTED + 1].sum(1)
        return np.where(got > 0, t[:, self.DUP] / np.maximum(got, 1), 0.0)

    def upload_bytes(self) -> np.ndarray:
        return self.node_bytes[:, 0]

    def download_bytes(self) -> np.ndarray:
        return self.node_bytes[:, 1]

    def load(self, unit: str = "bytes") -> np.ndarray:
        """[n_bins, 2] u64: the network's load per bin as (sent, arrived), in "bytes" or "copies"."""
        if unit == "bytes":
            return self.bin_bytes
        if unit == "copies":
            b = self.bins
            return np.stack([b[:, self.SENT], b[:, self.FIRST:self.GRAYLISTED + 1].sum(1, dtype=np.uint64)], 1)
        raise ValueError(f"load in {unit!r}")

    def peak_upload(self) -> np.ndarray:
        """[n] u64: the most bytes each node sent in one bin."""
        return self.node_peak[:, 0]

    def peak_download(self) -> np.ndarray:
        """[n] u64: the most bytes that reached each node in one bin."""
        return self.node_peak[:, 1]

    def busiest(self, k: int, by: str = "upload_bytes") -> np.ndarray:
        """The k node ids with the largest `by` ("upload_bytes", "download_bytes", "peak_upload",
        "peak_download", "sent" or "received" copies), largest first, ties broken by ascending id."""
        if by in ("upload_bytes", "download_bytes", "peak_upload", "peak_download"):
            key = getattr(self, by)()
        elif by == "sent":
            key = self.node[:, self.SENT]
        elif by == "received":
            key = self.node[:, self.FIRST:self.GRAYLISTED + 1].astype(np.int64).sum(1)
        else:
            raise ValueError(f"busiest by {by!r}")
        # ascending by (key, -id), reversed: key descending, equal keys by ascending id
        order = np.lexsort((-np.arange(len(key), dtype=np.int64), key))[::-1]
        return order[: max(int(k), 0)].astype(np.int64)

    def bytes_per_second(self, per_bin, tick_ns=None) -> np.ndarray:
        """A per-bin figure (load(), a peak) -> per second: a bin lasts bin_ticks * tick_ns ns
        (tick_ns: the call's tick length, taken from the call when not given)."""
        t = self.tick_ns if tick_ns is None else tick_ns
        if not t or t <= 0:
            raise ValueError("tick_ns (the call's tick length) is needed")
        return np.asarray(per_bin, dtype=np.float64) / (self.bin_ticks * float(t) * 1e-9)


class TimedStats:
    """Per-message arrival-time summary of a timed propagation (gsx_timed_stats):
    tick_hist[k, b] = nodes whose arrival tick a of message k has min(a // bin_ticks,
    n_bins - 1) == b (the source, tick 0, in bin 0); optionally node_received[u] =
    messages node u got at ticks >= 1 and node_tick_sum[u] = the sum of those ticks.
    tick_ns (the call's tick length) turns ticks into milliseconds.  Numpy on those
    integers; nothing here touches the device."""

    def __init__(self, tick_hist, bin_ticks, node_received=None, node_tick_sum=None, tick_ns=None):
        self.tick_hist = np.ascontiguousarray(tick_hist, dtype=np.uint32)
        if self.tick_hist.ndim != 2:
            raise ValueError("tick_hist is [messages, bins]")
        self.bin_ticks = int(bin_ticks)
        self.node_received = None if node_received is None else np.ascontiguousarray(node_received, dtype=np.uint32)
        self.node_tick_sum = None if node_tick_sum is None else np.ascontiguousarray(node_tick_sum, dtype=np.uint64)
        self.tick_ns = tick_ns

    @property
    def n_msgs(self) -> int:
        return self.tick_hist.shape[0]

    @property
    def n_bins(self) -> int:
        return self.tick_hist.shape[1]

    def _h(self) -> np.ndarray:
        return self.tick_hist.astype(np.int64)

    def reached(self) -> np.ndarray:
        """[m] i64: nodes that hold each message, its source not counted."""
        return self._h().sum(1) - 1

    def delivery_ratio(self, n_receivers) -> np.ndarray:
        """[m] f64: reached() / n_receivers."""
        return self.reached() / np.asarray(n_receivers, dtype=np.float64)

    def last_bin(self) -> np.ndarray:
        """[m] i64: the last bin with a node in it (-1: an empty row)."""
        nz = self.tick_hist != 0
        last = nz.shape[1] - 1 - np.argmax(nz[:, ::-1], axis=1)
        return np.where(nz.any(1), last, -1).astype(np.int64)

    def ticks_to_fraction(self, q: float, n_receivers) -> np.ndarray:
        """[m] i64: the end tick (exclusive) of the first bin after which at least a fraction q of
        n_receivers holds the message, i.e. an upper bound of the time to q at the bins' resolution
        (exact with bin_ticks = 1: the tick itself + 1); -1 if the call never got there, or only in
        the open last bin."""
        cum = np.cumsum(self._h(), axis=1) - 1  # the source is not a receipt
        ok = cum / np.asarray(n_receivers, dtype=np.float64).reshape(-1, 1) >= q
        b = np.argmax(ok, axis=1)
        good = ok.any(1) & ((b < self.n_bins - 1) | (self.n_bins == 1))
        return np.where(good, (b + 1) * self.bin_ticks, -1).astype(np.int64)

    def ms(self, ticks) -> np.ndarray:
        """ticks -> milliseconds (needs tick_ns); negative (never) stays negative."""
        t = np.asarray(ticks, dtype=np.float64)
        return np.where(t >= 0, t * (self.tick_ns / 1e6), -1.0)

    def node_mean_tick(self) -> np.ndarray:
        """[n] f64: mean arrival tick per node (nan: the node received nothing); needs per_node."""
        r = self.node_received.astype(np.float64)
        return np.where(r > 0, self.node_tick_sum.astype(np.float64) / np.maximum(r, 1), np.nan)

    def __add__(self, other: "TimedStats") -> "TimedStats":
        """Two calls over the same nodes and bins (e.g. two message batches): the rows follow one
        another, the per-node arrays (kept when both sides have them) add up."""
        if self.n_bins != other.n_bins or self.bin_ticks != other.bin_ticks:
            raise ValueError("histograms of different bins")
        both = self.node_received is not None and other.node_received is not None
        return TimedStats(np.concatenate([self.tick_hist, other.tick_hist], 0), self.bin_ticks,
                          self.node_received.astype(np.uint64) + other.node_received if both else None,
                          self.node_tick_sum + other.node_tick_sum if both else None, self.tick_ns)


class ScoreStats:
    """Threshold standings of the scores (gsx_score_stats): the selected pairs
    per score bin, bin(s) = the edges k with not s < edges[k] (a NaN score: the
    top bin, it is below no edge), as hist [B] u64 for
    the engine, obs_bins [n_local, B] u32 per observer row with obs_min
    [n_local] f64 (the row's lowest selected score that is no NaN, +inf if
    none), peer_bins
    [n_total, B] u32 per peer with peer_min [n_total] f64; B = len(edges) + 1.
    Any of them may be None.  Everything below is numpy on those tables."""

    def __init__(self, edges, hist=None, obs_bins=None, obs_min=None, peer_bins=None, peer_min=None):
        self.edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        B = len(self.edges) + 1
        self.hist = None if hist is None else np.ascontiguousarray(hist, dtype=np.uint64).reshape(B)
        self.obs_bins = None if obs_bins is None else np.ascontiguousarray(obs_bins, dtype=np.uint32).reshape(-1, B)
        self.obs_min = None if obs_min is None else np.ascontiguousarray(obs_min, dtype=np.float64).reshape(-1)
        self.peer_bins = None if peer_bins is None else np.ascontiguousarray(peer_bins, dtype=np.uint32).reshape(-1, B)
        self.peer_min = None if peer_min is None else np.ascontiguousarray(peer_min, dtype=np.float64).reshape(-1)

    def _edge(self, x) -> int:
        k = np.nonzero(self.edges == x)[0]
        if len(k) == 0:
            raise ValueError(f"{x} is not one of the edges {self.edges.tolist()}")
        return int(k[0])

    def below(self, x):
        """The selected pairs with score < x, x one of the edges -> (hist: int, obs [n_local] i64,
        peer [n_total] i64); None for a table the call did not ask for."""
        k = self._edge(x) + 1
        return (None if self.hist is None else int(self.hist[:k].sum()),
                None if self.obs_bins is None else self.obs_bins[:, :k].sum(1, dtype=np.int64),
                None if self.peer_bins is None else self.peer_bins[:, :k].sum(1, dtype=np.int64))

    def degree(self) -> np.ndarray:
        """[n_local] i64: the selected pairs of each row (select="mesh", any edges: the mesh degree)."""
        return self.obs_bins.sum(1, dtype=np.int64)

    def indegree(self) -> np.ndarray:
        """[n_total] i64: the selected pairs that point at each node."""
        return self.peer_bins.sum(1, dtype=np.int64)

    def fraction_below(self, x):
        """below(x) over the totals -> (hist: float, obs [n_local] f64, peer [n_total] f64); nan where
        nothing is selected."""
        h, o, p = self.below(x)

        def frac(a, tot):
            tot = np.asarray(tot, dtype=np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(tot > 0, np.asarray(a, dtype=np.float64) / np.maximum(tot, 1), np.nan)

        return (None if h is None else float(frac(h, int(self.hist.sum()))),
                None if o is None else frac(o, self.degree()),
                None if p is None else frac(p, self.indegree()))

    def __add__(self, other: "ScoreStats") -> "ScoreStats":
        """Range shards' local tables, in rank order: hist and the peer counters add up, peer_min
        takes the lower, the observer arrays follow one another (kept when both sides have them)."""
        if not np.array_equal(self.edges, other.edges):
            raise ValueError("tables over different edges")

        def both(a, b, f):
            return None if a is None or b is None else f(a, b)

        return ScoreStats(self.edges, both(self.hist, other.hist, np.add),
                          both(self.obs_bins, other.obs_bins, lambda a, b: np.concatenate([a, b], 0)),
                          both(self.obs_min, other.obs_min, lambda a, b: np.concatenate([a, b])),
                          both(self.peer_bins, other.peer_bins, np.add),
                          both(self.peer_min, other.peer_min, np.minimum))


class ScoreParts:
    """What the scores are made of (gsx_score_parts): the selected pairs per (score bin, cause) as
    cause_hist [B, 9] u64 and per (score bin, worst topic) as topic_hist [B, T + 1] u64 (last
    column: no topic is negative), per (observer row, cause) as obs_cause [n, 9] u32 and per
    (peer, cause) as peer_cause [n, 9] u32; B = len(edges) + 1, the bins gsx_score_stats's.  The
    cause of a pair is the lowest negative one of its parts P1 .. P7 (abi.CAUSE_NAMES; the last:
    none is negative).  With per_pair: parts [E, 10] f64 (abi.PART_NAMES), cause [E] u8 and
    worst_topic [E] u8 (abi.GSX_TOPIC_NONE: none).  Any of them may be None.  Everything below is
    numpy on those tables."""

    def __init__(self, edges, cause_hist=None, topic_hist=None, obs_cause=None, peer_cause=None, parts=None,
                 cause=None, worst_topic=None):
        self.edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        B, NC = len(self.edges) + 1, abi.GSX_CAUSES

        def arr(a, dtype, *shape):
            return None if a is None else np.ascontiguousarray(a, dtype=dtype).reshape(*shape)

        self.cause_hist = arr(cause_hist, np.uint64, B, NC)
        self.topic_hist = arr(topic_hist, np.uint64, B, -1)
        self.obs_cause = arr(obs_cause, np.uint32, -1, NC)
        self.peer_cause = arr(peer_cause, np.uint32, -1, NC)
        self.parts = arr(parts, np.float64, -1, abi.GSX_PARTS)
        self.cause = arr(cause, np.uint8, -1)
        self.worst_topic = arr(worst_topic, np.uint8, -1)

    def _bins(self, below) -> int:
        """The bins under edge `below` (None: all of them)."""
        if below is None:
            return len(self.edges) + 1
        k = np.nonzero(self.edges == below)[0]
        if len(k) == 0:
            raise ValueError(f"{below} is not one of the edges {self.edges.tolist()}")
        return int(k[0]) + 1

    @staticmethod
    def _cause(cause) -> int:
        return abi.CAUSE_NAMES.index(cause) if isinstance(cause, str) else int(cause)

    def blame(self, below=None) -> np.ndarray:
        """[9] i64: the selected pairs with score < below (one of the edges; None: all), per cause."""
        return self.cause_hist[: self._bins(below)].sum(0, dtype=np.int64)

    def blame_topics(self, below=None) -> np.ndarray:
        """[T + 1] i64: the same per worst topic; the last entry: no topic is negative."""
        return self.topic_hist[: self._bins(below)].sum(0, dtype=np.int64)

    def fraction(self, cause, below=None) -> float:
        """blame(below)[cause] over the selected pairs below the edge; nan if there is none."""
        b = self.blame(below)
        tot = int(b.sum())
        return float(b[self._cause(cause)]) / tot if tot else float("nan")

    def peers_blamed(self, cause) -> np.ndarray:
        """The nodes with at least one selected observer whose cause is this one, ascending."""
        return np.nonzero(self.peer_cause[:, self._cause(cause)])[0]


class MeshStats:
    """The shape of the mesh (gsx_mesh_stats): topic_tot [T, 16] u64 (columns abi.MS_COL_NAMES),
    deg_hist / out_hist / in_hist [T, n_bins] u64 (units by degree, outbound degree, in-degree;
    the last bin: >= n_bins - 1), age_hist [T, len(age_edges) + 1] u64 and class_links [T, C, C]
    u64 (mesh links by age bin, by (observer class, peer class)), node_deg / node_out / node_in
    [T, n] u32 and node_class_deg [T, n, C] u32.  Any of them may be None.  Everything below is
    numpy on those tables."""

    def __init__(self, n_topics, n_bins, age_edges_ns=(), n_classes=0, topic_tot=None, deg_hist=None, out_hist=None,
                 in_hist=None, age_hist=None, class_links=None, node_deg=None, node_out=None, node_in=None,
                 node_class_deg=None):
        self.n_topics, self.n_bins, self.n_classes = int(n_topics), int(n_bins), int(n_classes)
        self.age_edges_ns = np.ascontiguousarray(age_edges_ns, dtype=np.int64).reshape(-1)
        T, B, NC = self.n_topics, self.n_bins, self.n_classes

        def arr(a, dtype, *shape):
            return None if a is None else np.ascontiguousarray(a, dtype=dtype).reshape(*shape)

        self.topic_tot = arr(topic_tot, np.uint64, T, abi.GSX_MS_COLS)
        self.deg_hist = arr(deg_hist, np.uint64, T, B)
        self.out_hist = arr(out_hist, np.uint64, T, B)
        self.in_hist = arr(in_hist, np.uint64, T, B)
        self.age_hist = arr(age_hist, np.uint64, T, len(self.age_edges_ns) + 1)
        self.class_links = arr(class_links, np.uint64, T, NC, NC)
        self.node_deg = arr(node_deg, np.uint32, T, -1)
        self.node_out = arr(node_out, np.uint32, T, -1)
        self.node_in = arr(node_in, np.uint32, T, -1)
        self.node_class_deg = arr(node_class_deg, np.uint32, T, -1, NC) if NC else None

    @staticmethod
    def _col(col) -> int:
        return abi.MS_COL_NAMES.index(col) if isinstance(col, str) else int(col)

    def total(self, col, topic=None) -> int:
        """Column `col` (a name of abi.MS_COL_NAMES or GSX_MS_*) of one topic, or summed over the topics."""
        c = self.topic_tot[:, self._col(col)]
        return int(c.sum()) if topic is None else int(c[topic])

    def degree(self, t: int) -> np.ndarray:
        """[n] u32: the mesh degree of every node on topic t."""
        return self.node_deg[t]

    def outbound(self, t: int) -> np.ndarray:
        """[n] u32: the outbound mesh peers of every node on topic t."""
        return self.node_out[t]

    def indegree(self, t: int) -> np.ndarray:
        """[n] u32: the mesh links on topic t that point at each node."""
        return self.node_in[t]

    def _ratio(self, num, den, t):
        d = self.total(den, t)
        return sum(self.total(c, t) for c in num) / d if d else float("nan")

    def within_bounds(self, t: int) -> float:
        """The units of topic t with Dlo <= degree <= Dhi, over its units; nan without units."""
        d = self.total("units", t)
        return 1.0 - (self.total("below_dlo", t) + self.total("above_dhi", t)) / d if d else float("nan")

    def one_sided_ratio(self, t=None) -> float:
        """One-sided mesh links over mesh links (topic t, or all topics); nan without links."""
        return self._ratio(("one_sided",), "links", t)

    def eclipsed(self, t=None) -> int:
        return self.total("eclipsed", t)

    def below_honest(self, t=None) -> int:
        return self.total("below_honest", t)

    def class_share(self, t: int) -> np.ndarray:
        """[C, C] f64: row c = where the mesh links of class-c observers point, as shares of the row
        (nan for a class without mesh links)."""
        m = self.class_links[t].astype(np.float64)
        s = m.sum(1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(s > 0, m / np.maximum(s, 1), np.nan)


class ConnTrim:
    """A forced trim of every observer's connections (gsx_conn_trim): trim[p] = 1
    for the pairs it closes, node_trimmed[u] their number in u's row;
    trimmed(u) / kept(u) -> the pair indices of u's present and connected pairs
    the trim closes / keeps."""

    def __init__(self, row_ptr, trim, node_trimmed, conns):
        self.row_ptr, self.trim, self.node_trimmed, self.conns = row_ptr, trim, node_trimmed, conns

    def trimmed(self, u: int):
        b, e = int(self.row_ptr[u]), int(self.row_ptr[u + 1])
        return b + np.nonzero(self.trim[b:e])[0]

    def kept(self, u: int):
        b, e = int(self.row_ptr[u]), int(self.row_ptr[u + 1])
        return b + np.nonzero(self.conns[b:e] & (self.trim[b:e] == 0))[0]


class Engine:
    def __init__(self, n_topics: int, device: int = 0):
        self.lib = abi.load_library()
        cfg = abi.Config(n_topics=n_topics, device=device)
        h = C.c_void_p()
        rc = self.lib.gsx_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise GsxError(rc, "gsx_create (needs a gfx950 GPU)")
        self.h = h
        self.n_topics = n_topics
        self.n_pairs = 0

    # -- helpers ---------------------------------------------------------------
    def _chk(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.gsx_last_error(self.h)
            raise GsxError(rc, f"{what}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.gsx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- params ------------------------------------------------------------------
    def set_peer_params(self, p: abi.PeerScoreParams):
        self._chk(self.lib.gsx_set_peer_params(self.h, C.byref(p)), "gsx_set_peer_params")

    def set_thresholds(self, t: abi.Thresholds):
        self._chk(self.lib.gsx_set_thresholds(self.h, C.byref(t)), "gsx_set_thresholds")

    def set_topic_params(self, topic: int, p: abi.TopicScoreParams):
        self._chk(self.lib.gsx_set_topic_params(self.h, topic, C.byref(p)), "gsx_set_topic_params")

    # -- overlay -------------------------------------------------------------------
    def load_overlay(self, row_ptr, col, edge_flags=None, node_ips=None):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        n = len(row_ptr) - 1
        ef = None if edge_flags is None else np.ascontiguousarray(edge_flags, dtype=np.uint8)
        ips = None if node_ips is None else np.ascontiguousarray(node_ips, dtype=np.uint32).reshape(-1)
        self._chk(
            self.lib.gsx_load_overlay(
                self.h, n, _ptr(row_ptr, C.c_int64), _ptr(col, C.c_int32), _ptr(ef, C.c_uint8), _ptr(ips, C.c_uint32)
            ),
            "gsx_load_overlay",
        )
        v = C.c_uint64()
        self._chk(self.lib.gsx_num_pairs(self.h, C.byref(v)), "gsx_num_pairs")
        self.n_pairs = int(v.value)
        self.n_nodes = n
        self.node_lo = 0
        self.n_total = n
        self._row_ptr = row_ptr.copy()  # (ConnTrim's rows)

    def set_ip_whitelist(self, ips: Iterable[int]):
        a = np.ascontiguousarray(list(ips), dtype=np.uint32)
        self._chk(self.lib.gsx_set_ip_whitelist(self.h, _ptr(a, C.c_uint32), len(a)), "gsx_set_ip_whitelist")

    def set_app_scores(self, app):
        a = np.ascontiguousarray(app, dtype=np.float64)
        self._chk(self.lib.gsx_set_app_scores(self.h, _ptr(a, C.c_double), len(a)), "gsx_set_app_scores")

    # -- events ------------------------------------------------------------------
    def apply_events(self, events):
        ev = np.ascontiguousarray(events, dtype=abi.event_dtype())
        self._chk(self.lib.gsx_apply_events(self.h, ev.ctypes.data_as(C.c_void_p), len(ev)), "gsx_apply_events")

    def flush(self):
        self._chk(self.lib.gsx_flush(self.h), "gsx_flush")

    def trace_validate(self, pair, msg, topic, now):
        self._chk(self.lib.gsx_trace_validate(self.h, pair, msg, topic, now), "gsx_trace_validate")

    def trace_deliver(self, pair, msg, topic, now):
        self._chk(self.lib.gsx_trace_deliver(self.h, pair, msg, topic, now), "gsx_trace_deliver")

    def trace_reject(self, pair, msg, topic, reason, now):
        if isinstance(reason, str):
            reason = abi.REJECT_REASONS[reason]
        self._chk(self.lib.gsx_trace_reject(self.h, pair, msg, topic, reason, now), "gsx_trace_reject")

    def trace_duplicate(self, pair, msg, topic, now):
        self._chk(self.lib.gsx_trace_duplicate(self.h, pair, msg, topic, now), "gsx_trace_duplicate")

    def gc_deliveries(self, now):
        self._chk(self.lib.gsx_gc_deliveries(self.h, now), "gsx_gc_deliveries")

    def num_delivery_records(self) -> int:
        v = C.c_uint64()
        self._chk(self.lib.gsx_num_delivery_records(self.h, C.byref(v)), "gsx_num_delivery_records")
        return int(v.value)

    # -- refresh / score ---------------------------------------------------------------
    def refresh(self, now: int):
        self._chk(self.lib.gsx_refresh(self.h, now), "gsx_refresh")

    def scores(self) -> np.ndarray:
        out = np.empty(self.n_pairs, dtype=np.float64)
        self._chk(self.lib.gsx_scores(self.h, _ptr(out, C.c_double), self.n_pairs), "gsx_scores")
        return out

    def set_pair_ips(self, pairs, ips):
        """gsx_set_pair_ips: setIPs for these pairs (ips: [n, 2] u32, GSX_NO_IP for none)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1)
        ips = np.ascontiguousarray(ips, dtype=np.uint32).reshape(-1, 2)
        if len(ips) != len(pairs):
            raise ValueError("one IP pair per pair")
        self._chk(self.lib.gsx_set_pair_ips(self.h, _ptr(pairs, C.c_uint64), _ptr(ips, C.c_uint32), len(pairs)),
                  "gsx_set_pair_ips")

    def score(self, pair: int) -> float:
        v = C.c_double()
        self._chk(self.lib.gsx_score(self.h, pair, C.byref(v)), "gsx_score")
        return float(v.value)

    def score_many(self, pairs) -> np.ndarray:
        """Score(p) of many pairs with one flush / re-score / copy (gsx_score_many)."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint64)
        out = np.empty(len(pairs), dtype=np.float64)
        self._chk(self.lib.gsx_score_many(self.h, _ptr(pairs, C.c_uint64), len(pairs), _ptr(out, C.c_double)),
                  "gsx_score_many")
        return out

    def device_scores_ptr(self) -> int:
        v = C.c_void_p()
        self._chk(self.lib.gsx_device_scores(self.h, C.byref(v)), "gsx_device_scores")
        return int(v.value or 0)

    def sync(self):
        self._chk(self.lib.gsx_sync(self.h), "gsx_sync")

    def settle_scores(self):
        """gsx_settle_scores: the deferred re-scores of lazy credit folds, queued now."""
        self._chk(self.lib.gsx_settle_scores(self.h), "gsx_settle_scores")

    def last_refresh_ms(self) -> float:
        v = C.c_float()
        self._chk(self.lib.gsx_last_refresh_ms(self.h, C.byref(v)), "gsx_last_refresh_ms")
        return float(v.value)

    def propagate(self, msgs, cfg: abi.PropConfig, want_results: bool = False):
        """-> (PropOut, hop [m, n] or None, first_from [m, n] or None)"""
        ms = np.ascontiguousarray(msgs, dtype=abi.msg_dtype())
        out = abi.PropOut()
        self._chk(
            self.lib.gsx_propagate(self.h, ms.ctypes.data_as(C.c_void_p), len(ms), C.byref(cfg), C.byref(out)),
            "gsx_propagate",
        )
        self._traffic_m = len(ms)
        hop = frm = None
        if want_results:
            n = self.n_nodes
            hop = np.empty((len(ms), n), dtype=np.uint8)
            frm = np.empty((len(ms), n), dtype=np.int32) if self._track else None
            self._chk(self.lib.gsx_prop_results(self.h, _ptr(hop, C.c_uint8), _ptr(frm, C.c_int32)), "gsx_prop_results")
        return out, hop, frm

    _track = True

    # -- timed propagation (gsx.h: gsx_propagate_timed) ------------------------------------
    def set_link_latency(self, ticks):
        """gsx_set_link_latency: [n_pairs] ticks 1 .. 255 per pair (u -> v), the time a copy sent
        by v takes to reach u; None removes them."""
        if ticks is None:
            self._chk(self.lib.gsx_set_link_latency(self.h, None, 0), "gsx_set_link_latency")
            return
        t = np.ascontiguousarray(ticks)
        if t.size and (t.min() < 0 or t.max() > 255):
            raise ValueError("latencies are 1 .. 255 ticks")
        t = t.astype(np.uint8)
        self._chk(self.lib.gsx_set_link_latency(self.h, _ptr(t, C.c_uint8), len(t)), "gsx_set_link_latency")

    def propagate_timed(self, msgs, cfg: abi.PropConfig, max_ticks: int, want_results: bool = False):
        """gsx_propagate_timed (cfg.hop_latency_ns: the tick length) -> (TimedOut, tick [m, n] u16
        or None, first_from [m, n] i32 or None)"""
        ms = np.ascontiguousarray(msgs, dtype=abi.msg_dtype())
        out = abi.TimedOut()
        self._chk(self.lib.gsx_propagate_timed(self.h, ms.ctypes.data_as(C.c_void_p), len(ms), C.byref(cfg),
                                               int(max_ticks), C.byref(out)), "gsx_propagate_timed")
        self._tick_ns = int(cfg.hop_latency_ns)
        self._timed_m = len(ms)
        tick = frm = None
        if want_results:
            tick, frm = self.timed_results(len(ms))
        return out, tick, frm

    def timed_results(self, n_msgs: int):
        """-> (tick [m, n] u16, first_from [m, n] i32) of the last timed call."""
        tick = np.empty((n_msgs, self.n_nodes), dtype=np.uint16)
        frm = np.empty((n_msgs, self.n_nodes), dtype=np.int32)
        self._chk(self.lib.gsx_timed_results(self.h, _ptr(tick, C.c_uint16), _ptr(frm, C.c_int32)), "gsx_timed_results")
        return tick, frm

    def timed_stats(self, n_msgs: int, bin_ticks: int, n_bins: int, per_node: bool = False, out_ptrs=None):
        """gsx_timed_stats of the last timed call (n_msgs: its messages) -> TimedStats: tick_hist
        [m, n_bins] u32 and, with per_node, node_received [n] u32 and node_tick_sum [n] u64.

        out_ptrs = (hist, received, tick_sum): device pointers or tensors (None / 0 skips one)
        written in stream order with no host sync, as prop_stats takes them; then -> None."""
        if out_ptrs is not None:
            self._chk(self.lib.gsx_timed_stats(self.h, int(bin_ticks), int(n_bins),
                                               *[self._p(p) if p is not None else None for p in out_ptrs]),
                      "gsx_timed_stats")
            return None
        hist = np.zeros((n_msgs, n_bins), dtype=np.uint32)
        recv = np.zeros(self.n_nodes, dtype=np.uint32) if per_node else None
        tsum = np.zeros(self.n_nodes, dtype=np.uint64) if per_node else None
        self._chk(self.lib.gsx_timed_stats(self.h, int(bin_ticks), int(n_bins),
                                           C.c_void_p(hist.ctypes.data if hist.size else None),
                                           C.c_void_p(recv.ctypes.data if per_node and recv.size else None),
                                           C.c_void_p(tsum.ctypes.data if per_node and tsum.size else None)),
                  "gsx_timed_stats")
        return TimedStats(hist, bin_ticks, recv, tsum, getattr(self, "_tick_ns", None))

    _TT_OUTPUTS = ("msg", "node", "node_bytes", "pair", "pair_bytes", "bins", "bin_bytes", "node_peak", "node_peak_bin")

    def timed_traffic(self, n_msgs: int, msg_bytes=None, bin_ticks: int = 1, n_bins: int = 64, per_node: bool = True,
                      per_pair: bool = False, per_bin: bool = True, outputs=None, out_ptrs=None):
        """gsx_timed_traffic of the last timed call (n_msgs: its messages) -> TimedTraffic: msg
        [m, 7] u32; with per_node, node [n, 7] u32 and node_bytes [n, 2] u64; with per_pair, pair
        [n_pairs] u32 and pair_bytes [n_pairs] u64; with per_bin, bins [n_bins, 7] u64 and bin_bytes
        [n_bins, 2] u64; with per_node and per_bin, node_peak [n, 2] u64 and node_peak_bin [n, 2]
        u32.  msg_bytes: [m] u32 sizes (None: 1 byte each, so bytes == copies).  outputs: the
        names of the tables wanted (of TimedTraffic's attributes), instead of the per_* switches.

        out_ptrs = the nine outputs in that order, or a dict by name: device pointers or tensors
        (None / 0 skips one) written in stream order with no host sync; then -> None."""
        last = getattr(self, "_timed_m", None)
        if last is not None and int(n_msgs) != last:
            raise ValueError(f"n_msgs is {n_msgs}, the last timed call had {last} messages")
        sizes = None
        if msg_bytes is not None:
            sizes = np.ascontiguousarray(msg_bytes, dtype=np.uint32)
            if sizes.shape != (n_msgs,):
                raise ValueError("msg_bytes holds one size per message of the call")
        sp = C.c_void_p(sizes.ctypes.data if sizes is not None and sizes.size else None)
        names = self._TT_OUTPUTS
        o = abi.TimedTrafficOut()
        fields = [f for f, _ in abi.TimedTrafficOut._fields_]
        if out_ptrs is not None:
            ptrs = [out_ptrs.get(k) for k in names] if isinstance(out_ptrs, dict) else list(out_ptrs)
            if len(ptrs) != len(names):
                raise ValueError("out_ptrs holds the nine outputs")
            for f, p in zip(fields, ptrs):
                setattr(o, f, self._p(p) if p is not None else None)
            self._chk(self.lib.gsx_timed_traffic(self.h, sp, int(bin_ticks), int(n_bins), C.byref(o)), "gsx_timed_traffic")
            return None
        if outputs is None:
            want = {"msg"}
            want |= {"node", "node_bytes"} if per_node else set()
            want |= {"pair", "pair_bytes"} if per_pair else set()
            want |= {"bins", "bin_bytes"} if per_bin else set()
            want |= {"node_peak", "node_peak_bin"} if per_node and per_bin else set()
        else:
            want = set(outputs)
            if not want <= set(names):
                raise ValueError(f"outputs are of {names}")
        n, E, K, B = self.n_nodes, self.n_pairs, abi.GSX_TT_COLS, max(int(n_bins), 0)
        spec = {"msg": ((n_msgs, K), np.uint32), "node": ((n, K), np.uint32), "node_bytes": ((n, 2), np.uint64),
                "pair": ((E,), np.uint32), "pair_bytes": ((E,), np.uint64), "bins": ((B, K), np.uint64),
                "bin_bytes": ((B, 2), np.uint64), "node_peak": ((n, 2), np.uint64), "node_peak_bin": ((n, 2), np.uint32)}
        arrs = {k: np.zeros(*spec[k]) if k in want else None for k in names}
        for f, k in zip(fields, names):
            a = arrs[k]
            setattr(o, f, a.ctypes.data if a is not None and a.size else None)
        self._chk(self.lib.gsx_timed_traffic(self.h, sp, int(bin_ticks), int(n_bins), C.byref(o)), "gsx_timed_traffic")
        return TimedTraffic(*[arrs[k] for k in names], bin_ticks=bin_ticks, tick_ns=getattr(self, "_tick_ns", None))

    def prop_duplicates(self, n_msgs: int) -> np.ndarray:
        """gsx_prop_duplicates: [n_pairs, ceil(m / 64)] u64, bit m of row q = the
        pair's neighbour sent its observer a copy of message m it had already seen."""
        W = (n_msgs + 63) // 64
        rows = np.zeros((self.n_pairs, W), dtype=np.uint64)
        self._chk(self.lib.gsx_prop_duplicates(self.h, _ptr(rows, C.c_uint64), W), "gsx_prop_duplicates")
        return rows

    def set_prop_tracking(self, first_deliverers: bool):
        """gsx_prop_set_tracking: keep first-deliverer rows (results' first_from) or only counts."""
        self._chk(self.lib.gsx_prop_set_tracking(self.h, 1 if first_deliverers else 0), "gsx_prop_set_tracking")
        self._track = bool(first_deliverers)

    # -- the peer gater and AcceptFrom (gsx.h; peer_gater.go, gossipsub.go:583-594) --------
    def set_gater_params(self, p: "abi.GaterParams | None"):
        """gsx_set_gater_params: a fresh gater for the loaded overlay; None drops it."""
        self._chk(self.lib.gsx_set_gater_params(self.h, C.byref(p) if p is not None else None), "gsx_set_gater_params")

    def gater_events(self, events):
        """gsx_gater_events: rows of abi.gater_event_dtype() (kind, topic, pair, now_ns, reason),
        applied per observer in the order given."""
        ev = np.ascontiguousarray(events, dtype=abi.gater_event_dtype())
        self._chk(self.lib.gsx_gater_events(self.h, ev.ctypes.data_as(C.c_void_p), len(ev)), "gsx_gater_events")

    def gater_decay(self, now: int):
        self._chk(self.lib.gsx_gater_decay(self.h, now), "gsx_gater_decay")

    def accept_from(self, now: int, seed: int, draw: int, pairs=None, out_ptr=None):
        """gsx_accept_from -> [n] u8 of GSX_ACCEPT_* for `pairs` (None: every pair, which also
        leaves the decision bytes on the device).  out_ptr: a device pointer or tensor written
        in stream order; then -> None."""
        if pairs is None:
            pp, n = None, self.n_pairs
        else:
            pa = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1)
            pp, n = pa.ctypes.data_as(C.c_void_p), len(pa)
        if out_ptr is not None:
            self._chk(self.lib.gsx_accept_from(self.h, pp, n, now, seed, draw, self._p(out_ptr)), "gsx_accept_from")
            return None
        out = np.empty(max(n, 1), dtype=np.uint8)
        self._chk(self.lib.gsx_accept_from(self.h, pp, n, now, seed, draw, out.ctypes.data_as(C.c_void_p)),
                  "gsx_accept_from")
        return out[:n]

    def gater_num_groups(self) -> int:
        v = C.c_uint64()
        self._chk(self.lib.gsx_gater_num_groups(self.h, C.byref(v)), "gsx_gater_num_groups")
        return int(v.value)

    def gater_export(self) -> dict:
        """gsx_gater_export -> dict of arrays: validate, throttle, last_throttle_ns [n_nodes];
        connected, expire_ns, deliver, duplicate, ignore, reject [gater_num_groups()] (group
        u < n_nodes: observer u's unknown-IP group, n_nodes + g: the engine's (observer, IP)
        group g); bound_group [n_pairs] (GSX_GATER_UNBOUND: none)."""
        n, g, e = self.n_nodes, self.gater_num_groups(), self.n_pairs
        a = {
            "validate": np.zeros(n), "throttle": np.zeros(n), "last_throttle_ns": np.zeros(n, dtype=np.int64),
            "connected": np.zeros(g, dtype=np.uint32), "expire_ns": np.zeros(g, dtype=np.int64),
            "deliver": np.zeros(g), "duplicate": np.zeros(g), "ignore": np.zeros(g), "reject": np.zeros(g),
            "bound_group": np.zeros(e, dtype=np.uint32),
        }
        v = abi.GaterView(**{k: (x.ctypes.data if x.size else None) for k, x in a.items()})
        self._chk(self.lib.gsx_gater_export(self.h, C.byref(v)), "gsx_gater_export")
        return a

    def gater_fold_prop(self):
        """gsx_gater_fold_prop: the last propagation's receipts as the gater's tracer calls."""
        self._chk(self.lib.gsx_gater_fold_prop(self.h), "gsx_gater_fold_prop")

    def gater_enforce(self, on: bool):
        """gsx_gater_enforce: gossipsub propagation drops the payload of pairs the last full
        accept_from answered GSX_ACCEPT_CONTROL."""
        self._chk(self.lib.gsx_gater_enforce(self.h, 1 if on else 0), "gsx_gater_enforce")

    def gater_gate_pairs(self):
        """gsx_gater_gate_pairs -> (pairs with ACCEPT_NONE, pairs with ACCEPT_CONTROL) of the decision set."""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.gsx_gater_gate_pairs(self.h, C.byref(a), C.byref(b)), "gsx_gater_gate_pairs")
        return int(a.value), int(b.value)

    # -- the tag tracer and connection trims (gsx.h; tag_tracer.go) ------------------------
    def default_tag_params(self) -> "abi.TagParams":
        p = abi.TagParams()
        self._chk(self.lib.gsx_default_tag_params(C.byref(p)), "gsx_default_tag_params")
        return p

    def set_tag_params(self, p: "abi.TagParams | None"):
        """gsx_set_tag_params: a fresh tag tracer for the loaded overlay; None drops it."""
        self._chk(self.lib.gsx_set_tag_params(self.h, C.byref(p) if p is not None else None), "gsx_set_tag_params")

    def tag_trace_validate(self, pair, msg, topic, now):
        self._chk(self.lib.gsx_tag_trace_validate(self.h, pair, msg, topic, now), "gsx_tag_trace_validate")

    def tag_trace_duplicate(self, pair, msg, topic, now):
        self._chk(self.lib.gsx_tag_trace_duplicate(self.h, pair, msg, topic, now), "gsx_tag_trace_duplicate")

    def tag_trace_deliver(self, pair, msg, topic, now):
        self._chk(self.lib.gsx_tag_trace_deliver(self.h, pair, msg, topic, now), "gsx_tag_trace_deliver")

    def tag_trace_reject(self, pair, msg, topic, reason, now):
        if isinstance(reason, str):
            reason = abi.REJECT_REASONS[reason]
        self._chk(self.lib.gsx_tag_trace_reject(self.h, pair, msg, topic, reason, now), "gsx_tag_trace_reject")

    def tag_num_pending(self) -> int:
        v = C.c_uint64()
        self._chk(self.lib.gsx_tag_num_pending(self.h, C.byref(v)), "gsx_tag_num_pending")
        return int(v.value)

    def tag_events(self, events):
        """gsx_tag_events: rows of abi.tag_event_dtype() (pair, topic, count), or (pair, topic, count) tuples."""
        ev = np.ascontiguousarray(events, dtype=abi.tag_event_dtype())
        self._chk(self.lib.gsx_tag_events(self.h, ev.ctypes.data_as(C.c_void_p), len(ev)), "gsx_tag_events")

    def tag_decay(self, steps: int = 1):
        self._chk(self.lib.gsx_tag_decay(self.h, steps), "gsx_tag_decay")

    def tag_fold_prop(self):
        """gsx_tag_fold_prop: the last propagation's deliveries as the tag tracer's calls."""
        self._chk(self.lib.gsx_tag_fold_prop(self.h), "gsx_tag_fold_prop")

    def tag_export(self):
        """gsx_tag_export -> [n_topics, n_pairs] u8"""
        out = np.zeros(max(self.n_topics * self.n_pairs, 1), dtype=np.uint8)
        self._chk(self.lib.gsx_tag_export(self.h, out.ctypes.data_as(C.c_void_p)), "gsx_tag_export")
        return out[: self.n_topics * self.n_pairs].reshape(self.n_topics, self.n_pairs)

    def conn_values(self, value_ptr=None, protect_ptr=None):
        """gsx_conn_values -> (value [n_pairs] u32, protect [n_pairs] u8 of GSX_CONN_* bits).
        With a device pointer or tensor for either, both go there in stream order; then -> None."""
        if value_ptr is not None or protect_ptr is not None:
            self._chk(self.lib.gsx_conn_values(self.h, self._p(value_ptr), self._p(protect_ptr)), "gsx_conn_values")
            return None
        v = np.zeros(max(self.n_pairs, 1), dtype=np.uint32)
        p = np.zeros(max(self.n_pairs, 1), dtype=np.uint8)
        self._chk(self.lib.gsx_conn_values(self.h, v.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)),
                  "gsx_conn_values")
        return v[: self.n_pairs], p[: self.n_pairs]

    def conn_trim(self, low_water: int, trim_ptr=None, node_trimmed_ptr=None):
        """gsx_conn_trim -> ConnTrim.  With a device pointer or tensor for the trim bytes (and
        optionally the per-node counts) they are written in stream order; then -> None."""
        if trim_ptr is not None:
            self._chk(self.lib.gsx_conn_trim(self.h, low_water, self._p(trim_ptr), self._p(node_trimmed_ptr)),
                      "gsx_conn_trim")
            return None
        t = np.zeros(max(self.n_pairs, 1), dtype=np.uint8)
        nt = np.zeros(max(self.n_nodes, 1), dtype=np.uint32)
        self._chk(self.lib.gsx_conn_trim(self.h, low_water, t.ctypes.data_as(C.c_void_p),
                                         nt.ctypes.data_as(C.c_void_p)), "gsx_conn_trim")
        pf = np.zeros(max(self.n_pairs, 1), dtype=np.uint8)
        sv = abi.StateView()
        sv.pair_flags = pf.ctypes.data_as(C.POINTER(C.c_uint8))
        self._chk(self.lib.gsx_export_state(self.h, C.byref(sv)), "gsx_export_state")
        both = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
        return ConnTrim(self._row_ptr, t[: self.n_pairs], nt[: self.n_nodes], (pf[: self.n_pairs] & both) == both)

    # -- stepped / sharded propagation (gsx.h "range sharding") --------------------------
    def load_overlay_shard(self, n_total, node_lo, row_ptr, col, edge_flags=None, node_ips=None):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        n = len(row_ptr) - 1
        ef = None if edge_flags is None else np.ascontiguousarray(edge_flags, dtype=np.uint8)
        ips = None if node_ips is None else np.ascontiguousarray(node_ips, dtype=np.uint32).reshape(-1)
        self._chk(
            self.lib.gsx_load_overlay_shard(self.h, n_total, node_lo, n, _ptr(row_ptr, C.c_int64),
                                            _ptr(col, C.c_int32), _ptr(ef, C.c_uint8), _ptr(ips, C.c_uint32)),
            "gsx_load_overlay_shard",
        )
        v = C.c_uint64()
        self._chk(self.lib.gsx_num_pairs(self.h, C.byref(v)), "gsx_num_pairs")
        self.n_pairs = int(v.value)
        self.n_nodes = n
        self._row_ptr = row_ptr.copy()
        self.node_lo = node_lo
        self.n_total = n_total

    def shard_recv_plan(self, rank_lo):
        """-> (recv_counts [world] u64, recv_u, recv_v): this rank's receive list."""
        rl = np.ascontiguousarray(rank_lo, dtype=np.uint32)
        self._rank_lo = rl
        w = len(rl) - 1
        cnt = np.zeros(w, dtype=np.uint64)
        self._chk(self.lib.gsx_shard_recv_plan(self.h, w, _ptr(rl, C.c_uint32), _ptr(cnt, C.c_uint64), None, None),
                  "gsx_shard_recv_plan")
        n = int(cnt.sum())
        ru = np.empty(n, dtype=np.uint32)
        rv = np.empty(n, dtype=np.uint32)
        self._chk(self.lib.gsx_shard_recv_plan(self.h, w, _ptr(rl, C.c_uint32), _ptr(cnt, C.c_uint64),
                                               _ptr(ru, C.c_uint32), _ptr(rv, C.c_uint32)), "gsx_shard_recv_plan")
        return cnt, ru, rv

    def shard_send_plan(self, send_counts, req_u, req_v):
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        u = np.ascontiguousarray(req_u, dtype=np.uint32)
        v = np.ascontiguousarray(req_v, dtype=np.uint32)
        self._chk(self.lib.gsx_shard_send_plan(self.h, _ptr(sc, C.c_uint64), _ptr(u, C.c_uint32),
                                               _ptr(v, C.c_uint32)), "gsx_shard_send_plan")

    def shard_set_halo_bases(self, dest_halo_base):
        b = np.ascontiguousarray(dest_halo_base, dtype=np.uint64)
        self._chk(self.lib.gsx_shard_set_halo_bases(self.h, _ptr(b, C.c_uint64)), "gsx_shard_set_halo_bases")

    def prop_pack_compact(self, out) -> np.ndarray:
        """out: device buffer [n_send][words + 1] u64; -> entries per destination rank."""
        p = out.data_ptr() if hasattr(out, "data_ptr") else out
        w = len(self._rank_lo) - 1
        cnt = np.zeros(w, dtype=np.uint64)
        self._chk(self.lib.gsx_prop_pack_compact(self.h, C.c_void_p(p or None), _ptr(cnt, C.c_uint64)),
                  "gsx_prop_pack_compact")
        return cnt

    def prop_pack_compact_dev(self, out, counts):
        """As prop_pack_compact, the counts left on the device: counts (device
        tensor [n_ranks, 2] i64) = (entries for rank k, this rank's first
        receipts of the hop just run); no host sync."""
        p = out.data_ptr() if hasattr(out, "data_ptr") else out
        self._chk(self.lib.gsx_prop_pack_compact_dev(self.h, C.c_void_p(p or None), C.c_void_p(counts.data_ptr())),
                  "gsx_prop_pack_compact_dev")

    def prop_step_compact(self, entries, n: int, sync: bool = True):
        """-> this hop's first receipts on this rank; sync=False: no host sync, -> None."""
        p = entries.data_ptr() if hasattr(entries, "data_ptr") else entries
        v = C.c_uint64()
        self._chk(self.lib.gsx_prop_step_compact(self.h, C.c_void_p(p or None), n, C.byref(v) if sync else None),
                  "gsx_prop_step_compact")
        return int(v.value) if sync else None

    def shard_counts(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self.lib.gsx_shard_counts(self.h, C.byref(a), C.byref(b)), "gsx_shard_counts")
        return int(a.value), int(b.value)

    def set_stream(self, stream_handle: int):
        """Order the engine's work on a HIP stream (e.g. torch.cuda.current_stream().cuda_stream); 0 = own."""
        self._chk(self.lib.gsx_set_stream(self.h, C.c_void_p(stream_handle or None)), "gsx_set_stream")

    def prop_begin(self, msgs, cfg: abi.PropConfig):
        ms = np.ascontiguousarray(msgs, dtype=abi.msg_dtype())
        self._chk(self.lib.gsx_prop_begin(self.h, ms.ctypes.data_as(C.c_void_p), len(ms), C.byref(cfg)),
                  "gsx_prop_begin")
        self._prop_msgs = len(ms)
        self._traffic_m = len(ms)

    def prop_pack(self, send):
        """send: device buffer (torch tensor or pointer) of [n_send][words] u64 rows."""
        p = send.data_ptr() if hasattr(send, "data_ptr") else send
        self._chk(self.lib.gsx_prop_pack(self.h, C.c_void_p(p or None)), "gsx_prop_pack")

    def prop_step(self, recv, sync: bool = True):
        """recv: device buffer (torch tensor or pointer) of the received rows; -> this hop's first
        receipts (sync=False: no host sync, -> None)."""
        p = recv.data_ptr() if hasattr(recv, "data_ptr") else recv
        n = C.c_uint64()
        self._chk(self.lib.gsx_prop_step(self.h, C.c_void_p(p or None), C.byref(n) if sync else None),
                  "gsx_prop_step")
        return int(n.value) if sync else None

    def prop_hop_counts_dev(self, out):
        """out: device int64 buffer of GSX_MAX_HOPS + 1: the call's first receipts per hop (no host sync)."""
        p = out.data_ptr() if hasattr(out, "data_ptr") else out
        self._chk(self.lib.gsx_prop_hop_counts_dev(self.h, C.c_void_p(p)), "gsx_prop_hop_counts_dev")

    # -- range shards, replicated frontier (gsx.h gsx_prop_rep_*) --
    def prop_rep(self) -> bool:
        v = C.c_uint32()
        self._chk(self.lib.gsx_prop_rep(self.h, C.byref(v)), "gsx_prop_rep")
        return bool(v.value)

    def prop_rep_fwd_pack(self, out):
        self._chk(self.lib.gsx_prop_rep_fwd_pack(self.h, self._p(out)), "gsx_prop_rep_fwd_pack")

    def prop_rep_fwd_recv(self, inp):
        self._chk(self.lib.gsx_prop_rep_fwd_recv(self.h, self._p(inp)), "gsx_prop_rep_fwd_recv")

    def prop_rep_pack_dev(self, out, d_counts):
        """This rank's frontier rows of the hop just run as entries into out; (entries, receipts) into d_counts."""
        self._chk(self.lib.gsx_prop_rep_pack_dev(self.h, self._p(out), self._p(d_counts)), "gsx_prop_rep_pack_dev")

    def prop_rep_step(self, parts=(), counts=()):
        """The other ranks' entries (device tensors, counts[k] rows each), then the next hop."""
        n = len(parts)
        pp = (C.c_void_p * max(n, 1))(*[self._p(t).value for t in parts])
        cc = (C.c_uint64 * max(n, 1))(*[int(c) for c in counts])
        self._chk(self.lib.gsx_prop_rep_step(self.h, n, pp, cc), "gsx_prop_rep_step")

    def prop_rep_rows(self, on: bool = True):
        """This call's replicated frontier moves as dense row slices (gsx_prop_rep_rows)."""
        self._chk(self.lib.gsx_prop_rep_rows(self.h, 1 if on else 0), "gsx_prop_rep_rows")

    def prop_rep_rows_export(self, rows, occ):
        """This rank's rows of the hop just run (n_local x W) and its occupancy-bit row (device)."""
        self._chk(self.lib.gsx_prop_rep_rows_export(self.h, self._p(rows), self._p(occ)), "gsx_prop_rep_rows_export")

    def prop_rep_rows_step(self, parts, occ_sum):
        """Every rank's rows of the hop (parts[k], the shard plan's ranges) and the summed bit row, then the next hop."""
        n = len(parts)
        pp = (C.c_void_p * max(n, 1))(*[self._p(t).value for t in parts])
        self._chk(self.lib.gsx_prop_rep_rows_step(self.h, n, pp, self._p(occ_sum)), "gsx_prop_rep_rows_step")

    def prop_rep_sends_pack(self, out):
        self._chk(self.lib.gsx_prop_rep_sends_pack(self.h, self._p(out)), "gsx_prop_rep_sends_pack")

    def prop_rep_sends_recv(self, inp):
        self._chk(self.lib.gsx_prop_rep_sends_recv(self.h, self._p(inp)), "gsx_prop_rep_sends_recv")

    def prop_set_last_hop(self, last_hop: int):
        """gsx_prop_set_last_hop: the last hop that delivered on any rank (range shards)."""
        self._chk(self.lib.gsx_prop_set_last_hop(self.h, int(last_hop)), "gsx_prop_set_last_hop")

    def prop_end(self) -> abi.PropOut:
        out = abi.PropOut()
        self._chk(self.lib.gsx_prop_end(self.h, C.byref(out)), "gsx_prop_end")
        return out

    def prop_results(self, n_msgs: int):
        """-> (hop [m, n_local] u8, first_from [m, n_local] i32) of the last propagation."""
        hop = np.empty((n_msgs, self.n_nodes), dtype=np.uint8)
        frm = np.empty((n_msgs, self.n_nodes), dtype=np.int32) if self._track else None
        self._chk(self.lib.gsx_prop_results(self.h, _ptr(hop, C.c_uint8), _ptr(frm, C.c_int32)), "gsx_prop_results")
        return hop, frm

    def prop_stats(self, n_msgs: int, per_node: bool = False, out_ptrs=None):
        """gsx_prop_stats of the last propagation (n_msgs: its messages) -> PropStats:
        hop_hist [m, GSX_MAX_HOPS + 1] u32 and, with per_node, node_received
        [n_local] u32 and node_hop_sum [n_local] u64.

        out_ptrs = (hist, received, hop_sum): device pointers or tensors (None /
        0 skips one) written in stream order with no host sync, as
        pending_credits takes them; then -> None."""
        if out_ptrs is not None:
            self._chk(self.lib.gsx_prop_stats(self.h, *[self._p(p) if p is not None else None for p in out_ptrs]),
                      "gsx_prop_stats")
            return None
        hist = np.zeros((n_msgs, abi.GSX_MAX_HOPS + 1), dtype=np.uint32)
        recv = np.zeros(self.n_nodes, dtype=np.uint32) if per_node else None
        hsum = np.zeros(self.n_nodes, dtype=np.uint64) if per_node else None
        self._chk(self.lib.gsx_prop_stats(self.h, C.c_void_p(hist.ctypes.data if hist.size else None),
                                          C.c_void_p(recv.ctypes.data if per_node and recv.size else None),
                                          C.c_void_p(hsum.ctypes.data if per_node and hsum.size else None)),
                  "gsx_prop_stats")
        return PropStats(hist, recv, hsum)

    def prop_traffic(self, n_msgs: int, msg_bytes=None, per_node: bool = True, per_pair: bool = False, out_ptrs=None):
        """gsx_prop_traffic of the last propagation (n_msgs: its messages) -> PropTraffic: msg
        [m, 5] u32 and, with per_node, node [n, 5] u32 and node_bytes [n, 2] u64, with per_pair,
        pair [n_pairs] u32 and pair_bytes [n_pairs] u64.  msg_bytes: [m] u32 sizes (None: 1 byte
        each, so bytes == copies).  n_msgs must be the last call's message count, as for
        prop_stats: the library reads and writes that many entries; after a propagate() or
        prop_begin() through this handle a different n_msgs raises ValueError.

        out_ptrs = (msg, node, node_bytes, pair, pair_bytes): device pointers or tensors (None /
        0 skips one) written in stream order with no host sync, as prop_stats takes them; then
        -> None."""
        last = getattr(self, "_traffic_m", None)
        if last is not None and int(n_msgs) != last:
            raise ValueError(f"n_msgs is {n_msgs}, the last propagation had {last} messages")
        sizes = None
        if msg_bytes is not None:
            sizes = np.ascontiguousarray(msg_bytes, dtype=np.uint32)
            if sizes.shape != (n_msgs,):
                raise ValueError("msg_bytes holds one size per message of the call")
        sp = C.c_void_p(sizes.ctypes.data if sizes is not None and sizes.size else None)
        if sizes is not None and not sizes.size:
            sizes = None
        if out_ptrs is not None:
            self._chk(self.lib.gsx_prop_traffic(self.h, sp, *[self._p(p) if p is not None else None for p in out_ptrs]),
                      "gsx_prop_traffic")
            return None
        n, E, K = self.n_nodes, self.n_pairs, abi.GSX_TRAFFIC_COLS
        msg = np.zeros((n_msgs, K), dtype=np.uint32)
        node = np.zeros((n, K), dtype=np.uint32) if per_node else None
        nbytes = np.zeros((n, 2), dtype=np.uint64) if per_node else None
        pair = np.zeros(E, dtype=np.uint32) if per_pair else None
        pbytes = np.zeros(E, dtype=np.uint64) if per_pair else None
        self._chk(self.lib.gsx_prop_traffic(self.h, sp, *[C.c_void_p(a.ctypes.data if a is not None and a.size else None)
                                                          for a in (msg, node, nbytes, pair, pbytes)]),
                  "gsx_prop_traffic")
        return PropTraffic(msg, node, nbytes, pair, pbytes)

    def score_stats_edges(self) -> np.ndarray:
        """gsx_score_stats_edges: the sorted, de-duplicated thresholds of the last set_thresholds and 0.0."""
        sp = abi.ScoreStatsSpec()
        self._chk(self.lib.gsx_score_stats_edges(self.h, C.byref(sp)), "gsx_score_stats_edges")
        return np.array(sp.edges[: sp.n_edges], dtype=np.float64)

    def score_stats(self, edges=None, select="present", topic: int = 0, per_node: bool = True, peers: bool = True,
                    out_ptrs=None):
        """gsx_score_stats -> ScoreStats: the selected pairs (select: "present", "connected" or
        "mesh" on `topic`) per score bin over `edges` (None: score_stats_edges()), for the engine,
        with per_node per observer row (and the row's lowest score), with peers per peer.

        out_ptrs = (hist, obs_bins, obs_min, peer_bins, peer_min): device pointers or tensors
        (None / 0 skips one) written in stream order with no host sync, as prop_stats takes
        them; then -> None."""
        sp = abi.ScoreStatsSpec(select=abi.SS_SELECT[select] if isinstance(select, str) else int(select),
                                topic=int(topic))
        if edges is None:
            self._chk(self.lib.gsx_score_stats_edges(self.h, C.byref(sp)), "gsx_score_stats_edges")
        else:
            ed = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
            sp.n_edges = len(ed)
            for k, x in enumerate(ed[: abi.GSX_SS_MAX_EDGES]):
                sp.edges[k] = x
        if out_ptrs is not None:
            out = abi.ScoreStatsOut(*[self._p(p).value if p is not None else None for p in out_ptrs])
            self._chk(self.lib.gsx_score_stats(self.h, C.byref(sp), C.byref(out)), "gsx_score_stats")
            return None
        B = min(sp.n_edges, abi.GSX_SS_MAX_EDGES) + 1
        nl, nt = self.n_nodes, getattr(self, "n_total", self.n_nodes)
        hist = np.zeros(B, dtype=np.uint64)
        ob = np.zeros((nl, B), dtype=np.uint32) if per_node else None
        om = np.full(nl, np.inf) if per_node else None
        pb = np.zeros((nt, B), dtype=np.uint32) if peers else None
        pm = np.full(nt, np.inf) if peers else None
        out = abi.ScoreStatsOut(*[a.ctypes.data if a is not None and a.size else None for a in (hist, ob, om, pb, pm)])
        self._chk(self.lib.gsx_score_stats(self.h, C.byref(sp), C.byref(out)), "gsx_score_stats")
        return ScoreStats(np.array(sp.edges[: B - 1], dtype=np.float64), hist, ob, om, pb, pm)

    def score_parts(self, edges=None, select="present", topic: int = 0, per_pair: bool = False, per_node: bool = True,
                    out_ptrs=None):
        """gsx_score_parts -> ScoreParts: which of P1 .. P7 is the lowest negative part of each
        selected pair's score (its cause) and on which topic its weighted topic score is lowest,
        counted per score bin over `edges` (None: score_stats_edges()), with per_node per observer
        row and per peer, with per_pair also the parts, cause and worst topic of every pair.

        out_ptrs = (pair_parts, pair_cause, pair_topic, cause_hist, topic_hist, obs_cause,
        peer_cause): device pointers or tensors (None / 0 skips one) written in stream order with
        no host sync, as score_stats takes them; then -> None."""
        sp = abi.ScoreStatsSpec(select=abi.SS_SELECT[select] if isinstance(select, str) else int(select),
                                topic=int(topic))
        if edges is None:
            self._chk(self.lib.gsx_score_stats_edges(self.h, C.byref(sp)), "gsx_score_stats_edges")
        else:
            ed = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
            sp.n_edges = len(ed)
            for k, x in enumerate(ed[: abi.GSX_SS_MAX_EDGES]):
                sp.edges[k] = x
        if out_ptrs is not None:
            out = abi.ScorePartsOut(*[self._p(p).value if p is not None else None for p in out_ptrs])
            self._chk(self.lib.gsx_score_parts(self.h, C.byref(sp), C.byref(out)), "gsx_score_parts")
            return None
        B = min(sp.n_edges, abi.GSX_SS_MAX_EDGES) + 1
        n, E, NC = self.n_nodes, self.n_pairs, abi.GSX_CAUSES
        parts = np.zeros((E, abi.GSX_PARTS), dtype=np.float64) if per_pair else None
        cause = np.full(E, abi.GSX_CAUSE_NONE, dtype=np.uint8) if per_pair else None
        worst = np.full(E, abi.GSX_TOPIC_NONE, dtype=np.uint8) if per_pair else None
        ch = np.zeros((B, NC), dtype=np.uint64)
        th = np.zeros((B, self.n_topics + 1), dtype=np.uint64)
        oc = np.zeros((n, NC), dtype=np.uint32) if per_node else None
        pe = np.zeros((n, NC), dtype=np.uint32) if per_node else None
        out = abi.ScorePartsOut(*[a.ctypes.data if a is not None and a.size else None
                                  for a in (parts, cause, worst, ch, th, oc, pe)])
        self._chk(self.lib.gsx_score_parts(self.h, C.byref(sp), C.byref(out)), "gsx_score_parts")
        return ScoreParts(np.array(sp.edges[: B - 1], dtype=np.float64), ch, th, oc, pe, parts, cause, worst)

    def mesh_stats(self, now_ns: int, n_bins: int = 33, age_edges_ns=(), node_class=None, n_classes: int = 0,
                   hostile_mask: int = 0, min_honest: int = 0, per_node: bool = True, symmetry: bool = True,
                   out_ptrs=None):
        """gsx_mesh_stats -> MeshStats: per topic the mesh links and what they are, the backoff
        entries and the fanout, the units per degree bin and per heartbeat verdict; with per_node
        the degree, outbound degree and in-degree of every (topic, node); with node_class ([n] u8,
        an array or a device tensor, values < n_classes, hostile_mask bit c: class c is hostile) the
        links per class pair, the class degrees and the eclipsed / below-min_honest units.

        out_ptrs = abi.MS_OUT_FIELDS in order: device pointers or tensors (None / 0 skips one)
        written in stream order with no host sync, as score_stats takes them; then -> None."""
        ed = np.ascontiguousarray(age_edges_ns, dtype=np.int64).reshape(-1)
        sp = abi.MeshStatsSpec(now_ns=int(now_ns), n_bins=int(n_bins), n_age_edges=len(ed), n_classes=int(n_classes),
                               hostile_mask=int(hostile_mask), min_honest=int(min_honest), symmetry=int(bool(symmetry)))
        for k, x in enumerate(ed[: abi.GSX_MS_MAX_AGE_EDGES]):
            sp.age_edges_ns[k] = int(x)
        keep = None
        if node_class is not None:
            if hasattr(node_class, "data_ptr"):
                sp.node_class = node_class.data_ptr()
            else:
                keep = np.ascontiguousarray(node_class, dtype=np.uint8).reshape(-1)
                if len(keep) != self.n_nodes:
                    raise ValueError("node_class: one class per node")
                sp.node_class = keep.ctypes.data if len(keep) else None
        if out_ptrs is not None:
            out = abi.MeshStatsOut(*[self._p(p).value if p is not None else None for p in out_ptrs])
            self._chk(self.lib.gsx_mesh_stats(self.h, C.byref(sp), C.byref(out)), "gsx_mesh_stats")
            return None
        T, n = self.n_topics, self.n_nodes
        B = min(max(int(n_bins), 1), abi.GSX_MS_MAX_BINS)
        A = min(len(ed), abi.GSX_MS_MAX_AGE_EDGES) + 1
        NC = min(int(n_classes), abi.GSX_MS_MAX_CLASSES) if node_class is not None else 0
        tabs = {"topic_tot": np.zeros((T, abi.GSX_MS_COLS), dtype=np.uint64),
                "deg_hist": np.zeros((T, B), dtype=np.uint64), "out_hist": np.zeros((T, B), dtype=np.uint64),
                "in_hist": np.zeros((T, B), dtype=np.uint64), "age_hist": np.zeros((T, A), dtype=np.uint64),
                "class_links": np.zeros((T, NC, NC), dtype=np.uint64) if NC else None,
                "node_deg": np.zeros((T, n), dtype=np.uint32) if per_node else None,
                "node_out": np.zeros((T, n), dtype=np.uint32) if per_node else None,
                "node_in": np.zeros((T, n), dtype=np.uint32) if per_node else None,
                "node_class_deg": np.zeros((T, n, NC), dtype=np.uint32) if per_node and NC else None}
        out = abi.MeshStatsOut(*[tabs[f].ctypes.data if tabs[f] is not None and tabs[f].size else None
                                 for f in abi.MS_OUT_FIELDS])
        self._chk(self.lib.gsx_mesh_stats(self.h, C.byref(sp), C.byref(out)), "gsx_mesh_stats")
        del keep
        return MeshStats(T, B, ed[: A - 1], NC, **tabs)

    def pending_credits(self, first_ptr: int, dup_ptr: int):
        """Copy the pending (GSX_CREDIT_DEFER) counts to caller memory (host or device pointers)."""
        self._chk(self.lib.gsx_prop_pending_credits(self.h, C.c_void_p(first_ptr or None), C.c_void_p(dup_ptr or None)),
                  "gsx_prop_pending_credits")

    def pending_invalid(self, inv_ptr: int):
        """Copy the pending invalid-delivery counts (P4 of REJECT messages) to caller memory."""
        self._chk(self.lib.gsx_prop_pending_invalid(self.h, C.c_void_p(inv_ptr or None)), "gsx_prop_pending_invalid")

    def replace_pending_invalid(self, inv_ptr: int):
        self._chk(self.lib.gsx_prop_replace_pending_invalid(self.h, C.c_void_p(inv_ptr or None)),
                  "gsx_prop_replace_pending_invalid")

    def fold_credits(self, first_ptr: int = 0, dup_ptr: int = 0):
        self._chk(self.lib.gsx_prop_fold_credits(self.h, C.c_void_p(first_ptr or None), C.c_void_p(dup_ptr or None)),
                  "gsx_prop_fold_credits")

    # -- heartbeat (gossipsub.go:1303-1604) ----------------------------------------------
    def set_gossipsub_params(self, gp: abi.GossipSubParams):
        self._chk(self.lib.gsx_set_gossipsub_params(self.h, C.byref(gp)), "gsx_set_gossipsub_params")
        self._do_px = bool(gp.do_px)
        self._gx_on = bool(gp.gossip_exchange)

    _do_px = False

    def hb_px_enabled(self) -> bool:
        return self._do_px

    # peer exchange on range shards (gsx.h gsx_hb_px_*)
    def hb_px_entry_words(self) -> int:
        w = C.c_uint32()
        self._chk(self.lib.gsx_hb_px_entry_words(self.h, C.byref(w)), "gsx_hb_px_entry_words")
        return int(w.value)

    def hb_px_count(self, kind: int, n_ranks: int) -> np.ndarray:
        c = np.zeros(n_ranks, dtype=np.uint64)
        self._chk(self.lib.gsx_hb_px_count(self.h, kind, _ptr(c, C.c_uint64)), "gsx_hb_px_count")
        return c

    def hb_px_pack(self, kind: int, out):
        self._chk(self.lib.gsx_hb_px_pack(self.h, kind, self._p(out)), "gsx_hb_px_pack")

    def hb_px_recv(self, kind: int, entries, n: int):
        self._chk(self.lib.gsx_hb_px_recv(self.h, kind, self._p(entries), n), "gsx_hb_px_recv")

    def hb_reserve(self):
        """The heartbeat's device buffers allocated now (gsx_hb_reserve), not in the first round."""
        self._chk(self.lib.gsx_hb_reserve(self.h), "gsx_hb_reserve")

    def heartbeat(self, tick: int, now: int, seed: int) -> abi.HeartbeatOut:
        out = abi.HeartbeatOut()
        self._chk(self.lib.gsx_heartbeat(self.h, tick, now, seed, C.byref(out)), "gsx_heartbeat")
        return out

    @staticmethod
    def _p(t):
        return C.c_void_p((t.data_ptr() if hasattr(t, "data_ptr") else t) or None)

    def hb_begin(self, tick: int, now: int, seed: int):
        self._chk(self.lib.gsx_hb_begin(self.h, tick, now, seed), "gsx_hb_begin")

    def hb_pack_ctl(self, send):
        self._chk(self.lib.gsx_hb_pack_ctl(self.h, self._p(send)), "gsx_hb_pack_ctl")

    def hb_recv(self, halo_ctl):
        self._chk(self.lib.gsx_hb_recv(self.h, self._p(halo_ctl)), "gsx_hb_recv")

    def hb_pack_resp(self, send):
        self._chk(self.lib.gsx_hb_pack_resp(self.h, self._p(send)), "gsx_hb_pack_resp")

    def hb_end(self, halo_resp) -> abi.HeartbeatOut:
        out = abi.HeartbeatOut()
        self._chk(self.lib.gsx_hb_end(self.h, self._p(halo_resp), C.byref(out)), "gsx_hb_end")
        return out

    # ---- the gossip exchange across range shards (gsx_gx_*, gsx_gxf_*) ----
    def gx_pending(self):
        """-> the message sets of the sharded exchange in flight, or None."""
        n = C.c_uint32()
        rc = self.lib.gsx_gx_pending(self.h, C.byref(n))
        return int(n.value) if rc == 1 else None

    def gx_common(self, n_sets: int) -> np.ndarray:
        c = np.empty(64 * n_sets, dtype=np.uint64)
        self._chk(self.lib.gsx_gx_common(self.h, _ptr(c, C.c_uint64)), "gsx_gx_common")
        return c

    def gx_set_common(self, c: np.ndarray):
        c = np.ascontiguousarray(c, dtype=np.uint64)
        self._chk(self.lib.gsx_gx_set_common(self.h, _ptr(c, C.c_uint64)), "gsx_gx_set_common")

    def gx_pack_ihave(self, send):
        self._chk(self.lib.gsx_gx_pack_ihave(self.h, self._p(send)), "gsx_gx_pack_ihave")

    def gx_recv_ihave(self, recv):
        self._chk(self.lib.gsx_gx_recv_ihave(self.h, self._p(recv)), "gsx_gx_recv_ihave")

    def gx_rows_words(self) -> int:
        w = C.c_uint32()
        self._chk(self.lib.gsx_gx_rows_words(self.h, C.byref(w)), "gsx_gx_rows_words")
        return int(w.value)

    def gx_rows_pack(self, n_ranks: int, out=None) -> np.ndarray:
        """out None: the count pass -> entries per destination; else the pack."""
        cnt = np.zeros(n_ranks, dtype=np.uint64)
        self._chk(self.lib.gsx_gx_rows_pack(self.h, _ptr(cnt, C.c_uint64), self._p(out) if out is not None else None),
                  "gsx_gx_rows_pack")
        return cnt

    def gx_rows_recv(self, entries, n: int):
        self._chk(self.lib.gsx_gx_rows_recv(self.h, self._p(entries), n), "gsx_gx_rows_recv")

    def gx_exchange(self) -> int:
        n = C.c_uint32()
        self._chk(self.lib.gsx_gx_exchange(self.h, C.byref(n)), "gsx_gx_exchange")
        return int(n.value)

    def gxf_begin(self, run: int):
        self._chk(self.lib.gsx_gxf_begin(self.h, run), "gsx_gxf_begin")

    def gxf_entry_words(self) -> int:
        w = C.c_uint32()
        self._chk(self.lib.gsx_gxf_entry_words(self.h, C.byref(w)), "gsx_gxf_entry_words")
        return int(w.value)

    def gxf_pack_fout(self, send):
        self._chk(self.lib.gsx_gxf_pack_fout(self.h, self._p(send)), "gsx_gxf_pack_fout")

    def gxf_recv_fout(self, recv):
        self._chk(self.lib.gsx_gxf_recv_fout(self.h, self._p(recv)), "gsx_gxf_recv_fout")

    def gxf_pack(self, hop: int, n_ranks: int, out=None) -> np.ndarray:
        cnt = np.zeros(n_ranks, dtype=np.uint64)
        self._chk(self.lib.gsx_gxf_pack(self.h, hop, _ptr(cnt, C.c_uint64), self._p(out) if out is not None else None),
                  "gsx_gxf_pack")
        return cnt

    def gxf_step(self, hop: int, entries, n: int, sync: bool = True):
        """-> this rank's new frontier (sync=False: no host sync, -> None)."""
        f = C.c_uint64()
        self._chk(self.lib.gsx_gxf_step(self.h, hop, self._p(entries), n, C.byref(f) if sync else None),
                  "gsx_gxf_step")
        return int(f.value) if sync else None

    def gxf_pack_dev(self, hop: int, out, d_counts):
        """Entries into out (dense segments), (entries per rank, frontier of hop - 1) into d_counts; no sync."""
        self._chk(self.lib.gsx_gxf_pack_dev(self.h, hop, self._p(out), self._p(d_counts)), "gsx_gxf_pack_dev")

    def gxf_end(self):
        self._chk(self.lib.gsx_gxf_end(self.h), "gsx_gxf_end")

    def gx_got(self, n_sets: int) -> np.ndarray:
        g = np.zeros(max(n_sets, 1), dtype=np.uint8)
        self._chk(self.lib.gsx_gx_got(self.h, _ptr(g, C.c_uint8)), "gsx_gx_got")
        return g[:n_sets]

    def gx_end(self, got_all) -> abi.HeartbeatOut:
        out = abi.HeartbeatOut()
        g = np.ascontiguousarray(got_all, dtype=np.uint8)
        if len(g) == 0:
            g = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.gsx_gx_end(self.h, _ptr(g, C.c_uint8), C.byref(out)), "gsx_gx_end")
        return out

    def export_backoff(self) -> np.ndarray:
        b = np.empty((self.n_topics, self.n_pairs), dtype=np.int64)
        self._chk(self.lib.gsx_export_backoff(self.h, _ptr(b, C.c_int64)), "gsx_export_backoff")
        return b

    def import_backoff(self, b):
        b = np.ascontiguousarray(b, dtype=np.int64).reshape(self.n_topics, self.n_pairs)
        self._chk(self.lib.gsx_import_backoff(self.h, _ptr(b, C.c_int64)), "gsx_import_backoff")

    def gossip_results(self):
        """-> (ihave_len [T, E] u32, ihave_digest [T, E] u64) of the last heartbeat."""
        ln = np.empty((self.n_topics, self.n_pairs), dtype=np.uint32)
        dg = np.empty((self.n_topics, self.n_pairs), dtype=np.uint64)
        self._chk(self.lib.gsx_gossip_results(self.h, _ptr(ln, C.c_uint32), _ptr(dg, C.c_uint64)),
                  "gsx_gossip_results")
        return ln, dg

    def mcache_clear(self):
        self._chk(self.lib.gsx_mcache_clear(self.h), "gsx_mcache_clear")

    # -- message-parallel replicas: a batch from its message blocks (gsx.h gsx_mcache_*) --------
    # A block travels as one 1-D int64 device tensor: the cache rows, the
    # message set's rows, then its validation-code planes (the arrival hops,
    # vc_planes(cfg) of them), [n_nodes][words(n_msgs)] u64 each.
    def vc_planes(self, cfg) -> int:
        """Code planes a propagated block carries: the bits of its arrival hops
        and the code after the last (the room gsx_propagate leaves for a
        recovery round); none when every hop takes no time (every copy
        validated at now_ns), and none with the gossip exchange off (the
        calls then keep no hop codes, so the merged set keeps none either,
        as one engine's: gsx_mcache_copy_last refuses planes of such a set)."""
        if cfg is None or cfg.hop_latency_ns + cfg.validation_delay_ns <= 0 or not getattr(self, "_gx_on", True):
            return 0
        return int(cfg.max_hops + 1).bit_length()

    def mcache_part_size(self, n_msgs: int, cfg=None) -> int:
        return (2 + self.vc_planes(cfg)) * self.n_nodes * prop_words(n_msgs)

    def mcache_take_block(self, pad: int, device, cfg=None):
        """The newest cached batch (this replica's block) out of the cache ->
        (tensor of max(pad, its size) int64 on `device`, n_msgs); stream-ordered."""
        import torch

        W, m = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.gsx_mcache_last(self.h, C.byref(W), C.byref(m)), "gsx_mcache_last")
        n = self.n_nodes * W.value
        p = self.vc_planes(cfg)
        t = torch.zeros(max(pad, (2 + p) * n), dtype=torch.int64, device=device)
        self._chk(self.lib.gsx_mcache_copy_last(self.h, C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr() + 8 * n),
                                                C.c_void_p(t.data_ptr() + 16 * n), p), "gsx_mcache_copy_last")
        self._chk(self.lib.gsx_mcache_pop(self.h), "gsx_mcache_pop")
        return t, m.value

    def mcache_empty_block(self, pad: int, device):
        import torch

        return torch.zeros(pad, dtype=torch.int64, device=device)

    def mcache_put(self, msgs, cfg: abi.PropConfig, blocks, part_msgs):
        """gsx_mcache_put: msgs as one cached batch from the blocks (tensors as
        mcache_take_block returns them, block k = part_msgs[k] messages)."""
        ms = np.ascontiguousarray(msgs, dtype=abi.msg_dtype())
        k = len(blocks)
        sz = [self.n_nodes * prop_words(int(n)) for n in part_msgs]
        cp = (C.c_void_p * k)(*[b.data_ptr() for b in blocks])
        sp = (C.c_void_p * k)(*[b.data_ptr() + 8 * z for b, z in zip(blocks, sz)])
        vp = (C.c_void_p * k)(*[b.data_ptr() + 16 * z for b, z in zip(blocks, sz)])
        pm = np.ascontiguousarray(part_msgs, dtype=np.uint32)
        self._chk(self.lib.gsx_mcache_put(self.h, ms.ctypes.data_as(C.c_void_p), len(ms), C.byref(cfg), k,
                                          _ptr(pm, C.c_uint32), cp, sp, vp, self.vc_planes(cfg)), "gsx_mcache_put")

    def set_subscriptions(self, joined):
        """Joined topics per node (bit t of joined[v]); gsx_set_subscriptions."""
        j = np.ascontiguousarray(joined, dtype=np.uint64)
        self._chk(self.lib.gsx_set_subscriptions(self.h, _ptr(j, C.c_uint64)), "gsx_set_subscriptions")

    def export_membership(self):
        """-> (joined [N] u64, fanout [E] u64 topic bits, lastpub [N, T] i64)"""
        j = np.empty(self.n_nodes, dtype=np.uint64)
        f = np.empty(self.n_pairs, dtype=np.uint64)
        lp = np.empty((self.n_nodes, self.n_topics), dtype=np.int64)
        self._chk(self.lib.gsx_export_membership(self.h, _ptr(j, C.c_uint64), _ptr(f, C.c_uint64),
                                                 _ptr(lp, C.c_int64)), "gsx_export_membership")
        return j, f, lp

    def join(self, nodes, topics, now: int, seed: int) -> abi.HeartbeatOut:
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        tp = np.ascontiguousarray(topics, dtype=np.uint32)
        out = abi.HeartbeatOut()
        self._chk(self.lib.gsx_join(self.h, _ptr(nd, C.c_uint32), _ptr(tp, C.c_uint32), len(nd), now, seed,
                                    C.byref(out)), "gsx_join")
        return out

    def leave(self, nodes, topics, now: int) -> abi.HeartbeatOut:
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        tp = np.ascontiguousarray(topics, dtype=np.uint32)
        out = abi.HeartbeatOut()
        self._chk(self.lib.gsx_leave(self.h, _ptr(nd, C.c_uint32), _ptr(tp, C.c_uint32), len(nd), now,
                                     C.byref(out)), "gsx_leave")
        return out

    def hb_set_tracing(self, on: bool = True):
        self._chk(self.lib.gsx_hb_set_tracing(self.h, 1 if on else 0), "gsx_hb_set_tracing")

    def hb_set_px_log(self, cap: int):
        """Keep up to cap PX connection candidates per heartbeat (gsx_hb_set_px_log)."""
        self._chk(self.lib.gsx_hb_set_px_log(self.h, cap), "gsx_hb_set_px_log")

    def hb_px_records(self):
        """-> [n, 4] u32 (receiver, candidate, pruner, topic | kind << 8) of the last
        heartbeat, sorted (gsx_hb_px_records: min(px_connect, log cap) of them are kept)."""
        n = C.c_size_t()
        self._chk(self.lib.gsx_hb_px_records(self.h, None, 0, C.byref(n)), "gsx_hb_px_records")
        out = np.zeros((n.value, 4), dtype=np.uint32)
        self._chk(self.lib.gsx_hb_px_records(self.h, _ptr(out, C.c_uint32), n.value, C.byref(n)), "gsx_hb_px_records")
        return out

    def hb_trace_words(self):
        """-> (sent_graft, sent_prune, acc_graft, handled_prune) [E] u64 topic words
        of the last heartbeat (gsx_hb_trace_words; hb_set_tracing first)."""
        w = [np.empty(self.n_pairs, dtype=np.uint64) for _ in range(4)]
        self._chk(self.lib.gsx_hb_trace_words(self.h, *[_ptr(x, C.c_uint64) for x in w]), "gsx_hb_trace_words")
        return tuple(w)

    def mcache_ids(self, node: int, topic: int, n_windows: int) -> np.ndarray:
        """mcache.GetGossipIDs of `node` over its first n_windows windows."""
        n = C.c_size_t()
        self._chk(self.lib.gsx_mcache_ids(self.h, node, topic, n_windows, None, 0, C.byref(n)), "gsx_mcache_ids")
        out = np.empty(n.value, dtype=np.uint64)
        self._chk(self.lib.gsx_mcache_ids(self.h, node, topic, n_windows, _ptr(out, C.c_uint64), len(out),
                                          C.byref(n)), "gsx_mcache_ids")
        return out

    # -- the gossipTracer's promises (gossip_tracer.go:48-185) ------------------------------
    def promise_add(self, pair: int, handles, expire: int, seed: int = 0):
        """AddPromise(p, msgIDs): one of `handles` (Int31n, draws h(seed, 9, pair, k)) expiring at `expire`."""
        h = np.ascontiguousarray(handles, dtype=np.uint64)
        self._chk(self.lib.gsx_promise_add(self.h, pair, _ptr(h, C.c_uint64), len(h), expire, seed), "gsx_promise_add")

    def promise_broken(self, now: int):
        """GetBrokenPromises: -> (per-pair counts [n_pairs] u32, total); the broken ones are dropped."""
        cnt = np.zeros(self.n_pairs, dtype=np.uint32)
        tot = C.c_uint64()
        self._chk(self.lib.gsx_promise_broken(self.h, now, _ptr(cnt, C.c_uint32), C.byref(tot)), "gsx_promise_broken")
        return cnt, tot.value

    def promise_fulfill(self, node: int, handle: int):
        self._chk(self.lib.gsx_promise_fulfill(self.h, node, handle), "gsx_promise_fulfill")

    def promise_throttle(self, pair: int):
        self._chk(self.lib.gsx_promise_throttle(self.h, pair), "gsx_promise_throttle")

    def promise_count(self) -> int:
        n = C.c_uint64()
        self._chk(self.lib.gsx_promise_count(self.h, C.byref(n)), "gsx_promise_count")
        return n.value

    def timing_begin(self, max_launches: int):
        self._chk(self.lib.gsx_timing_begin(self.h, max_launches), "gsx_timing_begin")

    def timing_end(self):
        """-> (total_ms, min_ms, max_ms, n_launches) of the fused kernel over the region."""
        tot, lo, hi, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        self._chk(
            self.lib.gsx_timing_end(self.h, C.byref(tot), C.byref(lo), C.byref(hi), C.byref(n)), "gsx_timing_end"
        )
        return tot.value, lo.value, hi.value, n.value

    # -- state ---------------------------------------------------------------------------
    def _view(self, arrays: Dict[str, np.ndarray]) -> abi.StateView:
        sv = abi.StateView()
        for f in abi.STATE_FIELDS:
            a = arrays.get(f)
            ct = _CTYPES[abi.STATE_DTYPES[f]]
            setattr(sv, f, _ptr(a, ct))
        return sv

    def import_state(self, st: Dict[str, np.ndarray]):
        arrays = {f: np.ascontiguousarray(st[f], dtype=abi.STATE_DTYPES[f]).reshape(-1) for f in abi.STATE_FIELDS}
        R = self.n_topics * self.n_pairs
        for f in abi.RECORD_FIELDS:
            assert arrays[f].size == R, (f, arrays[f].size, R)
        for f in abi.PAIR_FIELDS:
            assert arrays[f].size == self.n_pairs, f
        sv = self._view(arrays)
        sv.last_refresh_ns = int(st.get("last_refresh_ns", 0))
        self._chk(self.lib.gsx_import_state(self.h, C.byref(sv)), "gsx_import_state")

    def synthesize_state(self, spec: abi.SynthSpec):
        self._chk(self.lib.gsx_synthesize_state(self.h, C.byref(spec)), "gsx_synthesize_state")

    def snapshot(self) -> Dict[str, np.ndarray]:
        """gsx_peer_score_snapshot (inspectScoresExtended, score.go:463-493): per pair and
        per [topic][pair] record, the PeerScoreSnapshot / TopicScoreSnapshot fields."""
        out = {f: np.empty(self.n_pairs, dtype=d) for f, d in abi.SNAPSHOT_PAIR.items()}
        out.update({f: np.empty(self.n_topics * self.n_pairs, dtype=d) for f, d in abi.SNAPSHOT_RECORD.items()})
        sv = abi.ScoreSnapshot(**{f: out[f].ctypes.data_as(dict(abi.ScoreSnapshot._fields_)[f]) for f in out})
        self._chk(self.lib.gsx_peer_score_snapshot(self.h, C.byref(sv)), "gsx_peer_score_snapshot")
        return out

    def export_state(self) -> Dict[str, np.ndarray]:
        R = self.n_topics * self.n_pairs
        out = {}
        for f in abi.STATE_FIELDS:
            n = R if f in abi.RECORD_FIELDS else self.n_pairs
            out[f] = np.empty(n, dtype=abi.STATE_DTYPES[f])
        sv = self._view(out)
        self._chk(self.lib.gsx_export_state(self.h, C.byref(sv)), "gsx_export_state")
        out["last_refresh_ns"] = int(sv.last_refresh_ns)
        return out

    def zero_map_violations(self) -> int:
        """gsx_zero_map_violations: zero-map entries that say zero over a non-zero counter (always 0)."""
        n = C.c_uint64()
        self._chk(self.lib.gsx_zero_map_violations(self.h, C.byref(n)), "gsx_zero_map_violations")
        return n.value

    def set_decay_writeback(self, k: int) -> None:
        """gsx_set_decay_writeback: the refresh pass stores the decayed counters every k-th refresh
        (1, 2, 4 or 16; 16 by default, 8 is not offered)."""
        self._chk(self.lib.gsx_set_decay_writeback(self.h, k), "gsx_set_decay_writeback")

    def zero_map_marked(self) -> int:
        """gsx_zero_map_marked: zero-map entries (tile, topic, counter) that say "maybe non-zero"."""
        n = C.c_uint64()
        self._chk(self.lib.gsx_zero_map_marked(self.h, C.byref(n)), "gsx_zero_map_marked")
        return n.value

    def decay_writeback(self) -> int:
        """gsx_get_decay_writeback: the write-back period in force."""
        k = C.c_uint32()
        self._chk(self.lib.gsx_get_decay_writeback(self.h, C.byref(k)), "gsx_get_decay_writeback")
        return k.value

    def pair_zero_map_violations(self) -> int:
        """gsx_pair_zero_map_violations: pair-zero-map entries that say zero over a non-zero
        application score or IP colocation factor (always 0)."""
        n = C.c_uint64()
        self._chk(self.lib.gsx_pair_zero_map_violations(self.h, C.byref(n)), "gsx_pair_zero_map_violations")
        return n.value

    def pair_zero_map_marked(self, which: int) -> int:
        """gsx_pair_zero_map_marked: tiles whose entry `which` (abi.GSX_PZ_APP, abi.GSX_PZ_P6) says "maybe non-zero"."""
        n = C.c_uint64()
        self._chk(self.lib.gsx_pair_zero_map_marked(self.h, which, C.byref(n)), "gsx_pair_zero_map_marked")
        return n.value

    def purge_launches(self) -> int:
        """gsx_purge_launches: launches of the purge of expired retained peers since the overlay was loaded."""
        n = C.c_uint64()
        self._chk(self.lib.gsx_purge_launches(self.h, C.byref(n)), "gsx_purge_launches")
        return n.value

    def dropin_launches(self) -> int:
        """gsx_dropin_launches: launches of the drop-in round trip (score / score_many on a small
        engine whose host score copy was current) since the overlay was loaded."""
        n = C.c_uint64()
        self._chk(self.lib.gsx_dropin_launches(self.h, C.byref(n)), "gsx_dropin_launches")
        return n.value

"""Shared cases of the gsx_prop_traffic tests: one small overlay (130 nodes of degree
about 6, neither nodes nor pairs a multiple of 64, node 129 without pairs, a hub whose
row spans three 64-pair tiles), the routers and gates of propagation_cases.py, and the
expectation of a case, computed once: FIRST / INVALID / DUP from the CPU oracle's first
deliverers and duplicate rows, GRAYLISTED from traffic_model.py."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import oracle as orc
import propagation_cases as pc
import traffic_model as tm
from gsx import abi

FLOOD, GOSSIP, RANDOM = abi.GSX_ROUTER_FLOODSUB, abi.GSX_ROUTER_GOSSIPSUB, abi.GSX_ROUTER_RANDOMSUB
N, HUB, LONE = 130, 70, 129


def _with_hub(ov, hub):
    obs = ov.pair_observer()
    edges = {(int(u), int(v)): int(f) for u, v, f in zip(obs, ov.col, ov.edge_flags) if LONE not in (u, v)}
    rng = np.random.default_rng(5)
    f0 = abi.GSX_EDGE_GOSSIPSUB
    for v in rng.choice([x for x in range(N) if x not in (hub, LONE)], size=110, replace=False):
        edges.setdefault((hub, int(v)), f0)
        edges.setdefault((int(v), hub), f0)
    keys = sorted(edges)
    deg = np.zeros(N + 1, dtype=np.int64)
    for u, _ in keys:
        deg[u + 1] += 1
    return dataclasses.replace(ov, row_ptr=np.cumsum(deg), col=np.array([v for _, v in keys], dtype=np.int32),
                               edge_flags=np.array([edges[k] for k in keys], dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def overlay(mix=True):
    base = pc.overlay(N, 3, 11, mix_protocols=mix, direct_frac=0.03 if mix else 0.0)
    for hub in range(HUB, LONE):  # the first hub from HUB on whose row spans three tiles
        ov = _with_hub(base, hub)
        rp = ov.row_ptr
        if (rp[hub + 1] - 1) // 64 - rp[hub] // 64 >= 2:
            break
    else:
        raise AssertionError("no hub row over three tiles")
    assert rp[LONE] == rp[LONE + 1] and ov.n_pairs % 64 and N % 64
    return ov


# key -> router, m, mix, flood_publish, invalid, max_hops, partial subscriptions
CASES = {
    # message words: W = 1, 1, 1, 2, 3 (padded to 4), 5 (padded to 8)
    "flood-m1": (FLOOD, 1, True, 0, 0.0, 40, False),
    "gossip-m63": (GOSSIP, 63, True, 0, 0.0, 40, False),
    "flood-m64": (FLOOD, 64, True, 0, 0.0, 40, False),
    "gossip-m65": (GOSSIP, 65, True, 1, 0.0, 40, False),
    "gossip-m129": (GOSSIP, 129, True, 0, 0.0, 40, False),
    "gossip-m300": (GOSSIP, 300, True, 1, 0.0, 40, False),
    # routers and gates
    "random-m130": (RANDOM, 130, True, 0, 0.0, 40, False),
    "random-invalid": (RANDOM, 70, True, 0, 0.25, 40, False),
    "invalid": (GOSSIP, 130, True, 1, 0.3, 40, False),
    "cut1": (GOSSIP, 130, True, 0, 0.2, 1, False),
    "cut2": (GOSSIP, 130, True, 1, 0.0, 2, False),
    "fanout": (GOSSIP, 130, True, 0, 0.1, 40, True),
    "plain": (GOSSIP, 130, False, 0, 0.0, 40, False),  # (every edge gossipsub, no direct peer: the enforced case)
}
SEED = 11


def joined_mask():
    j = np.ones(N, dtype=np.uint64)
    j[np.random.default_rng(3).random(N) < 0.25] = 0
    return j


def inputs(key):
    router, m, mix, fp, invalid, max_hops, partial = CASES[key]
    ms = pc.messages(N, m, SEED + m, invalid=invalid)
    cfg = pc.config(router, flood_publish=fp, max_hops=max_hops, size=8, delay_ms=2.0 if invalid else 0.0)
    return overlay(mix), ms, cfg, partial


def load(be, key, score_spread=True):
    ov, ms, cfg, partial = inputs(key)
    pc.setup(be, ov, 1, SEED, score_spread=score_spread)  # (score_spread: senders below publish and graylist)
    if partial:
        be.set_subscriptions(joined_mask())
    return ov, ms, cfg


def model_applies(key) -> bool:
    """traffic_model covers floodsub and gossipsub with every node joined."""
    return CASES[key][0] != RANDOM and not CASES[key][6]


class Expect:
    """out: the oracle's gsx_prop_out dict; B [5, E, m] class bits (GRAYLISTED from the model, or
    zero with gray_known False); hop [m, n]."""


def expect_from(ora, ov, ms, cfg, model=None) -> Expect:
    """Runs the call on the oracle (dup tracking on) and builds the class bits; `model`: the
    traffic_model Result of the same call (GRAYLISTED rows), None where the model does not apply."""
    x = Expect()
    out, hop, frm = ora.propagate(ms, cfg, want_results=True)
    m = len(ms)
    first = tm.first_rows(frm, ov.row_ptr, ov.col)
    dup = tm.bits_of_words(ora.prop_duplicates(m), m) if m else np.zeros((ov.n_pairs, 0), np.uint8)
    x.gray_known = model is not None or out.graylisted == 0
    gray = tm.bits_of_ints(model.rows[tm.GRAYLISTED], m) if model is not None else np.zeros_like(first)
    x.B = tm.class_bits(first, dup, gray, ms["validation"])
    x.out, x.hop = out.as_dict(), hop
    x.B.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(key) -> Expect:
    ora = orc.Oracle(1)
    ov, ms, cfg = load(ora, key)
    ora.set_dup_tracking(True)
    model = tm.run_on(ora, ov, ms, cfg) if model_applies(key) else None
    x = expect_from(ora, ov, ms, cfg, model)
    x.model = model
    return x


def sizes(kind, m):
    """msg_bytes of a case: None, all equal, all 0, every plane and the u64 carries, seeded random."""
    if kind == "null":
        return None
    if kind == "equal":
        return np.full(m, 1500, dtype=np.uint32)
    if kind == "zero":
        return np.zeros(m, dtype=np.uint32)
    if kind == "planes":
        s = (np.uint64(1) << (np.arange(m, dtype=np.uint64) % np.uint64(32))).astype(np.uint32)
        s[::7] = 0xFFFFFFFF
        return s
    return np.random.default_rng(m).integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)


SIZE_KINDS = ("null", "equal", "zero", "planes", "random")

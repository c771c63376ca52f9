#!/usr/bin/env python3
"""Finds, on the CPU alone, the seeds for which the scenarios of
tests/rejection_cases.py take the redraw branch of Go's Int31n where each one
wants it, and prints the table tests/rejection_cases.py keeps as SEEDS (with
the oracle's rejected-draw counts per tag).  numpy and the oracle only.

    python tools/find_rejection_seeds.py [--budget SECONDS per scenario]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("go-libp2p-pubsub_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import gossip_cases as gc  # noqa: E402
import oracle as orc  # noqa: E402
import rejection_cases as rc  # noqa: E402


def counted(fn):
    orc.rng_rejections_reset()
    res = fn()
    return res, orc.rng_rejections()


def find_promise(n_seeds=3):
    """n is known (PROMISE_N): the first seeds whose first draw is rejected, straight from the hash."""
    out, s = [], 0
    while len(out) < n_seeds:
        if rc.promise_seed_rejects(s):
            out.append(s)
        s += 1
    _, rej = counted(lambda: rc.promise_run(orc.Oracle(1), out))
    return {"seeds": out, "rej": rej}


def find_promise_eq(budget):
    """A seed whose first draw equals max for n = PROMISE_N, straight from the
    hash (about 2^31 seeds are expected to be needed)."""
    import numpy as np

    inner = rc.hash_inner(rc.TAG_IWANT, 0, 0)
    mx = int(rc.int31n_max(rc.PROMISE_N))
    t0, lo, step = time.time(), 0, 1 << 22
    while time.time() - t0 < budget:
        v = rc.draws_of_seeds(np.arange(lo, lo + step, dtype=np.uint64), inner)[:, 0]
        hit = np.flatnonzero(v == mx)
        if len(hit):
            s = lo + int(hit[0])
            assert rc.promise_eq(s)
            _, rej = counted(lambda: rc.promise_run(orc.Oracle(1), [s]))
            return {"seed": s, "rej": rej}
        lo += step
    return {"seed": None, "searched_up_to": lo}


def find_hub_eq(budget):
    """A heartbeat seed for which some step k < HUB_EQ_K of the hub's first
    shuffle draws exactly max of Int31n(k + 1), from the hash; confirmed on
    the oracle: the mesh is longer than HUB_EQ_K and round 59 redraws nothing
    (so counter k is step k)."""
    import numpy as np

    inner, mx, ok = rc.hub_eq_positions()
    t0, lo, step = time.time(), 0, 256
    while time.time() - t0 < budget:
        v = rc.draws_of_seeds(np.arange(lo, lo + step, dtype=np.uint64), inner)
        for i in np.flatnonzero(((v == mx[None, :]) & ok[None, :]).any(axis=1)):
            s = lo + int(i)
            pre = []
            _, rej = counted(lambda: rc.hub_run(orc.Oracle(2), s, ticks=1, pre=pre))
            if min(pre[0]) > rc.HUB_EQ_K and not rej.get(rc.TAG_SHUFFLE):
                return {"seed": s, "hits": rc.hub_eq_hits(s), "mesh": pre[0], "rej": rej}
        lo += step
    return {"seed": None, "searched_up_to": lo}


def find_hub(budget):
    t0, s = time.time(), 0
    while time.time() - t0 < budget:
        _, rej = counted(lambda: rc.hub_run(orc.Oracle(2), s))
        if rej.get(rc.TAG_SHUFFLE):
            return {"seed": s, "rej": rej}
        s += 1
    return None


def find_lane(budget):
    t0, lo = time.time(), 0
    while time.time() - t0 < budget:
        for s in rc.lane_prefilter(range(lo, lo + 200)):
            _, rej = counted(lambda: rc.lane_run(orc.Oracle(rc.LANE["T"]), s))
            if rej.get(rc.TAG_SHUFFLE):
                return {"seed": s, "rej": rej, "prefiltered_up_to": lo + 200}
        lo += 200
    return None


def find_trunc(budget):
    """One seed per placement (a seed may serve several)."""
    kw = rc.TRUNC
    want = {"lane0", "last_step", "two_in_batch"}
    found, t0, s = {}, time.time(), 0
    while want - set(found) and time.time() - t0 < budget:
        be = rc.ListLengths(orc.Oracle(kw["T"]), kw["n"], kw["T"], kw["history_gossip"])
        (ov, _, snaps, _), rej = counted(lambda: gc.exchange_run(be, seed=s, **kw))
        tot, hits = rc.trunc_placements(s, ov, be.L, snaps, kw["max_ihave_length"])
        # the replay from the hash must see exactly the oracle's redraws
        assert tot == rej.get(rc.TAG_IHAVE_SUB, 0), (s, tot, rej)
        for pl in rc.placements_of(hits):
            found.setdefault(pl, {"seed": s, "rej": rej})
        if tot and "any" not in found:
            found["any"] = {"seed": s, "rej": rej}
        s += 1
    found["searched_up_to"] = s
    return found


def find_iwant(kw, budget):
    t0, s = time.time(), 0
    while time.time() - t0 < budget:
        (_, outs, _, _), rej = counted(lambda: gc.exchange_run(orc.Oracle(kw["T"]), seed=s, **kw))
        if rej.get(rc.TAG_IWANT):
            return {"seed": s, "rej": rej, "iwant_ids": sum(o["iwant_ids"] for o in outs)}
        s += 1
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budget", type=float, default=120.0)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    jobs = {
        "promise": find_promise,
        "promise_eq": lambda: find_promise_eq(a.budget),
        "hub": lambda: find_hub(a.budget),
        "hub_eq": lambda: find_hub_eq(a.budget),
        "lane": lambda: find_lane(a.budget),
        "iwant_heavy": lambda: find_iwant(rc.IWANT_HEAVY, a.budget),
        "iwant_light": lambda: find_iwant(rc.IWANT_LIGHT, a.budget),
        "trunc": lambda: find_trunc(a.budget),
    }
    print("SEEDS = {")
    for name, fn in jobs.items():
        if a.only and name not in a.only.split(","):
            continue
        print(f"    {name!r}: {fn()!r},", flush=True)
    print("}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time gsx_propagate_timed against gsx_propagate, on one engine.

For 1M peers, d = 6, gossipsub (the bench's overlay and state) and batches of 64
and 1024 messages, a child process under its own `timeout` records
  1. gsx_propagate (hop kernels' device time, HIP events, and the call's wall clock),
  2. gsx_propagate_timed with every link at 1 tick: the same result (checked on the
     counters), so the difference is the price of the tick machinery,
  3. gsx_propagate_timed with synth.link_latency(lo=1, hi=16): ticks run, launches,
     marked nodes per tick; and gsx_timed_stats against gsx_timed_results + numpy for
     the same histogram, checked equal.
Each figure is the median of --reps calls after one warm-up call (buffers, fwd / pin
passes).  The parent merges the records into profiles/timed_prop_time.json.

    python tools/timed_prop_time.py [--peers N] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = (64, 1024)


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "go-libp2p-pubsub_amd"))
    import numpy as np

    import bench
    from gsx import abi, synth

    n, m = a.peers, a.one
    th = abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                        accept_px_threshold=0, opportunistic_graft_threshold=0)
    e = bench.prop_engine(n, 0, n, 6, synth.SEED, 0, th, None)

    class A:
        prop_hops = 24

    cfg = bench.prop_config(A, n)
    cfg.credit_scores = abi.GSX_CREDIT_OFF  # every call of a series starts from the same scores
    ov = synth.connect_some_overlay(n, d=6, seed=synth.SEED)
    assert ov.n_pairs == e.n_pairs
    ms = bench.prop_messages(n, m, synth.SEED, first=m)
    rec = {"peers": n, "msgs": m, "pairs": int(e.n_pairs), "reps": a.reps}

    def series(call):
        call()  # warm-up
        dev, wall, out = [], [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out, ms_dev = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(ms_dev)
        return out, {"device_ms_median": statistics.median(dev), "device_ms_min": min(dev), "device_ms_max": max(dev),
                     "wall_ms_median": statistics.median(wall)}

    def plain():
        o = e.propagate(ms, cfg)[0]
        return o, o.hop_kernel_ms

    def timed():
        o = e.propagate_timed(ms, cfg, 65534)[0]
        return o, o.kernel_ms

    po, rec["propagate"] = series(plain)
    rec["propagate"].update(hops=int(po.hops), launches=int(po.hop_launches), deliveries=int(po.deliveries))
    e.set_link_latency(np.ones(e.n_pairs, dtype=np.uint8))
    to, rec["timed_1_tick"] = series(timed)
    rec["timed_1_tick"].update(ticks_run=int(to.ticks_run), launches=int(to.launches))
    rec["timed_1_tick"]["same_counters"] = all(
        int(getattr(to, k)) == int(getattr(po, k))
        for k in ("deliveries", "duplicates", "transmissions", "rejected", "ignored", "graylisted"))
    e.set_link_latency(synth.link_latency(ov, synth.SEED, 1, 16))
    ho, rec["timed_1_16_ticks"] = series(timed)
    rec["timed_1_16_ticks"].update(ticks_run=int(ho.ticks_run), launches=int(ho.launches), last_tick=int(ho.last_tick),
                                   deliveries=int(ho.deliveries), duplicates=int(ho.duplicates),
                                   dup_in_window=int(ho.dup_in_window),
                                   marked_nodes_per_tick=ho.marked_nodes / max(int(ho.launches), 1))
    # gsx_timed_stats against the [message][node] export + numpy, the same histogram
    bins = 64
    e.timed_stats(m, 4, bins)  # warm-up
    e.timing_begin(a.reps)
    for _ in range(a.reps):
        st = e.timed_stats(m, 4, bins)
    e.sync()
    tot, lo, hi, k = e.timing_end()
    t0 = time.perf_counter()
    tick, _ = e.timed_results(m)
    t1 = time.perf_counter()
    want = np.zeros((m, bins), dtype=np.uint32)
    for j in range(m):
        got = tick[j] != 0xFFFF
        want[j] = np.bincount(np.minimum(tick[j][got].astype(np.int64) // 4, bins - 1), minlength=bins)
    t2 = time.perf_counter()
    rec["timed_stats"] = {"device_ms_mean": tot / max(k, 1), "device_ms_min": lo, "device_ms_max": hi,
                          "results_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3,
                          "exact_match": bool(np.array_equal(st.tick_hist, want))}
    rec["timed_stats"]["speedup_over_results_numpy"] = (t2 - t0) * 1e3 / rec["timed_stats"]["device_ms_mean"]
    rec["ratio_1_tick_over_propagate"] = rec["timed_1_tick"]["device_ms_median"] / rec["propagate"]["device_ms_median"]
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds per workload (its own timeout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed_prop_time.json"))
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return child(a)
    recs = []
    for m in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(m),
               "--peers", str(a.peers), "--reps", str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [x for x in p.stdout.splitlines() if x.startswith("RECORD ")]
        if p.returncode != 0 or not line:
            print(f"workload {m} messages ended with status {p.returncode}; stopping", file=sys.stderr)
            sys.exit(p.returncode or 1)
        recs.append(json.loads(line[-1][7:]))
        print(json.dumps(recs[-1]), flush=True)
    doc = {"tool": "tools/timed_prop_time.py", "device": "MI355X (gfx950), one GPU",
           "timing": "device_ms: HIP events around the hop / tick launches of one call (host read-backs between "
                     "batches of ticks included); wall_ms: the whole call; medians of `reps` calls after a warm-up; "
                     "credits off so every call starts from the same scores",
           "workloads": recs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

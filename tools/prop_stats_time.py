#!/usr/bin/env python3
"""Time gsx_prop_stats against the route it replaces, on one engine.

For each propagation workload of the README (1M peers x 64 messages, 1M peers
x 1024 messages; gossipsub, the bench's overlay and state) a child process
under its own `timeout`:
  * propagates one warm-up batch and the measured batch,
  * times gsx_prop_stats with device-pointer output over --reps calls with HIP
    events (gsx_timing_begin / gsx_timing_end: memsets + kernel, per call),
  * times the existing route once by wall clock: gsx_prop_results (the
    [message][node] hop bytes through the host) plus the numpy reduction to
    the same three arrays,
  * checks the two agree exactly,
  * counts the bytes the kernel has to read: the occupied history rows (8 B per
    word of every (node, hop) whose occupancy bit is set), the occupancy words
    and, written, the zeroed outputs.
The parent merges the children's records into profiles/prop_stats_time.json.

    python tools/prop_stats_time.py [--peers N] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s
WORKLOADS = (64, 1024)


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "go-libp2p-pubsub_amd"))
    import numpy as np
    import torch

    import bench
    from gsx import abi, synth

    n, m = a.peers, a.one
    H = abi.GSX_MAX_HOPS + 1
    th = abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                        accept_px_threshold=0, opportunistic_graft_threshold=0)
    e = bench.prop_engine(n, 0, n, 6, synth.SEED, 0, th, None)

    class A:
        prop_hops = 24

    cfg = bench.prop_config(A, n)
    e.propagate(bench.prop_messages(n, m, synth.SEED, first=0), cfg)  # warm-up: buffers, fwd / pin passes
    out = e.propagate(bench.prop_messages(n, m, synth.SEED, first=m), cfg)[0]
    hist = torch.zeros((m, H), dtype=torch.int32, device="cuda:0")
    recv = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    hsum = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    e.prop_stats(m, out_ptrs=(hist, recv, hsum))  # warm-up of the kernel itself
    e.sync()
    rec = {"peers": n, "msgs": m, "deliveries": int(out.deliveries), "hops": int(out.hops)}
    for name, ptrs in (("hist_and_per_node", (hist, recv, hsum)), ("hist_only", (hist, None, None))):
        e.timing_begin(a.reps)
        for _ in range(a.reps):
            e.prop_stats(m, out_ptrs=ptrs)
        e.sync()
        tot, lo, hi, k = e.timing_end()
        rec[f"prop_stats_ms_{name}"] = {"mean": tot / max(k, 1), "min": lo, "max": hi, "calls": k}
    e.prop_stats(m, out_ptrs=(hist, recv, hsum))
    e.sync()
    got = (hist.cpu().numpy().view(np.uint32), recv.cpu().numpy().view(np.uint32), hsum.cpu().numpy().view(np.uint64))

    if a.kernel_only:  # (A/B runs of the kernel's knobs)
        rec["env"] = {k: v for k, v in os.environ.items() if k.startswith("GSX_STATS")}
        e.close()
        print("RECORD " + json.dumps(rec), flush=True)
        return
    # the existing route: the hop bytes through the host, then numpy
    t0 = time.perf_counter()
    hop, _ = e.prop_results(m)
    t1 = time.perf_counter()
    want_hist = np.zeros((m, H), dtype=np.uint32)
    for k in range(m):
        want_hist[k] = np.bincount(hop[k], minlength=256)[:H]
    rcv = np.zeros(n, dtype=np.uint32)
    hs = np.zeros(n, dtype=np.uint64)
    occ = np.zeros((n, 2), dtype=np.uint64)  # per node: the hops it was occupied at, as bits (hop 64 apart)
    for k in range(m):
        r = hop[k]
        ok = (r >= 1) & (r <= abi.GSX_MAX_HOPS)
        rcv += ok
        hs += np.where(ok, r, 0).astype(np.uint64)
    t2 = time.perf_counter()
    rec["prop_results_ms"] = (t1 - t0) * 1e3
    rec["numpy_reduction_ms"] = (t2 - t1) * 1e3
    rec["existing_route_ms"] = (t2 - t0) * 1e3
    rec["exact_match"] = bool(np.array_equal(got[0], want_hist) and np.array_equal(got[1], rcv)
                              and np.array_equal(got[2], hs))
    for k in range(m):
        r = hop[k]
        lo_h = r < 64
        occ[:, 0] |= np.where(lo_h, np.uint64(1) << (r & 63).astype(np.uint64), np.uint64(0))
        occ[:, 1] |= (r == 64).astype(np.uint64)
    rows = int(np.unpackbits(occ.view(np.uint8)).sum())
    words = (m + 63) // 64
    n_hops = int(out.hops) + 1
    b_rows = 8 * words * rows  # the occupied history rows, read once
    b_occ = 8 * ((n + 63) // 64) * n_hops * words  # every word's blocks read the tiles' occupancy words
    b_out = 4 * m * H + 12 * n  # the zeroed outputs (the non-zero counters' atomics come on top)
    rec["bytes"] = {"occupied_rows": b_rows, "occupancy_words": b_occ, "outputs_zeroed": b_out,
                    "total": b_rows + b_occ + b_out, "occupied_node_hops": rows}
    ms = rec["prop_stats_ms_hist_and_per_node"]["mean"]
    rec["achieved_GBps"] = rec["bytes"]["total"] / (ms * 1e-3) / 1e9
    rec["frac_of_8TBps"] = rec["bytes"]["total"] / (ms * 1e-3) / HBM_PEAK
    rec["speedup_over_existing_route"] = rec["existing_route_ms"] / ms
    rec["env"] = {k: v for k, v in os.environ.items() if k.startswith("GSX_STATS")}
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds per workload (its own timeout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prop_stats_time.json"))
    ap.add_argument("--kernel-only", action="store_true", help="time gsx_prop_stats alone and write no file")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return child(a)
    recs = []
    for m in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(m),
               "--peers", str(a.peers), "--reps", str(a.reps)] + (["--kernel-only"] if a.kernel_only else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [x for x in p.stdout.splitlines() if x.startswith("RECORD ")]
        if p.returncode != 0 or not line:
            print(f"workload {m} messages ended with status {p.returncode}; stopping", file=sys.stderr)
            sys.exit(p.returncode or 1)
        recs.append(json.loads(line[-1][7:]))
        print(json.dumps(recs[-1]), flush=True)
    if a.kernel_only:
        return
    doc = {"tool": "tools/prop_stats_time.py", "device": "MI355X (gfx950)", "hbm_peak_Bps": HBM_PEAK,
           "timing": "gsx_prop_stats: HIP events around its memsets + kernel (gsx_timing_begin/end), device-pointer "
                     "output; existing route: wall clock of gsx_prop_results + the numpy reduction, same process",
           "workloads": recs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

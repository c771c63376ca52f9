#!/usr/bin/env python3
"""Time gsx_score_stats against the route it replaces, on one engine.

A child process under its own `timeout` builds the bench's cfg3 state (1M peers
x 8 topics, one refresh) and
  * times gsx_score_stats with device-pointer outputs over --reps calls with
    HIP events (gsx_timing_begin / gsx_timing_end: fills + kernel + key pass,
    per call), separately for {hist + observer view} and {all five outputs},
    over the default edges of the bench's thresholds,
  * times the route it replaces once by wall clock: gsx_scores (every score
    through the host), gsx_export_state of the two flag arrays, and the numpy
    reduction to the same five tables (bincounts; the minima by reduceat and
    minimum.at),
  * checks the two agree exactly,
  * counts the bytes the kernel has to read per pair (score 8, pair flags 1,
    observer 4; peer 4 with the peer view) and the outputs it fills.
The parent writes the child's record to profiles/score_stats_time.json.

    python tools/score_stats_time.py [--peers N] [--topics T] [--reps R] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "go-libp2p-pubsub_amd"))
    import numpy as np
    import torch

    import bench
    from gsx import abi, synth

    n, T = a.peers, a.topics
    ov, e = bench.build_engine(n, T, 6, synth.SEED, 0)
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                    accept_px_threshold=0, opportunistic_graft_threshold=5))
    e.refresh(bench.T0 + abi.SECOND)
    E = ov.n_pairs
    edges = e.score_stats_edges()
    B = len(edges) + 1
    dev = "cuda:0"
    hist = torch.zeros(B, dtype=torch.int64, device=dev)
    ob = torch.zeros((n, B), dtype=torch.int32, device=dev)
    om = torch.zeros(n, dtype=torch.float64, device=dev)
    pb = torch.zeros((n, B), dtype=torch.int32, device=dev)
    pm = torch.zeros(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    e.score_stats(edges, out_ptrs=(hist, ob, om, pb, pm))  # warm-up
    e.sync()
    rec = {"peers": n, "topics": T, "pairs": E, "edges": edges.tolist(), "select": "present"}
    for name, ptrs in (("hist_and_observer", (hist, ob, om, None, None)), ("all_five", (hist, ob, om, pb, pm))):
        e.timing_begin(a.reps)
        for _ in range(a.reps):
            e.score_stats(edges, out_ptrs=ptrs)
        e.sync()
        tot, lo, hi, k = e.timing_end()
        rec[f"score_stats_ms_{name}"] = {"mean": tot / max(k, 1), "min": lo, "max": hi, "calls": k}
    e.score_stats(edges, out_ptrs=(hist, ob, om, pb, pm))
    e.sync()
    got = {"hist": hist.cpu().numpy().view(np.uint64), "obs_bins": ob.cpu().numpy().view(np.uint32),
           "obs_min": om.cpu().numpy(), "peer_bins": pb.cpu().numpy().view(np.uint32), "peer_min": pm.cpu().numpy()}

    # the route it replaces: the scores and the flags through the host, then numpy
    t0 = time.perf_counter()
    s = e.scores()
    t1 = time.perf_counter()
    pf = np.empty(E, dtype=np.uint8)
    rf = np.empty(T * E, dtype=np.uint8)
    sv = abi.StateView()
    sv.pair_flags = pf.ctypes.data_as(C.POINTER(C.c_uint8))
    sv.rec_flags = rf.ctypes.data_as(C.POINTER(C.c_uint8))
    e._chk(e.lib.gsx_export_state(e.h, C.byref(sv)), "gsx_export_state")
    t2 = time.perf_counter()
    q = np.nonzero(pf & abi.GSX_PAIR_PRESENT)[0]
    b = np.searchsorted(edges, s[q], side="right")
    obs = np.repeat(np.arange(n, dtype=np.int64), np.diff(ov.row_ptr))[q]
    col = ov.col[q].astype(np.int64)
    w_hist = np.bincount(b, minlength=B).astype(np.uint64)
    w_ob = np.bincount(obs * B + b, minlength=n * B).astype(np.uint32).reshape(n, B)
    w_pb = np.bincount(col * B + b, minlength=n * B).astype(np.uint32).reshape(n, B)
    w_om = np.full(n, np.inf)
    np.minimum.at(w_om, obs, s[q])
    w_pm = np.full(n, np.inf)
    np.minimum.at(w_pm, col, s[q])
    t3 = time.perf_counter()
    rec["scores_ms"] = (t1 - t0) * 1e3
    rec["export_flags_ms"] = (t2 - t1) * 1e3
    rec["numpy_reduction_ms"] = (t3 - t2) * 1e3
    rec["existing_route_ms"] = (t3 - t0) * 1e3
    want = {"hist": w_hist, "obs_bins": w_ob, "obs_min": w_om, "peer_bins": w_pb, "peer_min": w_pm}
    rec["exact_match"] = bool(all(np.array_equal(got[f].view(np.uint8), want[f].view(np.uint8)) for f in want))
    rec["selected_pairs"] = int(len(q))

    b_obs = 13 * E + 8 * B + 4 * n * B + 8 * n  # score, flags, observer per pair; the observer outputs filled
    b_all = b_obs + 4 * E + 4 * n * B + 8 * n   # + the peer per pair; the peer outputs filled
    ms_o = rec["score_stats_ms_hist_and_observer"]["mean"]
    ms_a = rec["score_stats_ms_all_five"]["mean"]
    rec["bytes"] = {"hist_and_observer": b_obs, "all_five": b_all,
                    "note": "loads per pair + outputs filled; the peer view's atomics (one 4-B add per selected "
                            "pair, a min where it lowers) come on top"}
    rec["achieved_GBps"] = {"hist_and_observer": b_obs / (ms_o * 1e-3) / 1e9, "all_five": b_all / (ms_a * 1e-3) / 1e9}
    rec["frac_of_8TBps"] = {"hist_and_observer": b_obs / (ms_o * 1e-3) / HBM_PEAK,
                            "all_five": b_all / (ms_a * 1e-3) / HBM_PEAK}
    rec["peer_view_ns_per_selected_pair"] = (ms_a - ms_o) * 1e6 / max(len(q), 1)
    rec["observer_call_ns_per_pair"] = ms_o * 1e6 / max(E, 1)
    rec["speedup_over_existing_route"] = rec["existing_route_ms"] / ms_a
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds for the child (its own timeout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_stats_time.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child",
           "--peers", str(a.peers), "--topics", str(a.topics), "--reps", str(a.reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = [x for x in p.stdout.splitlines() if x.startswith("RECORD ")]
    if p.returncode != 0 or not line:
        print(f"the measurement ended with status {p.returncode}", file=sys.stderr)
        sys.exit(p.returncode or 1)
    rec = json.loads(line[-1][7:])
    print(json.dumps(rec), flush=True)
    doc = {"tool": "tools/score_stats_time.py", "device": "MI355X (gfx950)", "hbm_peak_Bps": HBM_PEAK,
           "timing": "gsx_score_stats: HIP events around its fills + kernel + key pass (gsx_timing_begin/end), "
                     "device-pointer outputs; existing route: wall clock of gsx_scores + gsx_export_state of the two "
                     "flag arrays + the numpy reduction, same process",
           "workload": rec}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

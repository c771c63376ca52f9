#!/usr/bin/env python3
"""Time gsx_accept_from over every pair against the path a caller has without it.

A child process under its own `timeout` builds the bench's cfg3 overlay (1M
peers x 8 topics, one refresh), creates a gater, binds every pair, gives every
third pair one failed validation (so a hot lane goes all the way to the draw)
and lets 1 % and then 100 % of the observers throttle (hot).  For each of the
two it takes --runs alternating runs of
  A. gsx_accept_from(pairs = NULL) with a device-pointer output: the device
     time by HIP events (gsx_timing_begin / gsx_timing_end) and the wall clock
     of the call plus gsx_sync;
  B. the path of today, by wall clock: gsx_scores + gsx_export_state of the
     pair flags + gsx_gater_export + the vectorised numpy decision (the same
     canonical draw);
checks that A and B give the same bytes, and reports median, min and max of
each, with the bytes per pair the kernel reads (cold: edge flag 1, score 8,
pair flag 1, observer 4, the observer's hot byte 1; hot: + bound group 4 + the
group's record 32) and writes (1).  The parent writes the record to
profiles/gater_time.json.

    python tools/gater_time.py [--peers N] [--topics T] [--runs R] [--out FILE]
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
GRAYLIST = -300.0
TAG_GATER = 14


def numpy_decision(np, synth, abi, ov, obs, scores, pflags, x, gp, now, seed, draw):
    """GossipSubRouter.AcceptFrom per pair from host copies (gossipsub.go:583-594, peer_gater.go:320-363)."""
    E = len(scores)
    last, thr, val = x["last_throttle_ns"], x["throttle"], x["validate"]
    quiet = (last == abi.GSX_GATER_NEVER) | ((now >= last) & ((now - np.where(last == abi.GSX_GATER_NEVER, now, last)) > gp.quiet_ns))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio_ok = (val != 0) & (thr / np.where(val != 0, val, 1.0) < gp.threshold)
    hot = ~quiet & (thr != 0) & ~ratio_ok
    b = x["bound_group"]
    gate = hot[obs] & ((pflags & abi.GSX_PAIR_PRESENT) != 0) & (b != abi.GSX_GATER_UNBOUND)
    g = np.where(gate, b, 0).astype(np.int64)
    d = x["deliver"][g]
    total = d + gp.duplicate_weight * x["duplicate"][g]
    total = total + gp.ignore_weight * x["ignore"][g]
    total = total + gp.reject_weight * x["reject"][g]
    u = (synth.h(seed, TAG_GATER, np.arange(E, dtype=np.uint64), draw) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    control = gate & (total != 0) & ~(u < (1 + d) / (1 + total))
    out = np.full(E, abi.GSX_ACCEPT_ALL, dtype=np.uint8)
    out[control] = abi.GSX_ACCEPT_CONTROL
    out[scores < GRAYLIST] = abi.GSX_ACCEPT_NONE
    out[(ov.edge_flags & abi.GSX_EDGE_DIRECT) != 0] = abi.GSX_ACCEPT_ALL
    return out


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "go-libp2p-pubsub_amd"))
    import numpy as np
    import torch

    import bench
    from gsx import abi, synth

    n, T = a.peers, a.topics
    ov, e = bench.build_engine(n, T, 6, synth.SEED, 0)
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=GRAYLIST,
                                    accept_px_threshold=0, opportunistic_graft_threshold=5))
    now = bench.T0 + abi.SECOND
    e.refresh(now)
    E = ov.n_pairs
    obs = np.repeat(np.arange(n, dtype=np.int64), np.diff(ov.row_ptr))
    gp = abi.GaterParams()
    e.lib.gsx_default_gater_params(C.byref(gp))
    out_dev = torch.zeros(E, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rec = {"peers": n, "topics": T, "pairs": E, "runs": a.runs,
           "bytes_per_pair": {"cold_read": 15, "hot_read": 15 + 4 + 32, "written": 1}}
    dt = abi.gater_event_dtype()
    for frac in (0.01, 1.0):
        e.set_gater_params(gp)
        for lo in range(0, E, 1 << 21):  # AddPeer for every pair; one failed validation for every third
            p = np.arange(lo, min(E, lo + (1 << 21)), dtype=np.uint64)
            ev = np.zeros(len(p), dtype=dt)
            ev["kind"], ev["pair"], ev["now_ns"] = abi.GATER_ADD_PEER, p, now
            bad = ev[p % 3 == 0].copy()
            bad["kind"], bad["reason"] = abi.GATER_REJECT, abi.REJECT_REASONS["validation failed"]
            e.gater_events(np.concatenate([ev, bad]))
        hot_obs = np.nonzero(synth.uniform(synth.SEED, 99, np.arange(n), 0) < frac)[0] if frac < 1 else np.arange(n)
        hot_obs = hot_obs[np.diff(ov.row_ptr)[hot_obs] > 0]
        ev = np.zeros(len(hot_obs), dtype=dt)
        ev["kind"], ev["pair"], ev["now_ns"] = abi.GATER_REJECT, ov.row_ptr[hot_obs], now
        ev["reason"] = abi.REJECT_REASONS["validation throttled"]
        e.gater_events(ev)
        e.accept_from(now, 7, 0, out_ptr=out_dev)  # warm-up
        e.sync()
        dev_ms, wall_ms, today = [], [], {"scores": [], "flags": [], "gater_export": [], "numpy": [], "total": []}
        same = True
        for r in range(a.runs):
            draw = r + 1
            e.timing_begin(1)
            t0 = time.perf_counter()
            e.accept_from(now, 7, draw, out_ptr=out_dev)
            e.sync()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(e.timing_end()[0])
            got = out_dev.cpu().numpy()
            t0 = time.perf_counter()
            s = e.scores()
            t1 = time.perf_counter()
            pf = np.empty(E, dtype=np.uint8)
            sv = abi.StateView()
            sv.pair_flags = pf.ctypes.data_as(C.POINTER(C.c_uint8))
            e._chk(e.lib.gsx_export_state(e.h, C.byref(sv)), "gsx_export_state")
            t2 = time.perf_counter()
            x = e.gater_export()
            t3 = time.perf_counter()
            want = numpy_decision(np, synth, abi, ov, obs, s, pf, x, gp, now, 7, draw)
            t4 = time.perf_counter()
            for k, v in zip(("scores", "flags", "gater_export", "numpy", "total"),
                            (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
                today[k].append(v * 1e3)
            same = same and bool(np.array_equal(got, want))
        hot_pairs = int(np.diff(ov.row_ptr)[hot_obs].sum())

        def stat(v):
            return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}

        bytes_ = 16 * E + 36 * hot_pairs
        rec[f"hot_{frac:g}"] = {
            "hot_observers": int(len(hot_obs)), "hot_pairs": hot_pairs,
            "control": int((got == abi.GSX_ACCEPT_CONTROL).sum()), "none": int((got == abi.GSX_ACCEPT_NONE).sum()),
            "accept_from_device_ms": stat(dev_ms), "accept_from_wall_ms": stat(wall_ms),
            "today_ms": {k: stat(v) for k, v in today.items()}, "exact_match": same,
            "algorithmic_bytes": bytes_, "frac_of_8TBps": bytes_ / (float(np.median(dev_ms)) * 1e-3) / HBM_PEAK,
            "speedup_wall": float(np.median(today["total"]) / np.median(wall_ms)),
        }
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds for the child (its own timeout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gater_time.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child",
           "--peers", str(a.peers), "--topics", str(a.topics), "--runs", str(a.runs)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = [x for x in p.stdout.splitlines() if x.startswith("RECORD ")]
    if p.returncode != 0 or not line:
        print(f"the measurement ended with status {p.returncode}", file=sys.stderr)
        sys.exit(p.returncode or 1)
    rec = json.loads(line[-1][7:])
    print(json.dumps(rec), flush=True)
    doc = {"tool": "tools/gater_time.py", "device": "MI355X (gfx950)", "hbm_peak_Bps": HBM_PEAK,
           "timing": "gsx_accept_from over every pair, device-pointer output: HIP events (gsx_timing_begin/end) and wall "
                     "clock of call + gsx_sync; today's path: wall clock of gsx_scores + gsx_export_state (pair flags) + "
                     "gsx_gater_export + the numpy decision; alternating runs in one process; no pass bar",
           "workload": rec}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the tag tracer's device calls against the path a caller has without them.

A child process under its own `timeout` builds the bench's cfg3 overlay (--peers
x --topics, one refresh), turns the tag tracer on and, for gossipsub batches of
1024 and 64 messages with a validation delay, takes --runs (--runs-large for
the 1024-message batch) alternating runs, after one warm-up of the device calls, of
  A. gsx_tag_fold_prop, then gsx_tag_decay(1), gsx_conn_values and
     gsx_conn_trim into device memory: each by HIP events (gsx_timing_begin /
     gsx_timing_end) and by the wall clock of the call plus gsx_sync;
  B. the path of today, by wall clock: gsx_prop_results + gsx_prop_duplicates
     and the numpy fold of their rows; numpy's per-row selection for the trim
     from host copies of the values, protection bits and pair flags;
checks that A and B give the same tag bytes and the same trim bytes, and reports
median, min and max of each with the bytes the kernels move, counted from the
source.  The parent writes the record to profiles/tag_time.json.

    python tools/tag_time.py [--peers N] [--topics T] [--runs R] [--runs-large R] [--out FILE]
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
LOW_WATER = 6
CAP = 255


def numpy_fold(np, abi, ov, obs, ms, hop, frm, dup, delayed, cap):
    """gsx_tag_fold_prop's definition (gsx.h) on the host copies of the call's public results."""
    E, n = ov.n_pairs, ov.n
    col = np.asarray(ov.col, dtype=np.int64)
    key = obs * n + col  # ascending: rows by observer, sorted peers inside
    cnt = np.zeros(E, dtype=np.int64)
    acc = np.nonzero(ms["validation"] == abi.GSX_VALIDATION_ACCEPT)[0]
    for i, k in enumerate(acc):
        if i % 128 == 127:
            print(f"[tag_time] numpy fold: {i + 1} of {len(acc)} messages", file=sys.stderr, flush=True)
        u = np.nonzero(frm[k] >= 0)[0]
        p = np.searchsorted(key, u * n + frm[k, u].astype(np.int64))
        cnt += np.bincount(p, minlength=E)
        if delayed:
            sel = np.nonzero((dup[:, k // 64] >> np.uint64(k % 64)) & np.uint64(1))[0]
            near = sel[hop[k, col[sel]].astype(np.int64) + 1 == hop[k, obs[sel]]]
            cnt[near] += 1
    return np.minimum(cnt, cap).astype(np.uint8)


def numpy_trim(np, abi, row_ptr, obs, val, prot, pf, low):
    both = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
    conn = (pf & both) == both
    unp = conn & (prot == 0)
    n = len(row_ptr) - 1
    conns = np.bincount(obs[conn], minlength=n)
    k = np.minimum(np.maximum(conns - low, 0), np.bincount(obs[unp], minlength=n))
    idx = np.nonzero(unp)[0]
    order = idx[np.lexsort((idx, val[idx], obs[idx]))]  # by row, then (value, index)
    first = np.concatenate([[0], np.cumsum(np.bincount(obs[unp], minlength=n))])[:-1]
    rank = np.arange(len(order)) - first[obs[order]]
    trim = np.zeros(len(obs), dtype=np.uint8)
    trim[order[rank < k[obs[order]]]] = 1
    return trim


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "go-libp2p-pubsub_amd"))
    import numpy as np
    import torch

    import bench
    from gsx import abi, synth
    from gsx import engine as engine_mod

    n, T = a.peers, a.topics
    ov, e = bench.build_engine(n, T, 6, synth.SEED, 0)
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                    accept_px_threshold=0, opportunistic_graft_threshold=5))
    e.refresh(bench.T0 + abi.SECOND)
    e.set_gossipsub_params(engine_mod.default_gossipsub_params(gossip_exchange=0))
    E = ov.n_pairs
    obs = np.repeat(np.arange(n, dtype=np.int64), np.diff(ov.row_ptr))
    tp = abi.TagParams(bump=1, decay_amount=1, cap=CAP, decay_interval_ns=600 * abi.SECOND)
    d_val = torch.zeros(E, dtype=torch.int32, device="cuda:0")
    d_prot = torch.zeros(E, dtype=torch.uint8, device="cuda:0")
    d_trim = torch.zeros(E, dtype=torch.uint8, device="cuda:0")
    d_nt = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    tiles = (E + 63) // 64
    rec = {"peers": n, "topics": T, "pairs": E, "low_water": LOW_WATER, "cap": CAP,
           "bytes": {"tag_decay": "read T x 64 B per tile, written where a 16-byte word held a non-zero tag",
                     "conn_values": "per pair: pair flag 1 + T tags + T record flags + edge flag 1 read, value 4 + protect 1 written",
                     "conn_trim": "k_conn_values' reads + key 4 written; then per row ~17 passes over its 4-byte keys (L2) + 1 B per pair written",
                     "tag_fold": "per pair: observer 4 + peer 4 + W first-deliverer words + W duplicate words (k_prop_dup_rows writes them first) "
                                 "+ the frontier rows of the hops both ends were active in; 1 tag byte read and written where a count is non-zero"}}

    def stat(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}

    def timed(fn):
        e.timing_begin(1)
        t0 = time.perf_counter()
        fn()
        e.sync()
        wall = (time.perf_counter() - t0) * 1e3
        return e.timing_end()[0], wall

    for m in (1024, 64):
        cfg = abi.PropConfig(router=abi.GSX_ROUTER_GOSSIPSUB, topic=0, flood_publish=0, max_hops=40,
                             hop_latency_ns=10 * abi.MILLISECOND, now_ns=bench.T0 + 2 * abi.SECOND, credit_scores=0,
                             randomsub_size=n, seed=synth.SEED, validation_delay_ns=2 * abi.MILLISECOND)
        t = {k: [] for k in ("fold_dev", "fold_wall", "decay_dev", "decay_wall", "values_dev", "values_wall", "trim_dev",
                             "trim_wall", "today_results", "today_duplicates", "today_numpy_fold", "today_fold_total",
                             "today_trim_exports", "today_numpy_trim", "today_trim_total")}
        same_fold = same_trim = True
        nonzero = 0
        runs = a.runs_large if m >= 1024 else a.runs
        for r in range(runs + 1):  # (run 0 warms the device calls up and skips today's path)
            print(f"[tag_time] {m} messages, run {r} of {runs}", file=sys.stderr, flush=True)
            ms = bench.prop_messages(n, m, synth.SEED, first=r * m)
            e.propagate(ms, cfg)
            e.set_tag_params(tp)
            e.sync()
            fd, fw = timed(e.tag_fold_prop)
            if r == 0:
                e.conn_values(value_ptr=d_val, protect_ptr=d_prot)
                e.conn_trim(LOW_WATER, trim_ptr=d_trim, node_trimmed_ptr=d_nt)
                e.tag_decay(1)
                e.sync()
                continue
            tags = e.tag_export()
            t0 = time.perf_counter()
            hop, frm = e.prop_results(m)
            t1 = time.perf_counter()
            dup = e.prop_duplicates(m)
            t2 = time.perf_counter()
            want = numpy_fold(np, abi, ov, obs, ms, hop, frm, dup, True, CAP)
            t3 = time.perf_counter()
            same_fold = same_fold and bool(np.array_equal(tags[0], want)) and not tags[1:].any()
            nonzero = int((want != 0).sum())
            vd, vw = timed(lambda: e.conn_values(value_ptr=d_val, protect_ptr=d_prot))
            td, tw = timed(lambda: e.conn_trim(LOW_WATER, trim_ptr=d_trim, node_trimmed_ptr=d_nt))
            got_trim = d_trim.cpu().numpy()
            t4 = time.perf_counter()
            val, prot = e.conn_values()
            pf = np.empty(E, dtype=np.uint8)
            sv = abi.StateView()
            sv.pair_flags = pf.ctypes.data_as(C.POINTER(C.c_uint8))
            e._chk(e.lib.gsx_export_state(e.h, C.byref(sv)), "gsx_export_state")
            t5 = time.perf_counter()
            want_trim = numpy_trim(np, abi, ov.row_ptr, obs, val, prot, pf, LOW_WATER)
            t6 = time.perf_counter()
            same_trim = same_trim and bool(np.array_equal(got_trim, want_trim))
            dd, dw = timed(lambda: e.tag_decay(1))
            same_fold = same_fold and bool(np.array_equal(e.tag_export()[0], np.maximum(want.astype(np.int16) - 1, 0)))
            for k, v in zip(t, (fd, fw, dd, dw, vd, vw, td, tw, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3,
                                (t3 - t0) * 1e3, (t5 - t4) * 1e3, (t6 - t5) * 1e3, (t6 - t4) * 1e3)):
                t[k].append(v)
        W = (m + 63) // 64
        values_bytes = E * (2 + 2 * T + 5)
        decay_bytes = tiles * T * 64
        rec[f"m_{m}"] = {
            "runs": runs, **{k: stat(v) for k, v in t.items()}, "pairs_with_a_tag": nonzero, "trimmed_pairs": int(got_trim.sum()),
            "fold_bytes_equal": same_fold, "trim_bytes_equal": same_trim, "words": W,
            "conn_values_bytes": values_bytes,
            "conn_values_TBps": values_bytes / (float(np.median(t["values_dev"])) * 1e-3) / 1e12,
            "tag_decay_read_bytes": decay_bytes,
            "tag_decay_read_TBps": decay_bytes / (float(np.median(t["decay_dev"])) * 1e-3) / 1e12,
            "fold_row_bytes": E * (8 + 3 * 8 * W),
            "fold_speedup_wall": float(np.median(t["today_fold_total"]) / np.median(t["fold_wall"])),
            "trim_speedup_wall": float(np.median(t["today_trim_total"]) / np.median(t["trim_wall"])),
        }
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--runs-large", type=int, default=5,
                    help="runs of the 1024-message batch (today's path takes minutes per run at 1M peers)")
    ap.add_argument("--step-timeout", type=int, default=1100, help="seconds for the child (its own timeout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tag_time.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child",
           "--peers", str(a.peers), "--topics", str(a.topics), "--runs", str(a.runs), "--runs-large", str(a.runs_large)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = [x for x in p.stdout.splitlines() if x.startswith("RECORD ")]
    if p.returncode != 0 or not line:
        print(f"the measurement ended with status {p.returncode}", file=sys.stderr)
        sys.exit(p.returncode or 1)
    rec = json.loads(line[-1][7:])
    print(json.dumps(rec), flush=True)
    doc = {"tool": "tools/tag_time.py", "device": "MI355X (gfx950)", "hbm_peak_Bps": HBM_PEAK,
           "timing": "gsx_tag_fold_prop, gsx_tag_decay, gsx_conn_values, gsx_conn_trim with device-pointer outputs: HIP events "
                     "(gsx_timing_begin/end) and wall clock of call + gsx_sync; today's path: wall clock of gsx_prop_results + "
                     "gsx_prop_duplicates + the numpy fold, and of the host copies + numpy's per-row selection; alternating "
                     "runs in one process after one warm-up; no pass bar",
           "workload": rec}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time gsx_prop_traffic against the route it replaces, on one engine.

For each propagation workload of the README (1M peers x 64 messages, 1M peers
x 1024 messages; gossipsub, the bench's overlay and state, first deliverers
tracked) a child process under its own `timeout`:
  * propagates one warm-up batch and the measured batch,
  * times gsx_prop_traffic with device-pointer outputs, HIP events around its
    memsets + kernels (gsx_timing_begin / gsx_timing_end), in --rounds
    alternating rounds over the variants: every output with NULL sizes, every
    output with sizes that use all 32 planes, the per-message table alone, and
    message + pair tables without the per-node ones (what the node atomics cost);
    median [min, max] per variant,
  * times the existing route once by wall clock: gsx_prop_results (first
    deliverers) + gsx_prop_duplicates through the host, then a numpy fold to
    the FIRST / DUP columns per message, node and pair, and checks them against
    the device's (that route cannot attribute graylisted copies: those columns
    and SENT are not compared),
  * counts the bytes the kernels have to read from the source: the occupied
    history rows (sset pass), and per sending pair and word one gathered sset
    row and the first-deliverer rows of the pair and of its reverse, plus the
    per-pair bytes (rev, rfwd, pin, pair_obs, col), plus the outputs.
The parent merges the children's records into profiles/prop_traffic_time.json.

    python tools/prop_traffic_time.py [--peers N] [--rounds R] [--no-route-above M] [--out FILE]
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
    K = abi.GSX_TRAFFIC_COLS
    th = abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                        accept_px_threshold=0, opportunistic_graft_threshold=0)
    e = bench.prop_engine(n, 0, n, 6, synth.SEED, 0, th, None)
    e.set_prop_tracking(True)  # (the bench's throughput setting is off)

    class A:
        prop_hops = 24

    cfg = bench.prop_config(A, n)
    e.propagate(bench.prop_messages(n, m, synth.SEED, first=0), cfg)  # warm-up: buffers, fwd / pin passes
    out = e.propagate(bench.prop_messages(n, m, synth.SEED, first=m), cfg)[0]
    E = e.n_pairs
    dev = "cuda:0"
    msg = torch.zeros((m, K), dtype=torch.int32, device=dev)
    node = torch.zeros((n, K), dtype=torch.int32, device=dev)
    nbytes = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    pair = torch.zeros(E, dtype=torch.int32, device=dev)
    pbytes = torch.zeros(E, dtype=torch.int64, device=dev)
    sizes = (np.uint64(1) << (np.arange(m, dtype=np.uint64) % np.uint64(32))).astype(np.uint32)
    sizes[::7] = 0xFFFFFFFF
    variants = (("all_outputs_null_sizes", None, (msg, node, nbytes, pair, pbytes)),
                ("all_outputs_32_planes", sizes, (msg, node, nbytes, pair, pbytes)),
                ("per_message_only", None, (msg, None, None, None, None)),
                ("message_and_pair_no_node", None, (msg, None, None, pair, pbytes)))
    torch.cuda.synchronize()
    for _, sz, ptrs in variants:  # warm-up of each kernel variant
        e.prop_traffic(m, sz, out_ptrs=ptrs)
    e.sync()
    ms_of = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, sz, ptrs in variants:
            e.timing_begin(1)
            e.prop_traffic(m, sz, out_ptrs=ptrs)
            e.sync()
            ms_of[name].append(e.timing_end()[0])
    rec = {"peers": n, "msgs": m, "pairs": int(E), "deliveries": int(out.deliveries), "duplicates": int(out.duplicates),
           "graylisted": int(out.graylisted), "transmissions": int(out.transmissions), "hops": int(out.hops)}
    for name, v in ms_of.items():
        rec[f"prop_traffic_ms_{name}"] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "calls": len(v)}
    e.prop_traffic(m, None, out_ptrs=(msg, node, nbytes, pair, pbytes))
    e.sync()
    g_msg = msg.cpu().numpy().view(np.uint32)
    g_node = node.cpu().numpy().view(np.uint32)
    g_pair = pair.cpu().numpy().view(np.uint32)
    S, F, D, G = abi.GSX_TRAFFIC_SENT, abi.GSX_TRAFFIC_FIRST, abi.GSX_TRAFFIC_DUP, abi.GSX_TRAFFIC_GRAYLISTED
    rec["identities"] = bool(
        g_msg.sum(0, dtype=np.int64).tolist() == [out.transmissions, out.deliveries, out.duplicates,
                                                   out.rejected + out.ignored, out.graylisted]
        and g_node.sum(0, dtype=np.int64).tolist() == g_msg.sum(0, dtype=np.int64).tolist()
        and int(g_pair.sum(dtype=np.int64)) == out.transmissions)
    # bytes counted from the source
    import ctypes as C

    W = abi.prop_words(m)
    hop = np.empty((m, n), dtype=np.uint8)
    e._chk(e.lib.gsx_prop_results(e.h, hop.ctypes.data_as(C.POINTER(C.c_uint8)), None), "gsx_prop_results")
    occ = np.zeros((n, 2), dtype=np.uint64)  # per node: the hops it was occupied at, as bits (hop 64 apart)
    for k in range(m):
        r = hop[k]
        occ[:, 0] |= np.where(r < 64, np.uint64(1) << (r & 63).astype(np.uint64), np.uint64(0))
        occ[:, 1] |= (r == 64).astype(np.uint64)
    rows = int(np.unpackbits(occ.view(np.uint8)).sum())
    del hop, occ
    sending = int(np.count_nonzero(g_pair))  # (a lower bound of the pairs whose reverse sends: those that carried a copy)
    b_sset = 8 * W * rows + 8 * W * n  # occupied history rows read, the scratch rows written
    b_pairs = E * 17 + sending * W * 24  # per pair rev + rfwd + pin + pair_obs + col; per sending pair and word three rows
    b_out = 4 * m * K + n * (4 * K + 16) + E * 12  # outputs zeroed / stored
    rec["bytes"] = {"sset_pass": b_sset, "pair_pass": b_pairs, "outputs": b_out, "total": b_sset + b_pairs + b_out,
                    "occupied_node_hops": rows, "pairs_with_copies": sending}
    t_all = rec["prop_traffic_ms_all_outputs_null_sizes"]["median"]
    rec["achieved_TBps"] = rec["bytes"]["total"] / (t_all * 1e-3) / 1e12
    rec["frac_of_8TBps"] = rec["bytes"]["total"] / (t_all * 1e-3) / HBM_PEAK
    rec["node_atomics_ms"] = t_all - rec["prop_traffic_ms_message_and_pair_no_node"]["median"]
    if m > a.no_route_above:
        rec["existing_route"] = f"not run above {a.no_route_above} messages"
        e.close()
        print("RECORD " + json.dumps(rec), flush=True)
        return
    # the existing route: first deliverers and duplicate rows through the host, then numpy
    ov = synth.connect_some_overlay(n, d=6, seed=synth.SEED)  # (bench.prop_engine's overlay: the user has it)
    t0 = time.perf_counter()
    _, frm = e.prop_results(m)
    dup = np.zeros((E, W), dtype=np.uint64)
    e._chk(e.lib.gsx_prop_duplicates(e.h, dup.ctypes.data_as(C.POINTER(C.c_uint64)), W), "gsx_prop_duplicates")
    t1 = time.perf_counter()
    obs = np.repeat(np.arange(n, dtype=np.int64), np.diff(ov.row_ptr))
    key = obs * n + ov.col  # ascending: rows ascending, each row's neighbours ascending
    w_msg = np.zeros((m, 2), dtype=np.int64)
    w_node = np.zeros((n, 2), dtype=np.int64)
    w_pair = np.zeros(E, dtype=np.int64)
    for k in range(m):
        if k % 128 == 0:
            print(f"[route] first deliverers of message {k} / {m}", file=sys.stderr, flush=True)
        us = np.nonzero(frm[k] >= 0)[0]
        q = np.searchsorted(key, us * n + frm[k, us])
        w_msg[k, 0] = len(us)
        w_node[:, 0] += np.bincount(us, minlength=n)
        w_pair += np.bincount(q, minlength=E)
    for w in range((m + 63) // 64):
        print(f"[route] duplicate rows, word {w}", file=sys.stderr, flush=True)
        col_w = np.ascontiguousarray(dup[:, w])
        for b in range(min(64, m - 64 * w)):
            w_msg[64 * w + b, 1] = int(((col_w >> np.uint64(b)) & np.uint64(1)).sum(dtype=np.int64))
        pd = np.unpackbits(col_w.view(np.uint8).reshape(E, 8), axis=1).sum(1, dtype=np.int64)
        w_pair += pd
        w_node[:, 1] += np.bincount(obs, weights=pd, minlength=n).astype(np.int64)
    t2 = time.perf_counter()
    rec["existing_route_ms"] = {"exports": (t1 - t0) * 1e3, "numpy_fold": (t2 - t1) * 1e3, "total": (t2 - t0) * 1e3, "runs": 1}
    rec["existing_route_note"] = ("gsx_prop_results + gsx_prop_duplicates + numpy: FIRST / DUP per message and node, "
                                  "first + duplicate copies per pair; it cannot attribute graylisted copies, so SENT, "
                                  "GRAYLISTED and the byte tables are not compared")
    gray_pair = g_pair.astype(np.int64) - w_pair  # what is left per pair must be the graylisted copies
    rec["exact_match"] = bool(np.array_equal(g_msg[:, [F, D]], w_msg) and np.array_equal(g_node[:, [F, D]], w_node)
                              and (gray_pair >= 0).all() and int(gray_pair.sum()) == out.graylisted
                              and np.array_equal(np.bincount(obs, weights=gray_pair, minlength=n).astype(np.int64),
                                                 g_node[:, G]))
    rec["speedup_over_existing_route"] = rec["existing_route_ms"]["total"] / t_all
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-route-above", type=int, default=1024, help="skip the existing route above this many messages")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds per workload (its own timeout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prop_traffic_time.json"))
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return child(a)
    recs = []
    for m in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(m),
               "--peers", str(a.peers), "--rounds", str(a.rounds), "--no-route-above", str(a.no_route_above)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [x for x in p.stdout.splitlines() if x.startswith("RECORD ")]
        if p.returncode != 0 or not line:
            print(f"workload {m} messages ended with status {p.returncode}; stopping", file=sys.stderr)
            sys.exit(p.returncode or 1)
        recs.append(json.loads(line[-1][7:]))
        print(json.dumps(recs[-1]), flush=True)
    doc = {"tool": "tools/prop_traffic_time.py", "device": "MI355X (gfx950)", "hbm_peak_Bps": HBM_PEAK,
           "timing": "gsx_prop_traffic: HIP events around its memsets + kernels (gsx_timing_begin/end), device-pointer "
                     "output, alternating rounds, median [min, max]; existing route: wall clock, once, same process",
           "workloads": recs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time gsx_score_parts against the route it replaces, on one engine.

A child process under its own `timeout` builds the bench's cfg3 state (1M peers
x 8 topics, one refresh) and
  * times gsx_score_parts with device-pointer outputs over --reps calls with
    HIP events (gsx_timing_begin / gsx_timing_end: memsets + kernel, per call),
    in three runs: the four tables only; the tables plus pair_cause /
    pair_topic; everything (plus pair_parts),
  * times the score-only k_refresh_score pass of the same state (the scores
    invalidated, gsx_settle_scores) with HIP events on the stream the engine is
    given: it reads the same records and is the bound to compare with,
  * times the route it replaces once by wall clock: gsx_peer_score_snapshot +
    gsx_export_state (every counter of every record through the host) and the
    numpy reference of the contract (tests/score_parts_model.py),
  * asserts that the two agree on every table, raw bytes,
  * counts the bytes the kernel has to read.
The parent writes the child's record to profiles/score_parts_time.json.

    python tools/score_parts_time.py [--peers N] [--topics T] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s: what frac_of_8TBps is a fraction of, whatever the device


def child(a):
    for p in (ROOT, os.path.join(ROOT, "go-libp2p-pubsub_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import numpy as np
    import torch

    import bench
    import score_parts_model as spm
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
    parts = torch.zeros((E, abi.GSX_PARTS), dtype=torch.float64, device=dev)
    cause = torch.zeros(E, dtype=torch.uint8, device=dev)
    worst = torch.zeros(E, dtype=torch.uint8, device=dev)
    ch = torch.zeros((B, abi.GSX_CAUSES), dtype=torch.int64, device=dev)
    th = torch.zeros((B, T + 1), dtype=torch.int64, device=dev)
    oc = torch.zeros((n, abi.GSX_CAUSES), dtype=torch.int32, device=dev)
    pe = torch.zeros((n, abi.GSX_CAUSES), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    runs = (("counts_only", (None, None, None, ch, th, oc, pe)),
            ("counts_and_pair_bytes", (None, cause, worst, ch, th, oc, pe)),
            ("everything", (parts, cause, worst, ch, th, oc, pe)))
    e.score_parts(edges, out_ptrs=runs[2][1])  # warm-up
    e.sync()
    prop = torch.cuda.get_device_properties(0)
    rec = {"device": f"{prop.name} ({getattr(prop, 'gcnArchName', '?').split(':')[0]})", "peers": n, "topics": T,
           "pairs": E, "edges": edges.tolist(), "select": "present"}
    for name, ptrs in runs:
        e.timing_begin(a.reps)
        for _ in range(a.reps):
            e.score_parts(edges, out_ptrs=ptrs)
        e.sync()
        tot, lo, hi, k = e.timing_end()
        rec[f"score_parts_ms_{name}"] = {"mean": tot / max(k, 1), "min": lo, "max": hi, "calls": k}

    # the score-only pass over the same state, on a stream the events can be recorded on
    st = torch.cuda.Stream()
    e.sync()
    e.set_stream(st.cuda_stream)
    zeros = np.zeros(E)
    ms = []
    for _ in range(a.reps + 1):
        e.set_app_scores(zeros)  # the same values: the scores are invalid, the state is as it was
        st.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(st)
        e.settle_scores()
        t1.record(st)
        st.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms = ms[1:]
    rec["score_only_pass_ms"] = {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms), "calls": len(ms)}
    ms = []
    for _ in range(a.reps + 1):  # the counts-only call between the same events
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(st)
        e.score_parts(edges, out_ptrs=runs[0][1])
        t1.record(st)
        st.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms = ms[1:]
    rec["score_parts_ms_counts_only_same_events"] = {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms),
                                                     "calls": len(ms)}
    e.set_stream(0)
    e.score_parts(edges, out_ptrs=runs[2][1])
    e.sync()
    got = {"pair_parts": parts.cpu().numpy(), "pair_cause": cause.cpu().numpy(), "pair_topic": worst.cpu().numpy(),
           "cause_hist": ch.cpu().numpy().view(np.uint64), "topic_hist": th.cpu().numpy().view(np.uint64),
           "obs_cause": oc.cpu().numpy().view(np.uint32), "peer_cause": pe.cpu().numpy().view(np.uint32)}
    marked = e.zero_map_marked()
    app_tiles = e.pair_zero_map_marked(abi.GSX_PZ_APP)

    # the route it replaces: every counter of every record through the host, then numpy
    t0 = time.perf_counter()
    rec_in, pair_in = spm.engine_inputs(e)
    t1 = time.perf_counter()
    tp = synth.spam_test_topic_params()
    want = spm.reference(rec_in, pair_in, synth.bench_peer_params(), {t: tp for t in range(T)}, T, ov.row_ptr, ov.col, n,
                         edges)
    t2 = time.perf_counter()
    rec["snapshot_and_export_ms"] = (t1 - t0) * 1e3
    rec["numpy_reference_ms"] = (t2 - t1) * 1e3
    rec["existing_route_ms"] = (t2 - t0) * 1e3
    bad = [f for f in spm.FIELDS if not spm.same_bytes(got[f], want[f])]
    assert not bad, f"gsx_score_parts differs from the numpy reference in {bad}"
    rec["exact_match"] = True
    rec["cause_totals"] = dict(zip(abi.CAUSE_NAMES, want["cause_hist"].sum(0).tolist()))

    # per pair: pair flags 1, bp 8, IP groups 8 (P6 is weighted), observer 4, peer 4; per record: fmd, mmd,
    # graftTime 8 each, flags 1; the marked zero-map entries' 64 x 8 B lines; the app scores of marked tiles
    b_counts = E * (1 + 8 + 8 + 4 + 4) + T * E * 25 + marked * 64 * 8 + app_tiles * 64 * 8 + 4 * 2 * n * abi.GSX_CAUSES
    b_bytes = b_counts + 2 * E
    b_all = b_bytes + 8 * abi.GSX_PARTS * E
    rec["bytes"] = {"counts_only": b_counts, "counts_and_pair_bytes": b_bytes, "everything": b_all,
                    "note": "loads per pair and record (zero-map-skipped counters not counted) + outputs written; the "
                            "per-group IP counts gathered for P6 and the peer view's atomics come on top"}
    for name, b in (("counts_only", b_counts), ("counts_and_pair_bytes", b_bytes), ("everything", b_all)):
        m = rec[f"score_parts_ms_{name}"]["mean"]
        rec.setdefault("achieved_GBps", {})[name] = b / (m * 1e-3) / 1e9
        rec.setdefault("frac_of_8TBps", {})[name] = b / (m * 1e-3) / HBM_PEAK
    rec["counts_only_over_score_only_pass"] = (rec["score_parts_ms_counts_only_same_events"]["mean"]
                                               / rec["score_only_pass_ms"]["mean"])
    rec["speedup_over_existing_route"] = rec["existing_route_ms"] / rec["score_parts_ms_counts_only"]["mean"]
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds for the child (its own timeout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_parts_time.json"))
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
    doc = {"tool": "tools/score_parts_time.py", "device": rec.pop("device"), "hbm_peak_Bps": HBM_PEAK,
           "timing": "gsx_score_parts: HIP events around its memsets + kernel (gsx_timing_begin/end), device-pointer "
                     "outputs; score-only pass: HIP events on the engine's stream around gsx_settle_scores after the "
                     "scores were invalidated, the counts-only call between the same events beside it; existing "
                     "route: wall clock of gsx_peer_score_snapshot + gsx_export_state + the numpy reference, same "
                     "process",
           "workload": rec}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

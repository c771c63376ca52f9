#!/usr/bin/env python3
"""Time gsx_timed_traffic against today's path, on one engine.

For 1M peers, d = 6, gossipsub (the bench's overlay and state), links of 1 .. 16
ticks and batches of 64 and 1024 messages, a child process under its own
`timeout` records, after one gsx_propagate_timed call,
  1. gsx_timed_traffic with every output on, and with only the per-message and
     per-bin outputs: device time of the whole call (HIP events of a
     gsx_timing_begin region: its memsets and its kernel), the two variants run
     alternately, `reps` times each after one warm-up of each; median, minimum
     and maximum,
  2. at 64 messages (1024 with --compare-all), today's path in the same process:
     gsx_timed_results + the exported state + a numpy reconstruction of the same
     nine tables, vectorised over the pairs, one message at a time; wall clock, and
     the tables asserted equal to the engine's.
The parent merges the records into profiles/timed_traffic_time.json.

    python tools/timed_traffic_time.py [--peers N] [--reps R] [--out FILE]
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
BIN_TICKS, N_BINS = 4, 32
NAMES = ("msg", "node", "node_bytes", "pair", "pair_bytes", "bins", "bin_bytes", "node_peak", "node_peak_bin")
# bytes the kernel loads per (pair, 64-message word), counted from its source: arr[v] 128, origin[v] 8, the
# first-deliverer words of the pair and of its reverse 16, two rfwd bytes, two latencies, rev and col 8
PAIR_WORD_BYTES = 128 + 8 + 16 + 2 + 2 + 8
# ... and per (node, word): arr[u] 128, origin[u] 8, the sizes 256, the drop word 8
NODE_WORD_BYTES = 128 + 8 + 256 + 8
HBM_PEAK = 8e12


def numpy_tables(np, abi, ov, st, scores, th, cfg, lat, ms, tick, frm, sizes, max_ticks, window_ns):
    """The nine tables from [message][node] arrival ticks and first deliverers, the exported state and
    the scores of the call's start: include/gsx.h's rule, one message at a time over all pairs."""
    n, E, m = ov.n, ov.n_pairs, len(ms)
    obs = ov.pair_observer().astype(np.int64)
    col = np.asarray(ov.col).astype(np.int64)
    key = obs * n + col
    assert (np.diff(key) > 0).all()
    rev = np.searchsorted(key, col * n + obs)
    has_rev = (rev < E) & (key[np.minimum(rev, E - 1)] == col * n + obs)
    rev = np.where(has_rev, rev, 0)
    pf, ef = st["pair_flags"], np.asarray(ov.edge_flags)
    both = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
    in_topic = (pf & both) == both
    in_mesh = (st["rec_flags"].reshape(-1, E)[cfg.topic] & abi.GSX_REC_IN_MESH) != 0
    direct = (ef & abi.GSX_EDGE_DIRECT) != 0
    flood_peer = (ef & abi.GSX_EDGE_GOSSIPSUB) == 0
    above = ~direct & (flood_peer | bool(cfg.flood_publish)) & (scores >= th.publish_threshold)
    fwd = in_topic & (direct | (flood_peer & above) | in_mesh)
    pub = in_topic & (direct | above) if cfg.flood_publish else fwd
    gin = ~direct & (scores < th.graylist_threshold)
    tick_ns = cfg.hop_latency_ns
    vd = cfg.validation_delay_ns // tick_ns
    lim = vd + window_ns // tick_ns
    lat = lat.astype(np.int64)
    sz = np.ones(m, dtype=np.int64) if sizes is None else sizes.astype(np.int64)
    T = {"msg": np.zeros((m, 7), np.int64), "node": np.zeros((n, 7), np.int64), "node_bytes": np.zeros((n, 2), np.int64),
         "pair": np.zeros(E, np.int64), "pair_bytes": np.zeros(E, np.int64), "bins": np.zeros((N_BINS, 7), np.int64),
         "bin_bytes": np.zeros((N_BINS, 2), np.int64)}
    node_bin = np.zeros((2, n * N_BINS), np.int64)
    u, v = obs, col  # pair q = (u -> v): the copy v sent u
    for k in range(m):
        src, ok = int(ms["source"][k]), int(ms["validation"][k]) == abi.GSX_VALIDATION_ACCEPT
        a = tick[k].astype(np.int64)
        own_v = v == src
        f = np.where(own_v, 0, a[v] + vd)
        sent = has_rev & (a[v] != 0xFFFF) & (own_v | ok) & np.where(own_v, pub[rev], fwd[rev]) & (frm[k][v] != u) & \
            (u != src) & (f <= max_ticks)
        q = np.nonzero(sent)[0]
        if not len(q):
            continue
        fq, at = f[q], f[q] + lat[q]
        arrived = at <= max_ticks
        gated = gin[q]
        first = arrived & ~gated & (frm[k][u[q]] == v[q])
        cls = np.where(~arrived, 5, np.where(gated, 4, np.where(first, 1 if ok else 3, 2)))
        inw = (cls == 2) & (at - a[u[q]] <= lim)
        sb, ab = np.minimum(fq // BIN_TICKS, N_BINS - 1), np.minimum(at // BIN_TICKS, N_BINS - 1)
        b = int(sz[k])
        cnt = np.bincount(cls, minlength=7)
        T["msg"][k] = cnt
        T["msg"][k, 0], T["msg"][k, 6] = len(q), int(inw.sum())
        T["node"][:, 0] += np.bincount(v[q], minlength=n)
        T["node"][:, 5] += np.bincount(v[q][~arrived], minlength=n)
        T["node_bytes"][:, 0] += b * np.bincount(v[q], minlength=n)
        T["bins"][:, 0] += np.bincount(sb, minlength=N_BINS)
        T["bins"][:, 5] += np.bincount(sb[~arrived], minlength=N_BINS)
        T["bin_bytes"][:, 0] += b * np.bincount(sb, minlength=N_BINS)
        node_bin[0] += b * np.bincount(v[q] * N_BINS + sb, minlength=n * N_BINS)
        qa, ua, aba, ca = q[arrived], u[q][arrived], ab[arrived], cls[arrived]
        for c in (1, 2, 3, 4):
            T["node"][:, c] += np.bincount(ua[ca == c], minlength=n)
            T["bins"][:, c] += np.bincount(aba[ca == c], minlength=N_BINS)
        T["node"][:, 6] += np.bincount(u[q][inw], minlength=n)
        T["bins"][:, 6] += np.bincount(ab[inw], minlength=N_BINS)
        T["node_bytes"][:, 1] += b * np.bincount(ua, minlength=n)
        T["bin_bytes"][:, 1] += b * np.bincount(aba, minlength=N_BINS)
        node_bin[1] += b * np.bincount(ua * N_BINS + aba, minlength=n * N_BINS)
        T["pair"][qa] += 1
        T["pair_bytes"][qa] += b
    nbv = node_bin.reshape(2, n, N_BINS)
    T["node_peak"] = nbv.max(2).T.copy()
    T["node_peak_bin"] = np.where(T["node_peak"] > 0, nbv.argmax(2).T, 0)
    return T


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
    cfg.credit_scores = abi.GSX_CREDIT_OFF
    ov = synth.connect_some_overlay(n, d=6, seed=synth.SEED)
    assert ov.n_pairs == e.n_pairs
    ms = bench.prop_messages(n, m, synth.SEED, first=m)
    lat = synth.link_latency(ov, synth.SEED, 1, 16)
    sizes = ((np.arange(m, dtype=np.uint64) * 977 + 13) % 1500 + 100).astype(np.uint32)
    max_ticks = 65534
    st0, s0 = e.export_state(), e.scores().copy()
    e.set_link_latency(lat)
    out = e.propagate_timed(ms, cfg, max_ticks)[0]
    words = (m + 63) // 64
    algo = PAIR_WORD_BYTES * int(e.n_pairs) * words + NODE_WORD_BYTES * n * words
    rec = {"peers": n, "msgs": m, "pairs": int(e.n_pairs), "reps": a.reps, "bin_ticks": BIN_TICKS, "n_bins": N_BINS,
           "ticks_run": int(out.ticks_run), "transmissions": int(out.transmissions),
           "algorithmic_load_bytes": algo, "byte_count": "counted from the kernel's source; no counter run backs it"}
    variants = {"all_outputs": dict(per_pair=True), "msg_and_bins_only": dict(outputs=["msg", "bins", "bin_bytes"])}
    res, times = {}, {k: [] for k in variants}
    for k, kw in variants.items():  # warm-up: the engine's staging buffers
        e.timed_traffic(m, sizes, BIN_TICKS, N_BINS, **kw)
    for _ in range(a.reps):
        for k, kw in variants.items():
            e.timing_begin(1)
            res[k] = e.timed_traffic(m, sizes, BIN_TICKS, N_BINS, **kw)
            e.sync()
            tot, _, _, cnt = e.timing_end()
            assert cnt == 1
            times[k].append(tot)
    for k, t in times.items():
        med = statistics.median(t)
        rec[k] = {"device_ms_median": med, "device_ms_min": min(t), "device_ms_max": max(t), "device_ms_runs": t,
                  "algorithmic_gb_per_s": algo / (med * 1e-3) / 1e9, "fraction_of_8_tb_per_s": algo / (med * 1e-3) / HBM_PEAK}
    full = res["all_outputs"]
    for f in ("msg", "bins", "bin_bytes"):
        assert np.array_equal(getattr(full, f), getattr(res["msg_and_bins_only"], f)), f
    s = full.msg.astype(np.int64).sum(0)
    assert s[0] - s[5] == out.transmissions and s[2] == out.duplicates and s[6] == out.dup_in_window
    rec["in_flight"] = int(s[5])
    if m == 64 or a.compare_all:
        t0 = time.perf_counter()
        tick, frm = e.timed_results(m)
        t1 = time.perf_counter()
        T = numpy_tables(np, abi, ov, st0, s0, th, cfg, lat, ms, tick, frm, sizes, max_ticks,
                         synth.spam_test_topic_params().mesh_message_deliveries_window_ns)
        t2 = time.perf_counter()
        for f in NAMES:
            got, want = getattr(full, f).astype(np.int64), T[f]
            assert got.shape == want.shape and np.array_equal(got, want), f
        rec["results_numpy"] = {"results_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3, "tables_equal": True,
                                "speedup_of_all_outputs": (t2 - t0) * 1e3 / rec["all_outputs"]["device_ms_median"]}
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds per workload (its own timeout)")
    ap.add_argument("--compare-all", action="store_true", help="run the numpy comparison at 1024 messages too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed_traffic_time.json"))
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return child(a)
    recs = []
    for m in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", str(m),
               "--peers", str(a.peers), "--reps", str(a.reps)] + (["--compare-all"] if a.compare_all else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [x for x in p.stdout.splitlines() if x.startswith("RECORD ")]
        if p.returncode != 0 or not line:
            print(f"workload {m} messages ended with status {p.returncode}; stopping", file=sys.stderr)
            sys.exit(p.returncode or 1)
        recs.append(json.loads(line[-1][7:]))
        print(json.dumps(recs[-1]), flush=True)
    doc = {"tool": "tools/timed_traffic_time.py", "device": "MI355X (gfx950), one GPU",
           "timing": "device_ms: HIP events around one whole gsx_timed_traffic call (its memsets and its kernel; the "
                     "upload of the sizes and the copies to host memory are outside), the two variants alternating, "
                     "`reps` runs each after one warm-up; results_numpy: wall clock of gsx_timed_results and of the "
                     "numpy reconstruction of the nine tables in the same process",
           "workloads": recs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

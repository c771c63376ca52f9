#!/usr/bin/env python3
"""Time gsx_mesh_stats against the route it replaces, on one engine.

A child process under its own `timeout` builds the bench's cfg3 state (1M peers
x 8 topics), runs two heartbeats, and after one warm-up call
  * times gsx_mesh_stats with device-pointer outputs over --reps alternating
    rounds with HIP events (gsx_timing_begin / gsx_timing_end, per call) for
    {totals and histograms}, {with the per-node tables} and {totals and
    histograms, symmetry off}: median [min, max],
  * times the route it replaces once by wall clock: gsx_export_state,
    gsx_export_backoff, gsx_export_membership and the numpy reduction to the
    same tables,
  * asserts that the two agree exactly (a mismatch ends the child: nothing is
    written),
  * counts the bytes the pair pass has to read from its source: per record the
    1-B flag; per pair the pair flags (1), edge flag (1), observer (4), peer (4),
    reverse index (4) and one backoff presence byte per eight topics; per
    connected pair the reverse pair's flag byte; per mesh link the reverse
    record's flag byte, and once per pair with a mesh link the 8-B score.
    These are counted, not counter-profiled, bytes.
The parent writes the child's record to profiles/mesh_stats_time.json.

    python tools/mesh_stats_time.py [--peers N] [--topics T] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def numpy_route(e, ov, gp, now, n_bins):
    """The tables from the host exports -> (dict, seconds per stage)."""
    import numpy as np

    from gsx import abi

    T, n, E = e.n_topics, ov.n, ov.n_pairs
    t0 = time.perf_counter()
    st = e.export_state()
    t1 = time.perf_counter()
    bo = e.export_backoff()
    t2 = time.perf_counter()
    joined, fanout, _ = e.export_membership()
    sc = e.scores()
    t3 = time.perf_counter()
    pc = (st["pair_flags"] & 3) == 3
    rf = st["rec_flags"].reshape(T, E)
    obs = np.repeat(np.arange(n, dtype=np.int64), np.diff(ov.row_ptr))
    col = ov.col.astype(np.int64)
    key = obs * n + col
    order = np.argsort(key)
    pos = np.searchsorted(key[order], col * n + obs)
    pos = np.minimum(pos, E - 1)
    rev = np.where(key[order][pos] == col * n + obs, order[pos], -1)
    outb = (ov.edge_flags & abi.GSX_EDGE_OUTBOUND) != 0
    tot = np.zeros((T, abi.GSX_MS_COLS), dtype=np.uint64)
    deg = np.zeros((T, n), dtype=np.uint32)
    outd, ind = np.zeros_like(deg), np.zeros_like(deg)
    hists = {f: np.zeros((T, n_bins), dtype=np.uint64) for f in ("deg_hist", "out_hist", "in_hist")}
    for t in range(T):
        mesh = pc & ((rf[t] & abi.GSX_REC_IN_MESH) != 0)
        deg[t] = np.bincount(obs[mesh], minlength=n)
        outd[t] = np.bincount(obs[mesh & outb], minlength=n)
        ind[t] = np.bincount(col[mesh], minlength=n)
        rmesh = np.where(rev >= 0, mesh[np.maximum(rev, 0)], False)
        unit = ((joined >> np.uint64(t)) & np.uint64(1)) != 0
        b = bo[t]
        fb = ((fanout >> np.uint64(t)) & np.uint64(1)) != 0
        tot[t] = [unit.sum(), (unit & (deg[t] == 0)).sum(), (unit & (deg[t] < gp.d_lo)).sum(),
                  (unit & (deg[t] > gp.d_hi)).sum(), (unit & (outd[t] < gp.d_out)).sum(), mesh.sum(),
                  (mesh & outb).sum(), (mesh & ~rmesh).sum(), (mesh & (sc < 0)).sum(),
                  (mesh & ((rf[t] & abi.GSX_REC_ACTIVE) != 0)).sum(), len(np.unique(obs[fb])), fb.sum(),
                  ((b != 0) & (b > now)).sum(), ((b != 0) & (b <= now)).sum(), 0, 0]
        for f, a in (("deg_hist", deg), ("out_hist", outd), ("in_hist", ind)):
            hists[f][t] = np.bincount(np.minimum(a[t][unit], n_bins - 1), minlength=n_bins)
    t4 = time.perf_counter()
    tabs = dict(topic_tot=tot, node_deg=deg, node_out=outd, node_in=ind, **hists)
    links = int(tot[:, abi.GSX_MS_LINKS].sum())
    return tabs, links, int(pc.sum()), {"export_state_ms": (t1 - t0) * 1e3, "export_backoff_ms": (t2 - t1) * 1e3,
                                        "export_membership_and_scores_ms": (t3 - t2) * 1e3,
                                        "numpy_reduction_ms": (t4 - t3) * 1e3, "existing_route_ms": (t4 - t0) * 1e3}


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "go-libp2p-pubsub_amd"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import torch

    import bench
    import oracle as orc
    from gsx import abi, synth

    n, T, B = a.peers, a.topics, 33
    ov, e = bench.build_engine(n, T, 6, synth.SEED, 0)
    e.set_thresholds(abi.Thresholds(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300,
                                    accept_px_threshold=0, opportunistic_graft_threshold=5))
    gp = orc.default_gossipsub_params()
    e.set_gossipsub_params(gp)
    e.refresh(bench.T0 + abi.SECOND)
    for k in (1, 2):
        e.heartbeat(k, bench.T0 + (1 + k) * abi.SECOND, 7)
    now = bench.T0 + 4 * abi.SECOND
    E, dev = ov.n_pairs, "cuda:0"
    tot = torch.zeros((T, 16), dtype=torch.int64, device=dev)
    hs = [torch.zeros((T, B), dtype=torch.int64, device=dev) for _ in range(3)]
    nd = [torch.zeros((T, n), dtype=torch.int32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    small = [tot] + hs + [None] * 6
    full = [tot] + hs + [None, None] + nd + [None]
    variants = (("totals_and_histograms", small, True), ("with_node_tables", full, True),
                ("totals_and_histograms_no_symmetry", small, False))
    e.mesh_stats(now, n_bins=B, out_ptrs=full)  # warm-up (allocates the engine's scratch)
    e.mesh_stats(now, n_bins=B, out_ptrs=small)
    e.sync()
    ms = {name: [] for name, _, _ in variants}
    for _ in range(a.reps):  # alternating rounds
        for name, ptrs, sym in variants:
            e.timing_begin(1)
            e.mesh_stats(now, n_bins=B, symmetry=sym, out_ptrs=ptrs)
            e.sync()
            ms[name].append(e.timing_end()[0])
    rec = {"peers": n, "topics": T, "pairs": E, "records": T * E, "n_bins": B, "reps": a.reps}
    for name, v in ms.items():
        rec[f"mesh_stats_ms_{name}"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    e.mesh_stats(now, n_bins=B, out_ptrs=full)
    e.sync()
    got = {"topic_tot": tot.cpu().numpy().view(np.uint64)}
    for f, x in zip(("deg_hist", "out_hist", "in_hist"), hs):
        got[f] = x.cpu().numpy().view(np.uint64)
    for f, x in zip(("node_deg", "node_out", "node_in"), nd):
        got[f] = x.cpu().numpy().view(np.uint32)
    want, links, connected, stages = numpy_route(e, ov, gp, now, B)
    bad = [f for f in want if not np.array_equal(got[f], want[f])]
    assert not bad, f"gsx_mesh_stats differs from the numpy reduction in {bad}"
    rec.update(stages)
    rec["exact_match"] = True
    rec["mesh_links"] = links
    b_rec, b_pair = T * E, E * (1 + 1 + 4 + 4 + 4 + (T + 7) // 8)
    b_link = connected + links + 8 * min(links, E)
    rec["bytes"] = {"record_flags": b_rec, "per_pair": b_pair, "per_link_gathers_upper_bound": b_link,
                    "total": b_rec + b_pair + b_link,
                    "note": "counted from the source, not counter-profiled; the score term is an upper bound "
                            "(8 B per mesh link: a pair in several meshes loads it once)"}
    t_ms = rec["mesh_stats_ms_totals_and_histograms"]["median"]
    rec["implied_GBps"] = (b_rec + b_pair + b_link) / (t_ms * 1e-3) / 1e9
    rec["frac_of_8TBps"] = (b_rec + b_pair + b_link) / (t_ms * 1e-3) / HBM_PEAK
    rec["speedup_over_existing_route"] = rec["existing_route_ms"] / rec["mesh_stats_ms_with_node_tables"]["median"]
    e.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=500, help="seconds for the child (its own timeout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_stats_time.json"))
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
    doc = {"tool": "tools/mesh_stats_time.py", "device": "MI355X (gfx950)", "hbm_peak_Bps": HBM_PEAK,
           "timing": "gsx_mesh_stats: HIP events around its clears + two kernels (gsx_timing_begin/end), device-pointer "
                     "outputs, alternating rounds after one warm-up; existing route: wall clock of gsx_export_state + "
                     "gsx_export_backoff + gsx_export_membership + gsx_scores + the numpy reduction, same process",
           "workload": rec}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

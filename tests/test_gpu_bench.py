"""bench.py's plain run: the headline alone, --steps timed steps, and with
--dump-outputs the scores of the last timed step, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SECONDARY = ("single_observer", "cpu_baseline", "parity_vs_oracle", "propagation", "heartbeat", "adversarial", "dropin")


def test_dump_sample_is_fixed_and_bounded():
    import bench

    assert bench.dump_sample(bench.DUMP_MAX_SCORES) is None  # a shard that fits is dumped whole
    n = bench.DUMP_MAX_SCORES + 12345
    a, b = bench.dump_sample(n), bench.dump_sample(n)
    assert np.array_equal(a, b)
    assert len(a) == bench.DUMP_MAX_SCORES and len(a) * 8 <= 64 * 2**20
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < n


@pytest.mark.gpu
def test_plain_run_dumps_last_step_scores(gpu_ok, tmp_path):
    import bench
    from gsx import abi

    n, T, steps, warmup = 3001, 3, 3, 2
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
         "--peers", str(n), "--topics", str(T), "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["unit"] == "peer-topic score updates/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    # value is the records of the timed steps over their time
    assert line["value"] == pytest.approx(line["config"]["records_per_gpu"] / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["roofline"]["kernel_avg_ms"] > 0
    assert all(line[k] is None for k in SECONDARY)
    assert os.listdir(tmp_path) == ["scores.npy"]
    got = np.load(tmp_path / "scores.npy")
    assert got.dtype == np.float64
    # the same engine, inputs and warmup + steps refreshes in this process
    _, e = bench.build_engine(n, T, 6, bench.synth.SEED, 0)
    now = bench.T0
    for _ in range(warmup + steps):
        now += abi.SECOND
        e.refresh(now)
    want = e.scores()
    e.close()
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.count_nonzero(want) > 0

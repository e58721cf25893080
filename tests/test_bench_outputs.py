"""bench.py's plain run and `--dump-outputs`: the plain run times exactly `--steps` steps and carries only the headline
(the roofline, the CPU baseline and the extra legs are `--full`'s), and the dump holds what the last timed step computed
-- float32 / float64 arrays, at most 64 MB in all, sampled at indices that depend on the array length only, the same
in every run up to rounding."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_sample_is_fixed_distinct_and_bounded():
    n = 3 * bench.DUMP_SAMPLE + 5
    t = torch.arange(n, dtype=torch.float64)  # (every index exact in float32: n < 2**24)
    a = bench.sampled(t, 1)
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,)
    assert (a == bench.sampled(t, 1)).all()
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < n
    assert not (a == bench.sampled(t, 2)).all()
    assert (bench.sampled(torch.arange(10.0), 1) == np.arange(10)).all()  # short arrays whole


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 5 and a.warmup == 2
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(gpu, tmp_path):
    line = _plain_run(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "utterances/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] - line["config"]["per_gpu_batch"] * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    assert line["roofline"] is None and "cpu_baseline" not in line and "extra_configs" not in line["config"]
    assert line["config"]["hip_graph_replays_in_timed_steps"] == 3  # no eager (profiled) step inside the timed region
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["disc_exp_avg.npy", "disc_grads.npy", "gen_exp_avg.npy", "gen_grads.npy", "loss_d.npy", "loss_g.npy"]
    total = 0
    for f in files:
        arr = np.load(tmp_path / "a" / f)
        assert arr.dtype in (np.float32, np.float64) and arr.size > 0 and np.isfinite(arr).all(), f
        total += arr.nbytes
    assert total <= 64 << 20
    for f in ("gen_grads.npy", "disc_grads.npy", "gen_exp_avg.npy", "disc_exp_avg.npy"):
        assert np.abs(np.load(tmp_path / "a" / f)).max() > 0, f
    # a second run with the same arguments computes the same outputs, up to the rounding of the atomic reductions (two
    # 40-step runs: at most 2e-5 relative; at a nonzero learning rate the arrays drift apart to tens of percent)
    _plain_run(tmp_path / "b")
    for f in files:
        a, b = (np.load(tmp_path / d / f).astype(np.float64) for d in ("a", "b"))
        assert np.linalg.norm(a - b) <= 1e-4 * np.linalg.norm(b), (f, np.linalg.norm(a - b) / np.linalg.norm(b))

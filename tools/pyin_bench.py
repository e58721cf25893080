"""pYIN pitch tracking on the GPU: one JSON line per workload -- 64 x 10 s and 1 x 600 s of 16 kHz audio (seeded harmonic
"speech" with vibrato, glides and pauses): ms per batch from device events after warm-up, audio seconds per second, and
the float64 oracle's CPU time on the first 10 s of the first utterance for context.

    python tools/pyin_bench.py [--iters 10] [--warmup 2] [--no-oracle]

Per-stage kernel times come from a kernel trace in a run of its own (the three kernels have stable names:
pyin_yin_kernel, pyin_obs_kernel, pyin_viterbi_kernel):

    rocprofv3 --kernel-trace --stats -d OUT -o pyin -- python tools/pyin_bench.py --iters 3 --warmup 1 --no-oracle
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 16000


def speech_like(seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * SR)
    t = np.arange(n) / SR
    # a syllable every ~0.25 s: base pitch drifts, vibrato, 20 % pauses
    syl = np.repeat(rng.uniform(90, 400, size=n // 4000 + 1), 4000)[:n]
    f = syl * (1 + 0.02 * np.sin(2 * np.pi * 5.3 * t))
    phase = 2 * np.pi * np.cumsum(f) / SR
    y = sum((0.6 ** k) * np.sin((k + 1) * phase) for k in range(5))
    gate = np.repeat(rng.uniform(size=n // 4000 + 1) > 0.2, 4000)[:n]
    return (0.2 * y * gate + 0.002 * rng.standard_normal(n)).astype(np.float32)


def run(B, seconds, iters, warmup, dev):
    from vcvits_amd import ops
    y = torch.from_numpy(np.stack([speech_like(seconds, s) for s in range(B)])).to(dev)
    for _ in range(warmup):
        ops.pyin(y)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        a.record()
        ops.pyin(y, check_finite=False)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return y, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pyin_bench: needs a GPU")
    dev = torch.device("cuda:0")
    oracle_s = None
    for B, seconds in ((64, 10.0), (1, 600.0)):
        y, times = run(B, seconds, args.iters, args.warmup, dev)
        ms = float(np.median(times))
        if oracle_s is None and not args.no_oracle:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import pyin_f64
            t0 = time.perf_counter()
            pyin_f64.pyin(y[0, :10 * SR].cpu().numpy())
            oracle_s = time.perf_counter() - t0
        print(json.dumps({"workload": "pyin %d x %g s @ 16 kHz" % (B, seconds), "ms_per_batch_median": round(ms, 3),
                          "ms_min": round(min(times), 3), "ms_max": round(max(times), 3), "iters": args.iters,
                          "audio_s_per_s": round(B * seconds / (ms / 1e3), 1),
                          "oracle_cpu_s_first_10s": None if oracle_s is None else round(oracle_s, 3),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()

"""Resampling and pitch shift on the GPU: one JSON line per workload -- `ops.resample` of 64 x 10 s at 48 kHz -> 16 kHz,
44.1 kHz -> 16 kHz and 16 kHz -> 48 kHz, and `ops.pitch_shift` of 64 x 10 s at 16 kHz for n_steps = +1 (16951 -> 16000, the
coprime worst case) and +12.  Per stage (each stage is one kernel launch): ms from device events after warm-up (median, min,
max over --iters), the bytes the stage has to move (input + output + table, from the shapes) and that traffic as a fraction
of the attainable HBM bandwidth (6.3 TB/s).  The last line times the torch-CPU restatement (tests/audio_fx_f64.py, dense
filter bank, float32) of ONE 10 s utterance at n_steps = +1 for context, in a child process -- or says that it could not.

    python tools/audio_fx_bench.py [--iters 10] [--warmup 2] [--no-cpu]

Kernel names for a trace in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/audio_fx_bench.py --no-cpu):
resample_table_kernel, resample_apply_kernel, stft_complex_fwd_generic_kernel, phase_vocoder_kernel, istft_ordered_kernel.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12
B, SECONDS = 64, 10.0


def signal(rate, seed):
    rng = np.random.default_rng(seed)
    n = int(SECONDS * rate)
    t = np.arange(n) / rate
    f = rng.uniform(100, 300) * (1 + 0.02 * np.sin(2 * np.pi * 5.3 * t))
    phase = 2 * np.pi * np.cumsum(f) / rate
    y = sum((0.6 ** k) * np.sin((k + 1) * phase) for k in range(5))
    return (0.2 * y + 0.002 * rng.standard_normal(n)).astype(np.float32)


def timed(stages, iters, warmup):
    """stages: [(name, fn(prev) -> out)] run in sequence; returns {name: [ms per iteration]}, the last outputs."""
    times = {name: [] for name, _ in stages}
    for it in range(warmup + iters):
        prev = None
        for name, fn in stages:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            prev = fn(prev)
            b.record()
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
    return times


def report(workload, times, nbytes, iters, whole=None):
    stages = {}
    for name, ms in times.items():
        med = float(np.median(ms))
        stages[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                        "mbytes": round(nbytes[name] / 1e6, 2),
                        "hbm_fraction": round(nbytes[name] / (med / 1e3) / HBM_BYTES_PER_S, 4)}
    total = sum(s["ms_median"] for s in stages.values())
    line = {"workload": workload, "ms_sum_of_stage_medians": round(total, 4)}
    if whole is not None:  # the public call: the same launches without an event pair and a synchronise around each
        total = float(np.median(whole))
        line.update({"ms_per_call_median": round(total, 4), "ms_per_call_min": round(min(whole), 4),
                     "ms_per_call_max": round(max(whole), 4),
                     "hbm_fraction_per_call": round(sum(nbytes.values()) / (total / 1e3) / HBM_BYTES_PER_S, 4)})
    line.update({"audio_s_per_s": round(B * SECONDS / (total / 1e3), 1), "stages": stages, "iters": iters,
                 "device": torch.cuda.get_device_name(0)})
    print(json.dumps(line), flush=True)


def bench_resample(orig, new, iters, warmup, dev):
    from vcvits_amd import ops
    x = torch.from_numpy(np.stack([signal(orig, s) for s in range(B)])).to(dev)
    c, first, taps = ops.resample_table(dev, orig, new)  # built once per rate pair; not part of the timed call
    times = timed([("resample_apply", lambda _: ops.resample(x, orig, new))], iters, warmup)
    out = ops.resample_out_len(x.shape[1], orig, new)
    nbytes = {"resample_apply": 4 * (x.numel() + B * out + taps.numel() + first.numel())}
    report("resample %d x %g s %d -> %d Hz (W = %d taps, %d phases)" % (B, SECONDS, orig, new, c["W"], c["n"]), times, nbytes,
           iters)


def bench_pitch_shift(n_steps, iters, warmup, dev, sr=16000, n_fft=512):
    from vcvits_amd import ops
    x = torch.from_numpy(np.stack([signal(sr, s) for s in range(B)])).to(dev)
    T, hop, nf = x.shape[1], n_fft // 4, n_fft // 2 + 1
    p = ops.pitch_shift_consts(T, sr, n_steps)
    c, first, taps = ops.resample_table(dev, p["orig_freq"], sr)
    F0 = T // hop + 1
    F1 = ops.phase_vocoder_frames(F0, p["rate"])
    stages = [("stft_complex", lambda _: ops.stft_complex(x, n_fft=n_fft, hop=hop, pad=n_fft // 2, reflect=True)),
              ("phase_vocoder", lambda s: ops.phase_vocoder(s, p["rate"], hop)),
              ("istft_ordered", lambda s: ops.istft_ordered(s, n_fft, p["len_stretch"])),
              ("resample_apply", lambda y: ops._resample_rows(y, None, p["orig_freq"], sr, T))]
    times = timed(stages, iters, warmup)
    whole = timed([("pitch_shift", lambda _: ops.pitch_shift(x, sr, n_steps))], iters, warmup)
    nbytes = {"stft_complex": 4 * B * T + 8 * B * nf * F0, "phase_vocoder": 8 * B * nf * (F0 + F1),
              "istft_ordered": 8 * B * nf * F1 + 4 * B * p["len_stretch"],
              "resample_apply": 4 * (B * p["len_stretch"] + B * T + taps.numel() + first.numel())}
    report("pitch_shift %d x %g s @ %d Hz, n_steps %+d (resample %d -> %d: W = %d taps, %d phases)"
           % (B, SECONDS, sr, n_steps, p["orig_freq"], sr, c["W"], c["n"]), times, nbytes, iters, whole["pitch_shift"])


_CPU_CHILD = r"""
import sys, time, torch
sys.path.insert(0, sys.argv[1])
import audio_fx_f64 as R
import numpy as np
torch.set_num_threads(int(sys.argv[2]))
R.DENSE_LIMIT = 1 << 62  # always the dense bank, as torchaudio forms it
x = torch.from_numpy((0.1 * np.random.default_rng(0).standard_normal(160000)).astype(np.float32))
t0 = time.perf_counter()
y = R.pitch_shift(x, 16000, 1, dtype=torch.float32)
print("%.3f" % (time.perf_counter() - t0))
"""


def cpu_dense_reference(threads=16, limit_s=420):
    try:
        r = subprocess.run([sys.executable, "-c", _CPU_CHILD, os.path.join(ROOT, "tests"), str(threads)], capture_output=True,
                           text=True, timeout=limit_s)
    except subprocess.TimeoutExpired:
        return {"cpu_s": None, "note": "did not finish in %d s" % limit_s}
    if r.returncode != 0:
        tail = (r.stderr.strip().splitlines() or ["killed"])[-1][:200]
        return {"cpu_s": None, "note": "could not run (exit %d): %s" % (r.returncode, tail)}
    return {"cpu_s": float(r.stdout.strip().splitlines()[-1]), "note": "dense [16000, 1, 16965] float32 bank"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("audio_fx_bench: needs a GPU")
    dev = torch.device("cuda:0")
    for orig, new in ((48000, 16000), (44100, 16000), (16000, 48000)):
        bench_resample(orig, new, args.iters, args.warmup, dev)
    for n_steps in (1, 12):
        bench_pitch_shift(n_steps, args.iters, args.warmup, dev)
    if not args.no_cpu:
        out = cpu_dense_reference()
        out["workload"] = "torch-CPU restatement, pitch_shift 1 x 10 s @ 16 kHz, n_steps +1, 16 threads"
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

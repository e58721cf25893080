"""Microbenchmark of the fused attention kernels (forward + backward) at the content encoder's shapes.
python tools/attn_bench.py [--dtype bf16] [--unfused] [--reps 20]

python tools/attn_bench.py --stream [--out profiles/attn_stream_bench.txt]: the no-grad forward without `attn`, the streamed
kernel (attention_stream.hip) against the path that runs today at the same shape (VCVITS_ATTN_STREAM_MIN_T = 0), alternating
in one process, three runs each, device events; median (min ... max), TFLOP/s as 4 B H T^2 dk / t, peak allocated bytes.

python tools/attn_bench.py --stream --bf16 [--out profiles/attn_stream_bf16_bench.txt]: the streamed forward in bf16 compute mode
with VCVITS_ATTN_STREAM_BF16 = 1 (attention_stream_bf16.hip, bf16 operands) against = 0 (the fp32-operand kernel, what bf16 mode
runs by default), alternating in one process, five runs each, device events; with --out the lines are appended.

python tools/attn_bench.py --stream-grad [--out profiles/attn_stream_grad_bench.txt]: forward + backward with want_attn=False at
p = 0 and p = 0.1, the streamed training kernels (attention_stream_grad.hip, VCVITS_ATTN_STREAM_GRAD_MIN_T = 1) against the path
that runs today (= 0) wherever that one can allocate, alternating, median of 3 from device events, peak allocated bytes, TFLOP/s
as (4 + 14) B H T^2 dk / t."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vcvits_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="f32")
ap.add_argument("--unfused", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--stream", action="store_true")
ap.add_argument("--stream-grad", action="store_true")
ap.add_argument("--bf16", action="store_true", help="with --stream: the bf16-operand streamed kernel against the fp32-operand one")
ap.add_argument("--out", default=None)
a = ap.parse_args()
ops.set_compute_dtype(a.dtype)
ops._ATTN_FUSED[0] = not a.unfused
dev = torch.device("cuda:0")

PEAK_F32_MFMA = 157.3  # TFLOP/s, v_mfma_f32_32x32x2_f32


def stream_leg():
    lines = ["# tools/attn_bench.py --stream --dtype %s: ops.rel_attention under no_grad, want_attn=False, ones mask, window 4." % a.dtype,
             "# today = VCVITS_ATTN_STREAM_MIN_T=0 (fused workgroup-per-tile kernel at T <= 896, the three-launch path past it);",
             "# streamed = VCVITS_ATTN_STREAM_MIN_T=1.  us per call: median (min ... max) of 3 runs, alternating, device events;",
             "# TFLOP/s = 4 B H T^2 dk / median; of peak: against %.1f TFLOP/s of fp32 MFMA; peak MB: allocated over one call." % PEAK_F32_MFMA]
    shapes = [(64, 4, 32, 500), (64, 4, 64, 500)]
    shapes += [(B, 4, dk, T) for T in (1000, 4000, 15000) for B in (1, 8) for dk in (32, 64)]
    old = ops._ATTN_STREAM_MIN_T[0]
    try:
        for B, H, dk, T in shapes:
            t = lambda *s: torch.randn(*s, device=dev)
            q, k, v = 2.0 * t(B, H * dk, T), t(B, H * dk, T), t(B, H * dk, T)
            ek, ev = t(1, 9, dk) * dk ** -0.5, t(1, 9, dk) * dk ** -0.5
            mask = torch.ones(B, T, device=dev)
            flops = 4.0 * B * H * T * T * dk
            # the three-launch path indexes its [B*H, T, T] tensors through int fields: not run past 2^31 elements
            legs = [("streamed", 1)] + ([("today", 0)] if B * H * T * T < 2 ** 31 else [])
            reps = max(2, min(10 * a.reps, int(4e12 / flops)))  # a timed window of tens of milliseconds at the least

            def call(min_t):
                ops._ATTN_STREAM_MIN_T[0] = min_t
                with torch.no_grad():
                    return ops.rel_attention(q, k, v, ek, ev, mask, H, 4, want_attn=False)[0]

            outs, times, peaks = {}, {n: [] for n, _ in legs}, {}
            for name, mt in legs:  # warm-up, peak memory of one call, and the outputs for the comparison
                call(mt)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.max_memory_allocated()
                outs[name] = call(mt)
                torch.cuda.synchronize()
                peaks[name] = torch.cuda.max_memory_allocated() - base
            for _ in range(3):
                for name, mt in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        call(mt)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
            diff = float((outs["streamed"] - outs["today"]).abs().max() / outs["today"].abs().max()) if "today" in outs else float("nan")
            for name, _ in legs:
                ts = sorted(times[name])
                lines.append("B=%-2d H=%d dk=%-2d T=%-5d %-8s %10.1f us (%9.1f ... %9.1f) %6.2f TFLOP/s %5.3f of peak  peak %9.1f MB  reps %d" % (
                    B, H, dk, T, name, ts[1], ts[0], ts[2], flops / ts[1] / 1e6, flops / ts[1] / 1e6 / PEAK_F32_MFMA, peaks[name] / 1e6, reps))
            if "today" in outs:
                lines.append("    streamed / today = %.3f of the time; max|streamed - today| / max|today| = %.1e" % (
                    sorted(times["streamed"])[1] / sorted(times["today"])[1], diff))
            else:
                lines.append("    today: not run (B H T^2 = %.2e elements is past the int indexing of the three-launch path; 2 x %.1f GB)" % (
                    B * H * T * T, B * H * T * T * 4 / 1e9))
            print("\n".join(lines[-3:]), flush=True)
            del outs
    finally:
        ops._ATTN_STREAM_MIN_T[0] = old
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def stream_bf16_leg():
    lines = ["# tools/attn_bench.py --stream --bf16: ops.rel_attention under no_grad, want_attn=False, ones mask, window 4, H = 4, bf16",
             "# compute mode, VCVITS_ATTN_STREAM_MIN_T=1.  fp32 = VCVITS_ATTN_STREAM_BF16=0 (rel_attn_stream_fwd_kernel, fp32 operands, the",
             "# default); bf16 = 1 (rel_attn_stream_fwd_bf16_kernel).  us per call: median (min ... max) of 5 runs after a warm-up call,",
             "# alternating in one process, device events; TFLOP/s = 4 B H T^2 dk / median; rel_l2: ||bf16 - fp32|| / ||fp32|| of the outputs."]
    shapes = [(B, 4, dk, T) for T in (1000, 4000, 15000) for B in (1, 8) for dk in (32, 64)]
    old = ops._ATTN_STREAM_MIN_T[0], ops._ATTN_STREAM_BF16[0], ops.compute_dtype()
    ops._ATTN_STREAM_MIN_T[0] = 1
    ops.set_compute_dtype("bf16")
    try:
        for B, H, dk, T in shapes:
            t = lambda *s: torch.randn(*s, device=dev)
            q, k, v = 2.0 * t(B, H * dk, T), t(B, H * dk, T), t(B, H * dk, T)
            ek, ev = t(1, 9, dk) * dk ** -0.5, t(1, 9, dk) * dk ** -0.5
            mask = torch.ones(B, T, device=dev)
            flops = 4.0 * B * H * T * T * dk
            reps = max(2, min(10 * a.reps, int(4e12 / flops)))  # a timed window of tens of milliseconds at the least
            legs = (("fp32", 0, "attn_stream"), ("bf16", 1, "attn_stream_bf16"))

            def call(sw):
                ops._ATTN_STREAM_BF16[0] = sw
                with torch.no_grad():
                    return ops.rel_attention(q, k, v, ek, ev, mask, H, 4, want_attn=False)[0]

            outs, times = {}, {n: [] for n, _, _ in legs}
            for name, sw, key in legs:  # warm-up, the outputs for the comparison, and that the leg ran the kernel it names
                before = ops.LAUNCH_COUNTS[key]
                outs[name] = call(sw)
                torch.cuda.synchronize()
                assert ops.LAUNCH_COUNTS[key] == before + 1, (name, key)
            for _ in range(5):
                for name, sw, _ in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        call(sw)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
            n0 = len(lines)
            for name, _, _ in legs:
                ts = sorted(times[name])
                lines.append("B=%-2d H=%d dk=%-2d T=%-5d %-5s %10.1f us (%9.1f ... %9.1f) %7.2f TFLOP/s  reps %d" % (
                    B, H, dk, T, name, ts[2], ts[0], ts[4], flops / ts[2] / 1e6, reps))
            lines.append("    bf16 / fp32 = %.3f of the time; rel_l2 = %.1e" % (
                sorted(times["bf16"])[2] / sorted(times["fp32"])[2], float((outs["bf16"] - outs["fp32"]).norm() / outs["fp32"].norm())))
            print("\n".join(lines[n0:]), flush=True)
            del outs
    finally:
        ops._ATTN_STREAM_MIN_T[0], ops._ATTN_STREAM_BF16[0] = old[0], old[1]
        ops.set_compute_dtype(old[2])
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def stream_grad_leg():
    lines = ["# tools/attn_bench.py --stream-grad --dtype %s: ops.rel_attention forward + backward, want_attn=False, ones mask, window 4." % a.dtype,
             "# today = VCVITS_ATTN_STREAM_GRAD_MIN_T=0 (fused kernels at T <= 896, the three-launch path past it); streamed = 1.",
             "# us per forward + backward: median (min ... max) of 3 runs, alternating, device events; TFLOP/s = 18 B H T^2 dk / median",
             "# (4 forward + 14 backward, the streamed count, for both legs); of peak: against %.1f TFLOP/s of fp32 MFMA;" % PEAK_F32_MFMA,
             "# peak MB: allocated over one forward + backward, inputs and dO not counted."]
    shapes = [(16, 4, dk, T) for dk in (64, 32) for T in (500, 1000, 2000)] + [(1, 4, dk, T) for T in (4000, 15000) for dk in (64, 32)]
    old = ops._ATTN_STREAM_GRAD_MIN_T[0]
    try:
        for B, H, dk, T in shapes:
            t = lambda *s: torch.randn(*s, device=dev)
            q, k, v = (2.0 * t(B, H * dk, T)).requires_grad_(True), t(B, H * dk, T).requires_grad_(True), t(B, H * dk, T).requires_grad_(True)
            ek, ev = (t(1, 9, dk) * dk ** -0.5).requires_grad_(True), (t(1, 9, dk) * dk ** -0.5).requires_grad_(True)
            gy = t(B, H * dk, T)
            mask = torch.ones(B, T, device=dev)
            flops = 18.0 * B * H * T * T * dk
            reps = max(2, min(50, int(2e12 / flops)))
            for p in (0.0, 0.1):
                def call(min_t):
                    ops._ATTN_STREAM_GRAD_MIN_T[0] = min_t
                    for x in (q, k, v, ek, ev):
                        x.grad = None
                    o, _ = ops.rel_attention(q, k, v, ek, ev, mask, H, 4, p, training=p > 0, want_attn=False)
                    o.backward(gy)

                legs, times, peaks, why = [("streamed", 1)], {}, {}, None
                if B * H * T * T >= 2 ** 31:
                    why = "B H T^2 = %.2e elements is past the int indexing of the three-launch path" % (B * H * T * T)
                else:
                    legs.append(("today", 0))
                for name, mt in list(legs):  # warm-up and the peak memory of one forward + backward
                    try:
                        call(mt)
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        call(mt)
                        torch.cuda.synchronize()
                        peaks[name] = torch.cuda.max_memory_allocated() - base
                        times[name] = []
                    except torch.cuda.OutOfMemoryError as e:
                        legs.remove((name, mt))
                        why = "out of memory (%s)" % str(e).split(".")[0]
                        torch.cuda.empty_cache()
                for _ in range(3):
                    for name, mt in legs:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(reps):
                            call(mt)
                        e1.record()
                        torch.cuda.synchronize()
                        times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
                n0 = len(lines)
                for name, _ in legs:
                    ts = sorted(times[name])
                    lines.append("B=%-2d H=%d dk=%-2d T=%-5d p=%-3g %-8s %10.1f us (%9.1f ... %9.1f) %6.2f TFLOP/s %5.3f of peak  peak %9.1f MB  reps %d" % (
                        B, H, dk, T, p, name, ts[1], ts[0], ts[2], flops / ts[1] / 1e6, flops / ts[1] / 1e6 / PEAK_F32_MFMA, peaks[name] / 1e6, reps))
                if "today" in times and "streamed" in times:
                    lines.append("    streamed / today = %.3f of the time, %.4f of the memory" % (
                        sorted(times["streamed"])[1] / sorted(times["today"])[1], peaks["streamed"] / max(peaks["today"], 1)))
                else:
                    lines.append("    today: not run (%s)" % why)
                print("\n".join(lines[n0:]), flush=True)
    finally:
        ops._ATTN_STREAM_GRAD_MIN_T[0] = old
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if a.stream:
    stream_bf16_leg() if a.bf16 else stream_leg()
    sys.exit(0)
if a.stream_grad:
    stream_grad_leg()
    sys.exit(0)
for name, B, H, dk, T in (("base B16", 16, 4, 64, 204), ("base B32", 32, 4, 64, 204), ("48k B16", 16, 4, 32, 204), ("infer 48k", 64, 4, 32, 500)):
    t = lambda *s: torch.randn(*s, device=dev)
    q, k, v, gy = (t(B, H * dk, T).requires_grad_(True) for _ in range(4))
    ek, ev = t(1, 9, dk).requires_grad_(True), t(1, 9, dk).requires_grad_(True)
    mask = torch.ones(B, T, device=dev)

    def fwd():
        with torch.no_grad():
            return ops.rel_attention(q, k, v, ek, ev, mask, H, 4, want_attn=False)

    def fb():
        o, _ = ops.rel_attention(q, k, v, ek, ev, mask, H, 4, 0.1, training=True, want_attn=False)
        o.backward(gy)

    import ctypes
    from vcvits_amd import _lib
    LIB = _lib.lib()
    res = []
    for f, mult in ((fwd, 1.0), (fb, 3.0)):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        LIB.vcv_prof_begin(8 * a.reps + 8)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            f()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.reps
        out = (ctypes.c_double * 15)()
        LIB.vcv_prof_end(out, 5)
        kern = (out[1] + out[13]) / a.reps * 1e-3 if (out[0] + out[12]) > 0 else float("nan")  # GPU time of the GEMM-shaped launches
        flops = mult * 4.0 * B * H * T * T * dk
        res.append((dt * 1e6, flops / dt / 1e12, kern * 1e6, flops / kern / 1e12))
    print("%-10s B=%d H=%d dk=%d T=%d | fwd %7.1f us wall, %7.1f us in the kernels: %6.1f TFLOP/s | fwd+bwd %7.1f us wall, %7.1f us in the kernels: %6.1f TFLOP/s" % (
        name, B, H, dk, T, res[0][0], res[0][2], res[0][3], res[1][0], res[1][2], res[1][3]))

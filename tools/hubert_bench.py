"""Throughput of the HuBERT feature extractor (vcvits_amd/model/hubert.py) on one GPU: base widths with 12 layers and
xtralarge widths with 48 layers, random weights, a batch of equal-length rows, in fp32 mode and in bf16 mode.

One JSON line per (architecture, mode):
  ms_per_batch, audio_s_per_s     wall time of extract_features between device events around `--steps` calls
  classes_ms                      per kernel class, from a separate pass with an event pair around every launch wrapper:
                                  conv front end (layer 0, C_in = 1, apart), GroupNorm / LayerNorm + GELU of the front end,
                                  GELU passes, GEMMs (the 1-tap convs), the grouped position conv, attention, residual + LayerNorm
  attention_mfma_fraction         4 B H T'^2 d flops per call over the attention time, against the fp32-input MFMA peak
                                  (157.3 TFLOP/s: the attention kernel runs on that pipe in both modes)
  groupnorm_hbm_fraction          read once + write once (8 bytes per element) over the GroupNorm + GELU time of conv layer 0,
                                  against 8 TB/s (base only; the kernel's second read is served by L2 while a row fits)

    python tools/hubert_bench.py [--arch base,xtralarge] [--batch 16] [--seconds 10] [--modes f32,bf16] [--out FILE]

--ragged replaces those lines by one line per mode for rows of unequal length (base widths, 12 layers, 16 rows whose padded
lengths are spread evenly over 3 to 10 s), extract_features(lengths=) and preprocess.hubert_features_batch:
  files      audio-s/s of hubert_features_batch over the 16 files against hubert_features file by file (wall time, host
             copies included: what filling the feature cache costs)
  padded     ms per batch of the padded [16, 10 s] batch with lengths= and without (without, the rows are not the rows alone)
  equal      ms per batch of 16 equal rows of 10 s with lengths= (all rows full) and without
Every pair is measured as alternating runs in one process, three each; the median and the range (min, max) are reported.

--attn-bf16 replaces them by one line: bf16 mode with VCVITS_ATTN_STREAM_BF16 = 0 (the fp32-operand attention kernel, the
default) and = 1 (the bf16-operand kernel, attention_stream_bf16.hip) at one architecture (--arch, default base: 12 layers) and
--batch x --seconds, alternating in one process, five runs of --steps calls each after --warmup calls: ms per batch, the attention
class of a separate pass with an event pair around every launch wrapper, and the relative L2 distance of the two outputs.

There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vcvits_amd import ops  # noqa: E402
from vcvits_amd.model.hubert import HubertFeatureExtractor  # noqa: E402

ARCHS = {
    "base": dict(conv_dim=512, embed_dim=768, ffn_dim=3072, layers=12, heads=12, extractor_mode="default",
                 layer_norm_first=False, conv_bias=False),
    "xtralarge": dict(conv_dim=512, embed_dim=1280, ffn_dim=5120, layers=48, heads=16, extractor_mode="layer_norm",
                      layer_norm_first=True, conv_bias=True),
}
PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12


class Classes:
    """Event pairs around the launch wrappers the model calls, summed per kernel class."""

    def __init__(self):
        self.events, self.saved = [], {}

    def _wrap(self, name, classify):
        fn = getattr(ops, name)

        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            self.events.append((classify(a, kw), e0, e1))
            return out

        self.saved[name] = ops.replace(name, timed)

    def __enter__(self):
        def conv_class(a, kw):
            w = a[1]
            if kw.get("groups", 1) > 1:
                return "pos_conv"
            if w.shape[2] == 1:
                return "gemm"
            return "conv_frontend_layer0" if w.shape[1] == 1 else "conv_frontend_layers1_6"

        self._wrap("conv_forward", conv_class)
        self._wrap("groupnorm_gelu", lambda a, kw: "frontend_norm_gelu")
        self._wrap("layernorm_c_gelu", lambda a, kw: "frontend_norm_gelu")
        self._wrap("bias_gelu", lambda a, kw: "gelu")
        self._wrap("hubert_attention_qkv", lambda a, kw: "attention")
        self._wrap("layernorm_c", lambda a, kw: "layernorm")
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            ops.replace(name, fn)

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for cls, e0, e1 in self.events:
            out[cls] = out.get(cls, 0.0) + e0.elapsed_time(e1)
        return out


def bench(arch, mode, batch, seconds, steps, warmup):
    torch.manual_seed(0)
    model = HubertFeatureExtractor(**ARCHS[arch]).to("cuda")
    T = int(seconds * 16000)
    frames = model.out_frames(T)
    src = (0.1 * torch.randn(batch, T, generator=torch.Generator().manual_seed(1))).to("cuda")
    ops.set_compute_dtype("bf16" if mode == "bf16" else "f32")
    try:
        for _ in range(warmup):
            model.extract_features(src)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            out, _ = model.extract_features(src)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        with Classes() as c:
            model.extract_features(src)
            cls = c.totals()
        # the GroupNorm + GELU launch alone (base: conv layer 0's output)
        gn = None
        if ARCHS[arch]["extractor_mode"] == "default":
            t0 = (T - 10) // 5 + 1
            x = torch.randn(batch, 512, t0, device="cuda")
            g, b = torch.ones(512, device="cuda"), torch.zeros(512, device="cuda")
            for _ in range(2):
                ops.groupnorm_gelu(x, g, b)
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0.record()
            for _ in range(5):
                ops.groupnorm_gelu(x, g, b)
            g1.record()
            torch.cuda.synchronize()
            gn_ms = g0.elapsed_time(g1) / 5
            gn = {"ms": round(gn_ms, 4), "elements": x.numel(),
                  "groupnorm_hbm_fraction": round(8.0 * x.numel() / (gn_ms * 1e-3) / PEAK_HBM, 4)}
            del x
    finally:
        ops.set_compute_dtype("f32")
    a = ARCHS[arch]
    d = a["embed_dim"] // a["heads"]
    attn_flops = 4.0 * batch * a["heads"] * frames * frames * d * a["layers"]
    line = {"tool": "hubert_bench", "arch": arch, "mode": mode, "layers": a["layers"], "batch": batch, "seconds": seconds,
            "frames": frames, "ms_per_batch": round(ms, 3), "audio_s_per_s": round(batch * seconds / (ms * 1e-3), 1),
            "classes_ms": {k: round(v, 3) for k, v in sorted(cls.items())},
            "attention_mfma_fraction": round(attn_flops / (cls["attention"] * 1e-3) / PEAK_F32_MFMA, 4),
            "finite": bool(torch.isfinite(out).all()), "device": torch.cuda.get_device_name(0)}
    if gn is not None:
        line["groupnorm_gelu_layer0"] = gn
    return line


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def _alternate(fa, fb, runs=3):
    """fa and fb (each returns one figure) as alternating runs; (stats of fa, stats of fb)"""
    a, b = [], []
    for _ in range(runs):
        a.append(fa())
        b.append(fb())
    return _stats(a), _stats(b)


def attn_bf16(arch, batch, seconds, steps, warmup):
    torch.manual_seed(0)
    model = HubertFeatureExtractor(**ARCHS[arch]).to("cuda")
    T = int(seconds * 16000)
    src = (0.1 * torch.randn(batch, T, generator=torch.Generator().manual_seed(1))).to("cuda")
    old = ops._ATTN_STREAM_BF16[0]
    ops.set_compute_dtype("bf16")

    def per_batch(sw):
        def run():
            ops._ATTN_STREAM_BF16[0] = sw
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                model.extract_features(src)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps
        return run

    try:
        outs, attn_ms, launches = {}, {}, {}
        for sw in (0, 1):
            ops._ATTN_STREAM_BF16[0] = sw
            for _ in range(warmup):
                model.extract_features(src)
            before = ops.LAUNCH_COUNTS["attn_stream_bf16"]
            with Classes() as c:
                outs[sw] = model.extract_features(src)[0]
                attn_ms[sw] = c.totals()["attention"]
            launches[sw] = ops.LAUNCH_COUNTS["attn_stream_bf16"] - before
        off, on = _alternate(per_batch(0), per_batch(1), runs=5)
    finally:
        ops._ATTN_STREAM_BF16[0] = old
        ops.set_compute_dtype("f32")
    a = ARCHS[arch]
    assert launches == {0: 0, 1: a["layers"]}, launches
    d = a["embed_dim"] // a["heads"]
    frames = model.out_frames(T)
    attn_flops = 4.0 * batch * a["heads"] * frames * frames * d * a["layers"]
    return {"tool": "hubert_bench", "leg": "attn_bf16", "arch": arch, "mode": "bf16", "layers": a["layers"], "batch": batch,
            "seconds": seconds, "frames": frames, "head_dim": d,
            "ms_per_batch": {"switch_0_fp32_operands": off, "switch_1_bf16_operands": on},
            "attention_ms": {"switch_0_fp32_operands": round(attn_ms[0], 3), "switch_1_bf16_operands": round(attn_ms[1], 3)},
            "attention_tflops": {"switch_0_fp32_operands": round(attn_flops / (attn_ms[0] * 1e-3) / 1e12, 1),
                                 "switch_1_bf16_operands": round(attn_flops / (attn_ms[1] * 1e-3) / 1e12, 1)},
            "rel_l2_on_vs_off": float((outs[1] - outs[0]).norm() / outs[0].norm()),
            "finite": bool(torch.isfinite(outs[1]).all()), "device": torch.cuda.get_device_name(0)}


def ragged(mode, steps, warmup, rows=16, shortest=3.0, longest=10.0):
    import time

    from vcvits_amd.preprocess import hubert_features, hubert_features_batch
    torch.manual_seed(0)
    model = HubertFeatureExtractor(**ARCHS["base"]).to("cuda")
    g = torch.Generator().manual_seed(1)
    # padded rows (40 + 40 samples around a file) of 3 .. 10 s: the longest batch is the default budget of 16 x 10 s
    lengths = [int(round((shortest + (longest - shortest) * i / (rows - 1)) * 16000)) for i in range(rows)]
    audios = [0.1 * torch.randn(1, n - 80, generator=g) for n in lengths]
    T = lengths[-1]
    padded = torch.zeros(rows, T)
    for b, a in enumerate(audios):
        padded[b, 40:40 + a.shape[1]] = a[0]
    padded = padded.to("cuda")
    equal = (0.1 * torch.randn(rows, T, generator=g)).to("cuda")
    audio_s = sum(lengths) / 16000.0

    def wall(fn):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return audio_s / (time.perf_counter() - t0)
        return run

    def per_batch(src, lens):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                model.extract_features(src, lengths=lens)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps
        return run

    ops.set_compute_dtype("bf16" if mode == "bf16" else "f32")
    try:
        legs = {"files": (wall(lambda: hubert_features_batch(model, audios)), wall(lambda: [hubert_features(model, a) for a in audios])),
                "padded": (per_batch(padded, lengths), per_batch(padded, None)),
                "equal": (per_batch(equal, [T] * rows), per_batch(equal, None))}
        out = {}
        for name, (fa, fb) in legs.items():
            for _ in range(warmup):
                fa()
                fb()
            out[name] = _alternate(fa, fb)
        feats, pm = model.extract_features(padded, lengths=lengths)
        finite = bool(torch.isfinite(feats).all())
    finally:
        ops.set_compute_dtype("f32")
    return {"tool": "hubert_bench", "leg": "ragged", "arch": "base", "mode": mode, "layers": ARCHS["base"]["layers"], "rows": rows,
            "row_seconds": [shortest, longest], "audio_s": round(audio_s, 2), "valid_fraction": round(sum(lengths) / (rows * T), 3),
            "files_audio_s_per_s": {"hubert_features_batch": out["files"][0], "hubert_features_one_at_a_time": out["files"][1]},
            "padded_ms_per_batch": {"lengths": out["padded"][0], "no_lengths": out["padded"][1]},
            "equal_ms_per_batch": {"lengths_all_full": out["equal"][0], "no_lengths": out["equal"][1]},
            "finite": finite, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="base,xtralarge")
    ap.add_argument("--modes", default="f32,bf16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--ragged", action="store_true", help="the rows-of-unequal-length leg (base x 12 layers) instead")
    ap.add_argument("--attn-bf16", action="store_true", help="bf16 mode with VCVITS_ATTN_STREAM_BF16 = 0 and 1 instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hubert_bench: no GPU (there is no CPU path to time)")
    if args.attn_bf16:
        for arch in (args.arch.split(",") if args.arch != "base,xtralarge" else ["base"]):
            line = json.dumps(attn_bf16(arch, args.batch, args.seconds, args.steps, args.warmup))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            torch.cuda.empty_cache()
        return 0
    if args.ragged:
        for mode in args.modes.split(","):
            line = json.dumps(ragged(mode, args.steps, args.warmup))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            torch.cuda.empty_cache()
        return 0
    for arch in args.arch.split(","):
        for mode in args.modes.split(","):
            line = json.dumps(bench(arch, mode, args.batch, args.seconds, args.steps, args.warmup))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())

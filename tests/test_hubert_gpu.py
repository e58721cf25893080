"""GPU: the HuBERT feature extractor (vcvits_amd/model/hubert.py over csrc/hubert.hip and the conv kernels) against the
float64 restatement of fairseq's extract_features (tests/hubert_f64.py), on seeded weights and inputs.

Distances are relative L2 (max-abs printed alongside) to the FLOAT64 restatement.
  fp32 mode: <= 1e-4 (the project's fp32 bar).
  bf16 mode: <= 2 x the distance of the restatement run under torch.autocast("cpu", torch.bfloat16).
The float32 restatement's own distance is recorded next to the GPU's in profiles/hubert_parity.txt."""
import functools
import os

import pytest
import torch

import hubert_f64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_BOUND = 1e-4
_parity = {}

VARIANTS = {
    "A": dict(extractor_mode="default", conv_dim=64, embed_dim=128, ffn_dim=256, layers=2, conv_bias=False, heads=2, pre=False),
    "B": dict(extractor_mode="layer_norm", conv_dim=64, embed_dim=160, ffn_dim=320, layers=2, conv_bias=True, heads=2, pre=True),
    "base": dict(extractor_mode="default", conv_dim=512, embed_dim=768, ffn_dim=3072, layers=2, conv_bias=False, heads=12, pre=False),
    "xtralarge": dict(extractor_mode="layer_norm", conv_dim=512, embed_dim=1280, ffn_dim=5120, layers=2, conv_bias=True, heads=16, pre=True),
}


def _record(section, line):
    """Keep the printed figures in profiles/hubert_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "hubert_parity.txt"), "w") as f:
        f.write("# tests/test_hubert_gpu.py: relative L2 (max abs) distance from the float64 restatement (tests/hubert_f64.py):\n"
                "# the GPU model next to the float32 restatement (fp32 mode, asserted gpu <= 1e-4) or next to the restatement\n"
                "# under bf16 autocast (bf16 mode, asserted gpu <= 2 * ref).\n")
        for name in sorted(_parity):
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def _samples(frames):
    return 400 + 320 * (frames - 1)


@functools.lru_cache(maxsize=None)
def _sd(variant):
    v = VARIANTS[variant]
    return R.random_state_dict(1234 + len(variant), extractor_mode=v["extractor_mode"], conv_dim=v["conv_dim"],
                               embed_dim=v["embed_dim"], ffn_dim=v["ffn_dim"], layers=v["layers"], conv_bias=v["conv_bias"])


def _cfg(variant):
    v = VARIANTS[variant]
    return dict(extractor_mode=v["extractor_mode"], layer_norm_first=v["pre"], num_heads=v["heads"])


@functools.lru_cache(maxsize=None)
def _source(B, frames):
    g = torch.Generator().manual_seed(100 * B + frames)
    t = torch.arange(_samples(frames), dtype=torch.float64) / 16000.0
    rows = [0.3 * torch.sin(2 * torch.pi * (110.0 * (b + 1)) * t) + 0.1 * torch.randn(t.shape, generator=g, dtype=torch.float64)
            for b in range(B)]
    return torch.stack(rows).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _ref(variant, B, frames, output_layer, mode):
    """The restatement's output (float64 tensor), computed once per case and shared; never modified."""
    return R.run(_sd(variant), _source(B, frames), mode, output_layer=output_layer, **_cfg(variant))


_models = {}


def _model(variant, gpu):
    from vcvits_amd.model.hubert import HubertFeatureExtractor
    if variant not in _models:
        _models[variant] = HubertFeatureExtractor.from_state_dict(_sd(variant), heads=VARIANTS[variant]["heads"]).to(gpu)
    return _models[variant]


def _check_fp32(variant, B, frames, output_layer, gpu):
    out, pm = _model(variant, gpu).extract_features(_source(B, frames).to(gpu), output_layer=output_layer)
    assert pm is None and out.dtype == torch.float32
    ref = _ref(variant, B, frames, output_layer, "f64")
    assert tuple(out.shape) == tuple(ref.shape) == (B, frames, VARIANTS[variant]["embed_dim"])
    ref32 = _ref(variant, B, frames, output_layer, "f32")
    d_gpu, d_ref = R.rel_l2(out.cpu(), ref), R.rel_l2(ref32, ref)
    _record("fp32 mode", "%-9s B=%d T'=%-4d output_layer=%-4s gpu %.3e (%.3e)   float32 restatement %.3e (%.3e)   ratio %.2f"
            % (variant, B, frames, output_layer, d_gpu, R.max_abs(out.cpu(), ref), d_ref, R.max_abs(ref32, ref), d_gpu / d_ref))
    assert torch.isfinite(out).all()
    assert d_gpu <= FP32_BOUND


@pytest.mark.parametrize("output_layer", [None, 1])
@pytest.mark.parametrize("frames", [1, 37, 130, 1030])
@pytest.mark.parametrize("variant", ["A", "B"])
def test_small_widths_fp32(gpu, variant, frames, output_layer):
    """real head dims (2 x 64, 2 x 80) at toy widths; T' = a single frame, a partial tile, one past a 128-query block, and
    many key tiles with a ragged last one"""
    _check_fp32(variant, 3, frames, output_layer, gpu)


@pytest.mark.parametrize("variant", ["base", "xtralarge"])
def test_full_widths_fp32(gpu, variant):
    """the real conv and GEMM shapes (C_in = 1 first layer, 48- and 80-channel position-conv groups), 2 layers, 1 s of audio"""
    _check_fp32(variant, 1, 49, None, gpu)


@pytest.mark.parametrize("variant,frames", [("A", 130), ("B", 37)])
def test_bf16_mode(gpu, variant, frames):
    from vcvits_amd import ops
    ref = _ref(variant, 3, frames, None, "f64")
    d_ref = R.rel_l2(_ref(variant, 3, frames, None, "bf16"), ref)
    ops.set_compute_dtype("bf16")
    try:
        out, _ = _model(variant, gpu).extract_features(_source(3, frames).to(gpu))
        out = out.cpu()
    finally:
        ops.set_compute_dtype("f32")
    d_gpu = R.rel_l2(out, ref)
    _record("bf16 mode", "%-9s B=3 T'=%-4d gpu %.3e (%.3e)   bf16-autocast restatement %.3e (%.3e)"
            % (variant, frames, d_gpu, R.max_abs(out, ref), d_ref, R.max_abs(_ref(variant, 3, frames, None, "bf16"), ref)))
    assert d_gpu <= 2.0 * d_ref


def test_groupnorm_gelu_large_offset(gpu):
    """mean / std of about 1e3 over 70001 samples: a float32 sum of squares has no variance left here"""
    from vcvits_amd import ops
    g = torch.Generator().manual_seed(7)
    x = (1000.0 + torch.randn(2, 5, 70001, generator=g, dtype=torch.float64)).to(torch.float32)
    w = (1.0 + 0.1 * torch.randn(5, generator=g, dtype=torch.float64)).to(torch.float32)
    b = (0.1 * torch.randn(5, generator=g, dtype=torch.float64)).to(torch.float32)
    ref = R.group_norm_gelu(x.double(), w.double(), b.double())
    ref32 = R.group_norm_gelu(x, w, b)
    out = ops.groupnorm_gelu(x.to(gpu), w.to(gpu), b.to(gpu)).cpu()
    inplace = x.to(gpu)
    assert ops.groupnorm_gelu(inplace, w.to(gpu), b.to(gpu), inplace=True).data_ptr() == inplace.data_ptr()
    assert torch.equal(inplace.cpu(), out)
    d_gpu, d_ref = R.rel_l2(out, ref), R.rel_l2(ref32, ref)
    _record("GroupNorm + GELU [2, 5, 70001], mean / std 1e3", "gpu %.3e (%.3e)   float32 restatement %.3e (%.3e)"
            % (d_gpu, R.max_abs(out, ref), d_ref, R.max_abs(ref32, ref)))
    assert d_gpu <= FP32_BOUND


def test_attention_other_head_dims_raise(gpu):
    from vcvits_amd import ops
    assert ops.hubert_attention_supported(3, 2, 64, 37) and ops.hubert_attention_supported(1, 16, 80, 1499)
    assert not ops.hubert_attention_supported(1, 2, 96, 37)
    q = torch.zeros(1, 2 * 96, 8, device=gpu)
    with pytest.raises(RuntimeError, match="head dims"):
        ops.hubert_attention(q, q, q, 2)


@pytest.mark.parametrize("heads,d,T", [(2, 64, 70), (3, 80, 37)])
def test_attention_separate_and_fused_inputs(gpu, heads, d, T):
    """q, k, v as three tensors and as slices of one fused projection go through the same kernel: bit-identical, and within
    the fp32 bar of a float64 softmax(q^T k / sqrt(d)) v"""
    from vcvits_amd import ops
    g = torch.Generator().manual_seed(d + T)
    qkv = torch.randn(2, 3 * heads * d, T, generator=g, dtype=torch.float64).to(torch.float32)
    q, k, v = (t.contiguous() for t in qkv.chunk(3, dim=1))
    out = ops.hubert_attention(q.to(gpu), k.to(gpu), v.to(gpu), heads)
    assert torch.equal(out, ops.hubert_attention_qkv(qkv.to(gpu), heads))
    qd, kd, vd = (t.double().reshape(2, heads, d, T) for t in (q, k, v))
    w = torch.softmax(torch.einsum("bhdt,bhds->bhts", qd * d ** -0.5, kd), dim=-1)
    ref = torch.einsum("bhts,bhds->bhdt", w, vd).reshape(2, heads * d, T)
    assert R.rel_l2(out.cpu(), ref) <= FP32_BOUND


@pytest.mark.parametrize("variant", ["A", "B"])
def test_batch_invariance_and_determinism(gpu, variant):
    """rows of equal length computed together are bit-identical to the same rows computed alone; two runs are bit-identical"""
    m = _model(variant, gpu)
    src = _source(3, 130).to(gpu)
    together, _ = m.extract_features(src)
    again, _ = m.extract_features(src)
    assert torch.equal(together, again)
    for b in range(3):
        alone, _ = m.extract_features(src[b:b + 1])
        assert torch.equal(alone[0], together[b]), "row %d" % b


def test_hubert_features_is_preprocess(gpu):
    """preprocess.py:64-73: pad 40 + 40, extract, transpose, squeeze, to the CPU"""
    from vcvits_amd.preprocess import hubert_features
    g = torch.Generator().manual_seed(3)
    audio_norm = (0.2 * torch.randn(1, 320 * 20, generator=g, dtype=torch.float64)).to(torch.float32)
    out = hubert_features(_model("A", gpu), audio_norm)
    ref = R.hubert_features(_sd("A"), audio_norm, "f64", **_cfg("A"))
    assert out.device.type == "cpu" and tuple(out.shape) == tuple(ref.shape) == (128, 20)
    d = R.rel_l2(out, ref)
    _record("public surface", "hubert_features [1, 6400] -> [128, 20]: gpu %.3e (%.3e)" % (d, R.max_abs(out, ref)))
    assert d <= FP32_BOUND


def test_content_encoder_takes_the_model(gpu):
    from vcvits_amd.model.encoders.content_encoder import HubertContentEncoder
    enc = HubertContentEncoder(None, 8, 16, 32, 2, 1, 3, 0.0, hubert_channels=128, num_pitch=16).to(gpu)
    enc.set_feature_extractor(_model("A", gpu))
    T_src = 320 * 12
    wav = _source(2, 20)[:, :T_src].unsqueeze(1).to(gpu)
    feats = enc.extract(wav)
    assert tuple(feats.shape) == (2, 128, T_src // 320) and feats.dtype == torch.float32
    ref = R.run(_sd("A"), torch.nn.functional.pad(wav.cpu().squeeze(1), (40, 40)), "f64", **_cfg("A")).transpose(1, 2)
    assert R.rel_l2(feats.cpu(), ref) <= FP32_BOUND


def test_load_hubert_on_a_synthetic_checkpoint(gpu, tmp_path):
    import sys
    from vcvits_amd.preprocess import load_hubert
    sd = dict(_sd("B"))
    sd["mask_emb"] = torch.zeros(160)
    sd["final_proj.weight"] = torch.zeros(8, 160)
    path = str(tmp_path / "hubert.pt")
    torch.save({"cfg": {"model": {"extractor_mode": "layer_norm", "layer_norm_first": True, "encoder_attention_heads": 2,
                                  "conv_bias": True, "conv_pos": 128, "conv_pos_groups": 16}}, "model": sd}, path)
    model = load_hubert(path, gpu)
    assert not model.training and next(model.parameters()).is_cuda and not any(p.requires_grad for p in model.parameters())
    assert "fairseq" not in sys.modules and "transformers" not in sys.modules
    out, _ = model.extract_features(_source(3, 37).to(gpu))
    assert R.rel_l2(out.cpu(), _ref("B", 3, 37, None, "f64")) <= FP32_BOUND

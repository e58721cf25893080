"""GPU: rows of unequal length in one padded batch (extract_features(lengths=), vcvits_amd/model/hubert.py over the
length-aware kernels of csrc/hubert.hip): the features of a row in a padded batch are the features of that row computed alone.

The yardstick is the float64 restatement (tests/hubert_f64.py) run on each row ALONE, R.run(sd, source[b:b+1, :len_b], "f64").
Distances are relative L2 per row over the row's valid frames.
  fp32 mode: <= 1e-4 (the project's fp32 bar).
  bf16 mode: <= 2 x the distance of the restatement of the same row alone under torch.autocast("cpu", torch.bfloat16).
Frames behind a row's end are exact zeros.  The measured distances go to profiles/hubert_lengths_parity.txt."""
import functools
import os

import pytest
import torch

import hubert_f64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_BOUND = 1e-4
_parity = {}

# the variants and seeded weights of tests/test_hubert_gpu.py
VARIANTS = {
    "A": dict(extractor_mode="default", conv_dim=64, embed_dim=128, ffn_dim=256, layers=2, conv_bias=False, heads=2, pre=False),
    "B": dict(extractor_mode="layer_norm", conv_dim=64, embed_dim=160, ffn_dim=320, layers=2, conv_bias=True, heads=2, pre=True),
    "base": dict(extractor_mode="default", conv_dim=512, embed_dim=768, ffn_dim=3072, layers=2, conv_bias=False, heads=12, pre=False),
    "xtralarge": dict(extractor_mode="layer_norm", conv_dim=512, embed_dim=1280, ffn_dim=5120, layers=2, conv_bias=True, heads=16, pre=True),
}


def S(frames):
    """the sample count that gives `frames` frames"""
    return 400 + 320 * (frames - 1)


# name -> (samples per row, frames per row); the batch is padded to the longest row
BATCHES = {
    "six": ((S(130), S(129) - 1, S(33) + 319, S(32), S(1), S(97) + 5), (130, 128, 33, 32, 1, 97)),
    "long": ((S(1030), S(1000) + 7, S(257), S(5)), (1030, 1000, 257, 5)),
    "two": ((S(49), S(20)), (49, 20)),
}


def _record(section, line):
    """Keep the printed figures in profiles/hubert_lengths_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "hubert_lengths_parity.txt"), "w") as f:
        f.write("# tests/test_hubert_lengths_gpu.py: rows of a padded batch with lengths= against the float64 restatement\n"
                "# (tests/hubert_f64.py) of each row computed ALONE; relative L2 (max abs) over the row's valid frames.\n"
                "# fp32 mode asserts gpu <= 1e-4; bf16 mode asserts gpu <= 2 * (the restatement of the row alone under bf16 autocast).\n")
        for name in sorted(_parity):
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


@functools.lru_cache(maxsize=None)
def _sd(variant):
    v = VARIANTS[variant]
    return R.random_state_dict(1234 + len(variant), extractor_mode=v["extractor_mode"], conv_dim=v["conv_dim"],
                               embed_dim=v["embed_dim"], ffn_dim=v["ffn_dim"], layers=v["layers"], conv_bias=v["conv_bias"])


def _cfg(variant):
    v = VARIANTS[variant]
    return dict(extractor_mode=v["extractor_mode"], layer_norm_first=v["pre"], num_heads=v["heads"])


@functools.lru_cache(maxsize=None)
def _source(batch):
    """[B, T_max] float32, zeros behind each row's end; never modified (tests that change it clone it)"""
    lens, _ = BATCHES[batch]
    g = torch.Generator().manual_seed(1000 + len(lens) + max(lens))
    src = torch.zeros(len(lens), max(lens), dtype=torch.float32)
    for b, n in enumerate(lens):
        t = torch.arange(n, dtype=torch.float64) / 16000.0
        src[b, :n] = (0.3 * torch.sin(2 * torch.pi * (110.0 * (b + 1)) * t)
                      + 0.1 * torch.randn(t.shape, generator=g, dtype=torch.float64)).to(torch.float32)
    return src


@functools.lru_cache(maxsize=None)
def _ref(variant, batch, b, output_layer, mode):
    """The restatement of row b ALONE (float64 tensor [f_b, E]), computed once per case and shared; never modified."""
    n = BATCHES[batch][0][b]
    return R.run(_sd(variant), _source(batch)[b:b + 1, :n], mode, output_layer=output_layer, **_cfg(variant))[0]


_models = {}


def _model(variant, gpu):
    from vcvits_amd.model.hubert import HubertFeatureExtractor
    if variant not in _models:
        _models[variant] = HubertFeatureExtractor.from_state_dict(_sd(variant), heads=VARIANTS[variant]["heads"]).to(gpu)
    return _models[variant]


def _check_rows(section, variant, batch, output_layer, out, pm, ref_mode=None):
    """shape, mask, exact-zero tails, finiteness and the per-row distance; ref_mode None: the fp32 bar, "bf16": the 2 x rule"""
    lens, frames = BATCHES[batch]
    B, Tp, E = len(lens), max(frames), VARIANTS[variant]["embed_dim"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, Tp, E)
    assert pm.dtype == torch.bool and tuple(pm.shape) == (B, Tp) and pm.device == out.device
    out, pm = out.cpu(), pm.cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(pm, torch.arange(Tp)[None, :] >= torch.tensor(frames)[:, None])
    failures = []
    for b, f in enumerate(frames):
        assert f == Tp or out[b, f:].abs().max().item() == 0.0, "row %d has values behind its end" % b
        ref = _ref(variant, batch, b, output_layer, "f64")
        assert tuple(ref.shape) == (f, E), "row %d: the restatement gives %s frames" % (b, ref.shape[0])
        d_gpu = R.rel_l2(out[b, :f], ref)
        ref2 = _ref(variant, batch, b, output_layer, ref_mode or "f32")
        d_ref = R.rel_l2(ref2, ref)
        _record(section, "%-9s %-4s row %d samples=%-6d T'=%-4d output_layer=%-4s gpu %.3e (%.3e)   %s restatement alone %.3e (%.3e)"
                % (variant, batch, b, lens[b], f, output_layer, d_gpu, R.max_abs(out[b, :f], ref),
                   "bf16-autocast" if ref_mode else "float32", d_ref, R.max_abs(ref2, ref)))
        bound = 2.0 * d_ref if ref_mode else FP32_BOUND
        if not d_gpu <= bound:
            failures.append("row %d: %.3e > %.3e" % (b, d_gpu, bound))
    assert not failures, failures


def _run(variant, batch, gpu, output_layer=None, source=None, lengths=None):
    src = _source(batch) if source is None else source
    return _model(variant, gpu).extract_features(src.to(gpu), output_layer=output_layer,
                                                 lengths=list(BATCHES[batch][0]) if lengths is None else lengths)


# ------------------------------------------------------------------------------------------------------------ the kernels
def _attn_lengths(T):
    return (1, 32, 33, min(128, T), min(129, T), T)


@pytest.mark.parametrize("heads,d,T", [(2, 64, 70), (3, 80, 37), (1, 64, 300)])
def test_attention_with_lengths(gpu, heads, d, T):
    """test 1: a single key, both sides of a key tile, both sides of a query block (T = 300: one block wholly behind the
    end), and the full row, against a float64 masked softmax"""
    from vcvits_amd import ops
    B, lens = 6, _attn_lengths(T)
    g = torch.Generator().manual_seed(d + T)
    qkv = torch.randn(B, 3 * heads * d, T, generator=g, dtype=torch.float64).to(torch.float32)
    q, k, v = (t.contiguous() for t in qkv.chunk(3, dim=1))
    n = torch.tensor(lens, dtype=torch.int32, device=gpu)
    out = ops.hubert_attention(q.to(gpu), k.to(gpu), v.to(gpu), heads, lengths=n)
    assert torch.equal(out, ops.hubert_attention_qkv(qkv.to(gpu), heads, lengths=n))
    # NaN behind each row's end, in q, k and v: not a bit changes
    dirty = qkv.clone()
    for b, f in enumerate(lens):
        dirty[b, :, f:] = float("nan")
    assert torch.equal(out, ops.hubert_attention_qkv(dirty.to(gpu), heads, lengths=n))
    dq, dk, dv = (t.contiguous().to(gpu) for t in dirty.chunk(3, dim=1))
    assert torch.equal(out, ops.hubert_attention(dq, dk, dv, heads, lengths=n))
    out = out.cpu()
    for b, f in enumerate(lens):
        qd, kd, vd = (t[b, :, :f].double().reshape(heads, d, f) for t in (q, k, v))
        w = torch.softmax(torch.einsum("hdt,hds->hts", qd * d ** -0.5, kd), dim=-1)
        ref = torch.einsum("hts,hds->hdt", w, vd).reshape(heads * d, f)
        dist = R.rel_l2(out[b, :, :f], ref)
        _record("attention with lengths", "heads=%d d=%d T=%-3d row %d keys=%-3d gpu %.3e (%.3e)"
                % (heads, d, T, b, f, dist, R.max_abs(out[b, :, :f], ref)))
        assert dist <= FP32_BOUND, "row %d" % b
        assert f == T or out[b, :, f:].abs().max().item() == 0.0, "row %d" % b
    # all rows full: the kernel without lengths, bit for bit
    full = torch.full((B,), T, dtype=torch.int32, device=gpu)
    assert torch.equal(ops.hubert_attention_qkv(qkv.to(gpu), heads, lengths=full), ops.hubert_attention_qkv(qkv.to(gpu), heads))


def test_groupnorm_gelu_with_lengths(gpu):
    """test 2: mean / std of about 1e3, counts of the whole row, half of it, and one sample (variance 0: gelu(beta))"""
    from vcvits_amd import ops
    g = torch.Generator().manual_seed(11)
    T, counts = 70001, (70001, 35000, 1)
    x = (1000.0 + torch.randn(3, 5, T, generator=g, dtype=torch.float64)).to(torch.float32)
    w = (1.0 + 0.1 * torch.randn(5, generator=g, dtype=torch.float64)).to(torch.float32)
    bias = (0.1 * torch.randn(5, generator=g, dtype=torch.float64)).to(torch.float32)
    n = torch.tensor(counts, dtype=torch.int32, device=gpu)
    out = ops.groupnorm_gelu(x.to(gpu), w.to(gpu), bias.to(gpu), lengths=n)
    inplace = x.to(gpu)
    assert ops.groupnorm_gelu(inplace, w.to(gpu), bias.to(gpu), inplace=True, lengths=n).data_ptr() == inplace.data_ptr()
    assert torch.equal(inplace, out)
    dirty = x.clone()
    for b, c in enumerate(counts):
        dirty[b, :, c:] = float("nan")
    assert torch.equal(ops.groupnorm_gelu(dirty.to(gpu), w.to(gpu), bias.to(gpu), lengths=n), out)
    out = out.cpu()
    for b, c in enumerate(counts):
        ref = R.group_norm_gelu(x[b:b + 1, :, :c].double(), w.double(), bias.double())[0]
        ref32 = R.group_norm_gelu(x[b:b + 1, :, :c], w, bias)[0]
        d_gpu = R.rel_l2(out[b, :, :c], ref)
        _record("GroupNorm + GELU [3, 5, 70001] with counts, mean / std 1e3", "count=%-5d gpu %.3e (%.3e)   float32 restatement %.3e (%.3e)"
                % (c, d_gpu, R.max_abs(out[b, :, :c], ref), R.rel_l2(ref32, ref), R.max_abs(ref32, ref)))
        assert d_gpu <= FP32_BOUND, "row %d" % b
        assert c == T or out[b, :, c:].abs().max().item() == 0.0, "row %d" % b
    # all rows full: the kernel without lengths, bit for bit
    full = torch.full((3,), T, dtype=torch.int32, device=gpu)
    assert torch.equal(ops.groupnorm_gelu(x.to(gpu), w.to(gpu), bias.to(gpu), lengths=full),
                       ops.groupnorm_gelu(x.to(gpu), w.to(gpu), bias.to(gpu)))


def test_mask_frames_is_a_select(gpu):
    """test 3: NaN behind a row's end becomes 0, valid frames keep their bits, in place gives the same"""
    from vcvits_amd import ops
    g = torch.Generator().manual_seed(5)
    frames = (1, 37, 300, 129)
    x = torch.randn(4, 7, 300, generator=g)
    x[0, 0, 0] = float("inf")  # a valid frame is passed through, whatever it holds
    dirty = x.clone()
    want = x.clone()
    for b, f in enumerate(frames):
        dirty[b, :, f:] = float("nan")
        want[b, :, f:] = 0.0
    n = torch.tensor(frames, dtype=torch.int32, device=gpu)
    out = ops.mask_frames(dirty.to(gpu), n)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(ops.mask_frames(x.to(gpu), n).cpu(), want)
    inplace = dirty.to(gpu)
    assert ops.mask_frames(inplace, n, inplace=True).data_ptr() == inplace.data_ptr()
    assert torch.equal(inplace.cpu(), want)
    with pytest.raises(ValueError, match="int32"):
        ops.mask_frames(x.to(gpu), n.long())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_frames(x.to(gpu), n.cpu())


# -------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("output_layer", [None, 1])
@pytest.mark.parametrize("variant", ["A", "B"])
def test_rows_equal_rows_alone_fp32(gpu, variant, output_layer):
    """test 4: six rows whose sample counts sit on and off the 320-sample grid in both directions; frames 130 (full), 128
    (a whole query block), 33 / 32 (both sides of a key tile), 1 (a single key) and 97"""
    m = _model(variant, gpu)
    lens, frames = BATCHES["six"]
    assert m.frame_lengths(list(lens)).tolist() == list(frames)
    out, pm = _run(variant, "six", gpu, output_layer)
    _check_rows("fp32 mode", variant, "six", output_layer, out, pm)


@pytest.mark.parametrize("variant", ["A", "B"])
def test_rows_equal_rows_alone_many_key_tiles(gpu, variant):
    """test 4: up to 33 key tiles and 9 query blocks, rows that end inside a tile, inside a block, and whole blocks early"""
    assert _model(variant, gpu).frame_lengths(list(BATCHES["long"][0])).tolist() == list(BATCHES["long"][1])
    out, pm = _run(variant, "long", gpu)
    _check_rows("fp32 mode", variant, "long", None, out, pm)


@pytest.mark.parametrize("variant", ["A", "B"])
def test_padding_never_reaches_a_valid_frame(gpu, variant):
    """test 5: noise of scale 1e3 in the padding samples changes no bit; rows in another order keep their bits"""
    lens, frames = BATCHES["six"]
    out, pm = _run(variant, "six", gpu)
    noisy = _source("six").clone()
    g = torch.Generator().manual_seed(77)
    for b, n in enumerate(lens):
        noisy[b, n:] = 1e3 * torch.randn(noisy.shape[1] - n, generator=g)
    out2, pm2 = _run(variant, "six", gpu, source=noisy)
    assert torch.equal(out2, out) and torch.equal(pm2, pm)
    perm = [4, 2, 0, 5, 1, 3]
    out3, pm3 = _run(variant, "six", gpu, source=noisy[perm], lengths=torch.tensor([lens[p] for p in perm]))
    for i, p in enumerate(perm):
        assert torch.equal(out3[i], out[p]), "row %d moved to %d" % (p, i)
        assert torch.equal(pm3[i], pm[p])


@pytest.mark.parametrize("variant", ["A", "B"])
def test_full_lengths_are_no_lengths(gpu, variant):
    """test 6: every row full gives the bits of the call without lengths, and a mask without a True"""
    m = _model(variant, gpu)
    src = _source("six")[:3].clone()
    g = torch.Generator().manual_seed(3)
    src[1:] = 0.2 * torch.randn(2, src.shape[1], generator=g)
    src = src.to(gpu)
    plain, none = m.extract_features(src)
    assert none is None
    for lengths in ([src.shape[1]] * 3, torch.full((3,), src.shape[1], dtype=torch.int32, device=gpu)):
        out, pm = m(src, lengths=lengths)
        assert torch.equal(out, plain)
        assert pm.dtype == torch.bool and tuple(pm.shape) == (3, 130) and not pm.any()


@pytest.mark.parametrize("variant", ["base", "xtralarge"])
def test_full_widths_fp32(gpu, variant):
    """test 7: the real conv and GEMM shapes, 2 layers, rows of 49 and 20 frames"""
    out, pm = _run(variant, "two", gpu)
    _check_rows("fp32 mode", variant, "two", None, out, pm)


def test_bf16_mode(gpu):
    """test 8: variant A, the six rows, each within 2 x the bf16-autocast restatement of the row alone"""
    from vcvits_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        out, pm = _run("A", "six", gpu)
        out, pm = out.cpu(), pm.cpu()
    finally:
        ops.set_compute_dtype("f32")
    _check_rows("bf16 mode", "A", "six", None, out, pm, ref_mode="bf16")


def test_hubert_features_batch(gpu):
    """test 9: five files in at least two padded batches come back in input order, each what hubert_features gives for the
    file alone (pad 40 + 40, the padded length is the row's length)"""
    from vcvits_amd.preprocess import hubert_features, hubert_features_batch
    m = _model("A", gpu)
    g = torch.Generator().manual_seed(9)
    sizes = (6400, 2253, 400, 10560, 6400)
    audios = [(0.2 * torch.randn(1, n, generator=g, dtype=torch.float64)).to(torch.float32) for n in sizes]
    calls = []
    real = m.extract_features

    def counted(source, **kw):
        calls.append((tuple(source.shape), list(kw["lengths"])))
        return real(source, **kw)

    m.extract_features = counted
    try:
        got = hubert_features_batch(m, audios, max_batch_samples=13000)
    finally:
        del m.extract_features
    assert len(calls) >= 2 and all(B * T <= 13000 for (B, T), _ in calls)
    assert sorted(n for _, lens in calls for n in lens) == sorted(n + 80 for n in sizes)
    assert len(got) == len(sizes)
    for i, (n, feats) in enumerate(zip(sizes, got)):
        ref = R.hubert_features(_sd("A"), audios[i], "f64", **_cfg("A"))
        alone = hubert_features(m, audios[i])
        assert feats.device.type == "cpu" and feats.dtype == torch.float32
        assert tuple(feats.shape) == tuple(alone.shape) == tuple(ref.shape) == (128, (n + 80 - 400) // 320 + 1)
        d = R.rel_l2(feats, ref)
        _record("hubert_features_batch", "file %d samples=%-5d -> [128, %d]: gpu %.3e (%.3e)   against hubert_features alone %.3e"
                % (i, n, feats.shape[1], d, R.max_abs(feats, ref), R.rel_l2(feats, alone)))
        assert d <= FP32_BOUND
    assert got[2].shape[1] == 1
    # a budget below every file: one file per batch, the same results
    single = hubert_features_batch(m, audios, max_batch_samples=1)
    assert all(torch.equal(a, b) for a, b in zip(single, (hubert_features(m, a) for a in audios)))

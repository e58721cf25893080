"""Restatement of fairseq's HubertModel.extract_features in inference (test oracle only).

Plain functional torch-CPU code over a `state_dict` with fairseq's key names (fairseq/models/hubert/hubert.py,
fairseq/models/wav2vec/wav2vec2.py: ConvFeatureExtractionModel, TransformerEncoder, TransformerSentenceEncoderLayer,
MultiheadAttention), for the two published architectures: group-norm front end with a post-LN encoder (hubert_base_ls960)
and layer-norm front end with a pre-LN encoder (hubert_large / xtralarge_ll60k).  No masking, no padding mask, no dropout.
It shares no code with vcvits_amd/model/hubert.py.  The arithmetic runs in the dtype of the tensors it is given, so the same
text is the float64 yardstick, the float32 reference computation, and (under `torch.autocast("cpu", torch.bfloat16)`, see
`run`) the reduced-precision one.  tests/golden/hubert_small.npz (tools/make_goldens_hubert.py) pins it to
transformers.HubertModel, which restates the same model independently.

Points decided here (the product follows this file):
 1. conv front end, "default": conv without bias; GroupNorm(C, C) with affine on layer 0 only; GELU after every layer.
    "layer_norm": conv (with bias when present) -> LayerNorm over channels -> GELU at every layer.
 2. LayerNorm over the conv channels, then post_extract_proj.
 3. pos = gelu(conv1d(x, w, b, padding=64, groups=16)[..., :-1]) with w = weight_v * weight_g / ||weight_v|| and the norm
    over axes (0, 1) (weight_norm(dim=2)): one norm per tap.
 4. post-LN: x = LN(x + pos); layer: x = LN1(x + attn(x)); x = LN2(x + fc2(gelu(fc1(x)))).
    pre-LN:  x = x + pos;     layer: x = x + attn(LN1(x)); x = x + fc2(gelu(fc1(LN2(x)))); encoder.layer_norm at the end
    only when output_layer is None.
 5. attn(x) = out_proj(softmax(((Wq x + bq) * d ** -0.5) (Wk x + bk)^T) (Wv x + bv)) over all frames of the row.
 6. output_layer n (1-based) returns the output of layer n.  GELU is the erf form; every eps is 1e-5.
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
CONV_STRIDES = (5, 2, 2, 2, 2, 2, 2)
POS_GROUPS = 16


def gelu(x):
    return F.gelu(x)


def _wide(x):
    """Norms and softmax run in float32 at least, whatever the matmuls around them produce: fairseq's Fp32GroupNorm /
    Fp32LayerNorm, and what autocast does with layer_norm and softmax.  (A no-op in the float32 and float64 runs.)"""
    return x.float() if x.dtype in (torch.bfloat16, torch.float16) else x


def group_norm_gelu(x, weight, bias):
    """gelu(GroupNorm(C, C)(x)) for x [B, C, T]: per (b, c) statistics over T, biased variance."""
    x = _wide(x)
    mean = x.mean(dim=2, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=2, keepdim=True)
    return gelu((x - mean) / torch.sqrt(var + EPS) * weight[None, :, None] + bias[None, :, None])


def _ln(x, sd, prefix):
    return F.layer_norm(_wide(x), (x.shape[-1],), sd[prefix + ".weight"], sd[prefix + ".bias"], EPS)


def n_conv_layers(sd):
    n = 0
    while "feature_extractor.conv_layers.%d.0.weight" % n in sd:
        n += 1
    return n


def n_encoder_layers(sd):
    n = 0
    while "encoder.layers.%d.fc1.weight" % n in sd:
        n += 1
    return n


def conv_features(sd, source, extractor_mode, strides=CONV_STRIDES):
    """source [B, T] -> [B, C, T']"""
    x = source[:, None, :]
    for i in range(n_conv_layers(sd)):
        p = "feature_extractor.conv_layers.%d" % i
        x = F.conv1d(x, sd[p + ".0.weight"], sd.get(p + ".0.bias"), stride=strides[i])
        if extractor_mode == "layer_norm":
            x = gelu(_ln(x.transpose(1, 2), sd, p + ".2.1").transpose(1, 2))
        elif i == 0:
            x = group_norm_gelu(x, sd[p + ".2.weight"], sd[p + ".2.bias"])
        else:
            x = gelu(x)
    return x


def pos_conv_weight(sd):
    v, g = sd["encoder.pos_conv.0.weight_v"], sd["encoder.pos_conv.0.weight_g"]
    norm = torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))
    return v * (g / norm)


def _pos_conv(x, w, b, groups):
    """The position conv.  Under bf16 autocast x arrives as bfloat16, and torch's CPU bfloat16 conv1d returns wrong values at
    this shape (128 taps, padding 64, 16 groups of a few channels: relative error above 1 against float64, and the same for one
    group's channels convolved alone; a dense conv over all channels with the same taps is at 3e-3, like its 2- and 3-tap convs).  A bf16 conv is bf16 operands, float32 accumulation and one rounding of the result, so that is what runs here."""
    if x.dtype == torch.bfloat16:
        with torch.autocast("cpu", enabled=False):
            return F.conv1d(x.float(), w.bfloat16().float(), b.float(), padding=w.shape[2] // 2, groups=groups).bfloat16()
    return F.conv1d(x, w, b, padding=w.shape[2] // 2, groups=groups)


def attention(sd, p, x, num_heads):
    """x [B, T, E]"""
    B, T, E = x.shape
    d = E // num_heads
    q = F.linear(x, sd[p + ".q_proj.weight"], sd[p + ".q_proj.bias"]) * d ** -0.5
    k = F.linear(x, sd[p + ".k_proj.weight"], sd[p + ".k_proj.bias"])
    v = F.linear(x, sd[p + ".v_proj.weight"], sd[p + ".v_proj.bias"])
    q, k, v = (t.reshape(B, T, num_heads, d).transpose(1, 2) for t in (q, k, v))
    w = torch.softmax(_wide(torch.matmul(q, k.transpose(-1, -2))), dim=-1)
    o = torch.matmul(w, v).transpose(1, 2).reshape(B, T, E)
    return F.linear(o, sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"])


def extract_features(sd, source, *, extractor_mode, layer_norm_first, num_heads, output_layer=None,
                     strides=CONV_STRIDES, pos_groups=POS_GROUPS):
    """fairseq HubertModel.extract_features(source, padding_mask=None, mask=False, output_layer)[0]: [B, T', E]."""
    x = conv_features(sd, source, extractor_mode, strides).transpose(1, 2)
    x = _ln(x, sd, "layer_norm")
    x = F.linear(x, sd["post_extract_proj.weight"], sd["post_extract_proj.bias"])
    w = pos_conv_weight(sd)
    pos = _pos_conv(x.transpose(1, 2), w, sd["encoder.pos_conv.0.bias"], pos_groups)
    if w.shape[2] % 2 == 0:
        pos = pos[:, :, :-1]
    x = x + gelu(pos).transpose(1, 2)
    if not layer_norm_first:
        x = _ln(x, sd, "encoder.layer_norm")
    for i in range(n_encoder_layers(sd)):
        p = "encoder.layers.%d" % i
        if layer_norm_first:
            x = x + attention(sd, p + ".self_attn", _ln(x, sd, p + ".self_attn_layer_norm"), num_heads)
            h = _ln(x, sd, p + ".final_layer_norm")
            x = x + F.linear(gelu(F.linear(h, sd[p + ".fc1.weight"], sd[p + ".fc1.bias"])), sd[p + ".fc2.weight"], sd[p + ".fc2.bias"])
        else:
            x = _ln(x + attention(sd, p + ".self_attn", x, num_heads), sd, p + ".self_attn_layer_norm")
            h = F.linear(gelu(F.linear(x, sd[p + ".fc1.weight"], sd[p + ".fc1.bias"])), sd[p + ".fc2.weight"], sd[p + ".fc2.bias"])
            x = _ln(x + h, sd, p + ".final_layer_norm")
        if output_layer is not None and i + 1 == output_layer:
            return x
    if layer_norm_first:
        x = _ln(x, sd, "encoder.layer_norm")
    return x


def run(sd, source, mode, **cfg):
    """extract_features in `mode`: "f64", "f32", or "bf16" (float32 tensors under torch.autocast("cpu", torch.bfloat16));
    the result comes back as float64."""
    dt = torch.float64 if mode == "f64" else torch.float32
    sdc = {k: v.detach().to("cpu", dt) for k, v in sd.items() if v.is_floating_point()}
    src = source.detach().to("cpu", dt)
    with torch.no_grad():
        if mode == "bf16":
            with torch.autocast("cpu", torch.bfloat16):
                out = extract_features(sdc, src, **cfg)
        else:
            out = extract_features(sdc, src, **cfg)
    return out.to(torch.float64)


def hubert_features(sd, audio_norm, mode="f64", **cfg):
    """preprocess.py:64-73: pad 40 + 40, extract_features, transpose, squeeze: audio_norm [1, T] -> [E, T']."""
    wav = F.pad(audio_norm, ((400 - 320) // 2, (400 - 320) // 2))
    return run(sd, wav.squeeze(1), mode, **cfg).transpose(1, -1).squeeze(0)


def out_frames(T, kernels=(10, 3, 3, 3, 3, 2, 2), strides=CONV_STRIDES):
    for k, s in zip(kernels, strides):
        T = (T - k) // s + 1
    return T


def random_state_dict(seed, *, extractor_mode, conv_dim, embed_dim, ffn_dim, layers, conv_bias=False,
                      kernels=(10, 3, 3, 3, 3, 2, 2), pos_kernel=128, pos_groups=POS_GROUPS, dtype=torch.float32):
    """A seeded fairseq-named state_dict with weights at the scale of a trained model's (activations stay O(1) through the
    stack, norm gains near 1): what the GPU tests and the benchmark tool load."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)

    sd = {}
    cin = 1
    for i, k in enumerate(kernels):
        p = "feature_extractor.conv_layers.%d" % i
        sd[p + ".0.weight"] = rnd(conv_dim, cin, k, scale=math.sqrt(2.0 / (cin * k)))
        if conv_bias:
            sd[p + ".0.bias"] = rnd(conv_dim, scale=0.1)
        if extractor_mode == "layer_norm":
            sd[p + ".2.1.weight"] = 1.0 + rnd(conv_dim, scale=0.1)
            sd[p + ".2.1.bias"] = rnd(conv_dim, scale=0.1)
        elif i == 0:
            sd[p + ".2.weight"] = 1.0 + rnd(conv_dim, scale=0.1)
            sd[p + ".2.bias"] = rnd(conv_dim, scale=0.1)
        cin = conv_dim

    def lin(p, o, i):
        sd[p + ".weight"] = rnd(o, i, scale=1.0 / math.sqrt(i))
        sd[p + ".bias"] = rnd(o, scale=0.1)

    def norm(p, c):
        sd[p + ".weight"] = 1.0 + rnd(c, scale=0.1)
        sd[p + ".bias"] = rnd(c, scale=0.1)

    norm("layer_norm", conv_dim)
    lin("post_extract_proj", embed_dim, conv_dim)
    sd["encoder.pos_conv.0.weight_v"] = rnd(embed_dim, embed_dim // pos_groups, pos_kernel)
    sd["encoder.pos_conv.0.weight_g"] = (1.0 + 0.1 * torch.rand(1, 1, pos_kernel, generator=g, dtype=torch.float64)).to(dtype)
    sd["encoder.pos_conv.0.bias"] = rnd(embed_dim, scale=0.1)
    for i in range(layers):
        p = "encoder.layers.%d" % i
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + ".self_attn." + n, embed_dim, embed_dim)
        norm(p + ".self_attn_layer_norm", embed_dim)
        lin(p + ".fc1", ffn_dim, embed_dim)
        lin(p + ".fc2", embed_dim, ffn_dim)
        norm(p + ".final_layer_norm", embed_dim)
    norm("encoder.layer_norm", embed_dim)
    return sd


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())

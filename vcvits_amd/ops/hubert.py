"""HuBERT inference kernels (csrc/hubert.hip): streamed softmax self-attention, GroupNorm + GELU over time, channel
LayerNorm + GELU, bias + GELU (+ residual).  With conv_forward (every linear layer and convolution) and layernorm_c these
are all of fairseq's HubertModel.extract_features (vcvits_amd/model/hubert.py).

Rows of unequal length in one padded batch: `hubert_attention(_qkv)` and `groupnorm_gelu` take `lengths=`, an int32 [B] tensor
on the GPU (keys, or samples, that exist in each row), and `mask_frames` zeroes what lies behind a row's end.  All three
select and never multiply, so nothing stored behind a row's end reaches a valid frame.  With `lengths=None` every function
is what it was.  The entries must lie in [1, T]: the wrappers do not read the tensor back (that would stall the queue once
per layer), the model checks its host copy before it uploads it, and the kernels clamp a value outside the range.

Part of `vcvits_amd.ops` (the package re-exports every name: `from vcvits_amd import ops; ops.hubert_attention(...)`).  All
tensors are float32 [B, C, T] on the GPU; nothing here records an autograd graph (the model is frozen).  There is no CPU
fallback: CPU tensors raise."""
import ctypes

import torch

from .._lib import check, lib, ptr, stream
from .core import LAUNCH_COUNTS
from .attention import attn_stream_bf16

HUBERT_HEAD_DIMS = (64, 80)


def _hb_gpu(t, what, dims=3):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("vcvits_amd: %s is not on the GPU; the HIP path has no CPU fallback" % what)
    if t.dtype != torch.float32 or t.dim() != dims:
        raise ValueError("%s must be a float32 tensor of %d dimensions" % (what, dims))
    return t.detach().contiguous()


def _hb_lengths(lengths, B, what):
    if not isinstance(lengths, torch.Tensor) or not lengths.is_cuda:
        raise RuntimeError("vcvits_amd: %s is not on the GPU; the HIP path has no CPU fallback" % what)
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
        raise ValueError("%s must be an int32 tensor of shape [%d] (one entry per batch row)" % (what, B))
    return lengths.detach().contiguous()


def hubert_attention_supported(B, H, head_dim, T):
    """True when the streamed attention kernel takes the shape (head_dim 64 or 80, B * H <= 65535, any T >= 1)."""
    return lib().vcv_hubert_attn_supported(int(B), int(H), int(head_dim), int(T)) == 0


def _attn_launch(q, k, v, out, B, n_heads, d, T, ldb, scale, lengths):
    """The fp32-operand kernels, or in bf16 mode with VCVITS_ATTN_STREAM_BF16 = 1 (attn_stream_bf16) their bf16-operand twins,
    which count as "attn_stream_bf16" in LAUNCH_COUNTS."""
    scale = float(d) ** -0.5 if scale is None else float(scale)
    bf = attn_stream_bf16()
    if lengths is None:
        name = "vcv_hubert_attn_fwd_bf16" if bf else "vcv_hubert_attn_fwd"
        check(getattr(lib(), name)(q, k, v, ptr(out), B, n_heads, d, T, ldb, scale, stream()), name)
    else:
        name = "vcv_hubert_attn_fwd_len_bf16" if bf else "vcv_hubert_attn_fwd_len"
        check(getattr(lib(), name)(q, k, v, ptr(out), B, n_heads, d, T, ldb, scale,
                                   ptr(_hb_lengths(lengths, B, "lengths")), stream()), name)
    if bf:
        LAUNCH_COUNTS["attn_stream_bf16"] += 1
    return out


def hubert_attention(q, k, v, n_heads, scale=None, lengths=None):
    """softmax((scale * q)^T k) v per head for q / k / v [B, n_heads * d, T] -> [B, n_heads * d, T]; scale defaults to
    d ** -0.5.  Keys and values are streamed in tiles with a running max and sum (no [T, T] tensor).  lengths (int32 [B] on
    the GPU, entries in [1, T]): row b attends to the keys s < lengths[b] only, q / k / v at or behind lengths[b] are never
    used, and the output there is exact 0."""
    q, k, v = _hb_gpu(q, "q"), _hb_gpu(k, "k"), _hb_gpu(v, "v")
    B, E, T = q.shape
    if k.shape != q.shape or v.shape != q.shape or E % n_heads:
        raise ValueError("hubert_attention: q, k, v must share one shape [B, n_heads * d, T]")
    d = E // n_heads
    if not hubert_attention_supported(B, n_heads, d, T):
        raise RuntimeError("vcvits_amd: hubert_attention has kernels for head dims %s and B * heads <= 65535; got "
                           "B=%d heads=%d head_dim=%d T=%d" % (HUBERT_HEAD_DIMS, B, n_heads, d, T))
    return _attn_launch(ptr(q), ptr(k), ptr(v), torch.empty_like(q), B, n_heads, d, T, E * T, scale, lengths)


def hubert_attention_qkv(qkv, n_heads, scale=None, lengths=None):
    """hubert_attention over the output [B, 3 * n_heads * d, T] of one fused projection (q rows, then k, then v)."""
    qkv = _hb_gpu(qkv, "qkv")
    B, E3, T = qkv.shape
    if E3 % (3 * n_heads):
        raise ValueError("hubert_attention_qkv: [B, 3 * n_heads * d, T] expected")
    E = E3 // 3
    d = E // n_heads
    if not hubert_attention_supported(B, n_heads, d, T):
        raise RuntimeError("vcvits_amd: hubert_attention has kernels for head dims %s and B * heads <= 65535; got "
                           "B=%d heads=%d head_dim=%d T=%d" % (HUBERT_HEAD_DIMS, B, n_heads, d, T))
    out = torch.empty((B, E, T), dtype=torch.float32, device=qkv.device)
    q = ptr(qkv)
    k, v = ctypes.c_void_p(q.value + 4 * E * T), ctypes.c_void_p(q.value + 8 * E * T)
    return _attn_launch(q, k, v, out, B, n_heads, d, T, E3 * T, scale, lengths)


def bias_gelu(x, bias=None, res=None, frames=None, inplace=False):
    """res + gelu(x[..., :frames] + bias[c]) (exact erf form) for x [B, C, T]; bias [C] and res [B, C, frames] optional."""
    x = _hb_gpu(x, "x")
    B, C, Tin = x.shape
    T = Tin if frames is None else int(frames)
    if not 0 < T <= Tin:
        raise ValueError("bias_gelu: frames outside (0, T]")
    if bias is not None and (_hb_gpu(bias, "bias", 1).shape[0] != C):
        raise ValueError("bias_gelu: bias must be [C]")
    if res is not None and tuple(_hb_gpu(res, "res").shape) != (B, C, T):
        raise ValueError("bias_gelu: res must be [B, C, frames]")
    y = x if (inplace and T == Tin) else torch.empty((B, C, T), dtype=torch.float32, device=x.device)
    check(lib().vcv_hubert_bias_gelu(ptr(x), ptr(None if bias is None else bias.detach().contiguous()),
                                     ptr(None if res is None else res.detach().contiguous()), ptr(y), B * C, C, Tin, T,
                                     stream()), "vcv_hubert_bias_gelu")
    return y


def groupnorm_gelu(x, weight, bias, eps=1e-5, inplace=False, lengths=None):
    """gelu(F.group_norm(x, C, weight, bias, eps)) for x [B, C, T]: one group per channel, statistics over T in float64.
    lengths (int32 [B] on the GPU, entries in [1, T]): the statistics of row b run over its first lengths[b] samples, samples
    behind them are never read, and the output there is exact 0."""
    x, weight, bias = _hb_gpu(x, "x"), _hb_gpu(weight, "weight", 1), _hb_gpu(bias, "bias", 1)
    B, C, T = x.shape
    if weight.shape[0] != C or bias.shape[0] != C:
        raise ValueError("groupnorm_gelu: weight and bias must be [C]")
    y = x if inplace else torch.empty_like(x)
    if lengths is None:
        check(lib().vcv_hubert_groupnorm_gelu(ptr(x), ptr(weight), ptr(bias), ptr(y), B, C, T, eps, stream()),
              "vcv_hubert_groupnorm_gelu")
    else:
        check(lib().vcv_hubert_groupnorm_gelu_len(ptr(x), ptr(weight), ptr(bias), ptr(y), B, C, T,
                                                  ptr(_hb_lengths(lengths, B, "lengths")), eps, stream()),
              "vcv_hubert_groupnorm_gelu_len")
    return y


def mask_frames(x, lengths, inplace=False):
    """x[b, c, t] where t < lengths[b], exact 0 elsewhere, for x [B, C, T] and lengths int32 [B] on the GPU.  A select: NaN
    or Inf behind a row's end becomes 0, and valid frames keep their bits."""
    x = _hb_gpu(x, "x")
    B, C, T = x.shape
    y = x if inplace else torch.empty_like(x)
    check(lib().vcv_hubert_mask_frames(ptr(x), ptr(y), B, C, T, ptr(_hb_lengths(lengths, B, "lengths")), stream()),
          "vcv_hubert_mask_frames")
    return y


def layernorm_c_gelu(x, weight, bias, eps=1e-5, inplace=False):
    """gelu(LayerNorm over the channels of x [B, C, T]), statistics in float64."""
    x, weight, bias = _hb_gpu(x, "x"), _hb_gpu(weight, "weight", 1), _hb_gpu(bias, "bias", 1)
    B, C, T = x.shape
    if weight.shape[0] != C or bias.shape[0] != C:
        raise ValueError("layernorm_c_gelu: weight and bias must be [C]")
    y = x if inplace else torch.empty_like(x)
    check(lib().vcv_hubert_layernorm_c_gelu(ptr(x), ptr(weight), ptr(bias), ptr(y), B, C, T, eps, stream()),
          "vcv_hubert_layernorm_c_gelu")
    return y

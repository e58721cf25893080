"""Relative-position multi-head attention: the batched-GEMM form and the fused kernels.

Part of `vcvits_amd.ops` (the package re-exports every name: `from vcvits_amd import ops; ops.conv1d(...)`).  Everything here
runs on the GPU through libvcvits_hip.so; there is no CPU fallback."""
import torch

from .. import tuning
from .._lib import (VcvConvArgs, check, lib, ptr, stream)
from .core import (LAUNCH_COUNTS, _COMPUTE, _f32c)
from .conv import (_common, _launch_conv)
from .blocks import (DROPOUT_TRACE, next_seed)


# ---------------------------------------------------------------------------------------------
# relative-position attention: QK^T and P.V on the MFMA GEMM kernel, banded softmax in between
# ---------------------------------------------------------------------------------------------
def _bgemm(x, w, out, G, Cg, Mg, T, a_mode, alpha=1.0, res=None):
    """out[g*Mg + m, t] = alpha * sum_c A_g(m, c) * x[g*Cg + c, t] (+ res): one grouped 1x1 'conv'
    per (batch, head) pair on vcv_conv_gemm."""
    a = VcvConvArgs()
    a.x, a.w, a.y = ptr(x), ptr(w), ptr(out)
    a.B, a.G, a.Cg, a.Mg = 1, G, Cg, Mg
    a.Tin, a.Tout, a.P, a.K = T, T, 1, 1
    a.s, a.dj, a.off, a.os, a.oo, a.phases, a.Q, a.a_mode = 1, 1, 0, 1, 0, 1, T, a_mode
    _common(a, alpha=alpha, res=res)
    _launch_conv(a)
    return out


class _RelAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, embk, embv, mask, n_heads, window, pdrop, seed):
        q, k, v, embk, embv, mask = (_f32c(t) for t in (q, k, v, embk, embv, mask))
        B, C, T = q.shape
        H = n_heads
        dk = C // H
        G = B * H
        qscale = 1.0 / (dk ** 0.5)
        dev = q.device
        S = torch.empty((G, T, T), device=dev, dtype=torch.float32)
        _bgemm(k, q, S, G, dk, T, T, a_mode=1, alpha=qscale)
        P = S  # softmax in place
        Pd = torch.empty_like(S) if pdrop > 0 else None
        Pt = torch.empty_like(S)
        check(lib().vcv_rel_softmax_fwd(ptr(S), ptr(q), ptr(embk), ptr(mask), ptr(P), ptr(Pd), ptr(Pt), B, H,
                                        dk, T, window, qscale, pdrop, seed, stream()), "vcv_rel_softmax_fwd")
        if Pd is None:
            Pd = P
        out = torch.empty_like(q)
        _bgemm(Pt, v, out, G, T, dk, T, a_mode=0)
        check(lib().vcv_rel_value_fwd(ptr(Pd), ptr(embv), ptr(out), B, H, dk, T, window, stream()),
              "vcv_rel_value_fwd")
        ctx.cfg = (H, window, qscale)
        ctx.save_for_backward(q, k, v, embk, embv, mask, P, Pd)
        attn = Pd.view(B, H, T, T)
        ctx.mark_non_differentiable(attn)
        return out, attn

    @staticmethod
    def backward(ctx, dout, _dattn):
        q, k, v, embk, embv, mask, P, Pd = ctx.saved_tensors
        H, window, qscale = ctx.cfg
        dout = _f32c(dout)
        B, C, T = q.shape
        dk = C // H
        G = B * H
        dv = torch.empty_like(v)
        _bgemm(Pd, dout, dv, G, T, dk, T, a_mode=0)
        dP = torch.empty_like(P)
        _bgemm(v, dout, dP, G, dk, T, T, a_mode=1)
        dSt = torch.empty_like(P)
        dqband = torch.empty_like(q)
        dembk = torch.empty_like(embk)
        dembv = torch.empty_like(embv)
        check(lib().vcv_rel_softmax_bwd(ptr(P), ptr(Pd), ptr(dP), ptr(dout), ptr(q), ptr(embk), ptr(embv),
                                        ptr(mask), ptr(dSt), ptr(dqband), ptr(dembk), ptr(dembv), B, H, dk, T,
                                        window, qscale, stream()), "vcv_rel_softmax_bwd")
        dS = dP
        dq = torch.empty_like(q)
        _bgemm(dSt, k, dq, G, T, dk, T, a_mode=0, alpha=qscale, res=dqband)
        dkk = torch.empty_like(k)
        _bgemm(dS, q, dkk, G, T, dk, T, a_mode=0, alpha=qscale)
        return dq, dkk, dv, dembk, dembv, None, None, None, None, None


class _RelAttnFusedFn(torch.autograd.Function):
    """The whole attention of one layer as ONE launch forward and two backward (attention.hip): both contractions on the
    matrix cores straight from the [B, C, T] activations, softmax / band terms / mask fill / dropout in between on the
    LDS tile.  The probabilities are written only for the backward pass or when `attn` is asked for; the dropped
    probabilities are never stored (the backward pass regenerates the mask from the seed)."""

    @staticmethod
    def forward(ctx, q, k, v, embk, embv, mask, n_heads, window, pdrop, seed, want_attn):
        q, k, v, embk, embv, mask = (_f32c(t) for t in (q, k, v, embk, embv, mask))
        B, C, T = q.shape
        H = n_heads
        dk = C // H
        G = B * H
        qscale = 1.0 / (dk ** 0.5)
        dev = q.device
        need_p = any(ctx.needs_input_grad[:5])
        bf = 1 if _COMPUTE[0] == "bf16" else 0
        P = torch.empty((G, T, T), device=dev, dtype=torch.float32) if (need_p or (want_attn and pdrop == 0)) else None
        Pd = torch.empty((G, T, T), device=dev, dtype=torch.float32) if (want_attn and pdrop > 0) else None
        out = torch.empty_like(q)
        check(lib().vcv_rel_attn_fwd(ptr(q), ptr(k), ptr(v), ptr(embk), ptr(embv), ptr(mask), ptr(out), ptr(P), ptr(Pd),
                                     B, H, dk, T, window, qscale, pdrop, seed, bf, stream()), "vcv_rel_attn_fwd")
        LAUNCH_COUNTS["attn_fused"] += 1
        ctx.cfg = (H, window, qscale, pdrop, seed, bf)
        ctx.save_for_backward(q, k, v, embk, embv, mask, P, out)
        attn = None
        if want_attn:
            attn = (Pd if pdrop > 0 else P).view(B, H, T, T)
            ctx.mark_non_differentiable(attn)
        return out, attn

    @staticmethod
    def backward(ctx, dout, _dattn):
        q, k, v, embk, embv, mask, P, out = ctx.saved_tensors
        H, window, qscale, pdrop, seed, bf = ctx.cfg
        dout = _f32c(dout)
        B, C, T = q.shape
        dk = C // H
        # workspace: dS [G, T, T] + the per-(head, query tile) partial tables of the two table gradients
        dS = torch.empty((P.numel() + B * H * ((T + 31) // 32) * 2 * embk.shape[-2] * dk,), device=P.device, dtype=torch.float32)
        dq, dkk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dembk, dembv = torch.empty_like(embk), torch.empty_like(embv)
        # (the forward's output rides along: sum_j dPd Pd = sum_d dO out lets the row pass form dS tile by tile)
        check(lib().vcv_rel_attn_bwd2(ptr(q), ptr(k), ptr(v), ptr(embk), ptr(embv), ptr(mask), ptr(P), ptr(out), ptr(dout),
                                      ptr(dS), ptr(dq), ptr(dkk), ptr(dv), ptr(dembk), ptr(dembv), B, H, dk, T, window, qscale,
                                      pdrop, seed, bf, stream()), "vcv_rel_attn_bwd2")
        return dq, dkk, dv, dembk, dembv, None, None, None, None, None, None


# the fused attention kernels (attention.hip) take every shape they support; VCVITS_ATTN_FUSED=0 keeps the unfused path
_ATTN_FUSED = [tuning.flag("VCVITS_ATTN_FUSED", True, "relative-position attention as the fused MFMA kernels (0: the three-launch form)")]
# the streamed forward (attention_stream.hip) takes the no-grad, no-dropout, no-`attn` calls from this T on; the default is
# one frame past the fused kernels' longest T, so no call that reaches a fused kernel changes its bits
_ATTN_STREAM_MIN_T = [tuning.integer("VCVITS_ATTN_STREAM_MIN_T", 897, "shortest T at which no-grad relative-position attention "
                                     "runs on the streamed kernel (memory linear in T; 0: never)")]


# bf16 compute mode: the streamed forward kernels (this one and HuBERT's, ops.hubert) with bf16 operands on the bf16 matrix
# pipe (attention_stream_bf16.hip); 0 (the default): bf16 mode keeps the fp32-operand kernels and their bits
_ATTN_STREAM_BF16 = [tuning.integer("VCVITS_ATTN_STREAM_BF16", 0, "bf16 mode: streamed attention (relative-position at long T, HuBERT) "
                                    "with bf16 operands on the bf16 matrix pipe (0: fp32 operands in both modes)")]


def attn_stream_bf16():
    """True when a streamed attention call goes to the bf16-operand kernels: the switch is 1 and the compute dtype is bf16."""
    return _ATTN_STREAM_BF16[0] == 1 and _COMPUTE[0] == "bf16"


def _rel_attn_stream(q, k, v, embk, embv, mask, n_heads, window):
    """One launch of vcv_rel_attn_stream_fwd (or of its bf16-operand twin, see attn_stream_bf16): out [B, C, T], nothing of
    size T x T allocated."""
    q, k, v, embk, embv, mask = (_f32c(t) for t in (q, k, v, embk, embv, mask))
    B, C, T = q.shape
    dk = C // n_heads
    out = torch.empty_like(q)
    bf = attn_stream_bf16()
    name = "vcv_rel_attn_stream_fwd_bf16" if bf else "vcv_rel_attn_stream_fwd"
    check(getattr(lib(), name)(ptr(q), ptr(k), ptr(v), ptr(embk), ptr(embv), ptr(mask), ptr(out), B, n_heads, dk, T,
                               window, 1.0 / (dk ** 0.5), stream()), name)
    LAUNCH_COUNTS["attn_stream_bf16" if bf else "attn_stream"] += 1
    return out


class _RelAttnStreamFn(torch.autograd.Function):
    """Training through the streamed kernels (attention_stream_grad.hip): one launch forward that keeps two floats per query
    (running max, sum), and a backward pass that recomputes the probabilities from them in two passes.  Nothing of size
    T x T is allocated in either direction; the dropout mask is regenerated from the seed."""

    @staticmethod
    def forward(ctx, q, k, v, embk, embv, mask, n_heads, window, pdrop, seed):
        q, k, v, embk, embv, mask = (_f32c(t) for t in (q, k, v, embk, embv, mask))
        B, C, T = q.shape
        H = n_heads
        dk = C // H
        qscale = 1.0 / (dk ** 0.5)
        out = torch.empty_like(q)
        stats = torch.empty((B * H, T, 2), device=q.device, dtype=torch.float32)
        check(lib().vcv_rel_attn_stream_train_fwd(ptr(q), ptr(k), ptr(v), ptr(embk), ptr(embv), ptr(mask), ptr(out), ptr(stats),
                                                  B, H, dk, T, window, qscale, pdrop, seed, stream()), "vcv_rel_attn_stream_train_fwd")
        LAUNCH_COUNTS["attn_stream_grad"] += 1
        ctx.cfg = (H, window, qscale, pdrop, seed)
        ctx.save_for_backward(q, k, v, embk, embv, mask, out, stats)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, embk, embv, mask, out, stats = ctx.saved_tensors
        H, window, qscale, pdrop, seed = ctx.cfg
        dout = _f32c(dout)
        B, C, T = q.shape
        dk = C // H
        ws = torch.empty((lib().vcv_rel_attn_stream_bwd_workspace(B, H, dk, T, window),), device=q.device, dtype=torch.float32)
        dq, dkk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dembk, dembv = torch.empty_like(embk), torch.empty_like(embv)
        check(lib().vcv_rel_attn_stream_bwd(ptr(q), ptr(k), ptr(v), ptr(embk), ptr(embv), ptr(mask), ptr(out), ptr(stats), ptr(dout),
                                            ptr(ws), ptr(dq), ptr(dkk), ptr(dv), ptr(dembk), ptr(dembv), B, H, dk, T, window, qscale,
                                            pdrop, seed, stream()), "vcv_rel_attn_stream_bwd")
        return dq, dkk, dv, dembk, dembv, None, None, None, None, None


# the streamed TRAINING path (attention_stream_grad.hip) takes the calls with gradients and without `attn` from this T on,
# dropout included; 0 (the default): never, every call keeps the path it had
_ATTN_STREAM_GRAD_MIN_T = [tuning.integer("VCVITS_ATTN_STREAM_GRAD_MIN_T", 0, "shortest T at which relative-position attention "
                                          "with gradients runs on the streamed kernels (memory linear in T; 0: never)")]


def rel_attention(q, k, v, emb_rel_k, emb_rel_v, mask, n_heads, window, pdrop=0.0, training=False, want_attn=True):
    """Self-attention with shared-head windowed relative embeddings; mask [B,T] (key/query
    validity).  Returns (out [B,C,T], attn [B,H,T,T] -- None when want_attn is False on the fused path)."""
    p = float(pdrop) if training else 0.0
    seed = next_seed() if p > 0 else 0
    B, C, T = q.shape
    if p > 0 and DROPOUT_TRACE[0] is not None:
        DROPOUT_TRACE[0].append(("attn", p, seed, (B * n_heads, T, T)))
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v, emb_rel_k, emb_rel_v))
    if (needs_grad and not want_attn and 0 < _ATTN_STREAM_GRAD_MIN_T[0] <= T and
            lib().vcv_rel_attn_stream_supported(B, n_heads, C // n_heads, T, window) == 0):
        return _RelAttnStreamFn.apply(q, k, v, emb_rel_k, emb_rel_v, mask, n_heads, window, p, seed), None
    if (p == 0 and not want_attn and 0 < _ATTN_STREAM_MIN_T[0] <= T and
            not needs_grad and
            lib().vcv_rel_attn_stream_supported(B, n_heads, C // n_heads, T, window) == 0):
        return _rel_attn_stream(q, k, v, emb_rel_k, emb_rel_v, mask, n_heads, window), None
    if _ATTN_FUSED[0] and lib().vcv_rel_attn_supported(B, n_heads, C // n_heads, T, window) == 0:
        return _RelAttnFusedFn.apply(q, k, v, emb_rel_k, emb_rel_v, mask, n_heads, window, p, seed, bool(want_attn))
    return _RelAttnFn.apply(q, k, v, emb_rel_k, emb_rel_v, mask, n_heads, window, p, seed)

"""Restatements of the streaming glue of csrc/vits_blocks.hip (test oracle only): the WaveNet gate and residual / skip update,
the posterior split and sample, the mean-only coupling, the prior sample, the KL loss, nearest interpolation (plain and with
the map of other sizes), segment slicing, counter-based dropout, row sums and the channel LayerNorm.

Plain torch-CPU / numpy code in the dtype it is asked for, so the same text is the float64 yardstick and the float32
reference computation (d32 of tests/test_vits_glue_abi_gpu.py).  It shares no code with vcvits_amd.  Gradients are written
out by hand; tests/test_vits_glue_f64_cpu.py pins every one of them to torch autograd on the model's own formulas.

Layouts: activations [B, C, T]; mask [B, T]; the gate's conditioning vector g [B, gstride] with this layer's 2H values at goff.

One thing is NOT float64 on purpose: nearest_index.  F.interpolate(mode="nearest") computes floor(to * (Tin / Tout)) in
float32, and so do the kernels; the exact rational map to * Tin // Tout differs from it at thousands of (Tin, Tout) pairs
(the first: (2, 82), (2, 94), (2, 110)), so the index map is restated in float32 and pinned to torch.
"""
import numpy as np
import torch

import attention_f64 as A

F64 = torch.float64


def _to(t, dtype):
    return None if t is None else t.to(dtype)


def _bt(mask, dtype):
    """mask [B, T] -> [B, 1, T] in dtype"""
    return mask.to(dtype).unsqueeze(1)


# ---- WaveNet gate ------------------------------------------------------------------------------------------------------
def _gate_args(xin, g, goff, dtype):
    xin = xin.to(dtype)
    B, H2, _ = xin.shape
    H = H2 // 2
    a, b = xin[:, :H], xin[:, H:]
    if g is not None:
        g = g.to(dtype).reshape(B, -1)
        a = a + g[:, goff:goff + H, None]
        b = b + g[:, goff + H:goff + 2 * H, None]
    return a, b


def wn_gate(xin, g, goff, dtype=F64):
    """acts [B, H, T] = tanh(xin[:, :H] + g[goff : goff+H]) * sigmoid(xin[:, H:] + g[goff+H : goff+2H]); g may be None"""
    a, b = _gate_args(xin, g, goff, dtype)
    return torch.tanh(a) * torch.sigmoid(b)


def wn_gate_bwd(xin, g, goff, dacts, dtype=F64):
    """dxin [B, 2H, T] for the upstream gradient dacts"""
    a, b = _gate_args(xin, g, goff, dtype)
    th, sg, d = torch.tanh(a), torch.sigmoid(b), dacts.to(dtype)
    return torch.cat([d * sg * (1 - th * th), d * th * sg * (1 - sg)], 1)


def row_sum_index(R, inner, ostride, ooff):
    """the word of `out` row r is written to"""
    r = torch.arange(R)
    return (r // inner) * ostride + ooff + r % inner


def row_sum(x, R, T, inner, ostride, ooff, out_prior, dtype=F64):
    """out[(r // inner) * ostride + ooff + r % inner] = sum_t x[r, t]; every other word keeps its prior"""
    out = out_prior.to(dtype).clone().reshape(-1)
    out[row_sum_index(R, inner, ostride, ooff)] = x.to(dtype).reshape(R, T).sum(1)
    return out.reshape(out_prior.shape)


# ---- WaveNet residual / skip update ------------------------------------------------------------------------------------
def wn_res_skip(x, out, rs, mask, last, dtype=F64):
    """last = 0: rs [B, 2H, T] -> (x_new = (x + rs[:, :H]) * mask, out_new = out + rs[:, H:]);
    last = 1: rs [B, H, T] -> (None, out_new = out + rs).  out may be None (zeros)."""
    rs = rs.to(dtype)
    if last:
        return None, (rs if out is None else out.to(dtype) + rs)
    H = rs.shape[1] // 2
    o = rs[:, H:] if out is None else out.to(dtype) + rs[:, H:]
    return (x.to(dtype) + rs[:, :H]) * _bt(mask, dtype), o


def wn_res_skip_bwd(dxn, don, mask, shape, dtype=F64):
    """(drs [B, 2H, T], dx [B, H, T]) of the middle layer; dxn / don may be None (zeros)"""
    z = torch.zeros(shape, dtype=dtype)
    d = (z if dxn is None else dxn.to(dtype)) * _bt(mask, dtype)
    return torch.cat([d, z if don is None else don.to(dtype)], 1), d


# ---- posterior split / sample ------------------------------------------------------------------------------------------
def split_sample(stats, eps, mask, dtype=F64):
    """(m, logs) = split(stats * mask); z = (m + eps * exp(logs)) * mask, or None without eps"""
    C = stats.shape[1] // 2
    mk = _bt(mask, dtype)
    s = stats.to(dtype) * mk
    m, logs = s[:, :C], s[:, C:]
    z = None if eps is None else (m + eps.to(dtype) * torch.exp(logs)) * mk
    return m, logs, z


def split_sample_bwd(dm, dlogs, dz, eps, logs, mask, shape, dtype=F64):
    """dstats [B, 2C, T]; each of dm, dlogs, dz may be None (zeros); dz is ignored without eps.  `logs` is the forward's
    (masked) output."""
    mk = _bt(mask, dtype)
    z = torch.zeros(shape, dtype=dtype)
    gm = z if dm is None else dm.to(dtype)
    gl = z if dlogs is None else dlogs.to(dtype)
    if dz is not None and eps is not None:
        gz = dz.to(dtype) * mk
        gm = gm + gz
        gl = gl + gz * eps.to(dtype) * torch.exp(logs.to(dtype))
    return torch.cat([gm * mk, gl * mk], 1)


def coupling(x1, m, mask, reverse, dtype=F64):
    """forward: m + x1 * mask; reverse: (x1 - m) * mask"""
    mk = _bt(mask, dtype)
    return (x1.to(dtype) - m.to(dtype)) * mk if reverse else m.to(dtype) + x1.to(dtype) * mk


def prior_sample(m, logs, noise, noise_scale, dtype=F64):
    return m.to(dtype) + noise.to(dtype) * torch.exp(logs.to(dtype)) * noise_scale


# ---- KL loss -----------------------------------------------------------------------------------------------------------
def kl_terms(zp, lq, mp, lp, mask, dtype=F64):
    """(lp - lq - 0.5 + 0.5 (zp - mp)^2 exp(-2 lp)) * mask, per element"""
    zp, lq, mp, lp = (t.to(dtype) for t in (zp, lq, mp, lp))
    d = zp - mp
    return (lp - lq - 0.5 + 0.5 * d * d * torch.exp(-2.0 * lp)) * _bt(mask, dtype)


def kl(zp, lq, mp, lp, mask, dtype=F64):
    """(num, den): num = sum of kl_terms, den = sum(mask) over [B, T]; the loss is num / den"""
    return kl_terms(zp, lq, mp, lp, mask, dtype).sum(), mask.to(dtype).sum()


def kl_bwd(zp, mp, lp, mask, gout, den, dtype=F64):
    """(dzp, dlq, dmp, dlp) of num / den for the upstream gradient gout"""
    zp, mp, lp = (t.to(dtype) for t in (zp, mp, lp))
    k = (gout.to(dtype).reshape(()) / den.to(dtype).reshape(())) * _bt(mask, dtype)
    d = zp - mp
    e = torch.exp(-2.0 * lp)
    return k * d * e, (-k).expand_as(zp).clone(), -k * d * e, k * (1 - d * d * e)


# ---- nearest interpolation ---------------------------------------------------------------------------------------------
def nearest_index(Tin, Tout):
    """int64 [Tout]: floor(float32(to) * (float32(Tin) / float32(Tout))) in float32 arithmetic, clamped to Tin - 1"""
    scale = np.float32(Tin) / np.float32(Tout)
    prod = np.arange(Tout, dtype=np.float32) * scale
    assert prod.dtype == np.float32
    return torch.from_numpy(np.minimum(np.floor(prod).astype(np.int64), Tin - 1))


def nearest_raw_index(Tin, Tout, raw):
    """int64 [Tout], -1 where the output is zero: the map of the sizes raw = (Tin_raw, Tout_raw).  raw[0] <= 0 means Tin
    itself; zeros from raw[1] on; nothing at all if Tin_raw > Tin."""
    tir = int(raw[0]) if int(raw[0]) > 0 else Tin
    tor = int(raw[1])
    idx = torch.full((Tout,), -1, dtype=torch.int64)
    k = min(tor, Tout)
    if k > 0 and 0 < tir <= Tin:
        idx[:k] = nearest_index(tir, tor)[:k]
    return idx


def gather_t(x, idx, dtype=F64):
    """y[..., to] = x[..., idx[to]], 0 where idx < 0"""
    y = x.to(dtype)[..., idx.clamp(min=0)]
    return y * (idx >= 0).to(dtype)


def scatter_t(dy, idx, Tin, dtype=F64):
    """dx[..., ti] = sum of dy[..., to] over idx[to] == ti"""
    dy = dy.to(dtype) * (idx >= 0).to(dtype)
    dx = torch.zeros(dy.shape[:-1] + (Tin,), dtype=dtype)
    return dx.index_add_(dy.dim() - 1, idx.clamp(min=0), dy)


def nearest(x, Tout, dtype=F64):
    return gather_t(x, nearest_index(x.shape[-1], Tout), dtype)


def nearest_bwd(dy, Tin, dtype=F64):
    return scatter_t(dy, nearest_index(Tin, dy.shape[-1]), Tin, dtype)


def nearest_raw(x, Tout, raw, dtype=F64):
    return gather_t(x, nearest_raw_index(x.shape[-1], Tout, raw), dtype)


def nearest_raw_bwd(dy, Tin, raw, dtype=F64):
    return scatter_t(dy, nearest_raw_index(Tin, dy.shape[-1], raw), Tin, dtype)


# ---- segment slicing ---------------------------------------------------------------------------------------------------
def _slice_pos(ids, mul, S, T):
    t = ids.to(torch.int64).reshape(-1, 1) * mul + torch.arange(S)  # [B, S]
    return t, (t >= 0) & (t < T)


def slice(x, ids, mul, S, dtype=F64):
    """y[b, c, s] = x[b, c, ids[b] * mul + s], 0 outside [0, T)"""
    B, C, T = x.shape
    t, ok = _slice_pos(ids, mul, S, T)
    y = torch.gather(x.to(dtype), 2, t.clamp(0, T - 1).unsqueeze(1).expand(B, C, S))
    return y * ok.unsqueeze(1).to(dtype)


def slice_bwd(dy, ids, mul, T, dtype=F64):
    """dx [B, C, T]: zeros, the in-range positions written"""
    B, C, S = dy.shape
    t, ok = _slice_pos(ids, mul, S, T)
    dx = torch.zeros(B, C, T, dtype=dtype)
    for b in range(B):
        dx[b][:, t[b][ok[b]]] = dy[b].to(dtype)[:, ok[b]]
    return dx


# ---- dropout -----------------------------------------------------------------------------------------------------------
def dropout(x, p, seed, dtype=F64):
    """x * keep(seed, flat index) / (1 - p): the hash and the float32 factor of attention_f64"""
    keep = torch.from_numpy(A.keep_mask(seed, x.numel(), p)).reshape(x.shape)
    return x.to(dtype) * (keep.to(dtype) * A.inv_keep(p))


# ---- channel LayerNorm of x + y ----------------------------------------------------------------------------------------
def layernorm_c(x, y, gamma, beta, eps, dtype=F64):
    """(out [B, C, T], mean [B, T], rstd [B, T]) of LayerNorm over C of x + y (y may be None), biased variance"""
    v = x.to(dtype) if y is None else x.to(dtype) + y.to(dtype)
    mean = v.mean(1)
    var = ((v - mean.unsqueeze(1)) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (v - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    return xh * gamma.to(dtype)[None, :, None] + beta.to(dtype)[None, :, None], mean, rstd


def layernorm_c_bwd(x, y, gamma, dout, eps, dtype=F64):
    """(dx, dgamma, dbeta); the gradient of y, where there is one, is dx"""
    v = x.to(dtype) if y is None else x.to(dtype) + y.to(dtype)
    mean = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (v - mean) * rstd
    d = dout.to(dtype)
    g = d * gamma.to(dtype)[None, :, None]
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, (d * xh).sum((0, 2)), d.sum((0, 2))

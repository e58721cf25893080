"""Restatement of the relative-position self-attention at the op level (test oracle only).

vits/model/transformer/relative_attention_transformer.py:150-182 between the four 1x1 convolutions: q, k, v [B, H*dk, T] in,
the attention output [B, H*dk, T] out, with the shared-head relative tables embk / embv [1, 2w+1, dk] and the validity mask
[B, T].  Plain torch-CPU code with explicit band indexing (no pad / reshape skew), in the dtype it is asked for, so the same
text is the float64 yardstick and the float32 reference computation.  It shares no code with vcvits_amd.

Points decided here (the kernels of csrc/attention.hip and the unfused path of csrc/vits_blocks.hip follow this file):
 1. scores[i][j] = (q_i / sqrt(dk)) . k_j + (q_i / sqrt(dk)) . embk[j - i + w] for |j - i| <= w.
 2. scores.masked_fill(mask_i * mask_j == 0, -1e4), softmax over j.  A masked query row has every score at -1e4: it is
    uniform over all T keys, the masked ones included.  A masked key of an unmasked query gets exp(-1e4 - max) = 0, in
    float32 and in float64 alike.
 3. dropout is a GIVEN keep mask [B*H, T, T]: Pd = P * keep * f with f = 1 / (1 - p) formed in float32, as the kernels do.
 4. out_i = sum_j Pd[i][j] v_j + sum_{|j - i| <= w} Pd[i][j] embv[j - i + w].
 5. gradients: autograd of the above for the upstream gradient dO (the masked_fill sends no gradient into a masked score).

keep_mask restates the counter-based generator of the kernels (`drop_scale`, attention.hip; the same stream in vits_blocks.hip)
in numpy uint64: integer arithmetic, so it is exact.
"""
import collections
import math

import numpy as np
import torch

Result = collections.namedtuple("Result", "out P Pd dq dk dv dembk dembv")
NAMES = Result._fields


def inv_keep(p):
    """1 / (1 - p) as the kernels form it: float32 operands, float32 division."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def keep_mask(seed, n, p):
    """keep[idx] for idx = 0 .. n - 1 of the dropout draw (seed, p): splitmix64 of seed + idx * golden ratio (mod 2^64),
    u = (z >> 40) * 2^-24 (exact in float32: 24 bits), keep iff u >= float32(p).  The attention probabilities [B*H, T, T] use
    idx = (g * T + i) * T + j, their flat index."""
    with np.errstate(over="ignore"):
        z = np.full(n, int(seed) % (1 << 64), dtype=np.uint64) + np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def band_index(T, w):
    """off[i][j] = j - i + w clamped into the table, and whether (i, j) lies in the band."""
    i = torch.arange(T).unsqueeze(1)
    j = torch.arange(T).unsqueeze(0)
    off = j - i + w
    return off.clamp(0, 2 * w), (off >= 0) & (off <= 2 * w)


def rel_attention(q, k, v, embk, embv, mask, dO=None, dtype=torch.float64, keep=None, p=0.0):
    """-> Result(out [B, H*dk, T], P, Pd [B*H, T, T], dq, dk, dv [B, H*dk, T], dembk, dembv [1, 2w+1, dk]) in `dtype`; the
    gradients are None without dO.  keep: bool / 0-1 tensor or array [B*H, T, T] (None: no dropout, Pd is P)."""
    B, C, T = q.shape
    nr, dk = embk.shape[-2], embk.shape[-1]
    w, H = (nr - 1) // 2, C // dk
    assert C == H * dk and nr == 2 * w + 1 and tuple(mask.shape) == (B, T)
    lq, lk, lv, lek, lev = (t.detach().to("cpu", dtype).clone().requires_grad_(dO is not None) for t in (q, k, v, embk, embv))
    m = mask.detach().to("cpu", dtype)
    qs = lq.view(B, H, dk, T).transpose(2, 3) / math.sqrt(dk)
    kh = lk.view(B, H, dk, T).transpose(2, 3)
    vh = lv.view(B, H, dk, T).transpose(2, 3)
    offc, band = band_index(T, w)
    scores = qs @ kh.transpose(2, 3)
    rel = qs @ lek[0].t()                                           # [B, H, T, 2w+1]
    scores = scores + torch.gather(rel, 3, offc.expand(B, H, T, T)) * band
    am = (m.unsqueeze(2) * m.unsqueeze(1)).unsqueeze(1)             # [B, 1, T, T]: mask_i * mask_j
    P = torch.softmax(scores.masked_fill(am == 0, -1e4), dim=-1)
    if keep is None:
        Pd = P
    else:
        kp = torch.as_tensor(np.asarray(keep)).reshape(B, H, T, T).to(dtype)
        Pd = P * kp * inv_keep(p)
    # relative values: pw[i][r] = Pd[i][i + r - w] where that key exists
    jr = torch.arange(T).unsqueeze(1) + torch.arange(nr).unsqueeze(0) - w  # [T, 2w+1]
    ok = (jr >= 0) & (jr < T)
    pw = torch.gather(Pd, 3, jr.clamp(0, T - 1).expand(B, H, T, nr)) * ok
    out = (Pd @ vh + pw @ lev[0]).transpose(2, 3).reshape(B, C, T)
    grads = (None,) * 5
    if dO is not None:
        grads = torch.autograd.grad(out, (lq, lk, lv, lek, lev), dO.detach().to("cpu", dtype))
    return Result(out.detach(), P.detach().reshape(B * H, T, T), Pd.detach().reshape(B * H, T, T), *grads)


def dist(a, b):
    """max|a - b| / max|b|, the distance of the project's attention tests."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-300)

"""Cases, inputs, references and the bound of the streamed training attention (csrc/attention_stream_grad.hip), shared by
tests/test_attention_stream_grad_cpu.py and tests/test_attention_stream_grad_gpu.py.  No test lives here.

Inputs are those of tests/test_attention_stream_gpu.py (q scaled by 2) plus a standard-normal dO.  The reference is
tests/attention_f64.py on float64 copies of the float32 inputs with keep_mask(seed, ...) as an input; d32 is the distance of its
float32 run from its float64 run.  Bound, the policy of tests/test_attention_abi_gpu.py: max(16 * d32, 2e-6), capped at 1e-4
(2e-4 for dembk / dembv).
"""
import functools
import math
import zlib

import numpy as np
import torch

import attention_f64 as A
import test_attention_stream_gpu as SG

Case, cid, make_mask = SG.Case, SG.cid, SG.make_mask
FACTOR, FLOOR, CAP, CAP_TABLE = 16, 2e-6, 1e-4, 2e-4
QB, QW, KT = 128, 32, 32  # lanes per workgroup, per wave; rows per streamed tile (queries and keys swap roles in the key pass)
GRADS = ("dq", "dk", "dv", "dembk", "dembv")

CASES = [
    Case(1, 1, 32, 1, 4, "ones"),              # one query, one key
    Case(2, 1, 32, 5, 7, "ragged"),            # T <= w
    Case(2, 2, 64, 32, 0, "hole"),             # w = 0, one exact tile
    Case(2, 1, 64, 33, 4, "ragged"),           # one key in the second tile
    Case(1, 2, 32, 128, 4, "ones"),            # one block
    Case(2, 1, 32, 129, 7, "ragged+hole"),     # band across wave and block
    Case(3, 1, 64, 257, 4, "mixed"),           # an all-masked batch row
    Case(2, 2, 64, 897, 4, "ragged+hole"),
    Case(1, 2, 32, 1030, 4, "head40"),         # first tile wholly masked; 33 tiles, odd tail
]
C129, C257 = CASES[5], CASES[6]
BIG_SEED = (1 << 63) + 0x1234567
HALF = (CASES[3], C129)  # the two cases that also run at p = 0.5


def seed_of(c):
    return zlib.crc32(("seed" + repr(tuple(c))).encode()) * 2654435761 + 17


# (case, p, seed)
RUNS = [(c, p, seed_of(c)) for c in CASES for p in (0.0, 0.1)] + [(c, 0.5, seed_of(c)) for c in HALF] + [(C129, 0.1, BIG_SEED)]
run_id = lambda r: "%s-p%g%s" % (cid(r[0]), r[1], "-seed2^63" if r[2] == BIG_SEED else "")


@functools.lru_cache(maxsize=None)
def inputs(c):
    """q, k, v, embk, embv, mask of tests/test_attention_stream_gpu.py, and dO (float32, CPU)"""
    rng = np.random.default_rng(zlib.crc32(("dO" + repr(tuple(c))).encode()))
    dO = torch.from_numpy(rng.standard_normal((c.B, c.H * c.dk, c.T)).astype(np.float32))
    return SG.inputs(c) + (dO,)


@functools.lru_cache(maxsize=None)
def keep_of(c, p, seed):
    if p == 0:
        return None
    G, T = c.B * c.H, c.T
    return torch.from_numpy(A.keep_mask(seed, G * T * T, p).reshape(G, T, T))


def row_stats(q, k, embk, mask, dtype=torch.float64):
    """-> scores [B*H, T, T] (filled), m [B*H, T] = max_j, l [B*H, T] = sum_j exp(s - m): what the training forward leaves
    per query.  tests/attention_f64.py points 1 and 2 restated; the CPU test ties exp(s - m) / l to that file's P."""
    B, C, T = q.shape
    nr, dk = embk.shape[-2], embk.shape[-1]
    w, H = (nr - 1) // 2, C // dk
    qs = q.to(dtype).view(B, H, dk, T).transpose(2, 3) / math.sqrt(dk)
    kh = k.to(dtype).view(B, H, dk, T).transpose(2, 3)
    offc, band = A.band_index(T, w)
    rel = qs @ embk[0].to(dtype).t()
    s = qs @ kh.transpose(2, 3) + torch.gather(rel, 3, offc.expand(B, H, T, T)) * band
    m_ = mask.to(dtype)
    s = s.masked_fill(((m_.unsqueeze(2) * m_.unsqueeze(1)).unsqueeze(1)) == 0, -1e4).reshape(B * H, T, T)
    m = s.max(dim=2).values
    return s, m, torch.exp(s - m.unsqueeze(2)).sum(2)


def lse64(m, l):
    """m + log l, combined in float64 whatever the parts were computed in"""
    return m.detach().cpu().double() + torch.log(l.detach().cpu().double())


def stats_dist(m, l, m_ref, l_ref):
    """max_i |expm1((m + log l) - (m + log l)_ref)|: the relative error of the softmax denominator"""
    return torch.expm1(lse64(m, l) - lse64(m_ref, l_ref)).abs().max().item()


@functools.lru_cache(maxsize=None)
def reference(c, p, seed):
    """(float64 Result, {tensor: d32}, (m, l) float64, d32 of the stats)"""
    q, k, v, ek, ev, mask, dO = inputs(c)
    keep = keep_of(c, p, seed)
    r64 = A.rel_attention(q, k, v, ek, ev, mask, dO, torch.float64, keep, p)
    r32 = A.rel_attention(q, k, v, ek, ev, mask, dO, torch.float32, keep, p)
    d32 = {n: A.dist(a, b) for n, a, b in zip(A.NAMES, r32, r64)}
    _, m64, l64 = row_stats(q, k, ek, mask, torch.float64)
    _, m32, l32 = row_stats(q, k, ek, mask, torch.float32)
    return r64, d32, (m64, l64), stats_dist(m32, l32, m64, l64)


def cap(name):
    return CAP_TABLE if name.startswith("demb") else CAP


def bound(name, d32):
    return min(max(FACTOR * d32, FLOOR), cap(name))


def cancel_scale(c, ref):
    """T = 1: dq, dk and dembk are exactly zero in the reference (the softmax of one score has no derivative); the kernels
    form dS = P (c dPd - delta) from two equal numbers summed in different orders, times qscale and q, k or embk.  Measured
    against qscale * max|delta| * max(|q|, |k|, |embk|), as tests/test_attention_abi_gpu.py does."""
    q, k, _, ek, _, _, dO = inputs(c)
    dot = (dO.double() * ref.out).view(c.B, c.H, c.dk, c.T).sum(2).abs().max().item()
    return c.dk ** -0.5 * dot * max(t.abs().max().item() for t in (q, k, ek)) + 1e-300

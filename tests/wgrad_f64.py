"""Restatement of the conv family's weight gradient at the C ABI (test oracle only), and of the launcher rules of
csrc/wgrad_bf16.hip.

1. The formula of include/vcvits_hip.h (VcvWgradArgs, G = 1), by explicit index gather -- no torch.nn.functional.conv*:
     dw[m, c, k] = sum_{b, q, p} tfa(a[b, m, q, p]) * tfb(x[b, c, q * s + k * dj + off, p]),  rows outside [0, Tb) read zero
   in the dtype it is asked for, so the same text is the float64 yardstick and the float32 reference computation.
   The derivative transforms of vcv_thin_wgrad (DLEAKY / DRELU / DTANH / DLOGCLAMP, each a function of an aux tensor of the
   operand's shape) are restated here too; the MFMA kernels refuse them.  wgrad_mag() is the sum of magnitudes behind every
   element, which scales the element-wise rounding bound of tests/test_conv_thin_abi_gpu.py.
   rounded=True rounds every operand to bf16 AFTER its leaky-ReLU (which the kernel forms in float32: fmaxf(f, f * slope)),
   as the bf16 entry point does, before the sum.  dbias(a) is the row sum of the UNROUNDED `a`: the kernel takes it from its
   fp32 staging registers in both arithmetics.
2. pick(), geometry(), the KT rule, scratch_want(), the cost-model split and the finish-kernel choice of launch(), as plain
   integer arithmetic: what the library decides for a VcvWgradArgs, without the library.  tests/test_wgrad_mfma_abi_gpu.py
   pins this restatement to vcv_wgrad_*_scratch and uses it to prove which branches its case table reaches.

Shares no code with vcvits_amd."""
import collections
import math

import torch

TF_NONE, TF_LEAKY, TF_DLEAKY, TF_DRELU, TF_DTANH, TF_DLOGCLAMP = 0, 1, 2, 3, 4, 5  # include/vcvits_hip.h


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------
def bf16_round(t):
    """float32 -> nearest bf16 (ties to even), as a float32 tensor."""
    return t.float().bfloat16().float()


def operand(t, tf, slope, rounded, dtype, aux=None):
    """tf(t) as the kernel sees it.  rounded: leaky-ReLU in float32 as the kernel forms it, then bf16.  aux: the tensor the
    derivative transforms are a function of (the activation's output; for the leaky-ReLU its input has the same sign)."""
    t = t.detach().cpu()
    if rounded:
        assert tf in (TF_NONE, TF_LEAKY)
        t = t.float()
        if tf == TF_LEAKY:
            t = torch.maximum(t, t * torch.tensor(slope, dtype=torch.float32))
        return bf16_round(t).to(dtype)
    t = t.to(dtype)
    if tf == TF_LEAKY:
        # the float32 NUMBER the library is handed as slope (the exact pass uses 0.5; 0.1 is not a float32)
        t = torch.maximum(t, t * float(torch.tensor(slope, dtype=torch.float32)))
    elif tf != TF_NONE:
        sl = float(torch.tensor(slope, dtype=torch.float32))
        x = aux.detach().cpu().to(dtype)
        assert x.shape == t.shape
        if tf == TF_DLEAKY:
            t = t * torch.where(x > 0, torch.ones_like(x), torch.full_like(x, sl))
        elif tf == TF_DRELU:
            t = torch.where(x > 0, t, torch.zeros_like(t))
        elif tf == TF_DTANH:
            t = t * (1 - x * x)
        elif tf == TF_DLOGCLAMP:
            t = torch.where(x > math.log(sl), t * torch.exp(-x), torch.zeros_like(t))
        else:
            raise ValueError("transform %r" % (tf,))
    return t


def wgrad(a, b, K, s, dj, off, a_tf=TF_NONE, b_tf=TF_NONE, slope=0.1, rounded=False, dtype=torch.float64, aaux=None, baux=None,
          magnitudes=False):
    """a [B, M, Ta, P], b [B, C, Tb, P] -> dw [M, C, K] in `dtype`.  magnitudes: sum |tfa(a)| |tfb(b)| instead."""
    assert a.dim() == 4 and b.dim() == 4 and a.shape[0] == b.shape[0] and a.shape[3] == b.shape[3]
    Ta, Tb = a.shape[2], b.shape[2]
    ta = operand(a, a_tf, slope, rounded, dtype, aaux)
    tb = operand(b, b_tf, slope, rounded, dtype, baux)
    if magnitudes:
        ta, tb = ta.abs(), tb.abs()
    dw = torch.zeros(a.shape[1], b.shape[1], K, dtype=dtype)
    q = torch.arange(Ta)
    for k in range(K):
        rows = q * s + k * dj + off
        ok = (rows >= 0) & (rows < Tb)
        if not bool(ok.any()):
            continue
        xk = tb[:, :, rows.clamp(0, Tb - 1), :] * ok.to(dtype).view(1, 1, Ta, 1)  # [B, C, Ta, P]
        dw[:, :, k] = torch.einsum("bmqp,bcqp->mc", ta, xk)
    return dw


def wgrad_mag(a, b, K, s, dj, off, **kw):
    """S[m, c, k] = sum |tfa(a)| |tfb(b)| in float64"""
    return wgrad(a, b, K, s, dj, off, magnitudes=True, dtype=torch.float64, **kw)


def dbias(a, dtype=torch.float64):
    return a.detach().cpu().to(dtype).sum((0, 2, 3))


def dist(got, ref):
    """max|got - ref| / max|ref|"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the launcher's rules (wgrad_bf16.hip)
# ---------------------------------------------------------------------------------------------------------------------
Args = collections.namedtuple("Args", "B Mg Cg Ta Tb P K s dj off a_tf b_tf slope G transpose_out",
                              defaults=(TF_NONE, TF_NONE, 0.1, 1, 0))
CAND = ((4, 2, 1), (4, 1, 2), (2, 2, 2), (2, 1, 4), (1, 2, 4), (1, 1, 8))  # (WM, WC, WU), widest tile first
LDS_LIMIT = 160 * 1024
MAXT, MAXT_WS = 2, 3
Plan = collections.namedtuple("Plan", "cand WM WC WU KT BU ntg kn_last nmt nct XR nchunk_u total tiles n lds want")


def cdiv(a, b):
    return -(-a // b)


def kt_of(K, PL):
    kt = 1 if K == 1 else 3 if K <= 3 else 5 if K <= 5 else 8 if (K in (7, 8) or K >= 15) else 6
    return 4 if (PL == 3 and kt == 8) else kt  # (three term planes: the 8-tap groups run as 4-tap groups)


def geometry(a, cand, KT, PL, ws=True):
    """-> dict(nmt, nct, ntg, XR, nchunk_u, lds, BU), or why the candidate does not fit: "lds", "tasks" (staging budget) or "wu"
    (a 32-position stage has two 16-position steps).  ws: tuning key wgrad_bf16_ws (the three-plane launches always have
    producer waves)."""
    WM, WC, WU = CAND[cand]
    BU = 64 if PL == 1 else 32
    ws = ws or PL == 3
    NW = WM * WC * WU
    NS, maxt = (4, MAXT_WS) if ws else (NW, MAXT)
    BM, BC = 32 * WM, 32 * WC
    adj = abs(a.dj)
    qspan = (BU - 1) // a.P + 1
    kspan = min(KT, a.K) - 1
    rowmax = (qspan * a.s + kspan * adj + 1) * a.P
    XR = (rowmax + 3 + 63) & ~63
    pitch = lambda w: w * 2 + 64 if w * 2 >= 128 else w * 2
    pa, pb = pitch(BM), pitch(BC)
    buf = PL * BU * pa + PL * XR * pb + BU * 4
    lds = 2 * buf
    red = WM * WC * KT * 16 * 64 * 4 if WU > 1 else 0
    lds = max(lds, red)
    if lds > LDS_LIMIT:
        return "lds"
    if BM // 32 + (BC // 32) * (XR // 64) > maxt * NS:
        return "tasks"
    if PL == 3 and BU // 16 < WU:
        return "wu"
    return dict(nmt=cdiv(a.Mg, BM), nct=cdiv(a.Cg, BC), ntg=cdiv(a.K, KT), XR=XR, nchunk_u=cdiv(a.Ta * a.P, BU), lds=lds, BU=BU)


def pick(a, PL, x3_all=True, force_cand=-1, ws=True):
    """-> Plan, or None where the launcher refuses (vcv_wgrad_*_scratch returns 0, the run call VCV_EINVAL)."""
    tf_ok = a.a_tf in (TF_NONE, TF_LEAKY) and a.b_tf in (TF_NONE, TF_LEAKY) and 0.0 <= a.slope < 1.0
    U = a.Ta * a.P
    if a.G != 1 or not tf_ok or a.transpose_out or a.Mg < 32 or a.Cg < 16 or a.K > 16 or U * a.B < 256 or a.s < 1 or a.s > 3:
        return None
    if U * 4 >= 1 << 31 or a.Tb * a.P * 4 >= 1 << 31:
        return None
    KT = kt_of(a.K, PL)
    for i, (WM, WC, WU) in enumerate(CAND):
        if force_cand >= 0 and i != force_cand:
            continue
        bm, bc = 32 * WM, 32 * WC
        if bm > 32 and bm > a.Mg:
            continue
        if bc > 32 and bc > ((a.Cg + 31) & ~31):
            continue
        g = geometry(a, i, KT, PL, ws)
        if not isinstance(g, dict):
            continue
        if PL == 3 and not x3_all and not (WC == 2 and (a.K == 5 or a.K >= 9)):
            return None
        total = a.B * g["nchunk_u"]
        tiles = g["nmt"] * g["nct"] * g["ntg"]
        n = a.Mg * a.Cg * a.K
        z = max(1, min(cdiv(512, tiles), total))
        while z > 1 and z * n > (64 << 20):
            z -= 1
        z = min(z, 512)
        return Plan(i, WM, WC, WU, KT, g["BU"], g["ntg"], a.K - (g["ntg"] - 1) * KT, g["nmt"], g["nct"], g["XR"], g["nchunk_u"], total,
                    tiles, n, g["lds"], z * n)
    return None


def split(plan, scratch_floats, force_z=-1):
    """Z of launch(): the cost model over the splits the scratch allows, or the forced count clamped to scratch and stages."""
    occ = 2 if plan.lds * 2 <= LDS_LIMIT else 1
    slots = 256 * occ
    Z, best = 1, 1e30
    z = 1
    while z <= plan.total and z <= 512:
        if z * plan.n > scratch_floats:
            break
        rounds = float((plan.tiles * z + slots - 1) // slots)
        cost = rounds * (float((plan.total + z - 1) // z) + 2.0) / float(occ) + 0.02 * z
        if cost < best - 1e-9:
            best, Z = cost, z
        z += 1
    if force_z > 0:
        Z = force_z
        while Z > 1 and (Z * plan.n > scratch_floats or Z > plan.total):
            Z -= 1
    return Z


def finish_kernel(Z, K, Cg, aligned=True, finish_vec=True):
    """Which finishing kernel launch() takes: ("finish4", ZG, KB), ("rows",) (each 32-lane group walks all Z slabs of its own
    m row: Z <= 12) or ("zlanes",) (the 8 groups are z-lanes of one m row)."""
    if finish_vec and Cg % 4 == 0 and aligned:
        zg = 4 if Z <= 4 else 8 if Z <= 8 else 16 if Z <= 16 else 32
        kb = 1 if K <= 1 else 3 if K <= 3 else 5 if K <= 5 else 8 if K <= 8 else 11 if K <= 11 else 16
        return ("finish4", zg, kb)
    return ("rows",) if Z <= 12 else ("zlanes",)


def span_starts(a, plan):
    """First staged x position (before the kernel rounds it down to a multiple of 4) of every (tap group, stage of one
    batch element)."""
    out = []
    for tgi in range(plan.ntg):
        k0 = tgi * plan.KT
        kn = min(plan.KT, a.K - k0)
        tap_lo = k0 * a.dj if a.dj >= 0 else (k0 + kn - 1) * a.dj
        for st in range(plan.nchunk_u):
            qa = st * plan.BU // a.P
            out.append((qa * a.s + a.off + tap_lo) * a.P)
    return out

"""The MFMA weight-gradient kernel (csrc/wgrad_bf16.hip: one templated kernel and three finishing kernels behind vcv_wgrad_bf16
and vcv_wgrad_x3) at the edges of its launcher, against a float64 CPU reference of the same operation (tests/wgrad_f64.py).

The kernel is called THROUGH THE C ABI with a hand-filled VcvWgradArgs, so the routing of ops.conv_wgrad cannot send a case
elsewhere; test_routing_* then check that ops.conv_wgrad / ops.convT_wgrad reach the same kernel (same bits) and which shapes
the default setting hands to it.

Arithmetics: "bf16" (vcv_wgrad_bf16: operands rounded to bf16, reference = float64 sum of the ROUNDED operands), "x3-9" and
"x3-6" (vcv_wgrad_x3 with 9 / 6 product terms: exact fp32 operands, reference = float64 sum of the operands as they are).
vcv_conv_x3_set_all(1) admits every eligible shape; terms and the all-shapes setting are restored in `finally`.

Distances are max|got - ref| / max|ref|.  Bounds are the project's own: 1e-5 for bf16 dw (TOL_BF16 of
tests/test_switch_parity_gpu.py), 3e-5 for x3 dw (TOL_DW), 2e-5 for dbias.  Every case writes its distances to
profiles/wgrad_mfma_parity.txt next to d32, the distance of the FLOAT32 CPU run of the same reference from its float64 run.

kind = "exact" is a tolerance-free pass over the same cases: operands are integers in [-8, 8] (exact in bf16 and in the first
term plane), `b` goes through leaky-ReLU with slope 0.5, alpha = 0.5, dw and dbias are preloaded with integers; every partial
sum is a multiple of 1/4 far below 2^24 / 4 (test_case_table_reaches_every_branch asserts 8 * 8 * B * U < 2^24 / 4), so any
summation order is exact and the result must be BIT-EQUAL to the float64 reference cast to float32.

dw, dbias and the scratch are views inside larger buffers with 1024 sentinel floats on each side, which must be untouched
after the call; the scratch is pre-filled with NaN, so a slab word the finishing pass reads but no workgroup wrote shows in dw.
Every launch is made twice: dw must be bit-identical (slabs added in a fixed order).  dbias is collected with fp32 atomics
by the blocks of one (channel tile, tap group), in an order that varies: it is held to its bound on both launches, and to
bit-equality only in the exact pass.  dbias together with a_tf = LEAKY is outside the header's contract (the row sums are
taken before the transform) and is not tested.

No case is skipped: the table says for every case which arithmetics are eligible ("bx" both, "b" bf16 only, "-" none), the
restated rules must agree, and the library must report scratch > 0 exactly for those.

Notes on the table: (4, 63, 1) of the position edges has B * U = 252, below pick()'s 256, so it is a refusal case (both
arithmetics ineligible) and is tested as one; the offset group at Mg 64 / Cg 32 is bf16-only by the three-plane rule BU / 16 < WU, so four of its rows are repeated at Mg 128 ("D128", candidate 1) to put
negative tap steps, a stride and masked taps under the three-plane form too; the strided and wide-period rows of the position
edges are bf16-only at 64 output channels for the same reason (the 64 x 64 tile's three-plane images pass the LDS limit), so
three of them are repeated at Mg 128 ("C128"); and the widest period at Mg 128 is the only way to a fall-through from
candidate 0 because of LDS."""
import collections
import contextlib
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_f64 as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
TOL_BF16, TOL_DW, TOL_DB = 1e-5, 3e-5, 2e-5
GUARD, SENT = 1024, 12345.0
ARITHS = ("bf16", "x3-9", "x3-6")
PL_OF = {"bf16": 1, "x3-9": 3, "x3-6": 3}
KINDS = ("normal", "exact")

Case = collections.namedtuple("Case", "grp B Mg Cg Ta Tb P K s dj off")


def conv_tb(Ta, K, s, pad, dil=1):
    """input rows of the Conv whose output has Ta rows (no rows left over)"""
    return (Ta - 1) * s + (K - 1) * dil + 1 - 2 * pad


def fit_tb(Ta, K, s, dj, off):
    """the fewest rows of `b` that every tap of every position finds in range at the top end"""
    return (Ta - 1) * s + max(0, (K - 1) * dj) + off + 1


def convT_tb(Ta, K, s, pad):
    return (Ta - 1) * s - 2 * pad + K


def args_of(c, **kw):
    return W.Args(c.B, c.Mg, c.Cg, c.Ta, c.Tb, c.P, c.K, c.s, c.dj, c.off, **kw)


def cid(c):
    return "%s-B%d-M%d-C%d-Ta%d-Tb%d-P%d-K%d-s%d-dj%d-off%d" % tuple(c)


# ---------------------------------------------------------------------------------------------------------------------
# the case table: (case, eligible arithmetics)
# ---------------------------------------------------------------------------------------------------------------------
TABLE = []


def row(elig, grp, B, Mg, Cg, Ta, Tb, P, K, s, dj, off):
    c = Case(grp, B, Mg, Cg, Ta, Tb, P, K, s, dj, off)
    assert c not in [t[0] for t in TABLE], c
    TABLE.append((c, elig))
    return c


# A. tap groups
A_K = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 16)
GROUP_A = [row("bx", "A", 2, 64, 64, 130, conv_tb(130, K, 1, K // 2), 1, K, 1, 1, -(K // 2)) for K in A_K]
# B. channel tails; Mg < 64 leaves only the 32-row tiles, whose 4 / 8 position-split waves a 32-position stage cannot feed
B_MC = ((32, 16, "b"), (33, 17, "b"), (40, 20, "b"), (63, 31, "b"), (64, 33, "bx"), (96, 48, "bx"), (100, 66, "bx"), (128, 64, "bx"),
        (130, 130, "bx"), (160, 132, "bx"))
GROUP_B = [row(e, "B", 2, Mg, Cg, 130, 130, 1, 3, 1, 1, -1) for Mg, Cg, e in B_MC]
# C. position edges (K 5, pad 2); the P > 1 rows also at stride 3 (the period layers' roles), (2, 43, 3) at stride 2
C_BTP = ((1, 256, 1, "bx"), (1, 257, 1, "bx"), (4, 64, 1, "bx"), (4, 63, 1, "-"), (8, 32, 1, "bx"), (8, 33, 1, "bx"), (16, 16, 1, "bx"),
         (37, 7, 1, "bx"), (2, 64, 2, "bx"), (2, 43, 3, "bx"), (2, 10, 13, "b"), (3, 3, 37, "b"))
GROUP_C = [row(e, "C", B, 64, 64, Ta, conv_tb(Ta, 5, 1, 2), P, 5, 1, 1, -2) for B, Ta, P, e in C_BTP]
# (three term planes, 64 x 64 tile: the x image of a strided or wide-period stage does not fit the LDS, and the narrower tiles
# have too many position-split waves -- bf16 only at 64 output channels)
C_S3 = ((2, 64, 2, "b"), (2, 43, 3, "b"), (2, 10, 13, "b"), (3, 3, 37, "b"))
GROUP_C += [row(e, "C", B, 64, 64, Ta, conv_tb(Ta, 5, 3, 2), P, 5, 3, 1, -2) for B, Ta, P, e in C_S3]
C_2_43_3_S3 = GROUP_C[-3]
GROUP_C.append(row("b", "C", 2, 64, 64, 43, conv_tb(43, 5, 2, 2), 3, 5, 2, 1, -2))
# the widest period at 128 output channels: candidate 0's images do not fit the LDS, candidate 1 (128 x 32) does; and three
# period rows at 128 output channels, where the three-plane form has a tile (candidate 1) for them
C128 = row("b", "C128", 3, 128, 64, 3, conv_tb(3, 5, 3, 2), 37, 5, 3, 1, -2)
C128_X3 = [row("bx", "C128", 2, 128, 64, Ta, conv_tb(Ta, 5, s, 2), P, 5, s, 1, -2) for Ta, P, s in ((64, 2, 3), (43, 3, 3), (10, 13, 1))]
GROUP_C += [C128] + C128_X3
# D. offsets and tap steps: Tb fitting exactly, with four unused rows, and two rows short
D_KSDO = ((3, 1, 1, 0), (3, 1, 1, -1), (3, 1, 1, -25), (3, 1, 3, -3), (11, 1, 5, -25), (4, 2, 1, -1), (3, 2, 1, 0), (5, 3, 1, -2),
          (3, 1, -1, 2), (5, 1, -2, 4))
GROUP_D = [row("b", "D", 2, 64, 32, 130, fit_tb(130, K, s, dj, off) + e, 1, K, s, dj, off) for K, s, dj, off in D_KSDO for e in (0, 4, -2)]
GROUP_D += [row("b", "D", 2, 64, 32, 10, fit_tb(10, 5, 3, 1, -2) + e, 13, 5, 3, 1, -2) for e in (0, 4, -2)]
# the ConvTranspose roles of ops.convT_wgrad: a = x, b = dy, s = the stride, dj = 1, off = -pad
GROUP_D += [row("b", "DT", 2, 64, 32, 130, convT_tb(130, K, s, pad) + e, 1, K, s, 1, -pad) for K, s, pad in ((4, 2, 1), (7, 3, 2)) for e in (0, 4, -2)]
D128 = [row("bx", "D128", 2, 128, 32, 130, fit_tb(130, K, s, dj, off) - 2, 1, K, s, dj, off)
        for K, s, dj, off in ((3, 1, 1, -25), (4, 2, 1, -1), (3, 1, -1, 2), (5, 1, -2, 4))]
GROUP_D += D128
# E. split and finish: one shape per tap bucket with a channel count the 16-byte finish takes and one it does not; 40 stages
E_K = (1, 3, 5, 8, 11, 16)
GROUP_E = [row("bx", "E", 8, 64, Cg, 320, conv_tb(320, K, 1, K // 2), 1, K, 1, 1, -(K // 2)) for K in E_K for Cg in (64, 66)]
E_Z = (1, 2, 4, 5, 8, 9, 13, 16, 17, 32, 40)
E_Z_CLAMPED = 500
# F. epilogue
F_DW = row("bx", "F", 2, 64, 64, 130, 130, 1, 3, 1, 1, -1)
F_DB = row("bx", "F", 2, 96, 130, 130, 130, 1, 9, 1, 1, -4)
F_DB_Z = 5
# G. forced candidates
G_CASES = (C_2_43_3_S3, GROUP_B[6], C128_X3[1])
# tuning keys off on a subset of A and C
KEY_CASES = (GROUP_A[4], GROUP_A[6], GROUP_A[13], GROUP_C[1], GROUP_C[7], C_2_43_3_S3)

CASES = [c for c, _ in TABLE]
ELIG = dict(TABLE)
SWEEP = GROUP_A + GROUP_B + GROUP_C + GROUP_D  # groups A to D: every case x kind through test_parity


def eligible(c, ar):
    return {"bf16": "b", "x3-9": "x", "x3-6": "x"}[ar] in ELIG[c]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the reference itself, and the case table
# ---------------------------------------------------------------------------------------------------------------------
def _t64(rng, *sh):
    return torch.from_numpy(rng.standard_normal(sh))


@pytest.mark.parametrize("shape", [(2, 5, 7, 40, 1, 3, 1, 1, 1), (2, 6, 4, 33, 1, 5, 2, 2, 1), (1, 3, 5, 50, 1, 4, 3, 1, 2),
                                   (2, 4, 6, 41, 1, 11, 1, 5, 5), (2, 5, 3, 17, 3, 5, 3, 2, 1), (3, 4, 4, 9, 13, 5, 1, 2, 1),
                                   (2, 3, 4, 20, 2, 2, 2, 0, 3)],
                         ids=lambda s: "B%d-C%d-M%d-T%d-P%d-K%d-s%d-pad%d-dil%d" % s)
def test_reference_is_the_conv_weight_gradient(shape):
    """wgrad_f64.wgrad on the roles ops.conv_wgrad builds (a = dy, b = x, s = stride, dj = dilation, off = -pad) equals the
    float64 autograd weight gradient of conv1d / conv2d((k, 1)), to 1e-12."""
    B, C, M, T, P, K, s, pad, dil = shape
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    Tout = (T + 2 * pad - dil * (K - 1) - 1) // s + 1
    x, dy = _t64(rng, B, C, T, P), _t64(rng, B, M, Tout, P)
    w = torch.zeros(M, C, K, 1, dtype=torch.float64, requires_grad=True)
    if P == 1:
        y = F.conv1d(x[..., 0], w[..., 0], None, s, pad, dil).unsqueeze(-1)
    else:
        y = F.conv2d(x, w, None, (s, 1), (pad, 0), (dil, 1))
    ref = torch.autograd.grad(y, w, dy)[0][..., 0]
    got = W.wgrad(dy, x, K, s, dil, -pad)
    assert W.dist(got, ref) <= 1e-12, W.dist(got, ref)
    assert W.dist(W.dbias(dy), dy.sum((0, 2, 3))) <= 1e-12


@pytest.mark.parametrize("shape", [(2, 5, 7, 30, 4, 2, 1), (2, 4, 3, 25, 7, 3, 2), (1, 3, 6, 40, 16, 8, 4), (2, 4, 4, 31, 3, 1, 1)],
                         ids=lambda s: "B%d-Cin%d-Cout%d-T%d-K%d-s%d-pad%d" % s)
def test_reference_is_the_conv_transpose_weight_gradient(shape):
    """... and on the roles ops.convT_wgrad builds (a = x, b = dy, s = stride, dj = 1, off = -pad) the float64 autograd weight
    gradient [Cin, Cout, K] of conv_transpose1d, to 1e-12."""
    B, Cin, Cout, T, K, s, pad = shape
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    x, dy = _t64(rng, B, Cin, T), _t64(rng, B, Cout, convT_tb(T, K, s, pad))
    w = torch.zeros(Cin, Cout, K, dtype=torch.float64, requires_grad=True)
    ref = torch.autograd.grad(F.conv_transpose1d(x, w, None, s, pad), w, dy)[0]
    got = W.wgrad(x.unsqueeze(-1), dy.unsqueeze(-1), K, s, 1, -pad)
    assert W.dist(got, ref) <= 1e-12, W.dist(got, ref)


def test_reference_transforms_and_rounding():
    """The operand transforms of the reference: leaky-ReLU with the float32 slope, rounding to bf16 after it, and the float32
    run of the same text."""
    rng = np.random.default_rng(5)
    a, b = _t64(rng, 2, 3, 20, 2).float(), _t64(rng, 2, 4, 22, 2).float()
    lk = lambda t, sl: torch.where(t > 0, t, t * sl)
    s32 = float(np.float32(0.1))
    ref = W.wgrad(lk(a.double(), s32), lk(b.double(), s32), 3, 1, 1, 0)
    assert W.dist(W.wgrad(a, b, 3, 1, 1, 0, W.TF_LEAKY, W.TF_LEAKY, 0.1), ref) <= 1e-15
    rb = lambda t: t.bfloat16().double()
    ref = W.wgrad(rb(lk(a, np.float32(0.1))), rb(b), 3, 1, 1, 0)
    assert torch.equal(W.wgrad(a, b, 3, 1, 1, 0, W.TF_LEAKY, W.TF_NONE, 0.1, rounded=True), ref)
    assert 0 < W.dist(W.wgrad(a, b, 3, 1, 1, 0, dtype=torch.float32), W.wgrad(a, b, 3, 1, 1, 0)) < 1e-6
    # rows outside [0, Tb) read zero: an offset that puts every tap of every position out of range gives zeros
    assert not bool(W.wgrad(a, b, 3, 1, 1, -40).any()) and not bool(W.wgrad(a, b, 3, 1, 1, 40).any())


def plans(c):
    return {ar: W.pick(args_of(c), PL_OF[ar]) for ar in ARITHS}


def e_scratch_and_z(c, ar, z):
    """Group E at a forced split: scratch of z slabs, and the split the launcher then takes."""
    pl = W.pick(args_of(c), PL_OF[ar])
    return z * pl.n, W.split(pl, z * pl.n, z)


def test_case_table_reaches_every_branch():
    """The table above against the launcher's rules as wgrad_f64 restates them, and the branches this file claims to cover."""
    seen = collections.Counter()
    for c, elig in TABLE:
        assert 8 * 8 * c.B * c.Ta * c.P < (1 << 24) // 4, c  # the exact pass: every sum of quarter-integers stays exact
        assert c.Tb >= 1 and c.Ta >= 1
        for ar, pl in plans(c).items():
            assert (pl is not None) == eligible(c, ar), (c, ar, pl)
            if pl is None:
                continue
            assert c.B * c.Ta * c.P >= 256
            name = "bf16" if ar == "bf16" else "x3"
            seen.update(["%s cand %d" % (name, pl.cand), "%s KT %d" % (name, pl.KT)])
            seen.update(["%s ragged last group" % name] * (pl.ntg > 1 and pl.kn_last < pl.KT))
            seen.update(["%s full last group" % name] * (pl.ntg > 1 and pl.kn_last == pl.KT))
            seen.update(["%s four tap groups" % name] * (pl.ntg == 4))
            seen.update(["%s XR > 64" % name] * (pl.XR > 64))
            seen.update(["%s row shorter than a stage" % name] * (c.Ta * c.P < pl.BU))
            seen.update(["%s U is a multiple of the stage" % name] * (c.Ta * c.P % pl.BU == 0))
            seen.update(["%s U is one past a stage" % name] * (c.Ta * c.P % pl.BU == 1))
            seen.update(["%s B = 1" % name] * (c.B == 1))
            seen.update(["%s Cg in [16, 31]" % name] * (16 <= c.Cg < 32))
            seen.update(["%s channel tails" % name] * (c.Mg % 32 != 0 and c.Cg % 32 != 0))
            starts = W.span_starts(args_of(c), pl)
            seen.update(["%s span start not a multiple of 4" % name] * any(f % 4 for f in starts))
            seen.update(["%s negative span start" % name] * any(f < 0 for f in starts))
            seen.update(["%s negative span start not a multiple of 4" % name] * any(f < 0 and f % 4 for f in starts))
            seen.update(["%s negative dj" % name] * (c.dj < 0) + ["%s stride %d" % (name, c.s)] + ["%s P > 1" % name] * (c.P > 1))
            if pl.cand > 0 and c.Mg >= 128 and c.Cg > 32:
                assert W.geometry(args_of(c), 0, pl.KT, PL_OF[ar]) == "lds"
                seen.update(["%s fall-through from candidate 0 because of LDS" % name])
            if c.Mg >= 64 and c.Cg > 32 and pl.cand > 2 and W.geometry(args_of(c), 2, pl.KT, PL_OF[ar]) == "lds":
                seen.update(["%s fall-through from candidate 2 because of LDS" % name])
    assert ELIG[C128] == "b" and plans(C128)["bf16"].cand == 1
    for name in ("bf16", "x3"):
        for b in ("ragged last group", "full last group", "XR > 64", "row shorter than a stage", "U is a multiple of the stage",
                  "U is one past a stage", "B = 1", "channel tails", "span start not a multiple of 4", "negative span start",
                  "negative span start not a multiple of 4", "negative dj", "stride 1", "stride 2", "stride 3", "P > 1"):
            assert seen["%s %s" % (name, b)] > 0, (name, b)
    # (candidate 4, 32 x 64, is the first that fits only for Mg < 64 with Cg > 32: it runs forced, in group G)
    assert all(seen["bf16 cand %d" % i] > 0 for i in (0, 1, 2, 3, 5)), seen
    # the three-plane rule admits the candidates with at most two position-split waves
    assert all(seen["x3 cand %d" % i] > 0 for i in (0, 1, 2)) and not any(seen["x3 cand %d" % i] for i in (3, 4, 5))
    assert all(seen["bf16 KT %d" % k] > 0 for k in (1, 3, 5, 6, 8)) and all(seen["x3 KT %d" % k] > 0 for k in (1, 3, 5, 6, 4))
    assert seen["x3 four tap groups"] > 0 and seen["bf16 Cg in [16, 31]"] > 0
    assert seen["bf16 fall-through from candidate 0 because of LDS"] > 0 and seen["bf16 fall-through from candidate 2 because of LDS"] > 0
    # K = 7 -> 4 + 3, 8 -> 4 + 4, 15 / 16 -> four groups in the three-plane form; 7 / 8 one group, 15 / 16 two in the bf16 form
    kn = lambda K, PL: (W.pick(args_of(GROUP_A[A_K.index(K)]), PL).ntg, W.pick(args_of(GROUP_A[A_K.index(K)]), PL).kn_last)
    assert [kn(K, 3) for K in (7, 8, 15, 16)] == [(2, 3), (2, 4), (4, 3), (4, 4)]
    assert [kn(K, 1) for K in (7, 8, 15, 16, 10, 13)] == [(1, 7), (1, 8), (2, 7), (2, 8), (2, 4), (3, 1)]
    # group E: every finish4<ZG> x tap bucket, both scalar forms, and a forced split above the stages is clamped to them
    fin = collections.Counter()
    for c in GROUP_E:
        for ar in ARITHS:
            pl = plans(c)[ar]
            for z in E_Z:
                sf, Z = e_scratch_and_z(c, ar, z)
                assert Z == z, (c, ar, z, Z)  # (40 stages: no forced count of the list is clamped)
                fin[W.finish_kernel(Z, c.K, c.Cg)] += 1
            assert e_scratch_and_z(c, ar, E_Z_CLAMPED)[1] == pl.total and pl.total in (40, 80)
            if c.Cg % 4 == 0:
                fin[W.finish_kernel(W.split(pl, pl.n, -1), c.K, c.Cg, aligned=False)] += 1
                assert W.split(pl, pl.n, -1) == 1 and W.split(pl, 2 * pl.n + 1, -1) == 2
    for zg in (4, 8, 16, 32):
        for kb in (1, 3, 5, 8, 11, 16):
            assert fin[("finish4", zg, kb)] > 0, (zg, kb)
    assert fin[("rows",)] > 0 and fin[("zlanes",)] > 0
    assert W.finish_kernel(12, 5, 66) == ("rows",) and W.finish_kernel(13, 5, 66) == ("zlanes",)
    assert W.finish_kernel(4, 5, 64, finish_vec=False) == ("rows",) and W.finish_kernel(4, 5, 64, aligned=False) == ("rows",)
    # F: the bias row sums are shared by several channel tiles, tap groups and z-blocks
    for ar in ARITHS:
        pl = plans(F_DB)[ar]
        assert pl.nct > 1 and pl.ntg > 1 and pl.nmt > 1 and W.split(pl, F_DB_Z * pl.n, F_DB_Z) == F_DB_Z
    # G: all six candidates forced in the bf16 form somewhere, and the ones the three-plane rule admits
    forced = collections.Counter()
    for c in G_CASES:
        for cand in range(6):
            forced.update(["bf16 %d" % cand] * (W.pick(args_of(c), 1, force_cand=cand) is not None))
            forced.update(["x3 %d" % cand] * (W.pick(args_of(c), 3, force_cand=cand) is not None))
            forced.update(["refused"] * (W.pick(args_of(c), 1, force_cand=cand) is None))
    assert all(forced["bf16 %d" % i] > 0 for i in range(6)) and forced["x3 1"] > 0 and forced["x3 2"] > 0 and forced["refused"] > 0
    assert not any(forced["x3 %d" % i] for i in (3, 4, 5))
    # H: the refusals, each alone
    base = args_of(REFUSAL_BASE)
    assert W.pick(base, 1) is not None and W.pick(base, 3) is not None
    for what, over in REFUSALS:
        assert W.pick(base._replace(**over), 1) is None and W.pick(base._replace(**over), 3) is None, what
    # I: the default setting (all_shapes off) keeps the three-plane form for 64-channel tiles with K = 5 or K >= 9
    for c, want in ROUTING_DEFAULT:
        assert (W.pick(args_of(c), 3, x3_all=False) is not None) == want and W.pick(args_of(c), 1) is not None, c


REFUSAL_BASE = Case("H", 2, 64, 64, 130, 4 * 130 + 20, 1, 5, 1, 1, -2)
REFUSALS = (("G = 2", dict(G=2)), ("Mg 31", dict(Mg=31)), ("Cg 15", dict(Cg=15)), ("K 17", dict(K=17)), ("B * U = 255", dict(B=1, Ta=255)),
            ("s 0", dict(s=0)), ("s 4", dict(s=4)), ("a_tf DLEAKY", dict(a_tf=W.TF_DLEAKY)), ("transpose_out", dict(transpose_out=1)),
            ("slope 1.0", dict(slope=1.0)), ("slope -0.1", dict(slope=-0.1)))
ROUTING_DEFAULT = ((Case("I", 2, 64, 64, 130, 130, 1, 5, 1, 1, -2), True), (Case("I", 2, 64, 64, 130, 130, 1, 11, 1, 1, -5), True),
                   (Case("I", 2, 64, 64, 130, 130, 1, 3, 1, 1, -1), False), (Case("I", 2, 64, 32, 130, 130, 1, 5, 1, 1, -2), False),
                   (Case("I", 2, 64, 64, 130, 130, 1, 7, 1, 1, -3), False))


def fill(c, a=None, b=None, dw=None, db=None, alpha=1.0, a_tf=W.TF_NONE, b_tf=W.TF_NONE, slope=0.1, **over):
    from vcvits_amd._lib import VcvWgradArgs
    A = VcvWgradArgs()
    p = lambda t: None if t is None else t.data_ptr()
    A.a, A.b, A.aaux, A.baux, A.dw, A.dbias = p(a), p(b), None, None, p(dw), p(db)
    A.B, A.G, A.Cg, A.Mg, A.Ta, A.Tb, A.P, A.K = c.B, 1, c.Cg, c.Mg, c.Ta, c.Tb, c.P, c.K
    A.s, A.dj, A.off, A.a_tf, A.b_tf, A.transpose_out, A.alpha, A.slope = c.s, c.dj, c.off, a_tf, b_tf, 0, alpha, slope
    A.slab, A.slab_floats = None, 0
    for k, v in over.items():
        setattr(A, k, v)
    return A


def lib_scratch(c, ar, **over):
    from vcvits_amd._lib import lib
    fn = lib().vcv_wgrad_bf16_scratch if ar == "bf16" else lib().vcv_wgrad_x3_scratch
    return fn(ctypes.byref(fill(c, **over)))


@contextlib.contextmanager
def arithmetic(ar):
    """The number of product terms of `ar`, and every eligible shape admitted; both settings come back whatever happens."""
    from vcvits_amd._lib import lib
    L = lib()
    old = (L.vcv_conv_x3_get_terms(), L.vcv_conv_x3_get_all())
    try:
        if ar != "bf16":
            assert L.vcv_conv_x3_set_terms(9 if ar == "x3-9" else 6) == 0
        assert L.vcv_conv_x3_set_all(1) == 0
        yield
    finally:
        L.vcv_conv_x3_set_terms(old[0])
        L.vcv_conv_x3_set_all(old[1])


@contextlib.contextmanager
def forced(cand=-1, z=-1):
    from vcvits_amd._lib import lib
    lib().vcv_wgrad_bf16_set_force(cand, z)
    try:
        yield
    finally:
        lib().vcv_wgrad_bf16_set_force(-1, -1)


@contextlib.contextmanager
def switched(key, value):
    from vcvits_amd import tuning
    old = tuning.kernel_get(key)
    tuning.kernel_set(key, value)
    try:
        yield
    finally:
        tuning.kernel_set(key, old)


def test_restated_rules_are_the_librarys():
    """Host only (vcv_wgrad_*_scratch launches nothing): for every case of the table, every forced candidate of group G and
    every refusal the library reports the scratch the restated pick() / scratch_want() give -- which depends on the
    candidate's tile, the tap groups and the stages per element -- and 0 exactly where the table says ineligible.  With the
    all-shapes setting off, the three-plane form keeps the shapes ROUTING_DEFAULT says."""
    for ar in ARITHS:
        with arithmetic(ar):
            for c, _ in TABLE:
                pl = W.pick(args_of(c), PL_OF[ar])
                assert lib_scratch(c, ar) == (pl.want if pl else 0), (c, ar, pl)
                assert (lib_scratch(c, ar) > 0) == eligible(c, ar), (c, ar)
            for c in G_CASES:
                for cand in range(6):
                    with forced(cand):
                        pl = W.pick(args_of(c), PL_OF[ar], force_cand=cand)
                        assert lib_scratch(c, ar) == (pl.want if pl else 0), (c, ar, cand, pl)
            for c in KEY_CASES:
                with switched("wgrad_bf16_ws", 0):
                    pl = W.pick(args_of(c), PL_OF[ar], ws=False)
                    assert lib_scratch(c, ar) == (pl.want if pl else 0), (c, ar, "wgrad_bf16_ws=0")
            assert lib_scratch(REFUSAL_BASE, ar) > 0
            for what, over in REFUSALS:
                assert lib_scratch(REFUSAL_BASE._replace(**{k: v for k, v in over.items() if k in Case._fields}), ar,
                                   **{k: v for k, v in over.items() if k not in Case._fields}) == 0, (what, ar)
    from vcvits_amd._lib import lib
    old = lib().vcv_conv_x3_get_all()
    try:
        lib().vcv_conv_x3_set_all(0)
        for c, want in ROUTING_DEFAULT:
            assert (lib_scratch(c, "x3-6") > 0) == want and lib_scratch(c, "bf16") > 0, c
    finally:
        lib().vcv_conv_x3_set_all(old)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and float64 references: made once per (case, kind) and shared by every test
# ---------------------------------------------------------------------------------------------------------------------
EXACT = dict(alpha=0.5, b_tf=W.TF_LEAKY, slope=0.5)


@functools.lru_cache(maxsize=None)
def inputs(c, kind):
    """a [B, Mg, Ta, P], b [B, Cg, Tb, P], the dw and dbias preloads (float32, CPU).  normal: seeded standard normal.
    exact: integers in [-8, 8]."""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    if kind == "exact":
        t = lambda *sh: torch.from_numpy(rng.integers(-8, 9, sh).astype(np.float32))
    else:
        t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    return t(c.B, c.Mg, c.Ta, c.P), t(c.B, c.Cg, c.Tb, c.P), t(c.Mg, c.Cg, c.K), t(c.Mg)


@functools.lru_cache(maxsize=None)
def reference(c, kind, rounded, a_tf=W.TF_NONE, b_tf=W.TF_NONE, slope=0.1):
    """(float64 dw, float64 dbias, d32 of dw, d32 of dbias): without alpha and preloads."""
    a, b, _, _ = inputs(c, kind)
    dw = W.wgrad(a, b, c.K, c.s, c.dj, c.off, a_tf, b_tf, slope, rounded)
    dw32 = W.wgrad(a, b, c.K, c.s, c.dj, c.off, a_tf, b_tf, slope, rounded, dtype=torch.float32)
    db = W.dbias(a)
    return dw, db, W.dist(dw32, dw), W.dist(W.dbias(a, torch.float32), db)


@functools.lru_cache(maxsize=4)
def on_gpu(c, kind, gpu):
    return tuple(t.to(gpu) for t in inputs(c, kind))


class Guarded:
    """A float32 view pre-filled with `init` (a tensor or a number) between two runs of GUARD sentinel floats; `shift`
    floats after the first guard stay unused (a view that is not 16-byte aligned)."""

    def __init__(self, shape, device, init, shift=0):
        n = int(np.prod(shape))
        self.n, self.lo = n, GUARD + shift
        self.buf = torch.full((n + 2 * GUARD + shift,), SENT, device=device)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if torch.is_tensor(init):
            self.t.copy_(init)
        else:
            self.t.fill_(init)
        assert self.t.data_ptr() % 16 == (4 * shift) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.lo + self.n:] == SENT).all())


Out = collections.namedtuple("Out", "status dw db want")


def abi(gpu, c, ar, kind, *, alpha=1.0, a_tf=W.TF_NONE, b_tf=W.TF_NONE, slope=0.1, preload=False, want_db=True, scratch=None,
        shift=0, null_scratch=False, over=None, tensors=None):
    """One call of vcv_wgrad_bf16 / vcv_wgrad_x3 (inside `arithmetic(ar)`).  scratch: floats handed over (None: what
    vcv_wgrad_*_scratch asks for).  -> Out(status, dw, dbias or None, the library's scratch request); the sentinels around dw,
    dbias and the scratch are checked here."""
    from vcvits_amd._lib import lib, stream
    a, b, pre_dw, pre_db = tensors or on_gpu(c, kind, gpu)
    over = over or {}
    G = over.get("G", 1)
    dw = Guarded((G * c.Mg, c.Cg, c.K), gpu, pre_dw if preload else 0.0)
    db = Guarded((G * c.Mg,), gpu, pre_db if preload else 0.0) if want_db else None
    A = fill(c, a, b, dw.t, db.t if db else None, alpha, a_tf, b_tf, slope, **over)
    want = (lib().vcv_wgrad_bf16_scratch if ar == "bf16" else lib().vcv_wgrad_x3_scratch)(ctypes.byref(A))
    n = c.Mg * c.Cg * c.K
    floats = max(want, n) if scratch is None else scratch
    sc = Guarded((max(floats, 1),), gpu, float("nan"), shift)
    fn = lib().vcv_wgrad_bf16 if ar == "bf16" else lib().vcv_wgrad_x3
    st = fn(ctypes.byref(A), None if null_scratch else ctypes.c_void_p(sc.t.data_ptr()), floats, stream())
    torch.cuda.synchronize()
    assert dw.intact(), "a write outside dw"
    assert db is None or db.intact(), "a write outside dbias"
    assert sc.intact(), "a write outside the scratch handed over (%d floats)" % floats
    return Out(st, dw.t, db.t if db else None, want)


_parity = {}


def record(section, line):
    """Keep the measured distances in profiles/wgrad_mfma_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "wgrad_mfma_parity.txt"), "w") as f:
        f.write("# tests/test_wgrad_mfma_abi_gpu.py: max-norm distance of vcv_wgrad_bf16 / vcv_wgrad_x3 (9 and 6 terms) from the float64\n"
                "# CPU reference (tests/wgrad_f64.py), relative to max|reference|; d32 is the distance of the float32 CPU run of the\n"
                "# reference from its float64 run.  Bounds: bf16 dw 1e-5 (rounded-operand reference), x3 dw 3e-5, dbias 2e-5.  A `-` marks an\n"
                "# arithmetic the launcher refuses for the case.  Cases are group-B-Mg-Cg-Ta-Tb-P-K-s-dj-off.  The exact pass\n"
                "# (integer operands, bit-equal to float64) has no distances to report.\n")
        for name in _parity:
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def run_and_check(gpu, c, kind, section=None, tag="", ariths=ARITHS, expect_eligible=None, **kw):
    """Every arithmetic of `ariths` on one case: eligibility as the table has it, two launches with the same dw bits, sentinels,
    and the float64 reference -- within the bounds (normal) or bit for bit (exact).  kw: the call's options (see abi); in
    the exact pass alpha / b_tf / slope / preload are EXACT's unless given.  -> {arithmetic: dw}"""
    opts = dict(kw)
    if kind == "exact":
        for k, v in dict(EXACT, preload=True).items():
            opts.setdefault(k, v)
    alpha, preload = opts.get("alpha", 1.0), opts.get("preload", False)
    a_tf, b_tf, slope = opts.get("a_tf", W.TF_NONE), opts.get("b_tf", W.TF_NONE), opts.get("slope", 0.1)
    want_db = opts.setdefault("want_db", a_tf == W.TF_NONE)
    _, _, pre_dw, pre_db = inputs(c, kind)
    cells, got, fails = [], {}, []
    for ar in ariths:
        ok = eligible(c, ar) if expect_eligible is None else expect_eligible[ar]
        with arithmetic(ar):
            if not ok:
                assert lib_scratch(c, ar) == 0, "%s %s: the table says ineligible, the library wants scratch" % (cid(c), ar)
                assert abi(gpu, c, ar, kind, **opts).status == EINVAL
                cells.append("%s -" % ar)
                continue
            r1 = abi(gpu, c, ar, kind, **opts)
            r2 = abi(gpu, c, ar, kind, **opts)
        assert r1.want > 0, "%s %s: the table says eligible, the library wants no scratch" % (cid(c), ar)
        assert r1.status == 0 and r2.status == 0, (r1.status, r2.status)
        assert torch.equal(r1.dw, r2.dw), "%s %s %s: dw differs between two identical launches" % (cid(c), ar, tag)
        dw64, db64, d32, d32b = reference(c, kind, ar == "bf16", a_tf, b_tf, slope)
        if preload:
            dw64, db64 = pre_dw.double() + float(np.float32(alpha)) * dw64, pre_db.double() + db64
        else:
            dw64 = float(np.float32(alpha)) * dw64
        got[ar] = r1.dw
        if kind == "exact":
            assert torch.equal(r1.dw.cpu(), dw64.float()) and bool((dw64.float().double() == dw64).all()), \
                "%s %s %s: dw is not the float64 reference's bits (distance %.3e)" % (cid(c), ar, tag, W.dist(r1.dw, dw64))
            if want_db:
                for r in (r1, r2):
                    assert torch.equal(r.db.cpu(), db64.float()), "%s %s %s: dbias is not exact (distance %.3e)" % (
                        cid(c), ar, tag, W.dist(r.db, db64))
            continue
        e = W.dist(r1.dw, dw64)
        eb = max(W.dist(r.db, db64) for r in (r1, r2)) if want_db else None
        cells.append("%s dw=%.1e%s" % (ar, e, "" if eb is None else " db=%.1e" % eb))
        bound = TOL_BF16 if ar == "bf16" else TOL_DW
        if e > bound:
            fails.append("%s dw off by %.3e (bound %.1e)" % (ar, e, bound))
        if eb is not None and eb > TOL_DB:
            fails.append("%s dbias off by %.3e (bound %.1e)" % (ar, eb, TOL_DB))
    if kind == "normal" and section:
        d32, d32b = reference(c, kind, False, a_tf, b_tf, slope)[2:]
        record(section, "%-56s %-20s %s  | d32 dw=%.1e db=%.1e" % (cid(c), tag, "  ".join(cells), d32, d32b))
    assert not fails, "%s %s: %s" % (cid(c), tag, "; ".join(fails))
    return got


def kind_case_ids(v):
    return cid(v) if isinstance(v, Case) else str(v)


# ---------------------------------------------------------------------------------------------------------------------
# A - D. tap groups, channel tails, position edges, offsets and tap steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", SWEEP, ids=cid)
def test_parity(gpu, c, kind):
    """Every case of groups A to D in the three arithmetics, with the bias row sums collected in the same launch."""
    run_and_check(gpu, c, kind, "%s: %s" % (c.grp, {"A": "tap groups", "B": "channel tails", "C": "position edges", "C128": "position edges",
                                                     "D": "offsets and tap steps", "DT": "offsets and tap steps",
                                                     "D128": "offsets and tap steps"}[c.grp]))


# ---------------------------------------------------------------------------------------------------------------------
# E. split and finish
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", GROUP_E, ids=cid)
def test_split_and_finish(gpu, c, kind):
    """Forced reduction splits with scratch of exactly z slabs (every finish4<ZG> x tap bucket at Cg 64, the two 4-byte forms at
    Cg 66), a forced split above the stages (clamped), the cost model's own split with scratch of exactly one slab and of
    2 n + 1 floats, and a scratch pointer one float off 16-byte alignment (the 4-byte finish despite Cg % 4 == 0)."""
    n = c.Mg * c.Cg * c.K
    sec = "E: split and finish"
    for z in E_Z:
        with forced(-1, z):
            run_and_check(gpu, c, kind, sec, "z=%d" % z, scratch=z * n)
    for ar in ARITHS:  # (the clamp is to the stages, which differ between the two forms)
        total = plans(c)[ar].total
        with forced(-1, E_Z_CLAMPED):
            run_and_check(gpu, c, kind, sec, "z=%d->%d" % (E_Z_CLAMPED, total), ariths=(ar,), scratch=total * n)
    run_and_check(gpu, c, kind, sec, "scratch=n", scratch=n)
    run_and_check(gpu, c, kind, sec, "scratch=2n+1", scratch=2 * n + 1)
    run_and_check(gpu, c, kind, sec, "scratch+4B", scratch=2 * n, shift=1)
    with forced(-1, 13):
        run_and_check(gpu, c, kind, sec, "scratch+4B z=13", scratch=13 * n, shift=1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", ["wgrad_finish_vec", "wgrad_bf16_ws"])
@pytest.mark.parametrize("c", KEY_CASES, ids=cid)
def test_tuning_keys_off(gpu, c, key, kind):
    """wgrad_finish_vec = 0 (the 4-byte finish everywhere) and wgrad_bf16_ws = 0 (every wave of the bf16 form stages; the
    three-plane form keeps its producer waves) on a subset of groups A and C."""
    with switched(key, 0):
        elig = {ar: W.pick(args_of(c), PL_OF[ar], ws=key != "wgrad_bf16_ws") is not None for ar in ARITHS}
        run_and_check(gpu, c, kind, "E: tuning keys off", "%s=0" % key, expect_eligible=elig)
        with forced(-1, 13):
            run_and_check(gpu, c, kind, "E: tuning keys off", "%s=0 z=13" % key, expect_eligible=elig)


# ---------------------------------------------------------------------------------------------------------------------
# F. epilogue
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha", [1.0, 0.5, -2.0])
def test_alpha_onto_a_preloaded_dw(gpu, alpha, kind):
    run_and_check(gpu, F_DW, kind, "F: epilogue", "alpha=%g preload" % alpha, alpha=alpha, preload=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_dbias_is_counted_once(gpu, kind):
    """dbias onto a preloaded vector where 3 channel tiles x 2 tap groups x 5 z-blocks (x 2 row tiles) stage the same rows
    of `a`: only the blocks of the first (channel tile, tap group) may add their row sums."""
    n = F_DB.Mg * F_DB.Cg * F_DB.K
    with forced(-1, F_DB_Z):
        run_and_check(gpu, F_DB, kind, "F: epilogue", "dbias preload z=%d" % F_DB_Z, preload=True, scratch=F_DB_Z * n)
    run_and_check(gpu, F_DB, kind, "F: epilogue", "dbias preload", preload=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind_slope", [("normal", 0.1), ("normal", 0.5), ("exact", 0.5)], ids=lambda ks: "%s-slope%g" % ks)
@pytest.mark.parametrize("tf", [(1, 0), (0, 1), (1, 1)], ids=["a", "b", "ab"])
def test_operand_leaky_relu(gpu, tf, kind_slope):
    """a_tf / b_tf = LEAKY each alone and together, with slope 0.1 and 0.5 (the exact pass: 0.5 only -- 0.1 times an integer is
    no bf16 number), on a plain row and on a strided period row."""
    kind, slope = kind_slope
    for c in (F_DW, C_2_43_3_S3):
        run_and_check(gpu, c, kind, "F: epilogue", "a_tf=%d b_tf=%d slope=%g" % (tf[0], tf[1], slope), a_tf=tf[0], b_tf=tf[1], slope=slope)


# ---------------------------------------------------------------------------------------------------------------------
# G. forced candidates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cand", range(6))
@pytest.mark.parametrize("c", G_CASES, ids=cid)
def test_forced_candidate(gpu, c, cand, kind):
    """vcv_wgrad_bf16_set_force(cand, -1) on a wide-period row and on a shape with both channel tails: a candidate the restated
    rule rejects reports 0 scratch and VCV_EINVAL, every other one meets the reference."""
    elig = {ar: W.pick(args_of(c), PL_OF[ar], force_cand=cand) is not None for ar in ARITHS}
    with forced(cand, -1):
        run_and_check(gpu, c, kind, "G: forced candidates", "cand=%d" % cand, expect_eligible=elig)


# ---------------------------------------------------------------------------------------------------------------------
# H. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu):
    """Each alone: vcv_wgrad_*_scratch == 0 and VCV_EINVAL from the run call, dw / dbias / scratch untouched.  Every buffer has
    the size the refused arguments ask for, so a launch that should not happen stays in bounds.  A null scratch and a
    scratch one float short of a slab are refused by the run call alone (the arguments themselves are eligible)."""
    c0 = REFUSAL_BASE
    tried = []
    for ar in ARITHS:
        with arithmetic(ar):
            for what, over in REFUSALS:
                c = c0._replace(**{k: v for k, v in over.items() if k in Case._fields})
                rest = {k: v for k, v in over.items() if k not in Case._fields}
                G = rest.get("G", 1)
                g0 = torch.Generator().manual_seed(3)
                a = torch.randn(c.B, G * c.Mg, c.Ta, c.P, generator=g0).to(gpu)
                b = torch.randn(c.B, G * c.Cg, c.Tb, c.P, generator=g0).to(gpu)
                opts = {k: rest.pop(k) for k in ("a_tf", "slope") if k in rest}
                assert lib_scratch(c, ar, **opts, **rest) == 0, (what, ar)
                r = abi(gpu, c, ar, "normal", tensors=(a, b, None, None), over=rest, scratch=4 * G * c.Mg * c.Cg * c.K, **opts)
                assert r.status == EINVAL and r.want == 0, (what, ar, r.status)
                assert not bool(r.dw.any()) and not bool(r.db.any()), "%s %s: a refused call wrote to an output" % (what, ar)
                tried.append(what)
            n = c0.Mg * c0.Cg * c0.K
            for what, kw in (("null scratch", dict(null_scratch=True)), ("scratch_floats = n - 1", dict(scratch=n - 1))):
                r = abi(gpu, c0, ar, "normal", **kw)
                assert r.want > 0 and r.status == EINVAL, (what, ar, r.status)
                assert not bool(r.dw.any()) and not bool(r.db.any()), "%s %s: a refused call wrote to an output" % (what, ar)
                tried.append(what)
            r = abi(gpu, c0, ar, "normal", scratch=n)  # the same buffers are accepted when nothing is wrong with the call
            assert r.status == 0 and bool(r.dw.any())
    record("H: refusals", "%d calls refused with VCV_EINVAL, outputs untouched (each in the three arithmetics): %s" % (
        len(tried), "; ".join(dict.fromkeys(tried))))


# ---------------------------------------------------------------------------------------------------------------------
# I. routing
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def ops_mode(ar, all_shapes=True):
    """ops in bf16 mode, or in fp32 mode with split-operand weight gradients; everything comes back."""
    from vcvits_amd import ops
    from vcvits_amd._lib import lib
    old = (ops.compute_dtype(), ops._USE_X3[0], lib().vcv_conv_x3_get_terms(), lib().vcv_conv_x3_get_all(), ops._USE_X3_WGRAD[0])
    try:
        ops.set_compute_dtype("bf16" if ar == "bf16" else "f32")
        if ar != "bf16":
            ops.set_f32_split(True, terms=9 if ar == "x3-9" else 6, wgrad=True, all_shapes=all_shapes)
        yield ops
    finally:
        ops.set_compute_dtype(old[0])
        ops.set_f32_split(old[1], terms=old[2], all_shapes=bool(old[3]), wgrad=old[4])


def through_ops(ops, c, a, b):
    """The ops call whose VcvWgradArgs are the case's: conv roles for dj = dilation, ConvTranspose roles for group DT."""
    sq = (lambda t: t[..., 0].contiguous()) if c.P == 1 else (lambda t: t)
    if c.grp == "DT":
        return ops.convT_wgrad(sq(b), sq(a), (c.Mg, c.Cg, c.K), stride=c.s, pad=-c.off)
    return ops.conv_wgrad(sq(a), sq(b), (c.Mg, c.Cg, c.K), stride=c.s, pad=-c.off, dil=c.dj)


ROUTED = (GROUP_A[4], C_2_43_3_S3, [c for c in GROUP_D if c.grp == "DT"][0], D128[1])


@pytest.mark.gpu
@pytest.mark.parametrize("c", ROUTED, ids=cid)
def test_routing_same_bits_as_direct_calls(gpu, c):
    """ops.conv_wgrad / ops.convT_wgrad in bf16 mode and under set_f32_split(True, wgrad=True, all_shapes=True): one launch
    of this kernel wherever the table says eligible, with the bits of the direct call; where it says ineligible the launch
    goes elsewhere (the counter stays)."""
    a, b, _, _ = on_gpu(c, "normal", gpu)
    for ar in ("bf16", "x3-6"):
        key = "wgrad_bf16" if ar == "bf16" else "wgrad_x3"
        with ops_mode(ar) as ops:
            before = ops.LAUNCH_COUNTS[key]
            got = through_ops(ops, c, a, b)
            torch.cuda.synchronize()
            moved = ops.LAUNCH_COUNTS[key] - before
        assert moved == (1 if eligible(c, ar) else 0), (cid(c), ar, moved)
        if moved:
            with arithmetic(ar):
                r = abi(gpu, c, ar, "normal", want_db=False)
            assert r.status == 0 and torch.equal(got, r.dw), "%s %s: ops did not give the direct call's bits" % (cid(c), ar)
        record("I: routing", "%-56s %s: %s" % (cid(c), ar, "the direct call's bits" if moved else "not this kernel (ineligible)"))


@pytest.mark.gpu
def test_routing_default_setting(gpu):
    """all_shapes off (the default): the split-operand kernel takes (Cg 64, K 5) and (Cg 64, K 11) and leaves (Cg 64, K 3),
    (Cg 32, K 5) and (Cg 64, K 7) to vcv_conv_wgrad; either way the result meets float64 at the fp32 bound."""
    for c, want in ROUTING_DEFAULT:
        rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
        a = torch.from_numpy(rng.standard_normal((c.B, c.Mg, c.Ta, 1)).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal((c.B, c.Cg, c.Tb, 1)).astype(np.float32))
        with ops_mode("x3-6", all_shapes=False) as ops:
            before = ops.LAUNCH_COUNTS["wgrad_x3"]
            got = through_ops(ops, c, a.to(gpu), b.to(gpu))
            torch.cuda.synchronize()
            moved = ops.LAUNCH_COUNTS["wgrad_x3"] - before
        assert moved == (1 if want else 0), (cid(c), moved)
        e = W.dist(got, W.wgrad(a, b, c.K, c.s, c.dj, c.off))
        record("I: routing", "%-56s all_shapes off: %s dw=%.1e" % (cid(c), "vcv_wgrad_x3" if moved else "vcv_conv_wgrad", e))
        assert e <= TOL_DW, (cid(c), e)

"""The fused epilogue of the five forward-type conv families (vcv_conv_gemm, vcv_conv_dma_run, vcv_conv_pk_run,
vcv_conv_bf16_run, vcv_conv_x3_run with 9 and 6 product terms) at the C ABI, against a float64 CPU restatement of the
VcvConvArgs formula (tests/conv_f64.py, itself pinned to torch by tests/test_conv_f64_cpu.py).

Every kernel is called with a hand-filled VcvConvArgs -- `_plan`, a pack buffer of out[0] words, a scratch of out[1] floats,
`_run` with pack_valid = 0; vcv_conv_gemm directly -- so the router of ops/conv.py cannot send a case elsewhere, and
vcv_conv_plan_describe is read before every launch: tile variant, ks (split of the reduction), vec (16-byte epilogue) and
phases must be the ones the case was written for.  test_case_table_reaches_every_branch proves on the host which of the
restated epilogues the table reaches; test_routing_* check that ops.conv_forward / ops.conv_dgrad with the family forced give
the bits of the ABI call.

Two passes over one table of (geometry, operand set):
  exact    x and w are integers in [-8, 8], bias / res / the prior y integers in [-4, 4], mask in {0, 1}, oaux / xaux in
           {-1, -0.5, 0, 0.5, 1}, alpha = slope = 0.5, out_act NONE / LEAKY / RELU (TANH runs as RELU, LOGCLAMP as LEAKY):
           every partial sum is a multiple of 1/8 below 8 * 8 * Cg * K * alpha, far under 2^24 / 8 (asserted from the table),
           so any summation order is exact in fp32, in bf16 operands and in the first term plane of the split-operand kernel,
           and the result must be BIT-EQUAL to the float64 reference cast to float32 -- no tolerance.
  normal   Gaussian inputs, w scaled by (Cg * K)^-1/2.  Two bounds, both asserted:
           1. max|got - ref| / max|ref| <= 2e-5 (gemm, dma, pk, x3) or 1e-5 against the float64 convolution of the
              bf16-ROUNDED operands (bf16): the bounds of tests/test_conv_gpu.py and tests/test_bf16_gpu.py;
           2. element-wise |got - ref| <= gamma_n * S + a, gamma_n = n u / (1 - n u), u = 2^-24, valid for any order of an
              fp32 sum of n terms; S = the float64 sum of magnitudes behind the element (conv_f64.conv); n = Cg * JA + 6
              (9 * Cg * JA + 6 for the split-operand kernel, plus 3 * 2^-24 * S with six terms: the header's bound on the
              three products left out); a = 0 except where a transcendental is evaluated (out_act TANH / LOGCLAMP, the
              DTANH masks, in_tf DLOGCLAMP), where a = 4 * d32, d32 = max|float32 CPU run - float64 run| of the same
              reference (the device's tanhf / logf / expf may differ from the host's by a few ulp).
           LOGCLAMP runs with clamp (`slope`) = 1, where log(max(v, clamp)) does not amplify an error of v.

y, the pack buffer and the scratch are views inside larger buffers with 1024 sentinel floats on each side, which must be
untouched; pack and scratch are pre-filled with NaN (a word read but never written shows in y); y is pre-filled with the prior
the reference was given, so an element the contract does not write comes back bit-identical, and a masked element comes
back as exactly 0 (+ the prior under accumulate).  Every launch is made twice and must repeat its bits.

Distances go to profiles/conv_epilogue_parity.txt, one line per case, family and operand set.

No case is skipped at run time: a family that declines a case is listed with None in the table and asserted to return
VCV_EINVAL from its `_plan`."""
import collections
import contextlib
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import conv_f64 as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
TOL_F32, TOL_BF16 = 2e-5, 1e-5
GUARD, SENT = 1024, 12345.0
PLANNED = ("dma", "pk", "bf16", "x3")  # the `family` argument of vcv_conv_plan_describe, in order
ARITHS = ("gemm", "dma", "pk", "bf16", "x3-9", "x3-6")
FAM_OF = {"gemm": "gemm", "dma": "dma", "pk": "pk", "bf16": "bf16", "x3-9": "x3", "x3-6": "x3"}
KINDS = ("normal", "exact")

# ---------------------------------------------------------------------------------------------------------------------
# operand sets
# ---------------------------------------------------------------------------------------------------------------------
Ops = collections.namedtuple("Ops", "bias res mask acc alpha in_tf out_act out_tf slope", defaults=(0, 0, 0, 0, 1.0, C.TF_NONE, C.ACT_NONE, C.TF_NONE, 0.1))
OPS = {
    "bias": Ops(bias=1),
    "alpha": Ops(bias=1, alpha=0.5, out_act=C.ACT_LEAKY),
    "res_inleaky": Ops(res=1, in_tf=C.TF_LEAKY),
    "mask": Ops(bias=1, mask=1),
    "acc": Ops(acc=1),
    "acc_res_mask": Ops(acc=1, res=1, mask=1),
    "dleaky": Ops(out_tf=C.TF_DLEAKY),
    "drelu": Ops(out_tf=C.TF_DRELU),
    "dtanh": Ops(out_tf=C.TF_DTANH),
    "relu": Ops(bias=1, out_act=C.ACT_RELU),
    "tanh": Ops(bias=1, out_act=C.ACT_TANH),
    "logclamp": Ops(bias=1, out_act=C.ACT_LOGCLAMP, slope=1.0),
    "all": Ops(bias=1, res=1, mask=1, acc=1, alpha=0.5, in_tf=C.TF_LEAKY, out_act=C.ACT_LEAKY, out_tf=C.TF_DLEAKY),
    # vcv_conv_gemm only: the derivative masks on the input
    "in_dleaky": Ops(bias=1, in_tf=C.TF_DLEAKY),
    "in_drelu": Ops(bias=1, in_tf=C.TF_DRELU),
    "in_dtanh": Ops(bias=1, in_tf=C.TF_DTANH),
    "in_dlogclamp": Ops(bias=1, in_tf=C.TF_DLOGCLAMP, slope=0.5),
}
NOMASK = ("bias", "alpha", "res_inleaky", "acc", "dleaky", "drelu", "dtanh", "relu", "tanh", "logclamp")
MASKED = ("mask", "acc_res_mask", "all")
EVERY = NOMASK + MASKED
IN_AUX = ("in_dleaky", "in_drelu", "in_dtanh", "in_dlogclamp")


def exact_ops(o):
    """The operand set as the exact pass runs it."""
    act = {C.ACT_TANH: C.ACT_RELU, C.ACT_LOGCLAMP: C.ACT_LEAKY}.get(o.out_act, o.out_act)
    return o._replace(alpha=0.5, slope=0.5, out_act=act)


def transcendental(o):
    return o.out_act in (C.ACT_TANH, C.ACT_LOGCLAMP) or o.out_tf == C.TF_DTANH or o.in_tf in (C.TF_DTANH, C.TF_DLOGCLAMP)


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
# expect: per planned family (variant, ks, vec, phases) as vcv_conv_plan_describe reports them, or None where the family's
# _plan declines the case (VCV_EINVAL).  gemm: True (it takes every case) -- it has no plan entry.
Case = collections.namedtuple("Case", "name g flip ops expect")
TABLE = []


def case(name, g, ops, dma, pk, bf16, x3, flip=0):
    assert name not in [c.name for c in TABLE], name
    c = Case(name, g, flip, tuple(ops), dict(dma=dma, pk=pk, bf16=bf16, x3=x3))
    TABLE.append(c)
    return c


def fwd(B, Cg, Mg, T, P, K, s=1, dil=1, G=1, **kw):
    """a forward conv with "same"-style padding: T rows in, Tout rows out"""
    pad = dil * (K - 1) // 2
    Tout = (T + 2 * pad - dil * (K - 1) - 1) // s + 1
    return C.geom(B, G, Cg, Mg, T, Tout, P, K, s, dil, -pad, **kw)


def phased(B, Cg, Mg, T, K, s, pad, P=1):
    """ConvTranspose1d(stride s) forward as one phase per output residue (ops/conv.py, _phased)"""
    Tout = (T - 1) * s - 2 * pad + K
    return C.geom(B, 1, Cg, Mg, T, Tout, P, K, 1, -1, 0, s, -pad, s, (Tout - 1 + pad) // s + 1, 1)


SOME = ("bias", "alpha", "res_inleaky", "acc_res_mask", "all", "tanh")
# split reduction (ks > 1) in all four planned families, flipped weights, Mg 130 = one 128-row tile + 2 rows: U = 130 is no
# multiple of 4 and B Mg U is one, so the 16-byte finishing pass takes it and its groups of four straddle two rows
case("split-flip-U130", C.geom(1, 1, 64, 130, 130, 130, 1, 5, 1, 1, -2), EVERY, (23, 3, 0, 1), (1, 4, 1, 1), (1, 2, 1, 1), (1, 2, 1, 1), flip=1)
# ... U = 96: groups of four stay inside a row;  U = 97: B Mg U is no multiple of 4, the scalar finishing pass without a mask
case("split-U96", fwd(1, 64, 130, 96, 1, 5), ("bias", "res_inleaky", "acc", "dtanh", "mask"), None, (1, 4, 1, 1), (1, 2, 1, 1), (1, 2, 1, 1))
case("split-U97", fwd(1, 64, 130, 97, 1, 5), ("bias", "alpha", "acc", "dleaky"), None, (1, 4, 1, 1), (1, 2, 1, 1), (1, 2, 1, 1))
# a pointwise conv over 130 channels: the deepest splits (pk: 8 ways, slabs written by the scalar path)
case("split-pointwise", fwd(1, 130, 70, 130, 1, 1), ("bias", "all", "tanh", "logclamp"), (23, 2, 0, 1), (4, 8, 0, 1), (4, 1, 1, 1), (4, 3, 1, 1))
# one workgroup per tile: rows of 161 (the 224-column tiles; U % 4 = 1), 96 and 97 positions
case("row-U161", fwd(1, 32, 70, 161, 1, 5), EVERY, (23, 1, 0, 1), (6, 1, 1, 1), (6, 1, 0, 1), (3, 1, 1, 1))
case("row-U96", fwd(1, 40, 32, 96, 1, 5), EVERY, None, (5, 2, 0, 1), (5, 1, 1, 1), (5, 1, 1, 1))
case("row-U97", fwd(1, 40, 32, 97, 1, 5), EVERY, None, (5, 2, 0, 1), (5, 1, 1, 1), (5, 1, 1, 1))
case("row-U96-pointwise", fwd(1, 32, 32, 96, 1, 1), EVERY, None, (5, 1, 1, 1), (5, 1, 0, 1), (5, 1, 1, 1))
# the period layout (P = 3): rows of 54 x 3 positions without a mask (16-byte epilogue) and with one (scalar)
case("period-P3", fwd(1, 32, 70, 54, 3, 5), NOMASK, (23, 1, 0, 1), (6, 1, 1, 1), (6, 1, 0, 1), (3, 1, 1, 1))
case("period-P3-mask", fwd(1, 32, 70, 54, 3, 5), MASKED, (23, 1, 0, 1), (6, 1, 0, 1), (6, 1, 0, 1), (3, 1, 0, 1))
# (the bf16 kernel's LDS has room for the 16-byte epilogue on narrower layers than the fp32 kernel's, and not on these)
case("period-P3-mask-C40", fwd(1, 40, 32, 32, 3, 5), MASKED, None, (5, 2, 0, 1), (5, 1, 0, 1), (5, 1, 0, 1))
# output rows q * 2 (every other row of y stays), q - 1 (q = 0 falls above the tensor), and one position more than rows
case("os2", fwd(2, 32, 32, 96, 1, 3)._replace(os=2, Tout=191), EVERY, None, (5, 1, 0, 1), (5, 1, 0, 1), (5, 1, 0, 1))
case("oo-1", fwd(2, 32, 32, 96, 1, 3)._replace(oo=-1), ("bias", "all", "acc_res_mask", "dtanh"), None, (5, 1, 0, 1), (5, 1, 0, 1), (5, 1, 0, 1))
case("Q97-Tout96", fwd(2, 32, 32, 96, 1, 3)._replace(Q=97), ("bias", "all", "acc_res_mask", "dtanh"), None, (5, 1, 0, 1), (5, 1, 0, 1), (5, 1, 0, 1))
# transposed convs as 2, 3 and 4 phases: the first and last q write rows outside [0, Tout) for some residues
case("phased-2", phased(1, 32, 32, 100, 4, 2, 1), SOME, None, (5, 1, 0, 2), (5, 1, 0, 2), (5, 1, 0, 2))
case("phased-3", phased(1, 32, 70, 100, 7, 3, 2), SOME, None, (4, 1, 0, 3), (4, 1, 0, 3), (3, 1, 0, 3))
case("phased-4", phased(1, 64, 32, 100, 8, 4, 2), SOME, None, (5, 1, 0, 4), (5, 1, 0, 4), (5, 1, 0, 4))
# the LDS-DMA family takes a phased launch only with 128 workgroups or more: the smallest such launch (43 MFLOP)
case("phased-4-dma", phased(8, 16, 130, 160, 8, 4, 2), ("bias", "all"), (8, 1, 0, 4), None, (2, 1, 0, 4), (1, 1, 0, 4))
# vcv_conv_gemm alone: the derivative masks on x (the 7-wave tile: 160 < U <= 224, Mg >= 64), grouped launches (the grouped
# k = 41 layers at a short row; one channel per group), fewer than 32 output channels
case("in-aux-U161", fwd(1, 32, 70, 161, 1, 5), IN_AUX, None, None, None, None)
case("grouped-41", C.geom(2, 4, 4, 16, 160, 40, 1, 41, 4, 1, -20), ("bias", "alpha", "all") + IN_AUX, None, None, None, None)
case("grouped-C1", fwd(2, 1, 2, 100, 1, 5, G=8), ("bias", "all", "in_dtanh"), None, None, None, None)
case("narrow-M24", fwd(2, 16, 24, 100, 1, 3), ("bias", "all", "relu"), None, None, None, None)

CASES = {c.name: c for c in TABLE}


def U_of(c):
    return c.g.Q * c.g.P


# ---------------------------------------------------------------------------------------------------------------------
# VcvConvArgs by hand, the planners on the host
# ---------------------------------------------------------------------------------------------------------------------
PTR = 0x10000  # "this operand is given" for the host-only planner calls


def fill(c, o, t=None, y=None, gemm_flip=False):
    """VcvConvArgs of case c under operand set o.  t: the device tensors (None: stand-in pointers for the planners).
    gemm_flip: the register-staged kernel has no flip argument -- it is handed the flipped / transposed copy t["wf"]."""
    from vcvits_amd._lib import VcvConvArgs
    g = c.g
    a = VcvConvArgs()
    p = (lambda k: t[k].data_ptr()) if t is not None else (lambda k: PTR)
    a.x, a.w, a.y = p("x"), p("wf" if gemm_flip else "w"), (y.data_ptr() if y is not None else PTR)
    a.bias = p("bias") if o.bias else None
    a.res = p("res") if o.res else None
    a.mask = p("mask") if o.mask else None
    a.xaux = p("xaux") if o.in_tf >= C.TF_DLEAKY else None
    a.oaux = p("oaux_t" if o.out_tf == C.TF_DTANH else "oaux") if o.out_tf != C.TF_NONE else None
    a.B, a.G, a.Cg, a.Mg, a.Tin, a.Tout, a.P, a.K = g.B, g.G, g.Cg, g.Mg, g.Tin, g.Tout, g.P, g.K
    a.s, a.dj, a.off, a.os, a.oo, a.phases, a.Q, a.a_mode = g.s, g.dj, g.off, g.os, g.oo, g.phases, g.Q, g.a_mode
    a.in_tf, a.out_act, a.out_tf, a.accumulate, a.alpha, a.slope = o.in_tf, o.out_act, o.out_tf, o.acc, o.alpha, o.slope
    a.io, a.ms, a.post_scale = 0, 0, 0.0
    return a


@contextlib.contextmanager
def x3_setting(terms=None):
    """Every eligible shape admitted to the split-operand kernel, `terms` product terms; both come back whatever happens."""
    from vcvits_amd._lib import lib
    L = lib()
    old = (L.vcv_conv_x3_get_terms(), L.vcv_conv_x3_get_all())
    try:
        if terms is not None:
            assert L.vcv_conv_x3_set_terms(terms) == 0
        assert L.vcv_conv_x3_set_all(1) == 0
        yield
    finally:
        L.vcv_conv_x3_set_terms(old[0])
        L.vcv_conv_x3_set_all(old[1])


def plan(a, fam, flip):
    """(rc, the three _plan words)"""
    from vcvits_amd._lib import lib
    out = (ctypes.c_int64 * 3)()
    rc = getattr(lib(), "vcv_conv_%s_plan" % fam)(ctypes.byref(a), flip, out)
    return rc, list(out)


def describe(a, fam, flip):
    """(rc, the sixteen words of vcv_conv_plan_describe)"""
    from vcvits_amd._lib import lib
    d = (ctypes.c_int32 * 16)()
    rc = lib().vcv_conv_plan_describe(ctypes.byref(a), PLANNED.index(fam), flip, d)
    return rc, list(d)


def path_of(a, fam, flip):
    """(variant, ks, vec, phases) of the launch, or None where the family declines it"""
    rc, d = describe(a, fam, flip)
    prc, _ = plan(a, fam, flip)
    assert (rc == 0) == (prc == 0), "vcv_conv_plan_describe and vcv_conv_%s_plan disagree" % fam
    if rc != 0:
        assert rc == EINVAL
        return None
    return (d[0], d[8], d[9], d[6])


def finish_kernel(c, o, path):
    """The finishing pass conv_launch_tail takes for a split launch (csrc/conv_plan.h), restated."""
    variant, ks, vec, _ = path
    if ks <= 1:
        return None
    n = c.g.B * c.g.Mg * U_of(c)
    return "finish4" if (vec and not o.mask and n % 4 == 0 and c.g.Q == c.g.Tout and U_of(c) >= 4) else "finish"


def rows_written(g):
    """(some (q, r) of the launch falls outside [0, Tout), some falls inside)"""
    nph = g.phases if g.phases > 1 else 1
    t = (np.arange(g.Q)[:, None] * g.os + g.oo + np.arange(nph)[None, :]).ravel()
    return bool(((t < 0) | (t >= g.Tout)).any()), bool(((t >= 0) & (t < g.Tout)).any())


def branch_tags(c, o, fam, got, BM):
    """The branches of the restated epilogues that family `fam` takes for case c under operand set o, given its plan
    `got` = (variant, ks, vec, phases) and tile rows BM; the last tag names the epilogue that forms y."""
    g, U = c.g, U_of(c)
    variant, ks, vec, ph = got
    outside, _ = rows_written(g)
    tags = []
    if ks == 1 and vec:
        tags.append("vec U%4==0" if U % 4 == 0 else "vec U%4!=0")
    if ks == 1 and not vec:
        tags.append("scalar")
        if fam != "dma" and ph == 1:  # why the 16-byte epilogue is off (conv_vec, csrc/conv_plan.h), first reason that holds
            if g.os != 1:
                tags.append("scalar by os")
            elif g.oo != 0:
                tags.append("scalar by oo")
            elif g.Q > g.Tout:
                tags.append("scalar by Q > Tout")
            elif o.mask and g.P > 1 and path_of(fill(c, o._replace(mask=0)), fam, c.flip)[2] == 1:
                tags.append("scalar by mask with P > 1")
    fk = finish_kernel(c, o, got)
    if fk:
        tags.append(fk)
        if fk == "finish4" and U % 4 != 0:
            assert g.B * g.Mg * U % 4 == 0
            tags.append("finish4 straddles rows")
        if fk == "finish" and o.mask:
            tags.append("finish by mask")
        if fk == "finish" and not o.mask and vec and (g.B * g.Mg * U) % 4 != 0:
            tags.append("finish by n%4")
    if g.Mg % BM != 0:
        tags.append("mtail")
    if g.a_mode == 1 and ph in (2, 3, 4) and outside:
        tags += ["phased with rows outside", "phases %d" % ph]
    if c.flip:
        tags.append("flip")
    tags.append("ops %s on %s" % ([k for k, v in OPS.items() if v == o][0], fk or ("vec" if vec else "scalar")))
    return tags


def gemm_tags(c, oname):
    """vcv_conv_gemm has one epilogue; its tile follows from the shape alone (csrc/conv_gemm.hip)."""
    g, U = c.g, U_of(c)
    outside, _ = rows_written(g)
    return (["G > 1", "Cg %d grouped" % g.Cg] * (g.G > 1) + ["Mg <= 32"] * (g.Mg <= 32) + ["7-wave tile"] * (160 < U <= 224 and g.Mg >= 64) +
            ["phased with rows outside"] * (g.phases > 1 and outside) + ["Mg tail"] * (g.Mg % 32 != 0) + ["ops %s" % oname])


# what the table as a whole must reach, per family
NEED_VEC_FAMILY = ("vec U%4==0", "vec U%4!=0", "scalar by os", "scalar by oo", "scalar by mask with P > 1", "scalar by Q > Tout", "finish4",
                   "finish by mask", "finish by n%4", "finish4 straddles rows", "mtail", "phased with rows outside", "flip", "declined")
NEED = {fam: NEED_VEC_FAMILY + tuple("ops %s on vec" % o for o in EVERY) + tuple("ops %s on scalar" % o for o in EVERY) +
        tuple("ops %s on finish4" % o for o in NOMASK) + tuple("ops %s on finish" % o for o in MASKED) for fam in ("pk", "bf16", "x3")}
NEED["dma"] = ("scalar", "finish", "mtail", "phased with rows outside", "flip", "declined") + tuple("ops %s on scalar" % o for o in EVERY) + \
    tuple("ops %s on finish" % o for o in EVERY)
NEED["gemm"] = ("G > 1", "Cg 1 grouped", "Cg 4 grouped", "Mg <= 32", "7-wave tile", "phased with rows outside", "Mg tail") + \
    tuple("ops %s" % o for o in EVERY + IN_AUX)


def test_case_table_reaches_every_branch():
    """Host only.  The table against the planners (every case x family x operand set is on the path the table names, or is
    declined), and the branches this file claims to cover, per family that has them."""
    seen = collections.Counter()
    with x3_setting():
        for c in TABLE:
            g = c.g
            assert 8 * 8 * g.Cg * g.K * 0.5 < (1 << 24) // 8, c.name  # the exact pass: every sum of eighths stays exact
            assert rows_written(g)[1]
            for oname in c.ops:
                o = OPS[oname]
                if oname in IN_AUX:
                    assert all(v is None for v in c.expect.values()), "%s: the packed families take no derivative mask on x" % c.name
                for fam in PLANNED:
                    got = path_of(fill(c, o), fam, c.flip)
                    assert got == c.expect[fam], "%s %s %s: on %s, written for %s" % (c.name, oname, fam, got, c.expect[fam])
                    if got is None:
                        seen["%s declined" % fam] += 1
                        continue
                    BM = describe(fill(c, o), fam, c.flip)[1][1]
                    seen.update("%s %s" % (fam, tg) for tg in branch_tags(c, o, fam, got, BM))
                seen.update("gemm %s" % tg for tg in gemm_tags(c, oname))
    missing = [(fam, b) for fam in NEED for b in NEED[fam] if not seen["%s %s" % (fam, b)]]
    assert not missing, missing
    assert {p for p in (2, 3, 4) if any(seen["%s phases %d" % (f, p)] for f in ("pk", "bf16", "x3"))} == {2, 3, 4}


# ---------------------------------------------------------------------------------------------------------------------
# the contract's refusals, on the host: _plan and vcv_conv_plan_describe launch nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_out_of_contract_transforms_are_refused_by_every_planner():
    """out_tf outside {NONE, DLEAKY, DRELU, DTANH}, and out_tf != NONE without oaux: VCV_EINVAL from every family's _plan and
    from vcv_conv_plan_describe (the _run entries make the same eligibility test first).  The valid values stay eligible, and
    so does a given oaux with out_tf = NONE (the rows of tests/golden/conv_plan_census.npz)."""
    from vcvits_amd._lib import lib
    base = None
    for c in TABLE:
        if all(v is not None for v in c.expect.values()) and not c.flip:
            base = c
            break
    assert base is not None
    L = lib()
    with x3_setting():
        for fam in PLANNED:
            good = fill(base, OPS["bias"])
            assert plan(good, fam, 0)[0] == 0 and describe(good, fam, 0)[0] == 0
            good.oaux = PTR  # oaux given, out_tf NONE
            assert plan(good, fam, 0)[0] == 0
            for tf in (C.TF_DLEAKY, C.TF_DRELU, C.TF_DTANH):
                a = fill(base, OPS["bias"]._replace(out_tf=tf))
                assert plan(a, fam, 0)[0] == 0 and describe(a, fam, 0)[0] == 0, (fam, tf)
                a.oaux = None
                assert plan(a, fam, 0)[0] == EINVAL and describe(a, fam, 0)[0] == EINVAL, (fam, tf, "no oaux")
            for tf in (C.TF_LEAKY, C.TF_DLOGCLAMP, 6, 7, 100, -1):
                a = fill(base, OPS["bias"]._replace(out_tf=tf))
                assert a.oaux is not None
                assert plan(a, fam, 0)[0] == EINVAL and describe(a, fam, 0)[0] == EINVAL, (fam, tf)
            for tf in (C.TF_DLEAKY, C.TF_DRELU, C.TF_DTANH, C.TF_DLOGCLAMP, 6, -1):  # (in_tf: NONE / LEAKY only, as before)
                a = fill(base, OPS["bias"]._replace(in_tf=tf))
                assert plan(a, fam, 0)[0] == EINVAL, (fam, "in_tf", tf)
        a = fill(base, OPS["bias"]._replace(out_tf=C.TF_DLOGCLAMP))
        assert L.vcv_conv_dma_workspace(ctypes.byref(a)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# inputs and float64 references: made once per (case, kind) and shared
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(name, kind):
    """float32 CPU tensors of case `name`.  normal: seeded Gaussians, w scaled by (Cg K)^-1/2; exact: small integers and halves."""
    c = CASES[name]
    g = c.g
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    xs, ys = (g.B, g.G * g.Cg, g.Tin, g.P), (g.B, g.G * g.Mg, g.Tout, g.P)
    ws = (g.G * g.Mg * g.Cg * g.K,)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if kind == "exact":
        it = lambda lo, hi, sh: f(rng.integers(lo, hi + 1, sh))
        hv = lambda sh: f(rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], sh))
        t = dict(x=it(-8, 8, xs), w=it(-8, 8, ws), bias=it(-4, 4, (g.G * g.Mg,)), res=it(-4, 4, ys), prior=it(-4, 4, ys), oaux=hv(ys),
                 oaux_t=hv(ys), xaux=hv(xs), xaux_t=hv(xs), xaux_l=f(rng.choice([-1.0, 0.0], xs)))
    else:
        n = lambda sh: f(rng.standard_normal(sh))
        # DLOGCLAMP (clamp 0.5): aux = the logclamp output, kept clear of the threshold log(clamp) on both sides, so that the
        # comparison does not hang on the last bit of logf: clamped elements a quarter below it, the others 0.01 or more above
        lc = np.log(np.maximum(np.abs(rng.standard_normal(xs)) * 1.5, 0.5))
        lc = np.where(lc <= np.log(0.5) + 0.01, np.log(0.5) - 0.25, lc)
        t = dict(x=n(xs), w=n(ws) * float((g.Cg * g.K) ** -0.5), bias=n((g.G * g.Mg,)), res=n(ys), prior=n(ys), oaux=n(ys),
                 oaux_t=torch.tanh(n(ys)), xaux=n(xs), xaux_t=torch.tanh(n(xs)), xaux_l=f(lc))
    m = (rng.random((g.B, g.Tout)) < 0.7).astype(np.float32)
    m[:, -4:] = np.array([1.0, 0.0, 1.0, 0.0], dtype=np.float32)[-min(4, g.Tout):]  # zeros in the last partial group of four
    m[:, 0] = 0.0
    t["mask"] = f(m)
    if c.flip:  # the flipped / transposed copy the register-staged kernel reads ([Mg, Cg, K] of w [Cg, Mg, K])
        t["wf"] = t["w"].reshape(g.Cg, g.Mg, g.K).permute(1, 0, 2).flip(2).contiguous().reshape(-1)
    return t


def xaux_key(o):
    return {C.TF_DTANH: "xaux_t", C.TF_DLOGCLAMP: "xaux_l"}.get(o.in_tf, "xaux")


@functools.lru_cache(maxsize=None)
def reference(name, kind, oname, rounded):
    """(float64 y, S, d32): the whole expected y on top of the prior; d32 = max|float32 run - float64 run| where the operand
    set evaluates a transcendental, else 0."""
    c = CASES[name]
    o = exact_ops(OPS[oname]) if kind == "exact" else OPS[oname]
    t = inputs(name, kind)
    kw = dict(flip=c.flip, bias=t["bias"] if o.bias else None, res=t["res"] if o.res else None, mask=t["mask"] if o.mask else None,
              xaux=t[xaux_key(o)] if o.in_tf >= C.TF_DLEAKY else None,
              oaux=(t["oaux_t"] if o.out_tf == C.TF_DTANH else t["oaux"]) if o.out_tf != C.TF_NONE else None, in_tf=o.in_tf,
              out_act=o.out_act, out_tf=o.out_tf, accumulate=bool(o.acc), alpha=o.alpha, slope=o.slope, rounded=rounded)
    y, S = C.conv(c.g, t["x"], t["w"], t["prior"], **kw)
    d32 = 0.0
    if kind == "normal" and transcendental(o):
        y32, _ = C.conv(c.g, t["x"], t["w"], t["prior"], dtype=torch.float32, **kw)
        d32 = (y32.double() - y).abs().max().item()
    return y, S, d32


@functools.lru_cache(maxsize=2)
def on_gpu(name, kind, gpu):
    return {k: v.to(gpu) for k, v in inputs(name, kind).items()}


class Guarded:
    """A float32 view pre-filled with `init` (a tensor or a number) between two runs of GUARD sentinel floats."""

    def __init__(self, shape, device, init):
        n = int(np.prod(shape))
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENT, device=device)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if torch.is_tensor(init):
            self.t.copy_(init)
        else:
            self.t.fill_(init)

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())


def abi(gpu, c, ar, kind, oname, o=None):
    """One call through the C ABI (for x3 inside x3_setting).  -> (status, y or None).  The path the table names is asserted
    before the launch; the sentinels around y, the pack buffer and the scratch after it."""
    from vcvits_amd._lib import lib, stream
    fam = FAM_OF[ar]
    o = o or (exact_ops(OPS[oname]) if kind == "exact" else OPS[oname])
    t = dict(on_gpu(c.name, kind, gpu))
    t["xaux"] = t[xaux_key(o)]
    g = c.g
    y = Guarded((g.B, g.G * g.Mg, g.Tout, g.P), gpu, t["prior"])
    if fam == "gemm":
        a = fill(c, o, t, y.t, gemm_flip=bool(c.flip))
        st = lib().vcv_conv_gemm(ctypes.byref(a), stream())
        torch.cuda.synchronize()
        assert y.intact(), "%s %s %s: a write outside y" % (c.name, ar, oname)
        return st, y.t
    a = fill(c, o, t, y.t)
    assert path_of(a, fam, c.flip) == c.expect[fam], "%s %s %s: not the path the case was written for" % (c.name, ar, oname)
    rc, words = plan(a, fam, c.flip)
    if rc != 0:
        return rc, None
    pack = Guarded((max(words[0], 1),), gpu, float("nan"))
    scratch = Guarded((max(words[1], 1),), gpu, float("nan"))
    st = getattr(lib(), "vcv_conv_%s_run" % fam)(ctypes.byref(a), ctypes.c_void_p(pack.t.data_ptr()), ctypes.c_void_p(scratch.t.data_ptr()),
                                                  c.flip, 0, stream())
    torch.cuda.synchronize()
    assert y.intact(), "%s %s %s: a write outside y" % (c.name, ar, oname)
    assert pack.intact(), "%s %s %s: a write outside the pack buffer (%d words)" % (c.name, ar, oname, words[0])
    assert scratch.intact(), "%s %s %s: a write outside the scratch (%d floats)" % (c.name, ar, oname, words[1])
    return st, y.t


_parity = {}
HEADER = ("# tests/test_conv_epilogue_abi_gpu.py: distance of the five conv families at the C ABI from the float64 CPU reference\n"
          "# (tests/conv_f64.py), normal pass.  Per family: max|got - ref| / max|ref| (bounds: 2e-5; bf16 1e-5 against the reference of\n"
          "# the bf16-rounded operands) / the worst ratio of |got - ref| to its element-wise bound gamma_n * S + a (must be <= 1).\n"
          "# d32 = max|float32 CPU run - float64 run| of the reference, measured where the operand set evaluates a transcendental;\n"
          "# the allowance a is 4 * d32 there and 0 elsewhere, and gpu = max|got - ref| of the same operand set.  `-` marks a family\n"
          "# whose _plan declines the case (asserted).  The exact pass (integer operands) is bit-equal to float64 or fails: one line\n"
          "# per case and family says that it ran.\n")


def record(section, line):
    """Keep the measured distances in profiles/conv_epilogue_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "conv_epilogue_parity.txt"), "w") as f:
        f.write(HEADER)
        for name in _parity:
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def n_terms(c, ar):
    JA = -(-c.g.K // (c.g.phases if c.g.phases > 1 else 1))
    return (9 if FAM_OF[ar] == "x3" else 1) * c.g.Cg * JA + 6


def check(c, ar, kind, oname, got, fails):
    """got against the float64 reference: bit for bit (exact), or within both bounds (normal).  -> the cell for the profile."""
    o = exact_ops(OPS[oname]) if kind == "exact" else OPS[oname]
    y64, S, d32 = reference(c.name, kind, oname, ar == "bf16")
    prior = inputs(c.name, kind)["prior"]
    got = got.cpu()
    tag = "%s %s %s %s" % (c.name, ar, kind, oname)
    # what the contract does not write is the prior, bit for bit; a masked element is exactly 0 (+ the prior)
    g = c.g
    nph = g.phases if g.phases > 1 else 1
    trow = (np.arange(g.Q)[:, None] * g.os + g.oo + np.arange(nph)[None, :]).ravel()
    rows = np.zeros(g.Tout, dtype=bool)
    rows[trow[(trow >= 0) & (trow < g.Tout)]] = True
    keep = torch.from_numpy(~rows)
    if bool(keep.any()) and not torch.equal(got[:, :, keep], prior[:, :, keep]):
        fails.append("%s: rows the contract does not write were changed" % tag)
    if o.mask:
        m = (inputs(c.name, kind)["mask"] == 0) & torch.from_numpy(rows).view(1, -1)
        mm = m.view(g.B, 1, g.Tout, 1).expand_as(got)
        want = prior[mm] if o.acc else torch.zeros_like(got[mm])
        if not torch.equal(got[mm], want):
            fails.append("%s: a masked element is not exactly 0 (+ the prior)" % tag)
    if bool(torch.isnan(got).any()):
        fails.append("%s: NaN in y (a pack or scratch word read before it was written?)" % tag)
        return None
    if kind == "exact":
        assert bool((y64.float().double() == y64).all()), tag  # (the reference itself is a float32 number everywhere)
        if not torch.equal(got, y64.float()):
            bad = (got != y64.float()).nonzero()
            fails.append("%s: not the float64 reference's bits at %d elements, first %s (got %r, want %r)" % (
                tag, len(bad), bad[0].tolist(), got[tuple(bad[0])].item(), y64[tuple(bad[0])].item()))
        return None
    e = C.dist(got, y64)
    bound = TOL_BF16 if ar == "bf16" else TOL_F32
    el = C.gamma(n_terms(c, ar)) * S + 4.0 * d32 + (3 * 2.0 ** -24 * S if ar == "x3-6" else 0.0)
    diff = (got.double() - y64).abs()
    ratio = torch.where(diff > 0, diff / el.clamp(min=1e-300), torch.zeros_like(diff)).max().item()
    if e > bound:
        fails.append("%s: max-norm distance %.3e (bound %.1e)" % (tag, e, bound))
    if ratio > 1.0:
        i = tuple((diff / el.clamp(min=1e-300)).flatten().argmax().unsqueeze(0).tolist())
        fails.append("%s: element-wise, |got - ref| is %.3f x its bound (flat element %d)" % (tag, ratio, i[0]))
    return "%.1e/%.2f%s" % (e, ratio, " d32=%.1e gpu=%.1e" % (d32, diff.max().item()) if d32 else "")


def test_checker_notices_small_local_errors():
    """Host only, no library: what check() adds over the max-norm.  The float64 reference cast to float32 passes; then, one
    at a time: 1e-7 on an element the mask zeroes, one ulp on a row the contract does not write, 1.5 x its own bound on the
    element with the smallest S (under half of 2e-5 of max|ref|: the max-norm does not see it), and one ulp in the exact pass."""
    def run(name, kind, oname, poke=None, ar="pk"):
        got = reference(name, kind, oname, False)[0].float()
        if poke:
            poke(got)
        fails = []
        check(CASES[name], ar, kind, oname, got, fails)
        return fails

    ulp = lambda t, i: t.__setitem__(i, torch.nextafter(t[i], torch.tensor(float("inf"))))
    for name, kind, oname in (("row-U97", "normal", "mask"), ("os2", "normal", "bias"), ("row-U97", "normal", "res_inleaky"),
                              ("split-flip-U130", "exact", "all"), ("phased-3", "exact", "acc_res_mask")):
        assert run(name, kind, oname) == [], (name, kind, oname)
    g = CASES["row-U97"].g
    assert inputs("row-U97", "normal")["mask"][0, g.Tout - 1] == 0
    f = run("row-U97", "normal", "mask", lambda t: t.__setitem__((0, 3, g.Tout - 1, 0), 1e-7))
    assert len(f) == 1 and "masked element" in f[0], f
    f = run("os2", "normal", "bias", lambda t: ulp(t, (1, 5, 1, 0)))  # (row 1 of y is no q * 2)
    assert "does not write" in f[0], f  # (the element-wise bound, zero there, reports it too)
    y64, S, _ = reference("row-U97", "normal", "res_inleaky", False)
    i = tuple(np.unravel_index(int(S.argmin()), S.shape))
    delta = 1.5 * C.gamma(n_terms(CASES["row-U97"], "pk")) * S[i].item()
    assert delta < 0.5 * TOL_F32 * y64.abs().max().item()
    f = run("row-U97", "normal", "res_inleaky", lambda t: t.__setitem__(i, float(y64[i]) + delta))
    assert len(f) == 1 and "element-wise" in f[0], f
    f = run("split-flip-U130", "exact", "all", lambda t: ulp(t, (0, 129, 128, 0)))  # (the last row, unmasked column)
    assert len(f) == 1 and "bits at 1 elements" in f[0], f


# ---------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ar", ARITHS)
@pytest.mark.parametrize("name", [c.name for c in TABLE])
def test_epilogue_parity(gpu, name, ar, kind):
    """One case x family: every operand set of the case, each launched twice."""
    c = CASES[name]
    fam = FAM_OF[ar]
    fails, cells = [], []
    ctx = x3_setting(9 if ar == "x3-9" else 6) if fam == "x3" else contextlib.nullcontext()
    with ctx:
        for oname in c.ops:
            if fam != "gemm" and c.expect[fam] is None:
                st, y = abi(gpu, c, ar, kind, oname)
                assert st == EINVAL and y is None, "%s %s %s: the table says declined, _plan returned %d" % (name, ar, oname, st)
                cells.append("%s: -" % oname)
                continue
            st1, y1 = abi(gpu, c, ar, kind, oname)
            st2, y2 = abi(gpu, c, ar, kind, oname)
            assert st1 == 0 and st2 == 0, "%s %s %s: status %d / %d" % (name, ar, oname, st1, st2)
            if not torch.equal(y1.view(torch.int32), y2.view(torch.int32)):
                fails.append("%s %s %s: two identical launches differ" % (name, ar, oname))
            cell = check(c, ar, kind, oname, y1, fails)
            if cell:
                cells.append("%s: %s" % (oname, cell))
    if kind == "normal":
        record(name, "%-6s %s" % (ar, "  ".join(cells)))
    elif not fails:
        record(name, "%-6s exact pass: %s" % (ar, "declined" if cells else "%d operand sets bit-equal to float64, launches repeat" % len(c.ops)))
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# vcv_conv_gemm has no plan entry: its refusals on the device, with every operand valid and allocated
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gemm_refuses_out_of_contract_transforms(gpu):
    """vcv_conv_gemm tests out_tf / in_tf before any launch (csrc/conv_gemm.hip: the checks stand above the tile choice):
    VCV_EINVAL and an untouched y for out_tf in {LEAKY, DLOGCLAMP, 6, -1} and in_tf in {6, -1}, with x, xaux, oaux and y
    all valid and fully allocated; the same buffers are accepted with a selector of the contract."""
    c = TABLE[0]
    refused = []
    for what, o in [("out_tf=%d" % tf, OPS["bias"]._replace(out_tf=tf, in_tf=C.TF_DLEAKY)) for tf in (C.TF_LEAKY, C.TF_DLOGCLAMP, 6, -1)] + \
                   [("in_tf=%d" % tf, OPS["bias"]._replace(in_tf=tf, out_tf=C.TF_DLEAKY)) for tf in (6, 100, -1)]:
        st, y = abi(gpu, c, "gemm", "normal", "bias", o)
        assert st == EINVAL, (what, st)
        assert torch.equal(y.cpu(), inputs(c.name, "normal")["prior"]), "%s: a refused call wrote to y" % what
        refused.append(what)
    st, y = abi(gpu, c, "gemm", "normal", "bias", OPS["bias"]._replace(out_tf=C.TF_DLEAKY, in_tf=C.TF_DLOGCLAMP, slope=0.5))
    assert st == 0 and not torch.equal(y.cpu(), inputs(c.name, "normal")["prior"])
    record("refusals", "vcv_conv_gemm: VCV_EINVAL and y untouched for %s" % ", ".join(refused))


# ---------------------------------------------------------------------------------------------------------------------
# routing: ops.conv_forward / ops.conv_dgrad with the family forced reach the same kernel
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def ops_mode(ar):
    """ops with `ar`'s family first in line; everything comes back."""
    from vcvits_amd import ops
    from vcvits_amd._lib import lib
    from vcvits_amd.ops import core
    old = (ops.compute_dtype(), core._USE_X3[0], lib().vcv_conv_x3_get_terms(), lib().vcv_conv_x3_get_all(), core._USE_PK[0])
    try:
        ops.set_compute_dtype("bf16" if ar == "bf16" else "f32")
        if FAM_OF[ar] == "x3":
            ops.set_f32_split(True, terms=9 if ar == "x3-9" else 6, all_shapes=True)
        else:
            ops.set_f32_split(False)
        core._USE_PK[0] = ar != "dma"
        yield ops
    finally:
        ops.set_compute_dtype(old[0])
        ops.set_f32_split(old[1], terms=old[2], all_shapes=bool(old[3]))
        core._USE_PK[0] = old[4]


ROUTED = (("row-U161", "alpha"), ("split-flip-U130", "dleaky"), ("period-P3-mask", "acc_res_mask"))


@pytest.mark.gpu
@pytest.mark.parametrize("name,oname", ROUTED)
def test_routing_same_bits_as_the_abi_call(gpu, name, oname):
    """ops.conv_forward (a forward case) / ops.conv_dgrad (a flip case) with each packed family forced in turn: one launch of
    that family, and the bits of the ABI call."""
    c = CASES[name]
    g, o = c.g, OPS[oname]
    t = on_gpu(name, "normal", gpu)
    sq = (lambda v: v[..., 0]) if g.P == 1 else (lambda v: v)
    kw = dict(slope=o.slope, alpha=o.alpha, in_tf=o.in_tf, out_act=o.out_act, out_tf=o.out_tf, accumulate=bool(o.acc))
    if o.res:
        kw["res"] = sq(t["res"])
    if o.mask:
        kw["mask"] = t["mask"]
    if o.out_tf != C.TF_NONE:
        kw["oaux"] = sq(t["oaux_t" if o.out_tf == C.TF_DTANH else "oaux"])
    for ar in ("pk", "bf16", "x3-6", "dma"):
        fam = FAM_OF[ar]
        if c.expect[fam] is None:
            continue
        with ops_mode(ar) as ops:
            out = sq(t["prior"]).clone()
            before = dict(ops.LAUNCH_COUNTS)
            if c.flip:
                w = t["w"].view(g.Cg, g.Mg, g.K)  # the forward conv's weight [M, C, K] = the launch's [Cg, Mg, K]
                pad = g.off + (g.K - 1) * g.dj
                ops.conv_dgrad(sq(t["x"]), w, tuple(out.shape), stride=1, pad=pad, dil=g.dj, out=out, **kw)
            else:
                w = t["w"].view(g.Mg, g.Cg, g.K)
                ops.conv_forward(sq(t["x"]), w, t["bias"] if o.bias else None, stride=g.s, pad=-g.off, dil=g.dj, out=out, **kw)
            torch.cuda.synchronize()
            moved = {k: ops.LAUNCH_COUNTS[k] - before.get(k, 0) for k in ops.LAUNCH_COUNTS if ops.LAUNCH_COUNTS[k] != before.get(k, 0)}
        assert moved == {fam: 1}, "%s %s: ops launched %s" % (name, ar, moved)
        ctx = x3_setting(6) if fam == "x3" else contextlib.nullcontext()
        with ctx:
            st, y = abi(gpu, c, ar, "normal", oname)
        assert st == 0 and torch.equal(sq(y), out), "%s %s %s: ops did not give the ABI call's bits" % (name, ar, oname)
        record("routing", "%-28s %-12s %s: ops gives the ABI call's bits" % (name, oname, ar))

"""The thin conv kernels of csrc/conv_thin.hip (vcv_conv_m1_fwd, vcv_conv_c1_fwd / _masked / _flip, vcv_conv_c1_dgrad,
vcv_thin_wgrad, vcv_linear_t1_fwd / _dgrad / _wgrad) at the C ABI, at the edges of their launchers, against float64 CPU
restatements of the same operations: tests/conv_f64.py (conv(), dgrad()) for the convolutions, tests/wgrad_f64.py (wgrad())
for the weight gradient -- both pinned to torch in tests/test_conv_f64_cpu.py, tests/test_wgrad_f64_cpu.py and
tests/test_wgrad_mfma_abi_gpu.py -- and a float64 matmul for the one-frame layers.

Every kernel is called through ctypes with hand-filled arguments, so the router of ops/conv.py cannot send a case elsewhere.
Each launcher's dispatch arithmetic is restated below in plain Python (m1_rule, c1_rule, wgrad_rule, t1_dgrad_rule): every case
names the branches it was written for, test_case_table_reaches_every_branch proves on the host that the restated rules put it
there and that the table as a whole reaches every branch in NEED, and test_routing_* check that ops.* gives the bits of the ABI
call.  Tuning keys and the deterministic flag stay at their defaults (tests/test_switch_parity_gpu.py moves them), except for
the two cases of test_deterministic_mode_repeats.

Two passes over one table:
  exact    operands are integers in [-8, 8], bias and the prior dw integers in [-4, 4], oaux and the aux tensors in
           {-1, -0.5, 0, 0.5, 1} ({-1, 0} under DLOGCLAMP, where exp(-aux) must be a float32), slope = 0.5, alpha as the case
           says (1 or 0.5), out_act NONE / LEAKY / RELU (TANH runs as RELU).  Every partial sum is a multiple of a quantum and
           below 2^24 quanta (test_exact_pass_is_exact, from the table alone), so any summation order is exact, atomics
           included, and the result must be BIT-EQUAL to the float64 reference cast to float32.
  normal   Gaussian inputs, weights scaled by (C K)^-1/2.  Two bounds, both asserted:
           1. max|got - ref| / max|ref| <= 2e-5 (y, dx) or 3e-5 (dw): the bounds of tests/test_switch_parity_gpu.py;
           2. element-wise |got - ref| <= gamma_n * S + a, gamma_n = n u / (1 - n u), u = 2^-24; n = the number of terms behind
              the element + 6; S = the float64 sum of magnitudes behind it; a = 0 except under out_act TANH and the DTANH /
              DLOGCLAMP transforms, where a = 4 * d32, d32 = max|float32 CPU run - float64 run| of the same reference.

Every output is a view inside a larger buffer with 1024 sentinel floats on each side, which must come back untouched; outputs
the kernel overwrites are pre-filled with NaN, dw with the prior the reference was given; a refused call (VCV_EINVAL) must leave
its output bit-identical.  Launches that do not combine with atomics must repeat their bits on a second call; the atomic ones
are held to their bounds on both calls.  No case is skipped at run time.

Distances go to profiles/conv_thin_parity.txt, one line per case."""
import collections
import ctypes
import functools
import math
import os
import zlib

import numpy as np
import pytest
import torch

import conv_f64 as C
import wgrad_f64 as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
TOL, TOL_DW = 2e-5, 3e-5  # tests/test_switch_parity_gpu.py
GUARD, SENT = 1024, 12345.0
KINDS = ("exact", "normal")
NONE, LEAKY, RELU, TANH = C.ACT_NONE, C.ACT_LEAKY, C.ACT_RELU, C.ACT_TANH
TF_NAME = {W.TF_NONE: "NONE", W.TF_LEAKY: "LEAKY", W.TF_DLEAKY: "DLEAKY", W.TF_DRELU: "DRELU", W.TF_DTANH: "DTANH", W.TF_DLOGCLAMP: "DLOGCLAMP"}


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' rules, restated (csrc/conv_thin.hip) -- plain integer arithmetic, no library
# ---------------------------------------------------------------------------------------------------------------------
def m1_rule(p, det=False):
    """vcv_conv_m1_fwd -> dict(kernel="lds" | "reg", ...) or None (VCV_EINVAL)."""
    B, Cn, Tin, Tout, P, K, s, dil, pad = (p[k] for k in ("B", "C", "Tin", "Tout", "P", "K", "s", "dil", "pad"))
    U = Tout * P
    nt = cdiv(U, 256)
    splits = 1
    if p["act"] == NONE:
        while splits < 64 and nt * B * splits < 1024 and Cn // (splits * 2) >= 8:
            splits *= 2
    if det:
        splits = 1
    halo = (K - 1) * dil * P
    if s == 1 and halo <= 256 and Tin * P < 2 ** 31:
        TU = min(U, 256)
        R = 256 // TU
        ntl = cdiv(U, TU)
        splits = 1
        if p["act"] == NONE and not det:
            while splits < 64 and ntl * B * splits < 1024 and Cn // (splits * 2) >= 8 * R:
                splits *= 2
        cperl = cdiv(Cn, splits)
        Wd = TU + halo
        raw = (40 * 1024 // 4 - 256) // (Wd + K)
        cch = (min(raw, cperl) + 7) & ~7
        chunks = []  # per workgroup along z: the channel counts of its LDS chunks
        for z in range(cdiv(Cn, cperl)):
            lo, hi = z * cperl, min(Cn, z * cperl + cperl)
            chunks.append([min(cch, hi - c0) for c0 in range(lo, hi, cch)])
        flat = ntl == 1 and Tout == Tin + 2 * pad - dil * (K - 1)
        return dict(kernel="lds", TU=TU, R=R, ntl=ntl, splits=splits, cperl=cperl, W=Wd, raw=raw, cch=cch, chunks=chunks, flat=flat,
                    halo=halo, lds_floats=cch * (Wd + K) + 256)
    if K > 16:
        return None
    return dict(kernel="reg", splits=splits, cper=cdiv(Cn, splits), halo=halo)


def m1_tags(p, det=False):
    r = m1_rule(p, det)
    if r is None:
        return ["einval"]
    bias = "with bias" if p["bias"] else "no bias"
    if r["kernel"] == "reg":
        return ["reg", "reg stride %d" % p["s"], ("reg split " + bias) if r["splits"] > 1 else "reg no split"] + ["reg K 16"] * (p["K"] == 16)
    tags = ["lds", "R>1" if r["R"] > 1 else "R=1", "flat" if r["flat"] else "staged"]
    if r["R"] > 1:
        tags += ["TU does not divide 256"] * (256 % r["TU"] != 0)
        tags += ["a chunk is no multiple of R"] * any(n % r["R"] for ch in r["chunks"] for n in ch)
        tags += ["staged R>1"] * (not r["flat"])
    tags += ["cch rounded up past the LDS sizing"] * (r["raw"] < r["cperl"] and r["raw"] % 8 != 0)
    tags += ["chunks>1"] * (max(len(ch) for ch in r["chunks"]) > 1)
    tags += ["lds split " + bias] if r["splits"] > 1 else ["lds no split"]
    tags += ["K>16"] * (p["K"] > 16) + ["halo 256"] * (r["halo"] == 256) + ["tiles>1"] * (r["ntl"] > 1) + ["period"] * (p["P"] > 1)
    tags += ["pad 0"] * (p["pad"] == 0) + ["in_leaky"] * bool(p["leaky"]) + ["tanh"] * (p["act"] == TANH)
    return tags


def c1_rule(p):
    """vcv_conv_c1_fwd* -> dict(mch, R, ...) or None."""
    if p["K"] > 16:
        return None
    B, M, U = p["B"], p["M"], p["Tout"] * p["P"]
    top = mch = min(M, 64)
    tiles = cdiv(U, 256) * B
    floor_ch = 32 if U < 256 else 8
    while mch > floor_ch and tiles * cdiv(M, mch) < 2048:
        mch = (mch + 1) // 2
    TU = min(U, 256)
    return dict(mch=mch, top=top, floor=floor_ch, R=256 // TU, TU=TU, nch=cdiv(M, mch))


def c1_tags(p):
    r = c1_rule(p)
    if r is None:
        return ["einval"]
    tags = ["R>1" if r["R"] > 1 else "R=1"] + ["TU does not divide 256"] * (r["R"] > 1 and 256 % r["TU"] != 0)
    tags += ["chunks>1"] * (r["nch"] > 1) + ["chunk halved"] * (r["mch"] < r["top"]) + ["chunk below its floor"] * (r["mch"] < r["floor"] and r["mch"] < r["top"])
    tags += ["last chunk short"] * (p["M"] % r["mch"] != 0) + ["M > 64"] * (p["M"] > 64)
    tags += ["chunk is no multiple of R"] * (r["R"] > 1 and min(r["mch"], p["M"]) % r["R"] != 0)
    if p["flip"]:
        tags.append("flip K even" if p["K"] % 2 == 0 else "flip K odd")
    if p["oaux"]:
        tags.append("oaux with act" if p["act"] != NONE else "oaux")
    tags += ["act leaky"] * (p["act"] == LEAKY) + ["no bias"] * (not p["bias"]) + ["stride %d" % p["s"]] * (p["s"] > 1) + ["dil 2"] * (p["dil"] == 2)
    tags += ["period"] * (p["P"] > 1) + ["api " + p["api"]]
    return tags


def c1_dgrad_tags(p):
    if p["M"] > 64 or p["K"] > 16:
        return ["einval"]
    last = (p["Tout"] - 1) * p["s"] + (p["K"] - 1) * p["dil"] - p["pad"]
    tags = ["stride %d" % p["s"], "dil %d" % p["dil"]] + ["period"] * (p["P"] > 1)
    tags += ["rows past the last tap"] * (p["Tin"] - 1 > last) + ["rows end at the last tap"] * (p["Tin"] - 1 == last)
    tags += ["r % s"] * (p["s"] > 1) + ["tiles>1"] * (p["Tin"] * p["P"] > 256)
    return tags


def wgrad_rule(p, det=False):
    """vcv_thin_wgrad -> dict(kernel="pairs" | "row", ...) or None."""
    B, M, Cn, Ta, P, K, s, d = (p[k] for k in ("B", "M", "C", "Ta", "P", "K", "s", "d"))
    if K > 16 or (p["a_tf"] >= W.TF_DLEAKY and not p["aaux"]) or (p["b_tf"] >= W.TF_DLEAKY and not p["baux"]):
        return None
    fell = None
    if Cn == 1 and s == 1 and M * K <= 256 and p["a_tf"] == W.TF_NONE and p["b_tf"] == W.TF_NONE and not det and P <= 256:
        tq = min(256 // P, Ta)
        qper = tq * max(1024 // (tq * P), 1)
        rounded = qper > Ta
        if rounded:
            qper = cdiv(Ta, tq) * tq
        xw = ((qper - 1) * s + (K - 1) * d + 1) * P
        TUP = tq * P
        padded = TUP % 32 == 0
        if padded:
            TUP += 1
        smem = 4 * (xw + M * TUP)
        if smem <= 60 * 1024:
            return dict(kernel="pairs", tq=tq, qper=qper, xw=xw, TUP=TUP, padded=padded, rounded=rounded, smem=smem, nchunk=cdiv(Ta, qper))
        fell = "lds"
    splits = 1
    while splits < B and M * Cn * splits < 4096:
        splits *= 2
    splits = min(splits, B)
    if det:
        splits = 1
    bper = cdiv(B, splits)
    U = Ta * P
    usplit = 2048 // (M * Cn * cdiv(B, bper))
    usplit = min(usplit, U // 1024)
    if usplit < 1 or det:
        usplit = 1
    uper = (cdiv(U, usplit) + 255) & ~255
    blocks = [min(uper, U - z * uper) for z in range(cdiv(U, uper))]
    plain = p["a_tf"] == W.TF_NONE and p["b_tf"] == W.TF_NONE
    return dict(kernel="row", splits=splits, bper=bper, usplit=usplit, uper=uper, blocks=blocks, plain=plain,
                KT=(K if K in (3, 5, 7) else 0) if plain else 0, fell=fell)


def wgrad_tags(p, det=False):
    r = wgrad_rule(p, det)
    if r is None:
        return ["einval"]
    if r["kernel"] == "pairs":
        tags = ["pairs", "pairs TUP padded" if r["padded"] else "pairs TUP as is"]
        tags += ["pairs period"] * (p["P"] > 1) + ["pairs tq clipped to Ta"] * (r["tq"] == p["Ta"] and r["tq"] < 256 // p["P"])
        tags += ["pairs qper rounded past Ta"] * r["rounded"] + ["pairs tiles>1 per chunk"] * (r["qper"] > r["tq"]) + ["pairs chunks>1"] * (r["nchunk"] > 1)
        tags += ["pairs last tile short"] * (p["Ta"] % r["tq"] != 0) + ["pairs M*K 256"] * (p["M"] * p["K"] == 256) + ["pairs P 256"] * (p["P"] == 256)
        tags += ["pairs dil 2"] * (p["d"] == 2) + ["pairs off %d" % p["off"]] + ["pairs Tb short"] * (p["Tb"] < p["Ta"] + (p["K"] - 1) * p["d"] + p["off"])
        return tags
    long_ = [n >= 512 for n in r["blocks"]]
    tags = ["row", "row <%s,%d>" % ("PLAIN" if r["plain"] else "TF", r["KT"])]
    if not r["plain"]:
        tags.append("row tf %s,%s" % (TF_NAME[p["a_tf"]], TF_NAME[p["b_tf"]]))
    tags.append("row all long" if all(long_) else "row all short" if not any(long_) else "row mixed")
    tags += ["row last block short, others long"] * (len(long_) > 1 and all(long_[:-1]) and not long_[-1])
    tags += ["row batch split"] * (r["splits"] > 1) + ["row bper>1"] * (r["bper"] > 1) + ["row usplit>1"] * (len(r["blocks"]) > 1)
    tags += ["row by lds fall-through"] * (r["fell"] == "lds") + ["row by M*K 257"] * (p["C"] == 1 and p["s"] == 1 and p["M"] * p["K"] == 257)
    tags += ["row by P 257"] * (p["C"] == 1 and p["s"] == 1 and p["P"] == 257) + ["row C=1 strided"] * (p["C"] == 1 and p["s"] > 1)
    tags += ["row alpha 0.5 onto a prior"] * (p["alpha"] != 1.0 and bool(p["prior"])) + ["row alpha 0.5 onto zeros"] * (p["alpha"] != 1.0 and not p["prior"])
    tags += ["row period"] * (p["P"] > 1)
    return tags


def t1_dgrad_rule(p):
    nct = cdiv(p["C"], 256)
    by_c, by_m = 512 // nct, p["M"] // 16
    msplit = max(min(by_c, by_m), 1)
    mper = cdiv(p["M"], msplit)
    return dict(nct=nct, msplit=msplit, mper=mper, ny=cdiv(p["M"], mper), by="floor" if by_m < 1 else "M/16" if by_m <= by_c else "512/nct")


def t1_tags(entry, p):
    if p["B"] > 32 and entry != "t1_wgrad":
        return ["einval"]
    tags = ["C < 64"] * (p["C"] < 64) + ["C % 64"] * (p["C"] % 64 != 0 and p["C"] > 64) + ["C = 64 n"] * (p["C"] % 64 == 0)
    tags += ["M % 4"] * (p["M"] % 4 != 0) + ["B 32"] * (p["B"] == 32) + ["no bias"] * (entry == "t1_fwd" and not p["bias"])
    if entry == "t1_dgrad":
        r = t1_dgrad_rule(p)
        tags += ["msplit by " + r["by"]] + ["nct>1"] * (r["nct"] > 1) + ["last m block short"] * (p["M"] % r["mper"] != 0) + ["msplit>1"] * (r["msplit"] > 1)
    return tags


TAGS = {"m1": m1_tags, "c1": c1_tags, "c1_dgrad": c1_dgrad_tags, "wgrad": wgrad_tags, "t1_fwd": lambda p: t1_tags("t1_fwd", p),
        "t1_dgrad": lambda p: t1_tags("t1_dgrad", p), "t1_wgrad": lambda p: t1_tags("t1_wgrad", p)}

# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "entry name p want")
TABLE = []


def add(entry, name, p, want):
    assert (entry, name) not in [(c.entry, c.name) for c in TABLE], (entry, name)
    TABLE.append(Case(entry, name, p, tuple(want)))


def out_len(Tin, K, s, pad, dil):
    return (Tin + 2 * pad - dil * (K - 1) - 1) // s + 1


def m1(name, Cn, Tout, want, P=1, K=3, dil=1, pad=1, s=1, B=2, Tin=None, leaky=0, act=NONE, bias=1):
    """Tin by default: the one whose formula(Tin) = Tin + 2*pad - dil*(K-1) gives Tout rows (stride 1), or the shortest for it"""
    if Tin is None:
        Tin = (Tout - 1) * s + dil * (K - 1) + 1 - 2 * pad
    add("m1", name, dict(B=B, C=Cn, Tin=Tin, Tout=Tout, P=P, K=K, s=s, dil=dil, pad=pad, leaky=leaky, act=act, bias=bias), want)


# -- m1, stride 1 (LDS kernel): short rows x channel counts
for U_ in (2, 30, 100, 255, 256, 257, 513):
    for Cn_ in (16, 17, 40):
        w_ = ["lds", "flat" if U_ <= 256 else "staged", "R>1" if U_ <= 128 else "R=1"] + ["TU does not divide 256"] * (U_ in (30, 100)) + ["tiles>1"] * (U_ > 256)
        if U_ == 2 or (U_ in (30, 100) and Cn_ == 17):  # R = 128, 8, 2
            w_.append("a chunk is no multiple of R")
        m1("U%d-C%d" % (U_, Cn_), Cn_, U_, w_, act=(NONE, LEAKY, RELU)[(U_ + Cn_) % 3], bias=(U_ + Cn_) % 2)
# (U = 2 has R = 128 channel sub-rows per workgroup: the launcher splits only while C / (2 splits) >= 8 R, so 1024 channels stay
# in one workgroup per batch element there; U = 30, R = 8: 16 splits of 64 channels meet in atomics)
m1("U2-C1024-bias", 1024, 2, ("lds", "R>1", "lds no split"), bias=1)
m1("U2-C1024-nobias", 1024, 2, ("lds", "R>1", "lds no split"), bias=0)
m1("U30-C1024-bias", 1024, 30, ("lds", "R>1", "lds split with bias", "TU does not divide 256"), bias=1)
m1("U30-C1024-nobias", 1024, 30, ("lds", "R>1", "lds split no bias"), bias=0)
m1("U100-C1030", 1030, 100, ("lds", "R>1", "lds split with bias", "a chunk is no multiple of R"))
# -- chunks: 100 channels at 256 positions under tanh: no split, the LDS sizing gives 38 channels, rounded up to 40: 40 / 40 / 20
m1("chunks-tanh", 100, 256, ("lds", "chunks>1", "cch rounded up past the LDS sizing", "tanh", "lds no split"), act=TANH)
m1("chunks-tanh-inleaky", 100, 256, ("lds", "chunks>1", "cch rounded up past the LDS sizing", "tanh", "in_leaky"), act=TANH, leaky=1)
# -- taps
for K_ in (1, 2, 7, 16, 17, 41):
    m1("K%d" % K_, 16, 100, ["lds"] + ["K>16"] * (K_ > 16), K=K_, pad=K_ // 2, Tin=100 - 2 * (K_ // 2) + K_ - 1)
m1("K17-dil16-halo256", 16, 256, ("lds", "K>16", "halo 256", "flat"), K=17, dil=16, pad=128)
m1("K5-dil32-P2-halo256", 16, 50, ("lds", "halo 256", "period", "R>1"), K=5, dil=32, P=2, pad=64)
# -- period rows
for P_ in (2, 3, 37):
    for dil_ in (1, 2):
        m1("P%d-dil%d" % (P_, dil_), 17, 7, ("lds", "period"), P=P_, dil=dil_, pad=dil_)
# -- Tout off the formula at U < 256: the two-loads-per-lane staging with R > 1; the extra rows read zeros
m1("Tout-formula-minus-3", 17, 97, ("lds", "staged R>1"), Tin=100)
m1("Tout-formula-plus-2", 40, 102, ("lds", "staged R>1"), Tin=100, act=LEAKY)
m1("Tout-formula-plus-2-P3", 16, 32, ("lds", "staged R>1", "period"), Tin=30, P=3, leaky=1)
m1("pad0", 16, 98, ("lds", "pad 0", "flat"), pad=0)
m1("U100-C40-inleaky", 40, 100, ("lds", "in_leaky", "lds split with bias", "R>1"), leaky=1, B=4)
# -- m1, register kernel (any stride > 1)
for i_, (s_, K_, dil_, P_) in enumerate([(2, 1, 1, 1), (2, 3, 1, 2), (2, 5, 3, 1), (2, 16, 1, 1), (3, 1, 3, 2), (3, 3, 3, 1), (3, 5, 1, 2), (3, 16, 3, 1)]):
    m1("s%d-K%d-dil%d-P%d" % (s_, K_, dil_, P_), (16, 40)[i_ % 2], (100, 150)[i_ % 2] // P_, ("reg", "reg stride %d" % s_, "reg split no bias" if i_ % 2 == 0 else "reg split with bias"),
       s=s_, K=K_, dil=dil_, P=P_, pad=dil_ * (K_ - 1) // 2, bias=i_ % 2)
m1("s2-C40-tanh", 40, 300, ("reg", "reg no split"), s=2, K=5, pad=2, act=TANH, leaky=1)
m1("s2-C1024-bias", 1024, 30, ("reg", "reg split with bias"), s=2, K=3)
m1("s3-C1024-P2-bias", 1024, 15, ("reg", "reg split with bias"), s=3, K=3, P=2)
# -- refused: more than 16 taps where the LDS kernel does not take the launch
m1("K17-dil17-einval", 16, 100, ("einval",), K=17, dil=17, pad=136)
m1("K17-s2-einval", 16, 100, ("einval",), K=17, s=2, pad=8)


def c1(name, M, Tout, want, P=1, K=5, s=1, dil=1, pad=None, B=2, Tin=None, act=NONE, bias=1, oaux=0, flip=0, api=None):
    pad = dil * (K - 1) // 2 if pad is None else pad
    if Tin is None:
        Tin = (Tout - 1) * s + dil * (K - 1) + 1 - 2 * pad
    api = api or ("flip" if flip else "masked" if oaux else "fwd")
    add("c1", name, dict(B=B, M=M, Tin=Tin, Tout=Tout, P=P, K=K, s=s, dil=dil, pad=pad, act=act, bias=bias, oaux=oaux, flip=flip, api=api), want)


for M_ in (1, 16, 17, 32, 40, 64, 65, 100):
    for U_ in ((30, 257) if M_ % 2 else (100, 255, 256, 700)):
        w_ = ["R>1" if U_ <= 128 else "R=1"] + ["M > 64"] * (M_ > 64) + ["chunk below its floor"] * (M_ == 17 and U_ >= 256)
        c1("M%d-U%d" % (M_, U_), M_, U_, w_, act=(NONE, LEAKY)[(M_ + U_) % 2], bias=(M_ // 2 + U_) % 2)
c1("M1024-U30", 1024, 30, ("R>1", "M > 64", "chunks>1", "TU does not divide 256"), K=3)
c1("M1024-U60-P2", 1024, 30, ("R>1", "M > 64", "chunks>1", "period"), K=3, P=2, act=LEAKY)
for K_ in (1, 4, 15, 16):
    c1("K%d" % K_, 16, 100, ("R>1",), K=K_, pad=K_ // 2, Tin=100 - 2 * (K_ // 2) + K_ - 1)
c1("K17-einval", 16, 100, ("einval",), K=17, pad=8)
for s_, dil_, P_ in ((3, 1, 2), (3, 2, 1), (1, 2, 3), (3, 2, 3)):
    c1("s%d-dil%d-P%d" % (s_, dil_, P_), 32, 40, ["period"] * (P_ > 1) + ["stride 3"] * (s_ == 3) + ["dil 2"] * (dil_ == 2), s=s_, dil=dil_, P=P_, act=LEAKY)
c1("oaux", 32, 100, ("oaux", "api masked"), oaux=1)
c1("oaux-leaky", 40, 300, ("oaux with act", "api masked", "R=1"), oaux=1, act=LEAKY)
c1("oaux-leaky-nobias-short", 17, 30, ("oaux with act", "no bias", "R>1"), oaux=1, act=LEAKY, bias=0)
for K_ in (4, 5):
    for f_ in (0, 1):
        c1("flip%d-K%d" % (f_, K_), 33, 100, ["api flip"] + [("flip K even", "flip K odd")[K_ % 2]] * f_, K=K_, pad=2, Tin=100 - 4 + K_ - 1, flip=f_, api="flip", oaux=f_)
# the geometry ops.conv_dgrad builds for a discriminator head, conv_post = Conv(1024 -> 1, k3, pad 1): the data gradient is a
# one-input-channel conv of dy [B, 1, 30] with the flipped taps, pad' = (K-1)*dil - pad, onto 1024 channels
c1("head-dgrad", 1024, 30, ("flip K odd", "M > 64", "chunks>1", "R>1", "no bias"), K=3, pad=2 * 1 - 1, Tin=30, flip=1, bias=0)
c1("head-dgrad-dleaky-P3", 1024, 10, ("flip K odd", "oaux", "period"), K=3, pad=1, Tin=10, P=3, flip=1, bias=0, oaux=1)


def c1d(name, M, Tout, want, P=1, K=5, s=1, dil=1, pad=None, B=2, extra=0):
    pad = dil * (K - 1) // 2 if pad is None else pad
    last = (Tout - 1) * s + (K - 1) * dil - pad
    add("c1_dgrad", name, dict(B=B, M=M, Tin=last + 1 + extra, Tout=Tout, P=P, K=K, s=s, dil=dil, pad=pad), want)


for i_, (M_, s_, dil_, P_, K_) in enumerate([(1, 1, 1, 1, 1), (16, 2, 1, 3, 5), (33, 3, 2, 1, 15), (64, 1, 2, 3, 16), (16, 3, 1, 1, 16), (33, 2, 2, 3, 5),
                                             (64, 3, 1, 3, 15), (1, 2, 2, 1, 5), (64, 2, 1, 1, 1), (16, 1, 1, 3, 15)]):
    for extra_ in (0, 4):
        c1d("M%d-s%d-dil%d-P%d-K%d-extra%d" % (M_, s_, dil_, P_, K_, extra_), M_, 40, ["stride %d" % s_, "dil %d" % dil_] +
            ["rows past the last tap" if extra_ else "rows end at the last tap"], P=P_, K=K_, s=s_, dil=dil_, extra=extra_)
c1d("M65-einval", 65, 40, ("einval",))


def wg(name, M, Cn, Ta, want, P=1, K=5, s=1, d=1, off=None, B=2, short=0, a_tf=W.TF_NONE, b_tf=W.TF_NONE, aaux=None, baux=None, alpha=1.0, prior=1):
    """Tb fits exactly: the last tap of the last position is the last row of b; `short` rows fewer"""
    off = -(d * (K - 1) // 2) if off is None else off
    Tb = max((Ta - 1) * s + (K - 1) * d + off + 1 - short, 1)
    aaux = (a_tf >= W.TF_DLEAKY) if aaux is None else aaux
    baux = (b_tf >= W.TF_DLEAKY) if baux is None else baux
    add("wgrad", name, dict(B=B, M=M, C=Cn, Ta=Ta, Tb=Tb, P=P, K=K, s=s, d=d, off=off, a_tf=a_tf, b_tf=b_tf, aaux=int(aaux), baux=int(baux), alpha=alpha,
                            prior=prior), want)


# -- thin_wgrad, C = 1, stride 1 (the pairs kernel)
for M_, K_ in ((16, 15), (16, 16), (17, 15), (32, 5)):
    wg("pairs-M%d-K%d" % (M_, K_), M_, 1, 300, ["pairs"] + ["pairs M*K 256"] * (M_ * K_ == 256), K=K_)
# (64, 4) at P = 1, Ta >= 256: TUP = 257, 64 x 257 floats are past the 60 KiB the launcher allows itself: the row kernel
wg("pairs-M64-K4-lds", 64, 1, 300, ("row", "row by lds fall-through", "row <PLAIN,0>"), K=4)
wg("pairs-M64-K4-Ta100", 64, 1, 100, ("pairs", "pairs M*K 256", "pairs tq clipped to Ta"), K=4)
wg("MK257", 257, 1, 300, ("row", "row by M*K 257"), K=1)
for Ta_ in (7, 255, 1024, 1025, 2100):
    wg("pairs-Ta%d" % Ta_, 16, 1, Ta_, ["pairs"] + ["pairs tq clipped to Ta"] * (Ta_ < 256) + ["pairs chunks>1"] * (Ta_ > 1024) + ["pairs last tile short"] * (Ta_ in (1025, 2100)),
       K=15, d=(1, 2)[Ta_ % 2], off=(-7, 0, 2)[Ta_ % 3], short=(0, 2)[Ta_ % 2])
for P_, Ta_ in ((3, 1400), (37, 113), (256, 16), (257, 16)):
    wg("pairs-P%d" % P_, 32, 1, Ta_, ("row", "row by P 257") if P_ == 257 else ["pairs", "pairs period"] + ["pairs P 256"] * (P_ == 256), P=P_, K=5,
       d=(1, 2)[P_ % 2], off=(-7, 0, 2)[P_ % 3], short=(0, 2)[P_ % 2])
wg("pairs-P3-short-row", 32, 1, 50, ("pairs", "pairs period", "pairs tq clipped to Ta"), P=3, K=5, off=2, short=2)
# -- thin_wgrad, the row kernel
for P_ in (1, 2):
    wg("first-layer-s3-P%d" % P_, 32, 1, 400 // P_, ("row", "row C=1 strided", "row <PLAIN,5>"), P=P_, K=5, s=3)
for Cn_ in (16, 40, 1024):
    for K_ in (3, 5, 7, 1, 4, 16):
        if Cn_ == 1024 and K_ in (1, 4):
            continue
        wg("M1-C%d-K%d" % (Cn_, K_), 1, Cn_, 30 if Cn_ == 1024 else 130, ("row", "row <PLAIN,%d>" % (K_ if K_ in (3, 5, 7) else 0), "row all short"), K=K_, B=(4, 3)[K_ % 2])
# (2048 weight rows: the batch is split in two, not in four -- two batch elements per workgroup)
wg("M1-C2048-K3-B4", 1, 2048, 30, ("row", "row batch split", "row bper>1"), K=3, B=4)
wg("K17-einval", 1, 16, 100, ("einval",), K=17)
for U_ in (2, 511, 512, 513, 2100, 3073, 4100):
    w_ = ["row", "row all short" if U_ < 512 else "row last block short, others long" if U_ == 4100 else "row all long"] + ["row usplit>1"] * (U_ > 2048)
    wg("M1-C16-U%d" % U_, 1, 16, U_, w_, K=3, B=(1, 3, 4)[U_ % 3])
wg("M1-C16-U4100-P2", 1, 16, 2050, ("row", "row last block short, others long", "row period"), P=2, K=7, B=1)
for a_, b_ in ((W.TF_LEAKY, W.TF_NONE), (W.TF_NONE, W.TF_LEAKY), (W.TF_DLEAKY, W.TF_NONE), (W.TF_NONE, W.TF_DRELU), (W.TF_DTANH, W.TF_LEAKY), (W.TF_NONE, W.TF_DLOGCLAMP)):
    wg("tf-%s-%s" % (TF_NAME[a_], TF_NAME[b_]), 1, 40, 700, ("row", "row <TF,0>", "row tf %s,%s" % (TF_NAME[a_], TF_NAME[b_])), K=5, a_tf=a_, b_tf=b_, B=3)
wg("tf-DLEAKY-C1-short", 32, 1, 100, ("row", "row <TF,0>", "row all short"), K=5, a_tf=W.TF_DLEAKY, P=3, s=3)
wg("tf-DLEAKY-null-aux-einval", 1, 16, 100, ("einval",), a_tf=W.TF_DLEAKY, aaux=0)
wg("tf-b-DRELU-null-aux-einval", 1, 16, 100, ("einval",), b_tf=W.TF_DRELU, baux=0)
for al_ in (1.0, 0.5):
    for pr_ in (0, 1):
        wg("alpha%g-prior%d" % (al_, pr_), 1, 16, 600, ["row"] + (["row alpha 0.5 onto a prior" if pr_ else "row alpha 0.5 onto zeros"] if al_ != 1.0 else []), K=3, alpha=al_, prior=pr_)
wg("pairs-alpha0.5-prior", 16, 1, 300, ("pairs",), K=15, alpha=0.5)


def t1(entry, name, B, Cn, M, want, bias=1):
    add(entry, name, dict(B=B, C=Cn, M=M, bias=bias), want)


# (no one-element output: its max|ref| is that element alone, so where the prior dw and the product nearly cancel the max-norm
# distance measures the cancellation, not the kernel; the element-wise bound, which scales with S, is what holds such elements)
T1_SHAPES = [(1, 1, 16), (3, 63, 1), (32, 64, 15), (3, 65, 5), (1, 256, 192), (3, 300, 1000), (32, 300, 192), (3, 64, 1000)]
for B_, Cn_, M_ in T1_SHAPES:
    w_ = ["C < 64"] * (Cn_ < 64) + ["M % 4"] * (M_ % 4 != 0) + ["B 32"] * (B_ == 32)
    t1("t1_fwd", "B%d-C%d-M%d" % (B_, Cn_, M_), B_, Cn_, M_, w_ + ["no bias"] * (M_ % 2), bias=1 - M_ % 2)
    t1("t1_dgrad", "B%d-C%d-M%d" % (B_, Cn_, M_), B_, Cn_, M_, w_ + ["msplit by floor" if M_ < 16 else "msplit by M/16"])
    t1("t1_wgrad", "B%d-C%d-M%d" % (B_, Cn_, M_), B_, Cn_, M_, w_)
# (the 512 / nct side of the msplit rule needs M / 16 > 512 / cdiv(C, 256): ten column tiles)
t1("t1_dgrad", "B1-C2305-M1003", 1, 2305, 1003, ("msplit by 512/nct", "nct>1", "last m block short"))
t1("t1_fwd", "B33-einval", 33, 64, 16, ("einval",))
t1("t1_dgrad", "B33-einval", 33, 64, 16, ("einval",))
t1("t1_wgrad", "B33", 33, 64, 16, ())  # (the weight gradient loops over any B)

CASES = {"%s-%s" % (c.entry, c.name): c for c in TABLE}
IDS = list(CASES)

# what the table as a whole must reach (the list of the issue this file answers)
NEED = {
    "m1": ("lds", "reg", "R>1", "R=1", "TU does not divide 256", "a chunk is no multiple of R", "flat", "staged", "staged R>1", "cch rounded up past the LDS sizing",
           "chunks>1", "lds split with bias", "lds split no bias", "lds no split", "K>16", "halo 256", "tiles>1", "period", "pad 0", "in_leaky", "tanh",
           "reg stride 2", "reg stride 3", "reg split with bias", "reg split no bias", "reg no split", "reg K 16", "einval"),
    "c1": ("R>1", "R=1", "TU does not divide 256", "chunks>1", "chunk halved", "chunk below its floor", "last chunk short", "M > 64", "chunk is no multiple of R",
           "flip K even", "flip K odd", "oaux", "oaux with act", "act leaky", "no bias", "stride 3", "dil 2", "period", "api fwd", "api masked", "api flip", "einval"),
    "c1_dgrad": ("stride 1", "stride 2", "stride 3", "dil 1", "dil 2", "period", "rows past the last tap", "rows end at the last tap", "r % s", "tiles>1", "einval"),
    "wgrad": ("pairs", "pairs TUP padded", "pairs TUP as is", "pairs period", "pairs tq clipped to Ta", "pairs qper rounded past Ta", "pairs tiles>1 per chunk",
              "pairs chunks>1", "pairs last tile short", "pairs M*K 256", "pairs P 256", "pairs dil 2", "pairs off -7", "pairs off 0", "pairs off 2", "pairs Tb short",
              "row", "row <PLAIN,3>", "row <PLAIN,5>", "row <PLAIN,7>", "row <PLAIN,0>", "row <TF,0>", "row tf LEAKY,NONE", "row tf NONE,LEAKY", "row tf DLEAKY,NONE",
              "row tf NONE,DRELU", "row tf DTANH,LEAKY", "row tf NONE,DLOGCLAMP", "row all long", "row all short", "row mixed", "row last block short, others long",
              "row batch split", "row bper>1", "row usplit>1", "row by lds fall-through", "row by M*K 257", "row by P 257", "row C=1 strided",
              "row alpha 0.5 onto a prior", "row alpha 0.5 onto zeros", "row period", "einval"),
    "t1_fwd": ("C < 64", "C % 64", "C = 64 n", "M % 4", "B 32", "no bias", "einval"),
    "t1_dgrad": ("C < 64", "C % 64", "C = 64 n", "M % 4", "B 32", "msplit by floor", "msplit by M/16", "msplit by 512/nct", "nct>1", "last m block short", "msplit>1", "einval"),
    "t1_wgrad": ("C < 64", "C % 64", "C = 64 n", "M % 4", "B 32"),
}


def test_case_table_reaches_every_branch():
    """Host only, no library.  Every case is on the branches it was written for by the restated rules; the table reaches every
    branch of NEED; no two cases of an entry point are identical; the table keeps to the sizes the suite can afford."""
    seen = collections.Counter()
    for c in TABLE:
        tags = TAGS[c.entry](c.p)
        missing = [w for w in c.want if w not in tags]
        assert not missing, "%s %s: written for %s, the rules give %s" % (c.entry, c.name, missing, tags)
        seen.update("%s %s" % (c.entry, tg) for tg in tags)
        if c.entry in ("m1", "c1"):
            assert c.p["Tout"] * c.p["P"] <= 4200
        if c.entry == "wgrad":
            assert c.p["Ta"] * c.p["P"] <= 4200
        assert c.p["B"] <= 4 or c.p["B"] in (32, 33), c.name
    missing = [(e, b) for e in NEED for b in NEED[e] if not seen["%s %s" % (e, b)]]
    assert not missing, missing
    keys = [(c.entry, tuple(sorted(c.p.items()))) for c in TABLE]
    dup = [k for k, n in collections.Counter(keys).items() if n > 1]
    assert not dup, dup
    # the figures the table's comments state
    r = m1_rule(CASES["m1-chunks-tanh"].p)
    assert r["raw"] == 38 and r["chunks"] == [[40, 40, 20]] and r["splits"] == 1
    r = m1_rule(CASES["m1-U30-C1024-bias"].p)
    assert (r["R"], r["splits"], r["cperl"]) == (8, 16, 64)
    assert m1_rule(CASES["m1-U2-C1024-bias"].p)["R"] == 128
    r = m1_rule(CASES["m1-U100-C1030"].p)
    assert (r["R"], r["splits"], r["cperl"], len(r["chunks"])) == (2, 64, 17, 61) and r["chunks"][-1] == [10]
    assert m1_rule(CASES["m1-K17-dil16-halo256"].p)["W"] == 512
    assert c1_rule(CASES["c1-M17-U257"].p)["mch"] == 5 and c1_rule(CASES["c1-M1024-U30"].p)["mch"] == 32
    r = wgrad_rule(CASES["wgrad-pairs-M64-K4-lds"].p)
    assert r["kernel"] == "row" and r["fell"] == "lds"
    r = wgrad_rule(CASES["wgrad-pairs-M64-K4-Ta100"].p)
    assert r["kernel"] == "pairs" and r["TUP"] == 100
    assert wgrad_rule(CASES["wgrad-pairs-P256"].p)["TUP"] == 257
    assert wgrad_rule(CASES["wgrad-M1-C16-U4100"].p)["blocks"] == [1280, 1280, 1280, 260]
    for c in TABLE:  # every LDS request stays inside the 64 KiB a kernel gets without asking for more
        if c.entry == "m1" and m1_rule(c.p) and m1_rule(c.p)["kernel"] == "lds":
            assert 4 * m1_rule(c.p)["lds_floats"] <= 64 * 1024 and m1_rule(c.p)["W"] <= 512, c.name
    # deterministic mode (test_deterministic_mode_repeats): the split m1 case runs unsplit, the pairs case on the row kernel
    assert m1_rule(CASES[DET_CASES[0]].p)["splits"] > 1 and m1_rule(CASES[DET_CASES[0]].p, det=True)["splits"] == 1
    assert wgrad_rule(CASES[DET_CASES[1]].p)["kernel"] == "pairs"
    r = wgrad_rule(CASES[DET_CASES[1]].p, det=True)
    assert r["kernel"] == "row" and r["splits"] == 1 and len(r["blocks"]) == 1


DET_CASES = ("m1-U30-C1024-bias", "wgrad-pairs-Ta2100")


# ---------------------------------------------------------------------------------------------------------------------
# the exact pass is exact: from the table alone
# ---------------------------------------------------------------------------------------------------------------------
def tf_quantum(tf):
    """the quantum of tf(v) for an integer v, slope 0.5, aux in {-1, -0.5, 0, 0.5, 1} ({-1, 0} for DLOGCLAMP)"""
    return {W.TF_NONE: 1.0, W.TF_LEAKY: 0.5, W.TF_DLEAKY: 0.5, W.TF_DRELU: 1.0, W.TF_DTANH: 0.25, W.TF_DLOGCLAMP: 1.0}[tf]


def exact_budget(c):
    """(quantum of every partial sum, a bound on its magnitude) of case c in the exact pass."""
    p = c.p
    if c.entry == "m1":
        return (0.5 if p["leaky"] else 1.0), 64.0 * p["C"] * p["K"] + 4
    if c.entry == "c1":
        return 1.0, 64.0 * p["K"] + 4
    if c.entry == "c1_dgrad":
        return 1.0, 64.0 * p["M"] * p["K"]
    if c.entry == "wgrad":  # (the kernels scale their partial sums by alpha before the atomic add onto dw)
        q = tf_quantum(p["a_tf"]) * tf_quantum(p["b_tf"])
        return q * min(p["alpha"], 1.0), 64.0 * p["B"] * p["Ta"] * p["P"] + 4
    return 1.0, 64.0 * {"t1_fwd": p["C"], "t1_dgrad": p["M"], "t1_wgrad": p["B"]}[c.entry] + 4


def test_exact_pass_is_exact():
    """Host only.  Every partial sum of the exact pass is a multiple of its quantum (a power of two) and below 2^24 quanta, so
    it is a float32 whatever the order of the additions; the activation, the derivative factor and alpha (each 1, 0.5 or 0.75
    times a number of that kind) then give a float32 again: 3 more bits at most, on sums below 2^21 quanta."""
    for c in TABLE:
        q, bound = exact_budget(c)
        assert math.log2(q) == int(math.log2(q)), c.name
        assert bound < (1 << 24) * q, "%s %s: sums up to %g in steps of %g" % (c.entry, c.name, bound, q)
        if c.entry in ("m1", "c1"):
            assert bound < (1 << 21) * q, c.name


# ---------------------------------------------------------------------------------------------------------------------
# refusals on the host: a null required pointer is tested before anything is launched
# ---------------------------------------------------------------------------------------------------------------------
def test_null_required_pointers_are_refused():
    """Every entry point, every required pointer null in turn (the others stand-ins that are never read): VCV_EINVAL.  The
    optional ones (bias, oaux, the aux tensors under a transform that needs none) are not in the list."""
    from vcvits_amd._lib import lib
    L = lib()
    X = ctypes.c_void_p(0x10000)
    calls = {
        "vcv_conv_m1_fwd": (3, lambda a: L.vcv_conv_m1_fwd(a[0], a[1], X, a[2], 1, 16, 10, 10, 1, 3, 1, 1, 1, 0, 0, 0.1, None)),
        "vcv_conv_c1_fwd": (3, lambda a: L.vcv_conv_c1_fwd(a[0], a[1], X, a[2], 1, 16, 10, 10, 1, 3, 1, 1, 1, 0, 0.1, None)),
        "vcv_conv_c1_fwd_masked": (3, lambda a: L.vcv_conv_c1_fwd_masked(a[0], a[1], X, a[2], X, 1, 16, 10, 10, 1, 3, 1, 1, 1, 0, 0.1, None)),
        "vcv_conv_c1_fwd_flip": (3, lambda a: L.vcv_conv_c1_fwd_flip(a[0], a[1], X, a[2], X, 1, 16, 10, 10, 1, 3, 1, 1, 1, 0, 0.1, 1, None)),
        "vcv_conv_c1_dgrad": (3, lambda a: L.vcv_conv_c1_dgrad(a[0], a[1], a[2], 1, 16, 10, 10, 1, 3, 1, 1, 1, None)),
        "vcv_thin_wgrad": (3, lambda a: L.vcv_thin_wgrad(a[0], a[1], X, X, a[2], 1, 1, 16, 10, 10, 1, 3, 1, 1, -1, 0, 0, 0.1, 1.0, None)),
        "vcv_linear_t1_fwd": (3, lambda a: L.vcv_linear_t1_fwd(a[0], a[1], X, a[2], 1, 16, 16, None)),
        "vcv_linear_t1_dgrad": (3, lambda a: L.vcv_linear_t1_dgrad(a[0], a[1], a[2], 1, 16, 16, None)),
        "vcv_linear_t1_wgrad": (3, lambda a: L.vcv_linear_t1_wgrad(a[0], a[1], a[2], 1, 16, 16, None)),
    }
    for name, (n, call) in calls.items():
        for i in range(n):
            args = [X] * n
            args[i] = None
            assert call(args) == EINVAL, "%s: null pointer %d was not refused" % (name, i)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and float64 references: made once per (case, kind) and shared
# ---------------------------------------------------------------------------------------------------------------------
def settings(c, kind):
    """(slope, out_act) as the pass runs the case"""
    p = c.p
    if kind == "exact":
        return 0.5, {TANH: RELU}.get(p.get("act", NONE), p.get("act", NONE))
    slope = 0.5 if c.entry == "wgrad" and W.TF_DLOGCLAMP in (p["a_tf"], p["b_tf"]) else 0.1
    return slope, p.get("act", NONE)


def shapes(c):
    """name -> shape of every tensor of the case; "out" is the one the kernel writes"""
    p = c.p
    if c.entry == "m1":
        return dict(x=(p["B"], p["C"], p["Tin"], p["P"]), w=(1, p["C"], p["K"]), bias=(1,), out=(p["B"], 1, p["Tout"], p["P"]))
    if c.entry == "c1":
        o = (p["B"], p["M"], p["Tout"], p["P"])
        return dict(x=(p["B"], 1, p["Tin"], p["P"]), w=(p["M"], 1, p["K"]), bias=(p["M"],), oaux=o, out=o)
    if c.entry == "c1_dgrad":
        return dict(dy=(p["B"], p["M"], p["Tout"], p["P"]), w=(p["M"], 1, p["K"]), out=(p["B"], 1, p["Tin"], p["P"]))
    if c.entry == "wgrad":
        a, b = (p["B"], p["M"], p["Ta"], p["P"]), (p["B"], p["C"], p["Tb"], p["P"])
        return dict(a=a, b=b, aaux=a, baux=b, out=(p["M"], p["C"], p["K"]))
    B, Cn, M = p["B"], p["C"], p["M"]
    return {"t1_fwd": dict(x=(B, Cn), w=(M, Cn), bias=(M,), out=(B, M)), "t1_dgrad": dict(dy=(B, M), w=(M, Cn), out=(B, Cn)),
            "t1_wgrad": dict(dy=(B, M), x=(B, Cn), out=(M, Cn))}[c.entry]


def overwrites(c):
    """the kernel overwrites its output (pre-filled with NaN); else it adds onto the prior"""
    return c.entry not in ("wgrad", "t1_wgrad")


@functools.lru_cache(maxsize=None)
def inputs(key, kind):
    """float32 CPU tensors of case `key`.  normal: seeded Gaussians, w scaled by (C K)^-1/2; exact: small integers and halves."""
    c = CASES[key]
    p = c.p
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t = {}
    for name, sh in shapes(c).items():
        if name == "out":
            continue
        aux = name in ("oaux", "aaux", "baux")
        tf = p.get({"aaux": "a_tf", "baux": "b_tf"}.get(name, ""), W.TF_NONE)
        if kind == "exact":
            if aux:
                v = rng.choice([-1.0, 0.0], sh) if tf == W.TF_DLOGCLAMP else rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], sh)
            elif name == "bias":
                v = rng.integers(-4, 5, sh)
            else:
                v = rng.integers(-8, 9, sh)
        else:
            v = rng.standard_normal(sh)
            if name == "w":
                fan = p.get("C", 1) * p.get("K", 1)  # (one input channel: C = 1; one frame: K = 1)
                v = v * float(fan) ** -0.5
            if aux and tf == W.TF_DTANH:
                v = np.tanh(v)
            if aux and tf == W.TF_DLOGCLAMP:
                # aux = a logclamp output, kept clear of the threshold log(clamp) on both sides, so that the comparison does not
                # hang on the last bit of logf: clamped elements a quarter below it, the others 0.01 or more above
                v = np.log(np.maximum(np.abs(v) * 1.5, 0.5))
                v = np.where(v <= np.log(0.5) + 0.01, np.log(0.5) - 0.25, v)
        t[name] = f(v)
    sh = shapes(c)["out"]
    if overwrites(c) or not p.get("prior", 1):
        t["prior"] = torch.zeros(sh)
    else:
        t["prior"] = f(rng.integers(-4, 5, sh) if kind == "exact" else rng.standard_normal(sh))
    return t


def terms(c):
    p = c.p
    return {"m1": lambda: p["C"] * p["K"], "c1": lambda: p["K"], "c1_dgrad": lambda: p["M"] * p["K"], "wgrad": lambda: p["B"] * p["Ta"] * p["P"],
            "t1_fwd": lambda: p["C"], "t1_dgrad": lambda: p["M"], "t1_wgrad": lambda: p["B"]}[c.entry]()


def transcendental(c):
    return c.p.get("act") == TANH or (c.entry == "wgrad" and bool({c.p["a_tf"], c.p["b_tf"]} & {W.TF_DTANH, W.TF_DLOGCLAMP}))


def compute(c, kind, t, dtype):
    """(expected output in `dtype`, S float64) of case c from the CPU tensors t"""
    p = c.p
    slope, act = settings(c, kind)
    if c.entry == "m1":
        g = C.geom(p["B"], 1, p["C"], 1, p["Tin"], p["Tout"], p["P"], p["K"], p["s"], p["dil"], -p["pad"])
        return C.conv(g, t["x"], t["w"], t["prior"].view(p["B"], 1, p["Tout"], p["P"]), bias=t["bias"] if p["bias"] else None,
                      in_tf=C.TF_LEAKY if p["leaky"] else C.TF_NONE, out_act=act, slope=slope, dtype=dtype)
    if c.entry == "c1":
        g = C.geom(p["B"], 1, 1, p["M"], p["Tin"], p["Tout"], p["P"], p["K"], p["s"], p["dil"], -p["pad"])
        return C.conv(g, t["x"], t["w"], t["prior"], flip=p["flip"], bias=t["bias"] if p["bias"] else None, out_act=act,
                      out_tf=C.TF_DLEAKY if p["oaux"] else C.TF_NONE, oaux=t["oaux"] if p["oaux"] else None, slope=slope, dtype=dtype)
    if c.entry == "c1_dgrad":
        if p["s"] == 1:  # the a_mode-1 form of VcvConvArgs
            g = C.geom(p["B"], 1, p["M"], 1, p["Tout"], p["Tin"], p["P"], p["K"], 1, -p["dil"], p["pad"], Q=p["Tin"], a_mode=1)
            return C.conv(g, t["dy"], t["w"], t["prior"], dtype=dtype)
        return C.dgrad(t["dy"], t["w"], p["Tin"], p["s"], p["dil"], p["pad"], dtype=dtype)
    if c.entry == "wgrad":
        kw = dict(a_tf=p["a_tf"], b_tf=p["b_tf"], slope=slope, aaux=t["aaux"] if p["aaux"] else None, baux=t["baux"] if p["baux"] else None)
        al = C.f32(p["alpha"])
        dw = W.wgrad(t["a"], t["b"], p["K"], p["s"], p["d"], p["off"], dtype=dtype, **kw)
        S = W.wgrad_mag(t["a"], t["b"], p["K"], p["s"], p["d"], p["off"], **kw)
        return t["prior"].to(dtype) + al * dw, abs(al) * S + t["prior"].double().abs()
    d = lambda k: t[k].to(dtype)
    a = lambda k: t[k].double().abs()
    if c.entry == "t1_fwd":
        y, S = d("x") @ d("w").T, a("x") @ a("w").T
        return (y + d("bias"), S + a("bias")) if p["bias"] else (y, S)
    if c.entry == "t1_dgrad":
        return d("dy") @ d("w"), a("dy") @ a("w")
    return d("prior") + d("dy").T @ d("x"), a("prior") + a("dy").T @ a("x")


@functools.lru_cache(maxsize=None)
def reference(key, kind):
    """(float64 expectation, S, d32)"""
    c = CASES[key]
    t = inputs(key, kind)
    y, S = compute(c, kind, t, torch.float64)
    d32 = 0.0
    if kind == "normal" and transcendental(c):
        d32 = (compute(c, kind, t, torch.float32)[0].double() - y).abs().max().item()
    return y, S, d32


@functools.lru_cache(maxsize=2)
def on_gpu(key, kind, gpu):
    return {k: v.to(gpu) for k, v in inputs(key, kind).items()}


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


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def abi(gpu, c, kind):
    """One call through the C ABI -> (status, the output view, what it held before the call)."""
    from vcvits_amd._lib import lib, stream
    L, p = lib(), c.p
    key = "%s-%s" % (c.entry, c.name)
    t = on_gpu(key, kind, gpu)
    slope, act = settings(c, kind)
    out = Guarded(shapes(c)["out"], gpu, float("nan") if overwrites(c) else t["prior"])
    before = out.t.clone()
    o, st_ = ptr(out.t), stream()
    if c.entry == "m1":
        st = L.vcv_conv_m1_fwd(ptr(t["x"]), ptr(t["w"]), ptr(t["bias"]) if p["bias"] else None, o, p["B"], p["C"], p["Tin"], p["Tout"], p["P"], p["K"],
                               p["s"], p["dil"], p["pad"], p["leaky"], act, slope, st_)
    elif c.entry == "c1":
        head = (ptr(t["x"]), ptr(t["w"]), ptr(t["bias"]) if p["bias"] else None, o)
        tail = (p["B"], p["M"], p["Tin"], p["Tout"], p["P"], p["K"], p["s"], p["dil"], p["pad"], act, slope)
        oa = ptr(t["oaux"]) if p["oaux"] else None
        if p["api"] == "fwd":
            assert not p["oaux"] and not p["flip"]
            st = L.vcv_conv_c1_fwd(*head, *tail, st_)
        elif p["api"] == "masked":
            assert not p["flip"]
            st = L.vcv_conv_c1_fwd_masked(*head, oa, *tail, st_)
        else:
            st = L.vcv_conv_c1_fwd_flip(*head, oa, *tail, p["flip"], st_)
    elif c.entry == "c1_dgrad":
        st = L.vcv_conv_c1_dgrad(ptr(t["dy"]), ptr(t["w"]), o, p["B"], p["M"], p["Tin"], p["Tout"], p["P"], p["K"], p["s"], p["dil"], p["pad"], st_)
    elif c.entry == "wgrad":
        st = L.vcv_thin_wgrad(ptr(t["a"]), ptr(t["b"]), ptr(t["aaux"]) if p["aaux"] else None, ptr(t["baux"]) if p["baux"] else None, o, p["B"], p["M"],
                              p["C"], p["Ta"], p["Tb"], p["P"], p["K"], p["s"], p["d"], p["off"], p["a_tf"], p["b_tf"], slope, p["alpha"], st_)
    elif c.entry == "t1_fwd":
        st = L.vcv_linear_t1_fwd(ptr(t["x"]), ptr(t["w"]), ptr(t["bias"]) if p["bias"] else None, o, p["B"], p["C"], p["M"], st_)
    elif c.entry == "t1_dgrad":
        st = L.vcv_linear_t1_dgrad(ptr(t["dy"]), ptr(t["w"]), o, p["B"], p["C"], p["M"], st_)
    else:
        st = L.vcv_linear_t1_wgrad(ptr(t["dy"]), ptr(t["x"]), o, p["B"], p["C"], p["M"], st_)
    torch.cuda.synchronize()
    assert out.intact(), "%s: a write outside the output" % key
    return st, out.t, before


def bits(t):
    return t.contiguous().view(torch.int32)


def combines_with_atomics(c, det=False):
    """by the restated rules: the launch's workgroups meet in fp32 atomics, so two launches may differ in the last bits"""
    if c.entry == "m1":
        return m1_rule(c.p, det)["splits"] > 1
    return c.entry in ("wgrad", "t1_dgrad")


_parity = {}
HEADER = ("# tests/test_conv_thin_abi_gpu.py: distance of the thin conv kernels (csrc/conv_thin.hip) at the C ABI from their float64 CPU\n"
          "# references (tests/conv_f64.py, tests/wgrad_f64.py, a float64 matmul), normal pass.  Per case: the branch of the launcher by the\n"
          "# rules restated in the test file | max|got - ref| / max|ref| (bounds: 2e-5 for y and dx, 3e-5 for dw) / the worst ratio of\n"
          "# |got - ref| to its element-wise bound gamma_n * S + a (must be <= 1) | d32 = max|float32 CPU run - float64 run| of the\n"
          "# reference where a transcendental is evaluated (a = 4 * d32 there, 0 elsewhere).  The exact pass (integer operands) is\n"
          "# bit-equal to float64 or fails: it has no distances to report.  `EINVAL` marks a case the launcher must refuse (asserted).\n")


def record(section, line):
    """Keep the measured distances in profiles/conv_thin_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "conv_thin_parity.txt"), "w") as f:
        f.write(HEADER)
        for name in _parity:
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def check(c, kind, got, fails, what=""):
    """got against the float64 reference: bit for bit (exact), or within both bounds (normal).  -> (max-norm distance, ratio)"""
    key = "%s-%s" % (c.entry, c.name)
    y64, S, d32 = reference(key, kind)
    got = got.detach().cpu().reshape(y64.shape)
    tag = "%s %s%s" % (key, kind, what)
    if bool(torch.isnan(got).any()):
        fails.append("%s: NaN in the output (an element the kernel did not write?)" % tag)
        return None
    if c.entry == "c1_dgrad":  # rows of x no tap reaches are written as exact zeros
        last = (c.p["Tout"] - 1) * c.p["s"] + (c.p["K"] - 1) * c.p["dil"] - c.p["pad"]
        if bool(got[:, :, last + 1:].ne(0).any()) or bool(S[:, :, last + 1:].ne(0).any()):
            fails.append("%s: a row past the last tap is not exactly 0" % tag)
    if kind == "exact":
        assert bool((y64.float().double() == y64).all()), tag  # (the reference itself is a float32 number everywhere)
        if not torch.equal(got, y64.float()):
            bad = (got != y64.float()).nonzero()
            fails.append("%s: not the float64 reference's bits at %d elements, first %s (got %r, want %r)" % (
                tag, len(bad), bad[0].tolist(), got[tuple(bad[0])].item(), y64[tuple(bad[0])].item()))
        return None
    e = C.dist(got, y64)
    bound = TOL_DW if c.entry in ("wgrad", "t1_wgrad") else TOL
    el = C.gamma(terms(c) + 6) * S + 4.0 * d32
    diff = (got.double() - y64).abs()
    ratio = torch.where(diff > 0, diff / el.clamp(min=1e-300), torch.zeros_like(diff)).max().item()
    if e > bound:
        fails.append("%s: max-norm distance %.3e (bound %.1e)" % (tag, e, bound))
    if ratio > 1.0:
        fails.append("%s: element-wise, |got - ref| is %.3f x its bound (flat element %d)" % (tag, ratio, int((diff / el.clamp(min=1e-300)).flatten().argmax())))
    return e, ratio


def test_checker_notices_small_local_errors():
    """Host only, no library: the float64 reference cast to float32 passes check(); one ulp in the exact pass, 1.5 x its own
    bound on the element with the smallest S in the normal pass (far under the max-norm bound), and a 1e-30 on a row of dx no tap
    reaches do not."""
    def run(key, kind, poke=None):
        got = reference(key, kind)[0].float()
        if poke:
            poke(got)
        fails = []
        check(CASES[key], kind, got, fails)
        return fails

    for key in ("m1-U100-C1030", "c1-head-dgrad-dleaky-P3", "c1_dgrad-M33-s3-dil2-P1-K15-extra4", "wgrad-tf-DTANH-LEAKY", "t1_dgrad-B3-C300-M1000"):
        for kind in KINDS:
            assert run(key, kind) == [], (key, kind)
    f = run("m1-U100-C1030", "exact", lambda t: t.__setitem__((1, 0, 99, 0), torch.nextafter(t[1, 0, 99, 0], torch.tensor(float("inf")))))
    assert len(f) == 1 and "bits at 1 elements" in f[0], f
    key = "c1-M32-U100"
    y64, S, _ = reference(key, "normal")
    i = tuple(np.unravel_index(int(S.argmin()), S.shape))
    delta = 1.5 * C.gamma(terms(CASES[key]) + 6) * S[i].item()
    assert delta < 0.5 * TOL * y64.abs().max().item()
    f = run(key, "normal", lambda t: t.__setitem__(i, float(y64[i]) + delta))
    assert len(f) == 1 and "element-wise" in f[0], f
    f = run("c1_dgrad-M33-s3-dil2-P1-K15-extra4", "normal", lambda t: t.__setitem__((0, 0, -1, 0), 1e-30))
    assert any("past the last tap" in m for m in f), f


# ---------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------
def sweep(gpu, key, kind, det=False):
    """One case: two launches.  -> (fails, profile cell)"""
    c = CASES[key]
    tags = TAGS[c.entry](c.p, det) if det else TAGS[c.entry](c.p)
    fails = []
    if tags == ["einval"]:
        st, out, before = abi(gpu, c, kind)
        assert st == EINVAL, "%s: the launcher must refuse this case, it returned %d" % (key, st)
        assert torch.equal(bits(out), bits(before)), "%s: a refused call wrote to its output" % key
        return fails, "EINVAL"
    st1, y1, _ = abi(gpu, c, kind)
    st2, y2, _ = abi(gpu, c, kind)
    assert st1 == 0 and st2 == 0, "%s: status %d / %d" % (key, st1, st2)
    cell = check(c, kind, y1, fails)
    if combines_with_atomics(c, det):
        check(c, kind, y2, fails, " (second launch)")
    elif not torch.equal(bits(y1), bits(y2)):
        fails.append("%s %s: two identical launches differ" % (key, kind))
    d32 = reference(key, kind)[2]
    return fails, ("%.1e/%.2f" % cell + (" | d32=%.1e" % d32 if d32 else "")) if cell else None


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", IDS)
def test_parity(gpu, key, kind):
    c = CASES[key]
    fails, cell = sweep(gpu, key, kind)
    if kind == "normal" or cell == "EINVAL":
        record(c.entry, "%-44s %-70s | %s" % (c.name, ", ".join(TAGS[c.entry](c.p)), cell))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("key", DET_CASES)
def test_deterministic_mode_repeats(gpu, key, kind):
    """vcv_set_deterministic(1): the split one-output-channel forward runs unsplit and the pairs weight gradient on the row kernel
    with one workgroup per weight row (asserted from the restated rules on the host); both must then repeat their bits, and keep
    to their bounds.  The flag comes back whatever happens."""
    from vcvits_amd._lib import lib
    c = CASES[key]
    assert combines_with_atomics(c) and (c.entry != "m1" or not combines_with_atomics(c, det=True))
    old = lib().vcv_get_deterministic()
    try:
        assert lib().vcv_set_deterministic(1) == 0
        st1, y1, _ = abi(gpu, c, kind)
        st2, y2, _ = abi(gpu, c, kind)
    finally:
        lib().vcv_set_deterministic(old)
    assert st1 == 0 and st2 == 0
    assert torch.equal(bits(y1), bits(y2)), "%s: deterministic mode does not repeat its bits" % key
    fails = []
    cell = check(c, kind, y1, fails)
    if kind == "normal":
        record("deterministic", "%-44s %-70s | %s" % (key, ", ".join(TAGS[c.entry](c.p, True)), "%.1e/%.2f" % cell if cell else None))
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# routing: ops.* arrives at these kernels and gives the bits of the ABI call (exact pass)
# ---------------------------------------------------------------------------------------------------------------------
def _moved(ops, before):
    return {k: ops.LAUNCH_COUNTS[k] - before.get(k, 0) for k in ops.LAUNCH_COUNTS if ops.LAUNCH_COUNTS[k] != before.get(k, 0)}


def _sq(p):
    return (lambda v: v[..., 0]) if p["P"] == 1 else (lambda v: v)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["m1-U30-C1024-bias", "m1-U100-C40-inleaky", "m1-K5-dil32-P2-halo256", "m1-K41", "m1-s2-K3-dil1-P2", "c1-M32-U100", "c1-M17-U257", "c1-s3-dil1-P2"])
def test_routing_forward(gpu, key):
    """ops.conv_forward: no launch of the GEMM families, the ABI call's bits."""
    from vcvits_amd import ops
    c = CASES[key]
    p, t = c.p, on_gpu(key, "exact", gpu)
    slope, act = settings(c, "exact")
    sq = _sq(p)
    before = dict(ops.LAUNCH_COUNTS)
    y = ops.conv_forward(sq(t["x"]), t["w"], t["bias"] if p["bias"] else None, stride=p["s"], pad=p["pad"], dil=p["dil"], out_act=act, slope=slope,
                         in_tf=C.TF_LEAKY if p.get("leaky") else C.TF_NONE)
    torch.cuda.synchronize()
    assert _moved(ops, before) == {}, "%s: ops.conv_forward launched %s" % (key, _moved(ops, before))
    st, want, _ = abi(gpu, c, "exact")
    assert st == 0 and torch.equal(bits(y.reshape(want.shape)), bits(want)), "%s: ops.conv_forward did not give the ABI call's bits" % key
    record("routing", "%-44s ops.conv_forward gives the ABI call's bits" % key)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["c1_dgrad-M16-s2-dil1-P3-K5-extra0", "c1_dgrad-M64-s1-dil2-P3-K16-extra0", "c1-head-dgrad", "c1-head-dgrad-dleaky-P3"])
def test_routing_dgrad(gpu, key):
    """ops.conv_dgrad: C == 1 arrives at vcv_conv_c1_dgrad; M == 1, stride 1 at vcv_conv_c1_fwd_flip with the taps reversed, with
    and without out_tf = TF_DLEAKY."""
    from vcvits_amd import ops
    c = CASES[key]
    p, t = c.p, on_gpu(key, "exact", gpu)
    slope, _ = settings(c, "exact")
    sq = _sq(p)
    before = dict(ops.LAUNCH_COUNTS)
    if c.entry == "c1_dgrad":
        xs = (p["B"], 1, p["Tin"]) + ((p["P"],) if p["P"] > 1 else ())
        dx = ops.conv_dgrad(sq(t["dy"]), t["w"], xs, stride=p["s"], pad=p["pad"], dil=p["dil"])
    else:  # the forward conv: [B, C = 1024, Tin', P] -> [B, 1, Tout', P] with weight [1, C, K]; this case's x is its dy
        K, dil = p["K"], p["dil"]
        xs = (p["B"], p["M"], p["Tout"]) + ((p["P"],) if p["P"] > 1 else ())
        kw = dict(out_tf=C.TF_DLEAKY, oaux=sq(t["oaux"]), slope=slope) if p["oaux"] else {}
        dx = ops.conv_dgrad(sq(t["x"]), t["w"].view(1, p["M"], K), xs, stride=1, pad=(K - 1) * dil - p["pad"], dil=dil, **kw)
    torch.cuda.synchronize()
    assert _moved(ops, before) == {}, "%s: ops.conv_dgrad launched %s" % (key, _moved(ops, before))
    st, want, _ = abi(gpu, c, "exact")
    assert st == 0 and torch.equal(bits(dx.reshape(want.shape)), bits(want)), "%s: ops.conv_dgrad did not give the ABI call's bits" % key
    record("routing", "%-44s ops.conv_dgrad gives the ABI call's bits" % key)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["wgrad-pairs-M16-K15", "wgrad-first-layer-s3-P2", "wgrad-M1-C1024-K3", "wgrad-tf-DLEAKY-NONE", "wgrad-alpha0.5-prior1"])
def test_routing_wgrad(gpu, key):
    from vcvits_amd import ops
    c = CASES[key]
    p, t = c.p, on_gpu(key, "exact", gpu)
    slope, _ = settings(c, "exact")
    sq = _sq(p)
    out = t["prior"].clone()
    before = dict(ops.LAUNCH_COUNTS)
    ops.conv_wgrad(sq(t["a"]), sq(t["b"]), (p["M"], p["C"], p["K"]), stride=p["s"], pad=-p["off"], dil=p["d"], out=out, a_tf=p["a_tf"],
                   aaux=sq(t["aaux"]) if p["aaux"] else None, b_tf=p["b_tf"], baux=sq(t["baux"]) if p["baux"] else None, alpha=p["alpha"], slope=slope)
    torch.cuda.synchronize()
    assert _moved(ops, before) == {}, "%s: ops.conv_wgrad launched %s" % (key, _moved(ops, before))
    st, want, _ = abi(gpu, c, "exact")
    assert st == 0 and torch.equal(bits(out), bits(want)), "%s: ops.conv_wgrad did not give the ABI call's bits" % key
    record("routing", "%-44s ops.conv_wgrad gives the ABI call's bits" % key)


@pytest.mark.gpu
def test_routing_linear_t1(gpu):
    """ops.conv1d on one frame with M >= 32 is the linear-t1 autograd function: forward, data gradient and weight gradient give
    the bits of the three ABI calls (the weight gradient onto zeros)."""
    from vcvits_amd import ops
    rng = np.random.default_rng(7)
    B, Cn, M = 3, 65, 192
    f = lambda *sh: torch.from_numpy(rng.integers(-8, 9, sh).astype(np.float32)).to(gpu)
    x, w, bias, dy = f(B, Cn, 1).requires_grad_(), f(M, Cn, 1).requires_grad_(), f(M), f(B, M, 1)
    y = ops.conv1d(x, w, bias)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    torch.cuda.synchronize()
    from vcvits_amd._lib import lib, stream
    L = lib()
    want = {k: Guarded(sh, gpu, init) for k, sh, init in (("y", (B, M), float("nan")), ("dx", (B, Cn), float("nan")), ("dw", (M, Cn), 0.0))}
    assert L.vcv_linear_t1_fwd(ptr(x), ptr(w), ptr(bias), ptr(want["y"].t), B, Cn, M, stream()) == 0
    assert L.vcv_linear_t1_dgrad(ptr(dy), ptr(w), ptr(want["dx"].t), B, Cn, M, stream()) == 0
    assert L.vcv_linear_t1_wgrad(ptr(dy), ptr(x), ptr(want["dw"].t), B, Cn, M, stream()) == 0
    torch.cuda.synchronize()
    for k, got in (("y", y), ("dx", dx), ("dw", dw)):
        assert want[k].intact() and torch.equal(bits(got.detach().reshape(want[k].t.shape)), bits(want[k].t)), k
    x64, w64 = x.detach().cpu().double()[..., 0], w.detach().cpu().double()[..., 0]
    assert torch.equal(y.detach().cpu()[..., 0], (x64 @ w64.T + bias.cpu().double()).float())
    assert torch.equal(dx.cpu()[..., 0], (dy.cpu().double()[..., 0] @ w64).float()) and torch.equal(dw.cpu()[..., 0], (dy.cpu().double()[..., 0].T @ x64).float())
    record("routing", "%-44s ops.conv1d on one frame gives the bits of vcv_linear_t1_fwd / _dgrad / _wgrad" % "t1-B3-C65-M192")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 4, 100, 1, 7, 1, 3, 1), (2, 16, 100, 1, 17, 2, 8, 1), (2, 16, 20, 3, 17, 3, 8, 1)],
                         ids=lambda s: "B%d-C%d-T%d-P%d-K%d-s%d-pad%d-dil%d" % s)
def test_routing_keeps_away_from_m1(gpu, shape):
    """A 4 -> 1 conv (fewer than 16 channels) and a strided one-output-channel conv with 17 taps (the launcher refuses it: asserted)
    do not arrive at vcv_conv_m1_fwd: ops.conv_forward sends them to the GEMM families, and they still match the reference."""
    from vcvits_amd import ops
    from vcvits_amd._lib import lib, stream
    B, Cn, T, P, K, s, pad, dil = shape
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    x, w, bias = f(rng.standard_normal((B, Cn, T, P))), f(rng.standard_normal((1, Cn, K)) * float(Cn * K) ** -0.5), f(rng.standard_normal((1,)))
    Tout = out_len(T, K, s, pad, dil)
    xg, wg_, bg = x.to(gpu), w.to(gpu), bias.to(gpu)
    if K > 16:
        y0 = Guarded((B, 1, Tout, P), gpu, float("nan"))
        assert lib().vcv_conv_m1_fwd(ptr(xg), ptr(wg_), ptr(bg), ptr(y0.t), B, Cn, T, Tout, P, K, s, dil, pad, 0, 0, 0.1, stream()) == EINVAL
        torch.cuda.synchronize()
        assert bool(torch.isnan(y0.t).all()) and y0.intact()
    before = dict(ops.LAUNCH_COUNTS)
    y = ops.conv_forward(xg[..., 0] if P == 1 else xg, wg_, bg, stride=s, pad=pad, dil=dil)
    torch.cuda.synchronize()
    moved = _moved(ops, before)
    assert sum(moved.values()) == 1 and set(moved) <= {"gemm", "dma", "pk", "x3", "bf16"}, moved
    g = C.geom(B, 1, Cn, 1, T, Tout, P, K, s, dil, -pad)
    ref, _ = C.conv(g, x, w, torch.zeros(B, 1, Tout, P), bias=bias)
    e = C.dist(y.reshape(ref.shape), ref)
    record("routing", "%-44s ops.conv_forward launches %s, not vcv_conv_m1_fwd: %.1e from float64" % ("B%d-C%d-T%d-P%d-K%d-s%d-pad%d-dil%d" % shape, list(moved)[0], e))
    assert e <= TOL

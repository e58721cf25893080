"""The streaming glue of csrc/vits_blocks.hip at the C ABI, at the edges of its launchers, against the float64 CPU restatements
of tests/vits_glue_f64.py (pinned to torch autograd in tests/test_vits_glue_f64_cpu.py): vcv_wn_gate_fwd / _bwd, vcv_row_sum,
vcv_wn_res_skip_fwd / _bwd, vcv_split_sample_fwd / _bwd, vcv_coupling, vcv_prior_sample, vcv_kl_fwd / _bwd, vcv_nearest_fwd /
_bwd, vcv_nearest_raw_fwd / _bwd, vcv_slice_fwd / _bwd, vcv_dropout and vcv_layernorm_c_fwd / _bwd_ws.

Every kernel is called through ctypes with hand-filled arguments on the null stream; tuning keys and the deterministic flag stay
at their defaults.  Every case names what it is there for; test_case_table_reaches_every_edge proves on the host, from the table
alone, that every tag of NEED is reached.  test_routing_* check that ops.* gives the bits of the ABI call.

Two passes over one table:
  exact    operands are small integers, masks from {0, 0.5, 1} with holes (not a prefix), logs / lp = 0 wherever an exp is
           taken, noise_scale and gout / den powers of two.  Every result and every partial sum is a multiple of a quantum and
           below 2^24 quanta (test_exact_pass_is_exact in tests/test_vits_glue_f64_cpu.py, from the table alone), so the result
           must be BIT-EQUAL to the float64 reference cast to float32, atomics included.  The gate and LayerNorm have none.
  normal   Gaussian inputs, logs ~ 0.3 N(0, 1), masks from {0, 1} with holes.  Kernels that are one rounded operation per
           element (res/skip, coupling, slice, nearest forward, split without eps, dropout) stay bit-equal.  The others:
           1. max|got - ref| / max|ref| <= 2e-5 (tests/test_switch_parity_gpu.py; LayerNorm: its LN_TOLS);
           2. element-wise |got - ref| <= gamma_n * S + a, gamma_n = n u / (1 - n u), u = 2^-24; n = the operations or terms
              behind the element + 6; S = the float64 sum of magnitudes behind it; a = 4 * d32 where a transcendental is
              evaluated, d32 = max|float32 CPU run - float64 run| of the same reference (the KL numerator: a = 4 * the sum of
              |t32_i - t64_i| over its terms), 0 elsewhere.  The 4 is the margin the conv epilogue tests give tanhf / expf.

Every output is a view inside a larger buffer with 1024 sentinel floats on each side, which must come back untouched; outputs
the kernel overwrites and outputs the launcher must zero first (dx of nearest and slice, out2 of KL, dgamma / dbeta) are
pre-filled with NaN; the words vcv_row_sum does not address carry a prior that must survive bit for bit; optional inputs are
exercised as NULL; a refused call (VCV_EINVAL) leaves its outputs bit-identical.  Launches without atomics repeat their bits on
a second call; the atomic ones (nearest*_bwd, kl_fwd, the generic layernorm_c_bwd) are held to their bounds on both calls.  No
case is skipped at run time.

Distances go to profiles/vits_glue_parity.txt, one line per case."""
import collections
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import conv_f64 as C
import vits_glue_f64 as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
TOL = 2e-5  # tests/test_switch_parity_gpu.py
LN_TOLS = {k: 2e-5 for k in ("out", "mean", "rstd", "dx", "dgamma", "dbeta")}  # tests/test_switch_parity_gpu.py (LN_TOLS)
GUARD, SENT = 1024, 12345.0
KINDS = ("exact", "normal")
gamma, dist, f32 = C.gamma, C.dist, C.f32  # gamma_n; max|got - ref| / max|ref|; the float32 NUMBER a float argument becomes


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "entry name p want")
TABLE = []


def add(entry, name, p, want=()):
    assert (entry, name) not in [(c.entry, c.name) for c in TABLE], (entry, name)
    TABLE.append(Case(entry, name, p, tuple(want)))


# (B, H | C, T) of the element-wise kernels: 555 elements = two full workgroups and a tail, b, c and t all matter; a row of 300
# straddles a workgroup; T = 1; exactly one full workgroup
SHAPES = ((3, 5, 37), (1, 2, 300), (2, 3, 1), (1, 1, 256))


def shape_tags(B, H, T):
    n = B * H * T
    tags = ["blocks>1"] * (n > 256) + ["tail"] * (n % 256 != 0) + ["one full block"] * (n == 256) + ["T=1"] * (T == 1)
    tags += ["a row straddles a block"] * any((r * T) // 256 != (r * T + T - 1) // 256 for r in range(B * H))
    tags += ["B>1 with odd H and T"] * (B > 1 and H % 2 == 1 and T % 2 == 1 and T > 1)
    return tags


def sh(p):
    return "B%d-H%d-T%d" % (p["B"], p["H"], p["T"])


# -- gate: g = None | (gstride / H, goff / H)
GATE_G = {None: "g NULL", (2, 0): "gstride 2H, goff 0", (6, 2): "gstride 6H, goff 2H", (6, 4): "gstride 6H, goff 4H"}
for e_ in ("gate_fwd", "gate_bwd"):
    for B_, H_, T_ in SHAPES:
        for g_ in (None, (2, 0)) + (((6, 2), (6, 4)) if (B_, H_, T_) in SHAPES[:2] else ()):
            add(e_, "B%d-H%d-T%d-%s" % (B_, H_, T_, "gnull" if g_ is None else "g%dH+%dH" % g_), dict(B=B_, H=H_, T=T_, g=g_), [GATE_G[g_]])

# -- row_sum: the conditioning gradient of one layer of three (inner = 2H, ostride = 6H, ooff = 2H) and of a single layer, the
# way _WnGateFn.backward calls it: R = B * 2H rows of dxin, inner = 2H, ostride = gstride, ooff = goff
for T_ in (1, 63, 64, 65, 300):
    add("row_sum", "T%d-slice" % T_, dict(R=30, T=T_, inner=10, ostride=30, ooff=10), ["T %d" % T_, "a slice of a wider row"])
add("row_sum", "T37-dense", dict(R=30, T=37, inner=10, ostride=10, ooff=0), ["dense"])
add("row_sum", "T37-last-slice", dict(R=30, T=37, inner=10, ostride=30, ooff=20), ["the last slice"])

# -- res/skip
for B_, H_, T_ in SHAPES:
    for last_, out_ in ((0, 0), (0, 1), (1, 0), (1, 1)):
        add("rs_fwd", "B%d-H%d-T%d-last%d-out%d" % (B_, H_, T_, last_, out_), dict(B=B_, H=H_, T=T_, last=last_, out=out_),
            ["last %d, out %s" % (last_, "given" if out_ else "NULL")] + ["last 1: x, mask, xn NULL"] * last_)
    for dxn_, don_ in ((0, 1), (1, 0), (1, 1)):
        add("rs_bwd", "B%d-H%d-T%d-dxn%d-don%d" % (B_, H_, T_, dxn_, don_), dict(B=B_, H=H_, T=T_, dxn=dxn_, don=don_),
            ["dxn NULL"] * (not dxn_) + ["don NULL"] * (not don_) + ["dxn and don"] * (dxn_ and don_))

# -- split / sample
for B_, H_, T_ in SHAPES:
    for eps_ in (0, 1):
        add("split_fwd", "B%d-C%d-T%d-eps%d" % (B_, H_, T_, eps_), dict(B=B_, H=H_, T=T_, eps=eps_), ["eps given" if eps_ else "eps NULL, z NULL"])
for B_, H_, T_ in SHAPES[:2]:
    for dm_, dl_, dz_, eps_ in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 1), (1, 1, 1, 0), (1, 1, 0, 0)):
        w_ = ["dm NULL"] * (not dm_) + ["dlogs NULL"] * (not dl_) + ["dz NULL"] * (not dz_ and eps_) + ["all given"] * (dm_ and dl_ and dz_ and eps_)
        w_ += ["dz given, eps NULL"] * (dz_ and not eps_) + ["split only"] * (not dz_ and not eps_)
        add("split_bwd", "B%d-C%d-T%d-dm%d-dlogs%d-dz%d-eps%d" % (B_, H_, T_, dm_, dl_, dz_, eps_), dict(B=B_, H=H_, T=T_, dm=dm_, dlogs=dl_, dz=dz_, eps=eps_), w_)
add("split_bwd", "B2-C3-T1-all", dict(B=2, H=3, T=1, dm=1, dlogs=1, dz=1, eps=1), ["all given", "T=1"])

# -- coupling, prior sample
for B_, H_, T_ in SHAPES:
    for rev_ in (0, 1):
        add("coupling", "B%d-C%d-T%d-%s" % (B_, H_, T_, "reverse" if rev_ else "forward"), dict(B=B_, H=H_, T=T_, reverse=rev_), ["reverse" if rev_ else "forward"])
    add("prior", "B%d-C%d-T%d" % (B_, H_, T_), dict(B=B_, H=H_, T=T_))

# -- KL: 370 elements = one workgroup's 2048; 2532 = two workgroups; 2 097 408 > 1024 * 2048 = the grid-stride loop runs twice
# for the first 256 threads' worth.  `dead`: a fully masked batch row.  `small`: operands from {-1, 0, 1} and logs_q from {0, 1}
# in the exact pass, so that 2 Mi terms stay below 2^24 quanta.
add("kl_fwd", "n370", dict(B=2, H=5, T=37, dead=0, small=0), ["one workgroup"])
add("kl_fwd", "n2532", dict(B=2, H=6, T=211, dead=0, small=0), ["two workgroups"])
add("kl_fwd", "n2532-dead-row", dict(B=2, H=6, T=211, dead=1, small=0), ["a fully masked batch row"])
add("kl_fwd", "n2097408", dict(B=2, H=192, T=5462, dead=0, small=1), ["the grid-stride loop runs"])
for B_, H_, T_ in SHAPES + ((2, 6, 211),):
    for gout_ in ((1,) if (B_, H_, T_) in SHAPES[1:] else (0, 1)):
        add("kl_bwd", "B%d-C%d-T%d-gout%s" % (B_, H_, T_, "-not-1" if gout_ else "-1"), dict(B=B_, H=H_, T=T_, dead=int(B_ > 1 and T_ > 1), gout=gout_),
            ["gout != 1"] * gout_ + ["gout 1"] * (not gout_))

# -- nearest: (Tin, Tout) pairs.  f32: the float32 index map differs from the exact rational one, to * Tin // Tout
# (test_nearest_table_pairs_need_the_float32_map on the CPU); two with Tin > 100, one up- and one downsampling.
NEAREST = (((2, 82), 1), ((2, 94), 1), ((102, 194), 1), ((104, 22), 1), ((37, 37), 0), ((1, 9), 0), ((9, 1), 0), ((40, 300), 0))
for e_ in ("nearest_fwd", "nearest_bwd"):
    for (ti_, to_), f32_ in NEAREST:
        add(e_, "R3-Tin%d-Tout%d" % (ti_, to_), dict(R=3, Tin=ti_, Tout=to_, f32map=f32_), ["float32 map"] * f32_)
# -- nearest with the map of other sizes: raw = (Tin_raw, Tout_raw), a device int64 pair
RAW = (((40, 100), (0, 100), "raw[0] <= 0: Tin itself"), ((40, 100), (33, 82), "raw sizes below the padded ones"), ((5, 100), (2, 82), "float32 map"),
       ((40, 100), (33, 0), "raw[1] == 0: all zero"), ((40, 100), (41, 100), "raw[0] > Tin: all zero"), ((40, 300), (-3, 257), "raw[0] <= 0: Tin itself"))
for e_ in ("raw_fwd", "raw_bwd"):
    for (ti_, to_), raw_, w_ in RAW:
        add(e_, "R3-Tin%d-Tout%d-raw%d,%d" % (ti_, to_, raw_[0], raw_[1]), dict(R=3, Tin=ti_, Tout=to_, raw=raw_, f32map=int(w_ == "float32 map")), [w_])

# -- slice: per batch element a start index
SLICES = (dict(B=5, H=3, T=40, S=4, mul=1, ids=(3, 36, 38, 50, -2)), dict(B=5, H=2, T=320, S=300, mul=1, ids=(5, 20, 100, 400, -7)),
          dict(B=4, H=3, T=40, S=4, mul=4, ids=(2, 9, 12, -1)), dict(B=5, H=2, T=700, S=300, mul=4, ids=(10, 100, 150, 200, -3)),
          dict(B=1, H=1, T=1, S=4, mul=1, ids=(0,)))
for e_ in ("slice_fwd", "slice_bwd"):
    for p_ in SLICES:
        add(e_, "B%d-C%d-T%d-S%d-mul%d" % (p_["B"], p_["H"], p_["T"], p_["S"], p_["mul"]), dict(p_))

# -- dropout (the seed-offset pointer is NULL: asserted before the call)
for n_ in (1, 255, 257, 1000):
    for i_, pd_ in enumerate((0.0, 0.1, 0.5)):
        add("dropout", "n%d-p%g" % (n_, pd_), dict(n=n_, p=pd_, seed=(0x1234ABCD, 0xFEDCBA9876543210)[(n_ + i_) % 2]), ["n %d" % n_, "p %g" % pd_, "seed %d" % ((n_ + i_) % 2)])

CASES = {"%s-%s" % (c.entry, c.name): c for c in TABLE}
IDS = list(CASES)
NO_EXACT = ("gate_fwd", "gate_bwd")
ELEMENTWISE = ("gate_fwd", "gate_bwd", "rs_fwd", "rs_bwd", "split_fwd", "split_bwd", "coupling", "prior", "kl_bwd")


def slice_tags(p):
    tags = ["mul %d" % p["mul"], "S %d" % p["S"]]
    for i in p["ids"]:
        lo, hi = i * p["mul"], i * p["mul"] + p["S"]
        tags.append("starts negative" if lo < 0 else "beyond T" if lo >= p["T"] else "runs past T" if hi > p["T"] else "ends at T" if hi == p["T"] else "inside")
    return tags


def tags_of(c):
    p = c.p
    tags = list(c.want)
    if c.entry in ELEMENTWISE or c.entry == "kl_fwd":
        tags += shape_tags(p["B"], p["H"], p["T"])
    if c.entry in ("kl_fwd", "kl_bwd") and p["dead"]:
        tags.append("a fully masked batch row")
    if c.entry == "kl_fwd":
        n = p["B"] * p["H"] * p["T"]
        tags += ["one workgroup"] * (n <= 2048) + ["two workgroups"] * (2048 < n <= 4096) + ["the grid-stride loop runs"] * (n > 1024 * 2048)
    if c.entry in ("nearest_fwd", "nearest_bwd"):
        tags += ["Tin == Tout"] * (p["Tin"] == p["Tout"]) + ["Tin 1"] * (p["Tin"] == 1) + ["Tout 1"] * (p["Tout"] == 1) + ["R 3"] * (p["R"] == 3)
        tags += ["upsampling"] * (p["Tout"] > p["Tin"]) + ["downsampling"] * (p["Tout"] < p["Tin"])
        tags += ["float32 map, Tin > 100, up"] * (p["f32map"] and p["Tin"] > 100 and p["Tout"] > p["Tin"])
        tags += ["float32 map, Tin > 100, down"] * (p["f32map"] and p["Tin"] > 100 and p["Tout"] < p["Tin"])
    if c.entry in ("raw_fwd", "raw_bwd"):
        a, b = p["raw"]
        tags += ["tail of zeros"] * (0 < b < p["Tout"]) + ["dx beyond Tin_raw is zero"] * (0 < a < p["Tin"]) + ["blocks>1"] * (p["R"] * p["Tout"] > 256)
    if c.entry in ("slice_fwd", "slice_bwd"):
        tags += slice_tags(p)
    return sorted(set(tags), key=tags.index)


_EL = ("blocks>1", "tail", "one full block", "T=1", "a row straddles a block", "B>1 with odd H and T")
NEED = {
    "gate_fwd": _EL + tuple(GATE_G.values()),
    "gate_bwd": _EL + tuple(GATE_G.values()),
    "row_sum": ("T 1", "T 63", "T 64", "T 65", "T 300", "a slice of a wider row", "dense", "the last slice"),
    "rs_fwd": _EL + ("last 0, out NULL", "last 0, out given", "last 1, out NULL", "last 1, out given", "last 1: x, mask, xn NULL"),
    "rs_bwd": _EL + ("dxn NULL", "don NULL", "dxn and don"),
    "split_fwd": _EL + ("eps NULL, z NULL", "eps given"),
    "split_bwd": ("blocks>1", "tail", "a row straddles a block", "T=1", "B>1 with odd H and T", "dm NULL", "dlogs NULL", "dz NULL", "all given", "dz given, eps NULL", "split only"),
    "coupling": _EL + ("forward", "reverse"),
    "prior": _EL,
    "kl_fwd": ("one workgroup", "two workgroups", "the grid-stride loop runs", "a fully masked batch row", "B>1 with odd H and T"),
    "kl_bwd": _EL + ("gout != 1", "gout 1", "a fully masked batch row"),
    "nearest_fwd": ("float32 map", "float32 map, Tin > 100, up", "float32 map, Tin > 100, down", "Tin == Tout", "Tin 1", "Tout 1", "R 3", "upsampling", "downsampling"),
    "nearest_bwd": ("float32 map", "float32 map, Tin > 100, up", "float32 map, Tin > 100, down", "Tin == Tout", "Tin 1", "Tout 1", "R 3", "upsampling", "downsampling"),
    "raw_fwd": ("raw[0] <= 0: Tin itself", "raw sizes below the padded ones", "tail of zeros", "dx beyond Tin_raw is zero", "raw[1] == 0: all zero", "raw[0] > Tin: all zero", "float32 map", "blocks>1"),
    "raw_bwd": ("raw[0] <= 0: Tin itself", "raw sizes below the padded ones", "tail of zeros", "dx beyond Tin_raw is zero", "raw[1] == 0: all zero", "raw[0] > Tin: all zero", "float32 map", "blocks>1"),
    "slice_fwd": ("inside", "ends at T", "runs past T", "beyond T", "starts negative", "mul 1", "mul 4", "S 4", "S 300"),
    "slice_bwd": ("inside", "ends at T", "runs past T", "beyond T", "starts negative", "mul 1", "mul 4", "S 4", "S 300"),
    "dropout": ("n 1", "n 255", "n 257", "n 1000", "p 0", "p 0.1", "p 0.5", "seed 0", "seed 1"),
}


def test_case_table_reaches_every_edge():
    """Host only, no library.  Every case carries the tags it was written for, the table reaches every tag of NEED, no two cases
    of an entry point are identical, and the table keeps to the sizes the suite can afford (one 2 Mi-element case)."""
    seen = collections.Counter()
    for c in TABLE:
        tags = tags_of(c)
        seen.update("%s %s" % (c.entry, tg) for tg in tags)
        n = c.p["B"] * c.p["H"] * c.p["T"] if "B" in c.p else 0
        assert n <= 8192 or c.name == "n2097408", c.name
    assert set(NEED) == {c.entry for c in TABLE}
    missing = [(e, b) for e in NEED for b in NEED[e] if not seen["%s %s" % (e, b)]]
    assert not missing, missing
    keys = [(c.entry, tuple(sorted((k, str(v)) for k, v in c.p.items()))) for c in TABLE]
    assert not [k for k, n in collections.Counter(keys).items() if n > 1]
    assert shape_tags(3, 5, 37) == ["blocks>1", "tail", "a row straddles a block", "B>1 with odd H and T"]
    assert "a row straddles a block" in shape_tags(1, 2, 300) and shape_tags(1, 1, 256) == ["one full block"]
    assert 2 * 192 * 5462 == 2097408 > 1024 * 2048
    assert all(len(p["ids"]) == p["B"] for p in SLICES)  # one start index per batch element
    for c in LN_TABLE:
        assert ln_tags(c)
    seen_ln = {tg for c in LN_TABLE for tg in ln_tags(c)}
    assert not [tg for tg in LN_NEED if tg not in seen_ln], [tg for tg in LN_NEED if tg not in seen_ln]


# ---------------------------------------------------------------------------------------------------------------------
# tensors of a case: name -> (shape, generator); outputs: name -> (shape, "nan" | "prior")
# ---------------------------------------------------------------------------------------------------------------------
def spec(c):
    p, e = c.p, c.entry
    if "B" in p:
        B, H, T = p["B"], p["H"], p["T"]
        a, a2, bt = (B, H, T), (B, 2 * H, T), (B, T)
    if e in ("gate_fwd", "gate_bwd"):
        ins = dict(xin=(a2, "int"))
        if p["g"]:
            ins["g"] = ((B, p["g"][0] * H), "g")
        if e == "gate_bwd":
            ins["dacts"] = (a, "int")
            return ins, dict(dxin=(a2, "nan"))
        return ins, dict(acts=(a, "nan"))
    if e == "row_sum":
        return dict(x=((p["R"], p["T"]), "int")), dict(out=((p["R"] // p["inner"], p["ostride"]), "prior"))
    if e == "rs_fwd":
        ins = dict(rs=(a if p["last"] else a2, "int"))
        if p["out"]:
            ins["out"] = (a, "int")
        if not p["last"]:
            ins.update(x=(a, "int"), mask=(bt, "mask"))
            return ins, dict(xn=(a, "nan"), on=(a, "nan"))
        return ins, dict(on=(a, "nan"))
    if e == "rs_bwd":
        ins = dict(mask=(bt, "mask"))
        ins.update({k: (a, "int") for k in ("dxn", "don") if p[k]})
        return ins, dict(drs=(a2, "nan"), dx=(a, "nan"))
    if e == "split_fwd":
        ins = dict(stats=(a2, "stats"), mask=(bt, "mask"))
        outs = dict(m=(a, "nan"), logs=(a, "nan"))
        if p["eps"]:
            ins["eps"] = (a, "int")
            outs["z"] = (a, "nan")
        return ins, outs
    if e == "split_bwd":
        ins = dict(mask=(bt, "mask"), logs=(a, "logs"))
        ins.update({k: (a, "int") for k in ("dm", "dlogs", "dz", "eps") if p[k]})
        return ins, dict(dstats=(a2, "nan"))
    if e == "coupling":
        return dict(x1=(a, "int"), m=(a, "int"), mask=(bt, "mask")), dict(y=(a, "nan"))
    if e == "prior":
        return dict(m=(a, "int"), logs=(a, "logs"), noise=(a, "int")), dict(z=(a, "nan"))
    if e == "kl_fwd":
        return dict(zp=(a, "int"), lq=(a, "lq"), mp=(a, "int"), lp=(a, "logs"), mask=(bt, "mask")), dict(out2=((2,), "nan"))
    if e == "kl_bwd":
        return dict(zp=(a, "int"), mp=(a, "int"), lp=(a, "logs"), mask=(bt, "mask")), {k: (a, "nan") for k in ("dzp", "dlq", "dmp", "dlp")}
    if e in ("nearest_fwd", "raw_fwd"):
        return dict(x=((p["R"], p["Tin"]), "int")), dict(y=((p["R"], p["Tout"]), "nan"))
    if e in ("nearest_bwd", "raw_bwd"):
        return dict(dy=((p["R"], p["Tout"]), "int")), dict(dx=((p["R"], p["Tin"]), "nan"))
    if e == "slice_fwd":
        return dict(x=((p["B"], p["H"], p["T"]), "int")), dict(y=((p["B"], p["H"], p["S"]), "nan"))
    if e == "slice_bwd":
        return dict(dy=((p["B"], p["H"], p["S"]), "int")), dict(dx=((p["B"], p["H"], p["T"]), "nan"))
    assert e == "dropout"
    return dict(x=((p["n"],), "int")), dict(y=((p["n"],), "nan"))


def scalars(c, kind):
    """the float arguments of a case, as float32 numbers: noise_scale; gout and den of the KL backward (gout / den a power of two
    in the exact pass; den is an input of the launcher, not the mask's own sum)"""
    if c.entry == "prior":
        return dict(noise_scale=0.5 if kind == "exact" else f32(0.667))
    if c.entry == "kl_bwd":
        if kind == "exact":
            return dict(gout=0.5 if c.p["gout"] else 1.0, den=4.0 if c.p["gout"] else 1.0)
        return dict(gout=f32(0.37) if c.p["gout"] else 1.0, den=23.0)
    return {}


def make_mask(rng, B, T, kind, dead):
    """[B, T] with holes, not a prefix: {0, 0.5, 1} (exact) or {0, 1} (normal); T = 1 keeps one live and one empty row where it
    can; `dead`: the last batch row is all zero"""
    m = rng.choice([0.0, 0.5, 1.0] if kind == "exact" else [0.0, 1.0, 1.0], (B, T))
    m[0, 0] = 1.0
    if T > 2:
        m[:, 1] = 0.0  # a hole right after a live frame, in every row
        m[:, -1] = 1.0 if kind == "normal" else 0.5
    if dead:
        m[-1] = 0.0
    return m


@functools.lru_cache(maxsize=None)
def inputs(key, kind):
    """CPU tensors of case `key` (float32; raw and ids int64)."""
    c = CASES[key]
    p = c.p
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    f = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    small = p.get("small", 0)
    t = {}
    for name, (shape, gen) in spec(c)[0].items():
        if gen == "mask":
            v = make_mask(rng, shape[0], shape[1], kind, p.get("dead", 0))
        elif gen == "logs":
            v = np.zeros(shape) if kind == "exact" else 0.3 * rng.standard_normal(shape)
        elif gen == "stats":  # [B, 2C, T]: the second half becomes logs
            v = rng.integers(-8, 9, shape).astype(np.float64) if kind == "exact" else rng.standard_normal(shape)
            v[:, shape[1] // 2:] = 0.0 if kind == "exact" else 0.3 * v[:, shape[1] // 2:]
        elif gen == "g":  # [B, k * H]: this layer's 2H values at goff, a sentinel everywhere else
            H, goff = p["H"], p["g"][1] * p["H"]
            v = np.full(shape, SENT)
            v[:, goff:goff + 2 * H] = rng.standard_normal((shape[0], 2 * H))
        elif gen == "lq":
            v = (rng.integers(0, 2, shape) if small else rng.integers(-4, 5, shape)) if kind == "exact" else rng.standard_normal(shape)
        else:
            amp = 1 if small else 4 if c.entry in ("kl_fwd", "kl_bwd") else 8
            v = rng.integers(-amp, amp + 1, shape) if kind == "exact" else rng.standard_normal(shape)
        t[name] = f(v)
    if c.entry == "row_sum":
        sh_ = spec(c)[1]["out"][0]
        t["prior"] = f(rng.integers(-4, 5, sh_) if kind == "exact" else rng.standard_normal(sh_))
    if "raw" in p:
        t["raw"] = torch.tensor(p["raw"], dtype=torch.int64)
    if "ids" in p:
        t["ids"] = torch.tensor(p["ids"], dtype=torch.int64)
    return t


Out = collections.namedtuple("Out", "ref S n trans")  # S None: bit-equal in the normal pass as well


def compute(c, kind, t, dtype):
    """label -> Out of case c from the CPU tensors t; a label is an output's name, or (name, half) for one half along dim 1.
    S and n are the element-wise bound's; the float32 run (d32) reads only .ref."""
    p, e = c.p, c.entry
    g = lambda k: t.get(k)
    A = lambda k: t[k].double().abs()
    ex = lambda k: torch.exp(t[k].double())
    sc = scalars(c, kind)
    bit = lambda v: Out(v, None, 0, False)
    if "mask" in t:
        mk = t["mask"].double().unsqueeze(1)
    if e in ("gate_fwd", "gate_bwd"):
        goff = p["g"][1] * p["H"] if p["g"] else 0
        if e == "gate_fwd":
            r = V.wn_gate(t["xin"], g("g"), goff, dtype)
            return {"acts": Out(r, V.wn_gate(t["xin"], g("g"), goff).abs(), 8, True)}
        r = V.wn_gate_bwd(t["xin"], g("g"), goff, t["dacts"], dtype)
        a, b = V._gate_args(t["xin"], g("g"), goff, torch.float64)
        th, sg, d = torch.tanh(a), torch.sigmoid(b), A("dacts")
        return {"dxin": Out(r, torch.cat([d * sg * (1 + th * th), d * th.abs() * sg * (1 + sg)], 1), 10, True)}
    if e == "row_sum":
        r = V.row_sum(t["x"], p["R"], p["T"], p["inner"], p["ostride"], p["ooff"], t["prior"], dtype)
        S = V.row_sum(t["x"].abs(), p["R"], p["T"], p["inner"], p["ostride"], p["ooff"], torch.zeros_like(t["prior"]))
        return {"out": Out(r, S, p["T"], False)}
    if e == "rs_fwd":
        xn, on = V.wn_res_skip(g("x"), g("out"), t["rs"], g("mask"), p["last"], dtype)
        return {"on": bit(on)} if p["last"] else {"xn": bit(xn), "on": bit(on)}
    if e == "rs_bwd":
        drs, dx = V.wn_res_skip_bwd(g("dxn"), g("don"), t["mask"], (p["B"], p["H"], p["T"]), dtype)
        return {"drs": bit(drs), "dx": bit(dx)}
    if e == "split_fwd":
        m, logs, z = V.split_sample(t["stats"], g("eps"), t["mask"], dtype)
        out = {"m": bit(m), "logs": bit(logs)}
        if p["eps"]:
            m64, l64, _ = V.split_sample(t["stats"], None, t["mask"])
            out["z"] = Out(z, (m64.abs() + A("eps") * torch.exp(l64)) * mk, 5, True)
        return out
    if e == "split_bwd":
        shape = (p["B"], p["H"], p["T"])
        r = V.split_sample_bwd(g("dm"), g("dlogs"), g("dz"), g("eps"), t["logs"], t["mask"], shape, dtype)
        H = p["H"]
        if not (p["dz"] and p["eps"]):
            return {"dstats": bit(r)}
        z = torch.zeros(shape, dtype=torch.float64)
        Sm = ((A("dm") if p["dm"] else z) + A("dz") * mk) * mk
        Sl = ((A("dlogs") if p["dlogs"] else z) + A("dz") * mk * A("eps") * ex("logs")) * mk
        return {("dstats", 0): Out(r[:, :H], Sm, 3, False), ("dstats", 1): Out(r[:, H:], Sl, 6, True)}
    if e == "coupling":
        return {"y": bit(V.coupling(t["x1"], t["m"], t["mask"], p["reverse"], dtype))}
    if e == "prior":
        r = V.prior_sample(t["m"], t["logs"], t["noise"], sc["noise_scale"], dtype)
        return {"z": Out(r, A("m") + A("noise") * ex("logs") * sc["noise_scale"], 4, True)}
    if e == "kl_fwd":
        num, den = V.kl(t["zp"], t["lq"], t["mp"], t["lp"], t["mask"], dtype)
        d = t["zp"].double() - t["mp"].double()
        S = ((A("lp") + A("lq") + 0.5 + 0.5 * d * d * torch.exp(-2.0 * t["lp"].double())) * mk).sum()
        return {("out2", 0): Out(num.reshape(1), S.reshape(1), p["B"] * p["H"] * p["T"] + 10, True), ("out2", 1): bit(den.reshape(1))}
    if e == "kl_bwd":
        gout, den = torch.tensor(sc["gout"], dtype=torch.float64), torch.tensor(sc["den"], dtype=torch.float64)
        r = V.kl_bwd(t["zp"], t["mp"], t["lp"], t["mask"], gout, den, dtype)
        k = (gout / den).abs() * mk
        d = t["zp"].double() - t["mp"].double()
        ee = torch.exp(-2.0 * t["lp"].double())
        kde = k * d.abs() * ee
        return {"dzp": Out(r[0], kde, 8, True), "dlq": Out(r[1], k.expand_as(d), 2, False), "dmp": Out(r[2], kde, 8, True), "dlp": Out(r[3], k * (1 + d * d * ee), 10, True)}
    if e == "nearest_fwd":
        return {"y": bit(V.nearest(t["x"], p["Tout"], dtype))}
    if e == "raw_fwd":
        return {"y": bit(V.nearest_raw(t["x"], p["Tout"], p["raw"], dtype))}
    if e in ("nearest_bwd", "raw_bwd"):
        idx = V.nearest_index(p["Tin"], p["Tout"]) if e == "nearest_bwd" else V.nearest_raw_index(p["Tin"], p["Tout"], p["raw"])
        n = int(torch.bincount(idx[idx >= 0], minlength=1).max()) if bool((idx >= 0).any()) else 1
        return {"dx": Out(V.scatter_t(t["dy"], idx, p["Tin"], dtype), V.scatter_t(t["dy"].abs(), idx, p["Tin"]), n, False)}
    if e == "slice_fwd":
        return {"y": bit(V.slice(t["x"], t["ids"], p["mul"], p["S"], dtype))}
    if e == "slice_bwd":
        return {"dx": bit(V.slice_bwd(t["dy"], t["ids"], p["mul"], p["T"], dtype))}
    assert e == "dropout"
    return {"y": bit(V.dropout(t["x"], f32(p["p"]), p["seed"], dtype))}


@functools.lru_cache(maxsize=None)
def reference(key, kind):
    """label -> (float64 expectation, S, n, a): a = 4 * d32 where a transcendental is evaluated (normal pass), else 0"""
    c = CASES[key]
    t = inputs(key, kind)
    r64 = compute(c, kind, t, torch.float64)
    out = {}
    r32 = compute(c, kind, t, torch.float32) if kind == "normal" and any(o.trans for o in r64.values()) else None
    for label, o in r64.items():
        d32 = 0.0
        if r32 is not None and o.trans:
            d32 = (r32[label].ref.double() - o.ref).abs().max().item()
            if c.entry == "kl_fwd":  # the numerator: the sum of the terms' own float32 errors
                a = (t["zp"], t["lq"], t["mp"], t["lp"], t["mask"])
                d32 = (V.kl_terms(*a, dtype=torch.float32).double() - V.kl_terms(*a)).abs().sum().item()
        out[label] = (o.ref, o.S, o.n, d32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the exact pass is exact: from the table alone (asserted by tests/test_vits_glue_f64_cpu.py::test_exact_pass_is_exact)
# ---------------------------------------------------------------------------------------------------------------------
def exact_budget(c):
    """[(quantum, bound)]: every result and every partial sum of case c in the exact pass is a multiple of `quantum` (a power of
    two) and at most `bound` in magnitude.  Operands are integers in [-8, 8] ([-4, 4] for KL, {-1, 0, 1} with logs_q from {0, 1}
    for its `small` case), masks from {0, 0.5, 1}, exp(0) = 1.  None: one rounded product, nothing is summed (dropout)."""
    p, e = c.p, c.entry
    if e == "row_sum":
        return [(1.0, 8.0 * p["T"] + 4)]
    if e in ("rs_fwd", "rs_bwd", "coupling"):
        return [(0.5, 16.0)]
    if e == "split_fwd":  # m, logs = stats * mask: halves; z = (m + eps) * mask: quarters
        return [(0.5, 8.0), (0.25, 16.0)]
    if e == "split_bwd":  # gz = dz * mask; gm = dm + gz; gl = dlogs + gz * eps; each times mask
        return [(0.5, 8.0 + 8.0 * 8.0), (0.25, 8.0 + 8.0 * 8.0)]
    if e == "prior":  # m + noise * 1 * 0.5
        return [(0.5, 12.0)]
    if e == "kl_fwd":  # (0 - lq - 0.5 + 0.5 d^2) * mask, summed over every element in any order; sum(mask) in halves
        n = p["B"] * p["H"] * p["T"]
        top = 1.5 if p["small"] else 4 + 0.5 + 0.5 * 64
        return [(0.25, top * n), (0.5, float(p["B"] * p["T"]))]
    if e == "kl_bwd":  # k = (gout / den) * mask = 2^-3 * {0, 0.5, 1} (or 1 * ...); k d, k (1 - d^2), |d| <= 8
        return [(2.0 ** -4, 64.0)]
    if e in ("nearest_bwd", "raw_bwd"):
        return [(1.0, 8.0 * p["Tout"])]
    if e in ("nearest_fwd", "raw_fwd", "slice_fwd", "slice_bwd"):
        return [(1.0, 8.0)]
    assert e == "dropout"
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------------------------------------------------
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


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=2)
def on_gpu(key, kind, gpu):
    return {k: v.to(gpu) for k, v in inputs(key, kind).items()}


def launch(L, c, kind, t, o):
    """the one launcher of case c with the device tensors t (a missing name is NULL) and the output views o -> status"""
    p, e = c.p, c.entry
    g = lambda k: ptr(t.get(k))
    sc = scalars(c, kind)
    st = None  # the null stream
    if "B" in p:
        B, H, T = p["B"], p["H"], p["T"]
    if e in ("gate_fwd", "gate_bwd"):
        gstride, goff = (p["g"][0] * H, p["g"][1] * H) if p["g"] else (0, 0)
        if e == "gate_fwd":
            return L.vcv_wn_gate_fwd(g("xin"), g("g"), gstride, goff, ptr(o["acts"]), B, H, T, st)
        return L.vcv_wn_gate_bwd(g("xin"), g("g"), gstride, goff, g("dacts"), ptr(o["dxin"]), B, H, T, st)
    if e == "row_sum":
        return L.vcv_row_sum(g("x"), ptr(o["out"]), p["R"], p["T"], p["inner"], p["ostride"], p["ooff"], st)
    if e == "rs_fwd":
        return L.vcv_wn_res_skip_fwd(g("x"), g("out"), g("rs"), g("mask"), ptr(o.get("xn")), ptr(o["on"]), B, H, T, p["last"], st)
    if e == "rs_bwd":
        return L.vcv_wn_res_skip_bwd(g("dxn"), g("don"), g("mask"), ptr(o["drs"]), ptr(o["dx"]), B, H, T, st)
    if e == "split_fwd":
        return L.vcv_split_sample_fwd(g("stats"), g("eps"), g("mask"), ptr(o["m"]), ptr(o["logs"]), ptr(o.get("z")), B, H, T, st)
    if e == "split_bwd":
        return L.vcv_split_sample_bwd(g("dm"), g("dlogs"), g("dz"), g("eps"), g("logs"), g("mask"), ptr(o["dstats"]), B, H, T, st)
    if e == "coupling":
        return L.vcv_coupling(g("x1"), g("m"), g("mask"), ptr(o["y"]), B, H, T, p["reverse"], st)
    if e == "prior":
        return L.vcv_prior_sample(g("m"), g("logs"), g("noise"), ptr(o["z"]), B * H * T, sc["noise_scale"], st)
    if e == "kl_fwd":
        return L.vcv_kl_fwd(g("zp"), g("lq"), g("mp"), g("lp"), g("mask"), ptr(o["out2"]), B, H, T, st)
    if e == "kl_bwd":
        return L.vcv_kl_bwd(g("zp"), g("mp"), g("lp"), g("mask"), g("gout"), g("den"), ptr(o["dzp"]), ptr(o["dlq"]), ptr(o["dmp"]), ptr(o["dlp"]), B, H, T, st)
    if e == "nearest_fwd":
        return L.vcv_nearest_fwd(g("x"), ptr(o["y"]), p["R"], p["Tin"], p["Tout"], st)
    if e == "nearest_bwd":
        return L.vcv_nearest_bwd(g("dy"), ptr(o["dx"]), p["R"], p["Tin"], p["Tout"], st)
    if e == "raw_fwd":
        return L.vcv_nearest_raw_fwd(g("x"), ptr(o["y"]), p["R"], p["Tin"], p["Tout"], g("raw"), st)
    if e == "raw_bwd":
        return L.vcv_nearest_raw_bwd(g("dy"), ptr(o["dx"]), p["R"], p["Tin"], p["Tout"], g("raw"), st)
    if e == "slice_fwd":
        return L.vcv_slice_fwd(g("x"), g("ids"), p["mul"], ptr(o["y"]), B, H, T, p["S"], st)
    if e == "slice_bwd":
        return L.vcv_slice_bwd(g("dy"), g("ids"), p["mul"], ptr(o["dx"]), B, H, T, p["S"], st)
    assert e == "dropout"
    assert not L.vcv_get_seed_offset_ptr(), "the seed-offset pointer must be NULL outside graph capture"
    return L.vcv_dropout(g("x"), ptr(o["y"]), p["n"], f32(p["p"]), p["seed"], st)


def abi(gpu, c, kind):
    """One call through the C ABI -> (status, name -> the output view, name -> what it held before the call)."""
    from vcvits_amd._lib import lib
    key = "%s-%s" % (c.entry, c.name)
    t = dict(on_gpu(key, kind, gpu))
    for k, v in scalars(c, kind).items():
        if k in ("gout", "den"):
            t[k] = torch.tensor([v], device=gpu, dtype=torch.float32)
    outs = {k: Guarded(shape, gpu, float("nan") if init == "nan" else t["prior"]) for k, (shape, init) in spec(c)[1].items()}
    before = {k: v.t.clone() for k, v in outs.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.default_stream(gpu)):
        st = launch(lib(), c, kind, t, {k: v.t for k, v in outs.items()})
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert v.intact(), "%s: a write outside %s" % (key, k)
    return st, {k: v.t for k, v in outs.items()}, before


def uses_atomics(c):
    return c.entry in ("nearest_bwd", "raw_bwd", "kl_fwd")


def pick(outs, label):
    """the tensor a label of compute() names"""
    if isinstance(label, str):
        return outs[label]
    name, half = label
    if outs[name].dim() == 1:
        return outs[name][half:half + 1]
    h = outs[name].shape[1] // 2
    return outs[name][:, half * h:(half + 1) * h]


def label_name(label):
    return label if isinstance(label, str) else "%s[%d]" % label


def check(c, kind, outs, fails, what=""):
    """the outputs against the float64 reference: bit for bit (exact, and the one-rounding kernels), or within both bounds.
    -> (max-norm distance, worst ratio to the element-wise bound, d32) over the bounded outputs, or None"""
    key = "%s-%s" % (c.entry, c.name)
    worst = None
    for label, (y64, S, n, d32) in reference(key, kind).items():
        got = pick(outs, label).detach().cpu().reshape(y64.shape)
        tag = "%s %s %s%s" % (key, kind, label_name(label), what)
        if bool(torch.isnan(got).any()):
            fails.append("%s: NaN in the output (an element the kernel did not write, or a buffer the launcher did not zero)" % tag)
            continue
        if kind == "exact" or S is None:
            if kind == "exact":
                assert bool((y64.float().double() == y64).all()), tag  # (the reference itself is a float32 number everywhere)
            if not torch.equal(got, y64.float()):
                bad = (got != y64.float()).nonzero()
                fails.append("%s: not the float64 reference's bits at %d elements, first %s (got %r, want %r)" % (
                    tag, len(bad), bad[0].tolist(), got[tuple(bad[0])].item(), y64[tuple(bad[0])].item()))
            continue
        e = dist(got, y64)
        el = gamma(n + 6) * S + 4.0 * d32
        diff = (got.double() - y64).abs()
        ratio = torch.where(diff > 0, diff / el.clamp(min=1e-300), torch.zeros_like(diff)).max().item()
        if e > TOL:
            fails.append("%s: max-norm distance %.3e (bound %.1e)" % (tag, e, TOL))
        if ratio > 1.0:
            fails.append("%s: element-wise, |got - ref| is %.3f x its bound (flat element %d, d32 %.2e)" % (
                tag, ratio, int((diff / el.clamp(min=1e-300)).flatten().argmax()), d32))
        worst = (max(e, worst[0]), max(ratio, worst[1]), max(d32, worst[2])) if worst else (e, ratio, d32)
    return worst


def test_checker_notices_small_local_errors():
    """Host only, no library: the float64 reference cast to float32 passes check(); one ulp on one element of an exact or a
    one-rounding output, and 1.5 x its own bound on the element with the smallest S of a bounded one, do not."""
    def run(key, kind, poke=None):
        c = CASES[key]
        outs = {}
        for label, (y64, _, _, _) in reference(key, kind).items():
            name = label if isinstance(label, str) else label[0]
            if name not in outs:
                outs[name] = torch.zeros(spec(c)[1][name][0])
            pick(outs, label).copy_(y64.float())
        if poke:
            poke(outs)
        fails = []
        check(c, kind, outs, fails)
        return fails

    up = lambda v: torch.nextafter(v, torch.tensor(float("inf")))
    for key in ("gate_bwd-B3-H5-T37-g6H+2H", "split_bwd-B3-C5-T37-dm1-dlogs1-dz1-eps1", "kl_fwd-n2532", "kl_bwd-B3-C5-T37-gout-not-1", "raw_bwd-R3-Tin40-Tout100-raw33,82",
                "rs_fwd-B3-H5-T37-last0-out1", "row_sum-T65-slice"):
        for kind in KINDS:
            if kind == "normal" or CASES[key].entry not in NO_EXACT:
                assert run(key, kind) == [], (key, kind)
    f = run("rs_fwd-B3-H5-T37-last0-out1", "normal", lambda o: o["xn"].__setitem__((2, 4, 36), up(o["xn"][2, 4, 36])))
    assert len(f) == 1 and "bits at 1 elements" in f[0], f
    f = run("kl_fwd-n2532", "exact", lambda o: o["out2"].__setitem__(0, up(o["out2"][0])))
    assert len(f) == 1 and "bits at 1 elements" in f[0], f
    key = "split_bwd-B3-C5-T37-dm1-dlogs1-dz1-eps1"
    y64, S, n, d32 = reference(key, "normal")[("dstats", 0)]
    live = torch.where(S > 0, S, torch.full_like(S, float("inf")))
    i = tuple(np.unravel_index(int(live.argmin()), S.shape))
    delta = 1.5 * gamma(n + 6) * S[i].item()
    assert d32 == 0.0 and delta < 0.5 * TOL * y64.abs().max().item()
    f = run(key, "normal", lambda o: o["dstats"].__setitem__(i, float(y64[i]) + delta))
    assert len(f) == 1 and "element-wise" in f[0], f


# ---------------------------------------------------------------------------------------------------------------------
# the profile
# ---------------------------------------------------------------------------------------------------------------------
_parity = {}
HEADER = ("# tests/test_vits_glue_abi_gpu.py: distance of the streaming glue kernels (csrc/vits_blocks.hip) at the C ABI from their float64 CPU\n"
          "# references (tests/vits_glue_f64.py), normal pass.  Per case: what the case is there for | max|got - ref| / max|ref| (bound 2e-5) /\n"
          "# the worst ratio of |got - ref| to its element-wise bound gamma_n * S + a (must be <= 1) | d32 = max|float32 CPU run - float64 run|\n"
          "# of the reference where a transcendental is evaluated (a = 4 * d32 there, 0 elsewhere; the KL numerator: the sum of its terms'\n"
          "# |t32 - t64|).  `bit-equal`: one rounded operation per element, the float64 reference's bits (asserted).  The exact pass (integer\n"
          "# operands) is bit-equal to float64 or fails: it has no distances to report.  LayerNorm: max-norm distances per output (bound 2e-5).\n")


def record(section, line):
    """Keep the measured distances in profiles/vits_glue_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "vits_glue_parity.txt"), "w") as f:
        f.write(HEADER)
        for name in _parity:
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------
# (the gate has no exact pass: tanh and the sigmoid of an integer are no float32 numbers)
PARITY = [(key, kind) for key in IDS for kind in KINDS if kind == "normal" or CASES[key].entry not in NO_EXACT]


@pytest.mark.gpu
@pytest.mark.parametrize("key,kind", PARITY, ids=["%s-%s" % kk for kk in PARITY])
def test_parity(gpu, key, kind):
    """One case, two launches: status 0, the guards intact, every output within check() of float64; the second launch repeats the
    first one's bits, or (atomics) is held to the same bounds."""
    c = CASES[key]
    fails = []
    st1, y1, before = abi(gpu, c, kind)
    st2, y2, _ = abi(gpu, c, kind)
    assert st1 == 0 and st2 == 0, "%s: status %d / %d" % (key, st1, st2)
    cell = check(c, kind, y1, fails)
    if uses_atomics(c):
        check(c, kind, y2, fails, " (second launch)")
    elif not all(torch.equal(bits(y1[k]), bits(y2[k])) for k in y1):
        fails.append("%s %s: two identical launches differ" % (key, kind))
    if c.entry == "row_sum":  # the words no row is written to keep their prior, bit for bit
        keep = torch.ones(y1["out"].numel(), dtype=torch.bool)
        keep[V.row_sum_index(c.p["R"], c.p["inner"], c.p["ostride"], c.p["ooff"])] = False
        if not torch.equal(bits(y1["out"]).flatten().cpu()[keep], bits(before["out"]).flatten().cpu()[keep]):
            fails.append("%s %s: a word vcv_row_sum does not address changed" % (key, kind))
    if kind == "normal":
        record(c.entry, "%-44s %-80s | %s" % (c.name, ", ".join(tags_of(c)), ("%.1e/%.2f" % cell[:2] + (" | d32=%.1e" % cell[2] if cell[2] else "")) if cell else "bit-equal"))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-T%d" % s)
def test_coupling_round_trip(gpu, shape, kind):
    """reverse(forward(x1)) against x1 * mask.  With a {0, 1} mask (normal) the forward's m + x1 and the reverse's subtraction are
    one rounding each: |got - x1 mask| <= gamma_(2+6) (|m| + |x1| + |m|) there; integers and halves (exact) come back bit for bit
    as x1 * mask^2."""
    from vcvits_amd._lib import lib
    B, Cn, T = shape
    key = "coupling-B%d-C%d-T%d-forward" % shape
    t = on_gpu(key, kind, gpu)
    y, x2 = Guarded(shape, gpu, float("nan")), Guarded(shape, gpu, float("nan"))
    with torch.cuda.stream(torch.cuda.default_stream(gpu)):
        assert lib().vcv_coupling(ptr(t["x1"]), ptr(t["m"]), ptr(t["mask"]), ptr(y.t), B, Cn, T, 0, None) == 0
        assert lib().vcv_coupling(ptr(y.t), ptr(t["m"]), ptr(t["mask"]), ptr(x2.t), B, Cn, T, 1, None) == 0
    torch.cuda.synchronize()
    assert y.intact() and x2.intact()
    c = inputs(key, kind)
    mk = c["mask"].double().unsqueeze(1)
    want = c["x1"].double() * mk * mk
    got = x2.t.cpu().double()
    if kind == "exact":
        assert torch.equal(got, want)
        return
    S = (2 * c["m"].double().abs() + c["x1"].double().abs()) * mk
    ratio = ((got - want).abs() / (gamma(2 + 6) * S).clamp(min=1e-300)).max().item()
    record("coupling round trip", "%-44s %.1e/%.2f" % ("B%d-C%d-T%d" % shape, dist(got, want), ratio))
    assert ratio <= 1.0 and dist(got, want) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm over channels: forward and backward at the ABI (normal pass only)
# ---------------------------------------------------------------------------------------------------------------------
LnCase = collections.namedtuple("LnCase", "B C T y scratch")  # scratch: "exact" | "short" (one float short: the atomics form)
LN_TABLE = [LnCase(2, Cn_, 65, Cn_ % 2, "exact") for Cn_ in (1, 2, 3, 5, 33, 130)]
LN_TABLE += [LnCase(2, Cn_, T_, (Cn_ // 128 + T_) % 2, "exact") for Cn_ in (128, 256) for T_ in (1, 63, 64, 65)]
LN_TABLE += [LnCase(2, 128, 65, 1, "short"), LnCase(3, 256, 37, 0, "short")]
LN_NEED = ("generic", "waves with no channel", "a round of 32 ends inside", "regs 128", "regs 256", "T 1", "T 63", "T 64", "T 65", "y NULL", "y given",
           "scratch exact", "scratch one float short: atomics")


def ln_tags(c):
    regs = c.C in (128, 256)
    tags = ["regs %d" % c.C if regs else "generic"] + ["waves with no channel"] * (c.C < 4) + ["a round of 32 ends inside"] * (not regs and c.C % 32 != 0 and c.C > 32)
    tags += ["T %d" % c.T] * (c.T in (1, 63, 64, 65)) + ["y given" if c.y else "y NULL"]
    if regs:
        tags.append("scratch exact" if c.scratch == "exact" else "scratch one float short: atomics")
    return tags


@functools.lru_cache(maxsize=None)
def ln_case(c):
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    x, y, ga, be, dout = f(c.B, c.C, c.T), (f(c.B, c.C, c.T) if c.y else None), f(c.C), f(c.C), f(c.B, c.C, c.T)
    if c.C == 2:
        # Two channels normalise to +-d / sqrt(d^2 + eps), d = (x0 - x1) / 2: with d ~ 1 that is +-1 and dx is the residue
        # (g0 - g1) / 2 * eps / (d^2 + eps) of a cancellation, so max|dx| sits on the one frame with the smallest |d|, where half an
        # ulp of x moves d by ~1e-5 of itself and dx by three times that: the float32 CPU run of the reference is itself 1.1e-5
        # from float64 there.  Scaled to d ~ sqrt(eps) the operation is as well conditioned as at any other width (a power of two:
        # the significands stay), and the kernel's arithmetic is what the 2e-5 measures.
        x = x * 2.0 ** -8
    out, mean, rstd = V.layernorm_c(x, y, ga, be, f32(1e-5))
    dx, dgamma, dbeta = V.layernorm_c_bwd(x, y, ga, dout, f32(1e-5))
    return (x, y, ga, be, dout), dict(out=out, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.gpu
@pytest.mark.parametrize("c", LN_TABLE, ids=lambda c: "B%d-C%d-T%d-%s-%s" % (c.B, c.C, c.T, "y" if c.y else "noy", c.scratch))
def test_layernorm_abi(gpu, c):
    """vcv_layernorm_c_fwd and vcv_layernorm_c_bwd_ws against float64 (LN_TOLS), mean and rstd included; dgamma / dbeta arrive
    full of NaN; the scratch is exactly vcv_layernorm_c_bwd_scratch floats between guards, or one float short, where the launcher
    must take the atomics form and leave the scratch alone.  Without atomics two launches give the same bits."""
    from vcvits_amd._lib import lib
    L = lib()
    (x, y, ga, be, dout), ref = ln_case(c)
    xg, gg, bg, dg = (v.to(gpu) for v in (x, ga, be, dout))
    yg = y.to(gpu) if c.y else None
    B, Cn, T = c.B, c.C, c.T
    need = L.vcv_layernorm_c_bwd_scratch(B, Cn, T)
    assert (need > 0) == (Cn in (128, 256)) and (need == 0 or need == -(-T // 64) * B * 2 * Cn)
    nws = need if c.scratch == "exact" else need - 1
    atomics = need == 0 or c.scratch == "short"
    runs = []
    for _ in range(2):
        o = {k: Guarded(s, gpu, float("nan")) for k, s in (("out", (B, Cn, T)), ("mean", (B, T)), ("rstd", (B, T)), ("dx", (B, Cn, T)), ("dgamma", (Cn,)), ("dbeta", (Cn,)))}
        ws = Guarded((max(nws, 1),), gpu, 777.0)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.default_stream(gpu)):
            assert L.vcv_layernorm_c_fwd(ptr(xg), ptr(yg), ptr(gg), ptr(bg), ptr(o["out"].t), ptr(o["mean"].t), ptr(o["rstd"].t), B, Cn, T, f32(1e-5), None) == 0
            assert L.vcv_layernorm_c_bwd_ws(ptr(xg), ptr(yg), ptr(gg), ptr(o["mean"].t), ptr(o["rstd"].t), ptr(dg), ptr(o["dx"].t), ptr(o["dgamma"].t), ptr(o["dbeta"].t),
                                            B, Cn, T, ptr(ws.t) if nws > 0 else None, nws, None) == 0
        torch.cuda.synchronize()
        assert all(v.intact() for v in o.values()) and ws.intact(), "a write outside an output or the scratch"
        if atomics:
            assert bool((ws.t == 777.0).all()), "the atomics form wrote to the scratch"
        errs = {k: dist(o[k].t.cpu().reshape(ref[k].shape), ref[k]) for k in o}
        assert not any(bool(torch.isnan(v.t).any()) for v in o.values())
        runs.append((o, errs))
    for _, errs in runs if atomics else runs[:1]:
        bad = {k: v for k, v in errs.items() if v > LN_TOLS[k]}
        assert not bad, bad
    if not atomics:
        assert all(torch.equal(bits(runs[0][0][k].t), bits(runs[1][0][k].t)) for k in runs[0][0]), "two identical launches differ"
    else:
        assert all(torch.equal(bits(runs[0][0][k].t), bits(runs[1][0][k].t)) for k in ("out", "mean", "rstd", "dx"))
    record("layernorm", "%-44s %-70s | %s" % ("B%d-C%d-T%d" % (B, Cn, T), ", ".join(ln_tags(c)), " ".join("%s=%.1e" % kv for kv in runs[0][1].items())))


# ---------------------------------------------------------------------------------------------------------------------
# refusals: decided on the host, before any launch or memset (read off the launchers of csrc/vits_blocks.hip)
# ---------------------------------------------------------------------------------------------------------------------
X = ctypes.c_void_p(0x10000)  # a stand-in that is never read: every call below returns before its launch

# name -> (the number of pointer arguments, the indices of the REQUIRED ones, the call from the pointer list and the dimensions,
# the legal dimensions).  The optional pointers (g, out, dxn, don, eps, z, dm, dlogs, dz, logs) are not in the lists; with
# last = 0 the res/skip forward also requires x, mask and xn.
REFUSALS = {
    "vcv_wn_gate_fwd": (3, (0, 2), lambda L, a, d: L.vcv_wn_gate_fwd(a[0], a[1], 2 * d[1], 0, a[2], d[0], d[1], d[2], None), (2, 3, 4)),
    "vcv_wn_gate_bwd": (4, (0, 2, 3), lambda L, a, d: L.vcv_wn_gate_bwd(a[0], a[1], 2 * d[1], 0, a[2], a[3], d[0], d[1], d[2], None), (2, 3, 4)),
    "vcv_row_sum": (2, (0, 1), lambda L, a, d: L.vcv_row_sum(a[0], a[1], d[0], d[1], d[2], 6, 0, None), (6, 4, 6)),
    "vcv_wn_res_skip_fwd": (6, (0, 2, 3, 4, 5), lambda L, a, d: L.vcv_wn_res_skip_fwd(a[0], a[1], a[2], a[3], a[4], a[5], d[0], d[1], d[2], 0, None), (2, 3, 4)),
    "vcv_wn_res_skip_fwd (last)": (6, (2, 5), lambda L, a, d: L.vcv_wn_res_skip_fwd(a[0], a[1], a[2], a[3], a[4], a[5], d[0], d[1], d[2], 1, None), (2, 3, 4)),
    "vcv_wn_res_skip_bwd": (5, (2, 3, 4), lambda L, a, d: L.vcv_wn_res_skip_bwd(a[0], a[1], a[2], a[3], a[4], d[0], d[1], d[2], None), (2, 3, 4)),
    "vcv_split_sample_fwd": (6, (0, 2, 3, 4, 5), lambda L, a, d: L.vcv_split_sample_fwd(a[0], a[1], a[2], a[3], a[4], a[5], d[0], d[1], d[2], None), (2, 3, 4)),
    "vcv_split_sample_bwd": (7, (4, 5, 6), lambda L, a, d: L.vcv_split_sample_bwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], d[0], d[1], d[2], None), (2, 3, 4)),
    "vcv_coupling": (4, (0, 1, 2, 3), lambda L, a, d: L.vcv_coupling(a[0], a[1], a[2], a[3], d[0], d[1], d[2], 0, None), (2, 3, 4)),
    "vcv_prior_sample": (4, (0, 1, 2, 3), lambda L, a, d: L.vcv_prior_sample(a[0], a[1], a[2], a[3], d[0], 1.0, None), (24,)),
    "vcv_kl_fwd": (6, (0, 1, 2, 3, 4, 5), lambda L, a, d: L.vcv_kl_fwd(a[0], a[1], a[2], a[3], a[4], a[5], d[0], d[1], d[2], None), (2, 3, 4)),
    "vcv_kl_bwd": (10, tuple(range(10)), lambda L, a, d: L.vcv_kl_bwd(*a, d[0], d[1], d[2], None), (2, 3, 4)),
    "vcv_nearest_fwd": (2, (0, 1), lambda L, a, d: L.vcv_nearest_fwd(a[0], a[1], d[0], d[1], d[2], None), (3, 4, 9)),
    "vcv_nearest_bwd": (2, (0, 1), lambda L, a, d: L.vcv_nearest_bwd(a[0], a[1], d[0], d[1], d[2], None), (3, 4, 9)),
    "vcv_nearest_raw_fwd": (3, (0, 1, 2), lambda L, a, d: L.vcv_nearest_raw_fwd(a[0], a[1], d[0], d[1], d[2], a[2], None), (3, 4, 9)),
    "vcv_nearest_raw_bwd": (3, (0, 1, 2), lambda L, a, d: L.vcv_nearest_raw_bwd(a[0], a[1], d[0], d[1], d[2], a[2], None), (3, 4, 9)),
    "vcv_slice_fwd": (3, (0, 1, 2), lambda L, a, d: L.vcv_slice_fwd(a[0], a[1], 1, a[2], d[0], d[1], d[2], d[3], None), (2, 3, 9, 4)),
    "vcv_slice_bwd": (3, (0, 1, 2), lambda L, a, d: L.vcv_slice_bwd(a[0], a[1], 1, a[2], d[0], d[1], d[2], d[3], None), (2, 3, 9, 4)),
    "vcv_dropout": (2, (0, 1), lambda L, a, d: L.vcv_dropout(a[0], a[1], d[0], 0.5, 1, None), (24,)),
    "vcv_layernorm_c_fwd": (7, (0, 2, 3, 4, 5, 6), lambda L, a, d: L.vcv_layernorm_c_fwd(*a, d[0], d[1], d[2], 1e-5, None), (2, 3, 4)),
    "vcv_layernorm_c_bwd_ws": (9, (0, 2, 3, 4, 5, 6, 7, 8), lambda L, a, d: L.vcv_layernorm_c_bwd_ws(*a, d[0], d[1], d[2], None, 0, None), (2, 3, 4)),
    "vcv_rel_softmax_bwd": (12, tuple(range(12)), lambda L, a, d: L.vcv_rel_softmax_bwd(*a, d[0], d[1], d[2], d[3], 4, 1.0, None), (2, 2, 8, 9)),
}


def test_null_pointers_and_bad_sizes_are_refused():
    """No GPU needed: every call returns VCV_EINVAL before it launches or zeroes anything (the pointers are stand-ins).  Per
    launcher: each required pointer NULL in turn; each dimension 0 and -1 in turn (a negative one used to become an arbitrary
    grid); the split forward with eps but no z, the split backward with dz and eps but no logs; the gate with goff < 0 and with
    goff + 2H > gstride (and the same slice refused by neither rule when g is NULL); dropout with p outside [0, 1); the unfused
    attention backward with w < 0, 2w+1 > 16 and dk > 128."""
    from vcvits_amd._lib import lib
    L = lib()
    for name, (n, required, call, dims) in REFUSALS.items():
        for i in required:
            args = [X] * n
            args[i] = None
            assert call(L, args, dims) == EINVAL, "%s: null pointer %d was not refused" % (name, i)
        for j in range(len(dims)):
            for bad in (0, -1):
                d = list(dims)
                d[j] = bad
                assert call(L, [X] * n, d) == EINVAL, "%s: dimension %d = %d was not refused" % (name, j, bad)
    assert L.vcv_split_sample_fwd(X, X, X, X, X, None, 2, 3, 4, None) == EINVAL
    assert L.vcv_split_sample_bwd(X, X, X, X, None, X, X, 2, 3, 4, None) == EINVAL
    for gstride, goff in ((6, -1), (6, 1), (5, 0), (18, 13), (0, 0)):  # H = 3: the slice is goff .. goff + 6
        assert L.vcv_wn_gate_fwd(X, X, gstride, goff, X, 2, 3, 4, None) == EINVAL, (gstride, goff)
        assert L.vcv_wn_gate_bwd(X, X, gstride, goff, X, X, 2, 3, 4, None) == EINVAL, (gstride, goff)
    for p in (-0.1, 1.0, 1.5):
        assert L.vcv_dropout(X, X, 24, p, 1, None) == EINVAL
    a = [X] * 12
    assert L.vcv_rel_softmax_bwd(*a, 2, 2, 8, 9, -1, 1.0, None) == EINVAL
    assert L.vcv_rel_softmax_bwd(*a, 2, 2, 8, 9, 8, 1.0, None) == EINVAL
    assert L.vcv_rel_softmax_bwd(*a, 2, 2, 129, 9, 4, 1.0, None) == EINVAL


@pytest.mark.gpu
def test_refused_calls_leave_their_outputs(gpu):
    """On the device: a refused call leaves every output it was given bit-identical (pre-filled with a pattern), the two tables of
    vcv_rel_softmax_bwd included, which used to be zeroed before the launcher refused 2w+1 > 16 and dk > 128."""
    from vcvits_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(5)
    mk = lambda *s: Guarded(s, gpu, torch.from_numpy(rng.standard_normal(s).astype(np.float32)))
    src = torch.zeros(4096, device=gpu)
    raw = torch.tensor([4, 9], device=gpu, dtype=torch.int64)
    a, b, c2, d = mk(2, 3, 4), mk(2, 6, 4), mk(2, 3, 4), mk(2,)
    big = [mk(17 * 129) for _ in range(2)]
    calls = [
        ("gate_fwd goff", [a], lambda: L.vcv_wn_gate_fwd(ptr(src), ptr(src), 6, 1, ptr(a.t), 2, 3, 4, None)),
        ("gate_bwd goff", [b], lambda: L.vcv_wn_gate_bwd(ptr(src), ptr(src), 18, 13, ptr(src), ptr(b.t), 2, 3, 4, None)),
        ("gate_fwd T<0", [a], lambda: L.vcv_wn_gate_fwd(ptr(src), None, 0, 0, ptr(a.t), 2, 3, -4, None)),
        ("res_skip_fwd no mask", [a, c2], lambda: L.vcv_wn_res_skip_fwd(ptr(src), None, ptr(src), None, ptr(a.t), ptr(c2.t), 2, 3, 4, 0, None)),
        ("split_fwd eps, no z", [a, c2], lambda: L.vcv_split_sample_fwd(ptr(src), ptr(src), ptr(src), ptr(a.t), ptr(c2.t), None, 2, 3, 4, None)),
        ("kl_fwd B<0", [d], lambda: L.vcv_kl_fwd(ptr(src), ptr(src), ptr(src), ptr(src), ptr(src), ptr(d.t), -2, 3, 4, None)),
        ("nearest_bwd Tout 0", [a], lambda: L.vcv_nearest_bwd(ptr(src), ptr(a.t), 6, 4, 0, None)),
        ("nearest_raw_bwd R<0", [a], lambda: L.vcv_nearest_raw_bwd(ptr(src), ptr(a.t), -6, 4, 9, ptr(raw), None)),
        ("slice_bwd T 0", [a], lambda: L.vcv_slice_bwd(ptr(src), ptr(raw), 1, ptr(a.t), 2, 3, 0, 4, None)),
        ("slice_bwd S<0", [a], lambda: L.vcv_slice_bwd(ptr(src), ptr(raw), 1, ptr(a.t), 2, 3, 4, -4, None)),
        ("layernorm_c_bwd_ws C 0", [a, d], lambda: L.vcv_layernorm_c_bwd_ws(ptr(src), None, ptr(src), ptr(src), ptr(src), ptr(src), ptr(a.t), ptr(d.t), ptr(d.t), 2, 0, 4, None, 0, None)),
        ("rel_softmax_bwd 2w+1 = 17", big, lambda: L.vcv_rel_softmax_bwd(*([ptr(src)] * 10), ptr(big[0].t), ptr(big[1].t), 1, 1, 8, 4, 8, 1.0, None)),
        ("rel_softmax_bwd dk = 129", big, lambda: L.vcv_rel_softmax_bwd(*([ptr(src)] * 10), ptr(big[0].t), ptr(big[1].t), 1, 1, 129, 4, 4, 1.0, None)),
        ("rel_softmax_bwd T = 0", big, lambda: L.vcv_rel_softmax_bwd(*([ptr(src)] * 10), ptr(big[0].t), ptr(big[1].t), 1, 1, 8, 0, 4, 1.0, None)),
    ]
    for name, outs, call in calls:
        before = [o.buf.clone() for o in outs]
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.default_stream(gpu)):
            st = call()
        torch.cuda.synchronize()
        assert st == EINVAL, "%s: status %d" % (name, st)
        assert all(torch.equal(bits(o.buf), bits(w)) for o, w in zip(outs, before)), "%s: a refused call wrote to an output" % name
    record("refusals", "%d refused calls (VCV_EINVAL) left their outputs bit-identical, dembk / dembv of vcv_rel_softmax_bwd included" % len(calls))


# ---------------------------------------------------------------------------------------------------------------------
# routing: ops.* gives the bits of the ABI call, and its autograd gradients match the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def _abi_out(gpu, key, kind):
    st, outs, _ = abi(gpu, CASES[key], kind)
    assert st == 0
    return outs


def _same(got, want, what):
    assert torch.equal(bits(got.detach().reshape(want.shape)), bits(want)), "%s: not the ABI call's bits" % what


def _close(got, ref, what):
    e = dist(got.reshape(ref.shape), ref)
    assert e <= TOL, "%s: %.3e from the float64 reference" % (what, e)
    return e


def _leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.gpu
def test_routing_wavenet(gpu):
    """ops.wn_gate (g [B, 6H, 1] at goff = 2H) and ops.wn_res_skip (middle and last layer)."""
    from vcvits_amd import ops
    key, kb = "gate_fwd-B3-H5-T37-g6H+2H", "gate_bwd-B3-H5-T37-g6H+2H"
    t, tb = on_gpu(key, "normal", gpu), on_gpu(kb, "normal", gpu)
    _same(ops.wn_gate(t["xin"], t["g"].unsqueeze(-1), 10), _abi_out(gpu, key, "normal")["acts"], "ops.wn_gate")
    xin, g = _leaf(tb["xin"]), _leaf(tb["g"].unsqueeze(-1))
    dxin, dg = torch.autograd.grad(ops.wn_gate(xin, g, 10), (xin, g), tb["dacts"])
    _same(dxin, _abi_out(gpu, kb, "normal")["dxin"], "ops.wn_gate backward")
    c = inputs(kb, "normal")
    r = V.wn_gate_bwd(c["xin"], c["g"], 10, c["dacts"])
    want = torch.zeros(3, 30, dtype=torch.float64)
    want[:, 10:20] = r.sum(2)
    e1, e2 = _close(dxin.cpu(), r, "dxin"), _close(dg.cpu()[..., 0], want, "dg")
    assert bool((dg.cpu()[:, :10] == 0).all()) and bool((dg.cpu()[:, 20:] == 0).all())
    record("routing", "%-44s ops.wn_gate gives the ABI calls' bits; dxin %.1e, dg %.1e from float64" % (kb, e1, e2))
    for key in ("rs_fwd-B3-H5-T37-last0-out1", "rs_fwd-B3-H5-T37-last1-out1", "rs_fwd-B3-H5-T37-last0-out0"):
        p, t, c = CASES[key].p, on_gpu(key, "exact", gpu), inputs(key, "exact")
        want = _abi_out(gpu, key, "exact")
        x = _leaf(t["x"] if "x" in t else torch.zeros(3, 5, 37, device=gpu))
        out, rs = (_leaf(t["out"]) if p["out"] else None), _leaf(t["rs"])
        mask = t.get("mask", torch.ones(3, 37, device=gpu))
        res = ops.wn_res_skip(x, out, rs, mask, bool(p["last"]))
        rng = np.random.default_rng(11)
        gr = lambda: torch.from_numpy(rng.integers(-8, 9, (3, 5, 37)).astype(np.float32))
        if p["last"]:
            _same(res, want["on"], "ops.wn_res_skip (last)")
            don = gr()
            dout, drs = torch.autograd.grad(res, (out, rs), don.to(gpu))
            assert torch.equal(dout.cpu(), don) and torch.equal(drs.cpu(), don)
        else:
            _same(res[0], want["xn"], "ops.wn_res_skip xn")
            _same(res[1], want["on"], "ops.wn_res_skip on")
            dxn, don = gr(), gr()
            leaves = (x, rs) + ((out,) if p["out"] else ())
            grads = torch.autograd.grad(res, leaves, (dxn.to(gpu), don.to(gpu)))
            drs64, dx64 = V.wn_res_skip_bwd(dxn, don, c["mask"], (3, 5, 37))
            assert torch.equal(grads[0].cpu().double(), dx64) and torch.equal(grads[1].cpu().double(), drs64)
            if p["out"]:
                assert torch.equal(grads[2].cpu(), don)
        record("routing", "%-44s ops.wn_res_skip gives the ABI call's bits and float64's gradients" % key)


@pytest.mark.gpu
def test_routing_split_coupling_prior(gpu):
    from vcvits_amd import ops
    rng = np.random.default_rng(12)
    gr = lambda *s: torch.from_numpy(rng.integers(-8, 9, s).astype(np.float32))
    for key in ("split_fwd-B3-C5-T37-eps0", "split_fwd-B3-C5-T37-eps1"):
        p, t, c = CASES[key].p, on_gpu(key, "exact", gpu), inputs(key, "exact")
        want = _abi_out(gpu, key, "exact")
        stats = _leaf(t["stats"])
        res = ops.posterior_sample(stats, t["eps"], t["mask"]) if p["eps"] else ops.split_stats(stats, t["mask"])
        names = ("z", "m", "logs") if p["eps"] else ("m", "logs")
        for k, v in zip(names, res):
            _same(v, want[k], "ops split %s" % k)
        gs = {k: gr(3, 5, 37) for k in names}
        (dstats,) = torch.autograd.grad(res, (stats,), tuple(gs[k].to(gpu) for k in names))
        logs64 = V.split_sample(c["stats"], None, c["mask"])[1]
        r = V.split_sample_bwd(gs["m"], gs["logs"], gs.get("z"), c.get("eps"), logs64, c["mask"], (3, 5, 37))
        assert torch.equal(dstats.cpu().double(), r), key
        record("routing", "%-44s ops.%s gives the ABI call's bits and float64's gradient" % (key, "posterior_sample" if p["eps"] else "split_stats"))
    for key in ("coupling-B3-C5-T37-forward", "coupling-B3-C5-T37-reverse"):
        p, t, c = CASES[key].p, on_gpu(key, "exact", gpu), inputs(key, "exact")
        x1, m = _leaf(t["x1"]), _leaf(t["m"])
        y = ops.coupling(x1, m, t["mask"], reverse=bool(p["reverse"]))
        _same(y, _abi_out(gpu, key, "exact")["y"], "ops.coupling")
        dy = gr(3, 5, 37)
        dx1, dm = torch.autograd.grad(y, (x1, m), dy.to(gpu))
        x64, m64 = c["x1"].double().requires_grad_(True), c["m"].double().requires_grad_(True)
        V.coupling(x64, m64, c["mask"], p["reverse"]).backward(dy.double())
        assert torch.equal(dx1.cpu().double(), x64.grad) and torch.equal(dm.cpu().double(), m64.grad), key
        record("routing", "%-44s ops.coupling gives the ABI call's bits and float64's gradients" % key)
    key = "prior-B3-C5-T37"
    t = on_gpu(key, "exact", gpu)
    _same(ops.prior_sample(t["m"], t["logs"], t["noise"], 0.5), _abi_out(gpu, key, "exact")["z"], "ops.prior_sample")
    record("routing", "%-44s ops.prior_sample gives the ABI call's bits" % key)


@pytest.mark.gpu
def test_routing_kl_nearest_slice_dropout(gpu):
    from vcvits_amd import ops
    rng = np.random.default_rng(13)
    gr = lambda *s: torch.from_numpy(rng.integers(-8, 9, s).astype(np.float32))
    key = "kl_fwd-n2532-dead-row"
    t, c = on_gpu(key, "normal", gpu), inputs(key, "normal")
    leaves = [_leaf(t[k]) for k in ("zp", "lq", "mp", "lp")]
    loss = ops.kl_loss(*leaves, t["mask"])
    num, den = V.kl(c["zp"], c["lq"], c["mp"], c["lp"], c["mask"])
    e = _close(loss.detach().cpu(), num / den, "ops.kl_loss")
    grads = torch.autograd.grad(loss, leaves, torch.tensor(0.37, device=gpu))
    r = V.kl_bwd(c["zp"], c["mp"], c["lp"], c["mask"], torch.tensor(f32(0.37), dtype=torch.float64), den)
    es = [_close(grads[i].cpu(), r[j], "kl grad %d" % i) for i, j in ((0, 0), (1, 1), (2, 2), (3, 3))]
    record("routing", "%-44s ops.kl_loss %.1e, its gradients %s from float64" % (key, e, " ".join("%.1e" % v for v in es)))
    key = "kl_fwd-n2532"  # exact operands: the two sums are float64's, so the loss is the ABI call's out2[0] / out2[1], bit for bit
    t = on_gpu(key, "exact", gpu)
    want = _abi_out(gpu, key, "exact")["out2"]
    num, den = V.kl(*(inputs(key, "exact")[k] for k in ("zp", "lq", "mp", "lp", "mask")))
    assert torch.equal(want.cpu().double(), torch.stack([num, den]))
    _same(ops.kl_loss(t["zp"], t["lq"], t["mp"], t["lp"], t["mask"]), want[0] / want[1], "ops.kl_loss")
    record("routing", "%-44s ops.kl_loss gives out2[0] / out2[1] of the ABI call, bit for bit" % key)
    for key, kb in (("nearest_fwd-R3-Tin2-Tout82", "nearest_bwd-R3-Tin2-Tout82"), ("raw_fwd-R3-Tin5-Tout100-raw2,82", "raw_bwd-R3-Tin5-Tout100-raw2,82")):
        p, t, tb = CASES[key].p, on_gpu(key, "exact", gpu), on_gpu(kb, "exact", gpu)
        x = _leaf(t["x"].view(1, 3, p["Tin"]))
        y = ops.interpolate_nearest(x, p["Tout"], raw_sizes=t.get("raw"))
        _same(y, _abi_out(gpu, key, "exact")["y"], "ops.interpolate_nearest")
        (dx,) = torch.autograd.grad(y, (x,), tb["dy"].view(1, 3, p["Tout"]))
        _same(dx, _abi_out(gpu, kb, "exact")["dx"], "ops.interpolate_nearest backward")
        assert torch.equal(dx.cpu().double().view(3, -1), reference(kb, "exact")["dx"][0])
        record("routing", "%-44s ops.interpolate_nearest gives the ABI calls' bits and float64's gradient" % key)
    key, kb = "slice_fwd-B5-C2-T700-S300-mul4", "slice_bwd-B5-C2-T700-S300-mul4"
    p, t, tb = CASES[key].p, on_gpu(key, "exact", gpu), on_gpu(kb, "exact", gpu)
    x = _leaf(t["x"])
    y = ops.slice_segments(x, t["ids"], segment_size=p["S"], mul=p["mul"])
    _same(y, _abi_out(gpu, key, "exact")["y"], "ops.slice_segments")
    (dx,) = torch.autograd.grad(y, (x,), tb["dy"])
    _same(dx, _abi_out(gpu, kb, "exact")["dx"], "ops.slice_segments backward")
    assert torch.equal(dx.cpu().double(), reference(kb, "exact")["dx"][0])
    record("routing", "%-44s ops.slice_segments gives the ABI calls' bits and float64's gradient" % key)
    key = "dropout-n1000-p0.1"
    p = CASES[key].p
    got = ops.dropout_mask((10, 100), p["p"], p["seed"], gpu)
    want = V.dropout(torch.ones(1000), f32(p["p"]), p["seed"]).float().view(10, 100)
    assert torch.equal(got.cpu(), want)
    record("routing", "%-44s ops.dropout_mask gives float64's bits" % key)


@pytest.mark.gpu
def test_gate_grad_share(gpu):
    """Three wn_gate calls on one g of width 6H (goff = 0, 2H, 4H) share one GateGradShare(3): g.grad is float64's, bit for bit
    the share=None result, and the object works a second time (the buffer is handed over and reset)."""
    from vcvits_amd import ops
    from vcvits_amd.ops.blocks import GateGradShare
    B, H, T = 3, 5, 37
    rng = np.random.default_rng(14)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    xins, dacts, g0 = [f(B, 2 * H, T) for _ in range(3)], [f(B, H, T) for _ in range(3)], f(B, 6 * H, 1)
    want = torch.cat([V.wn_gate_bwd(xins[l], g0[..., 0], 2 * H * l, dacts[l]).sum(2) for l in range(3)], 1)

    def run(share):
        g = _leaf(g0.to(gpu))
        total = sum((ops.wn_gate(xins[l].to(gpu), g, 2 * H * l, share) * dacts[l].to(gpu)).sum() for l in range(3))
        total.backward()
        return g.grad.detach().clone()

    plain = run(None)
    share = GateGradShare(3)
    first, second = run(share), run(share)
    assert share.buf is None
    assert torch.equal(bits(first), bits(plain)) and torch.equal(bits(second), bits(plain))
    S = torch.cat([V.wn_gate_bwd(xins[l], g0[..., 0], 2 * H * l, dacts[l]).abs().sum(2) for l in range(3)], 1)
    e = dist(plain.cpu()[..., 0], want)
    ratio = ((plain.cpu()[..., 0].double() - want).abs() / (gamma(T + 10 + 6) * S)).max().item()
    record("routing", "%-44s GateGradShare(3): g.grad %.1e from float64 (%.2f of gamma_(T+16) S), the share=None bits, twice" % ("B3-H5-T37-g6H", e, ratio))
    assert e <= TOL

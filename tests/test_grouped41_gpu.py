"""GPU: the grouped k = 41 / stride 4 / padding 20 convolutions of DiscriminatorS (csrc/conv_grouped.hip: nine kernels behind
vcv_grouped41_{fwd,dgrad,wgrad} and their _bf16 forms) at the edges of every launcher's kernel choice, against a float64
CPU reference of the same operation.

The kernels are called THROUGH THE C ABI (vcvits_amd._lib.lib().vcv_grouped41_*), so the shape test in ops/conv.py cannot
send a case to the generic GEMM kernels; test_python_routing then checks that ops.conv_forward / conv_dgrad / conv_wgrad
reach the same kernels (same bits).

Reference: torch.nn.functional.conv1d(stride=4, padding=20, groups=G) on float64 copies of the float32 inputs, float64
autograd of the same expression for dx and dw.  The auxiliary tensor of the fused leaky-ReLU derivative (yaux, the
activation output) is an INPUT of both sides: dye = dy * where(yaux > 0, 1, slope) on the same float32 yaux (a y recomputed
in float64 could flip the derivative where y is within rounding of zero, on one side only).  yaux holds exact +0.0 and -0.0
too: both take the slope.

All distances are max-norm relative to max|reference|.  Bounds: 2e-5 for y and dx (TOL of tests/test_conv_gpu.py), 3e-5
for dw (tests/test_conv_fuzz_gpu.py), 1e-5 for the bf16 forms on operands that are bf16 numbers already (products exact,
only the fp32 summation order differs; TOL_BF16 of tests/test_switch_parity_gpu.py).  With the fused derivative the bf16
kernels round dy * leaky'(yaux) -- an fp32 product -- to bf16 on its way into the matrix cores (pack_bf16x4: a plain
float -> __bf16 conversion, round to nearest even); the reference rounds the same fp32 product the same way.

Every case writes its distances to profiles/grouped41_parity.txt."""
import collections
import contextlib
import functools
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vcvits_amd._lib import ACT_LEAKY, ACT_NONE, TF_DLEAKY, TF_NONE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOPE = 0.1
TOL, TOL_DW, TOL_BF16 = 2e-5, 3e-5, 1e-5
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
CG, K, S, PAD = 4, 41, 4, 20

Shape = collections.namedtuple("Shape", "B G Mg Tin")


def tout(Tin):
    return (Tin + 2 * PAD - K) // S + 1  # == (Tin - 1) // 4 + 1 == ceil(Tin / 4)


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' rules, restated (conv_grouped.hip: vcv_grouped41_fwd, vcv_grouped41_dgrad, grouped41_wgrad_impl)
# ---------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def plan(s, det=False):
    """Which kernel each launcher picks for a shape, and how the weight gradient splits its reduction."""
    B, G, Mg, Tin = s
    To = tout(Tin)
    if Mg == 16:
        # MFMA kernels on 256-time tiles, one group per workgroup.  Weight gradient: units = (batch element, 256-time stage),
        # min(512 / G, nunit) workgroups per group (deterministic mode: one), uper units each.
        nunit = B * cdiv(To, 256)
        wgs = 1 if det else min(max(512 // G, 1), nunit)
        uper = cdiv(nunit, wgs)
        return {"fwd": "fwd_mfma", "dgrad": "dgrad_mfma", "wgrad": "wgrad_mfma", "tiles": cdiv(To, 256), "nunit": nunit,
                "uper": uper, "wgs": cdiv(nunit, uper), "short_last_wg": nunit % uper != 0}
    # 4-channel groups: <4,64> / <4,128> / <4,256> by Tout (forward) and by ceil(Tin / 4) (data gradient) -- the same number;
    # 256 / TT groups share a workgroup, `g0 + gg < G` guards the last one
    nq = cdiv(Tin, 4)
    tt_f = 64 if To <= 64 else 128 if To <= 128 else 256
    tt_d = 64 if nq <= 64 else 128 if nq <= 128 else 256
    # weight gradient: time chunks doubled while the grid is short of 1024 workgroups and a chunk keeps >= 128 times, then
    # rounded up to 128; batch elements per workgroup doubled while the grid keeps >= 1024 workgroups
    nchunk = 1
    while G * B * nchunk < 1024 and To // (nchunk * 2) >= 128:
        nchunk *= 2
    if det:
        nchunk = 1
    tchunk = cdiv(cdiv(To, nchunk), 128) * 128
    bper = 1
    while bper * 2 <= B and G * cdiv(To, tchunk) * (B // (bper * 2)) >= 1024:
        bper *= 2
    if det:
        bper = B
    return {"fwd": "fwd<4,%d>" % tt_f, "dgrad": "dgrad<4,%d>" % tt_d, "wgrad": "wgrad<4>", "tiles": cdiv(To, tt_f),
            "partial_last_wg": G % (256 // tt_f) != 0, "nchunk": nchunk, "tchunk": tchunk, "time_wgs": cdiv(To, tchunk),
            "short_last_chunk": To % tchunk != 0, "bper": bper, "batch_wgs": cdiv(B, bper), "short_last_z": B % bper != 0}


# (shape, what plan() must say of it).  The smallest shapes that reach each branch.
TABLE = [
    # rows shorter than the kernel: almost every tap is padding (Tout = 1, 2, 6, 11; 1, 2)
    (Shape(3, 4, 4, 1), {"fwd": "fwd<4,64>", "dgrad": "dgrad<4,64>"}),
    (Shape(3, 4, 4, 5), {"fwd": "fwd<4,64>"}),
    (Shape(2, 4, 4, 21), {"fwd": "fwd<4,64>"}),
    (Shape(2, 4, 4, 43), {"fwd": "fwd<4,64>"}),
    (Shape(2, 64, 16, 1), {"fwd": "fwd_mfma", "dgrad": "dgrad_mfma", "wgrad": "wgrad_mfma"}),
    (Shape(2, 64, 16, 7), {"fwd": "fwd_mfma"}),
    # <4,64>: four groups per workgroup, the last workgroup half empty (G = 6), Tout = 64 exactly
    (Shape(2, 6, 4, 253), {"fwd": "fwd<4,64>", "dgrad": "dgrad<4,64>", "partial_last_wg": True, "tiles": 1}),
    (Shape(2, 6, 4, 256), {"fwd": "fwd<4,64>", "dgrad": "dgrad<4,64>", "partial_last_wg": True, "tiles": 1}),
    # <4,128>: two groups per workgroup, odd G, Tout = 65 / 128 / 128
    (Shape(2, 3, 4, 257), {"fwd": "fwd<4,128>", "dgrad": "dgrad<4,128>", "partial_last_wg": True, "tiles": 1}),
    (Shape(1, 3, 4, 511), {"fwd": "fwd<4,128>", "dgrad": "dgrad<4,128>", "partial_last_wg": True, "tiles": 1}),
    (Shape(2, 2, 4, 512), {"fwd": "fwd<4,128>", "dgrad": "dgrad<4,128>", "partial_last_wg": False, "tiles": 1}),
    # <4,256>: Tout = 129, and Tout = 258 = a full tile and a ragged second one
    (Shape(2, 2, 4, 513), {"fwd": "fwd<4,256>", "dgrad": "dgrad<4,256>", "tiles": 1}),
    (Shape(1, 2, 4, 1030), {"fwd": "fwd<4,256>", "dgrad": "dgrad<4,256>", "tiles": 2}),
    # MFMA kernels: Tout = 256 / 256 / 257 / 257 / 513 / 65; Tin mod 4 = 1, 0, 1, 2, 3, 3 (the data gradient stores 16 bytes
    # per lane only when Tin mod 4 == 0; Tin = 1026 is not in the issue's list -- without it no 16-channel case has residue 2)
    (Shape(2, 4, 16, 1021), {"fwd": "fwd_mfma", "tiles": 1}),
    (Shape(2, 4, 16, 1024), {"fwd": "fwd_mfma", "tiles": 1}),
    (Shape(1, 4, 16, 1025), {"fwd": "fwd_mfma", "tiles": 2}),
    (Shape(1, 4, 16, 1026), {"fwd": "fwd_mfma", "tiles": 2}),
    (Shape(1, 16, 16, 2051), {"fwd": "fwd_mfma", "tiles": 3, "nunit": 3, "wgs": 3}),
    (Shape(2, 16, 16, 259), {"fwd": "fwd_mfma", "tiles": 1}),
    # Mg == 16 weight gradient: 3 units over 2 workgroups (2 + 1); 6 units, one each; 6 units over 3 workgroups
    (Shape(3, 256, 16, 200), {"wgrad": "wgrad_mfma", "nunit": 3, "uper": 2, "wgs": 2, "short_last_wg": True}),
    (Shape(2, 4, 16, 2400), {"wgrad": "wgrad_mfma", "nunit": 6, "uper": 1, "wgs": 6, "short_last_wg": False}),
    (Shape(3, 128, 16, 1500), {"wgrad": "wgrad_mfma", "nunit": 6, "uper": 2, "wgs": 3, "short_last_wg": False}),
    # Mg == 4 weight gradient: nchunk = 4 -> 150 times per chunk, rounded up to 256: the grid has 3 time chunks of 256, 256 and
    # 88 times; bper = 2 with B = 9 (five z-blocks, the last with one element); bper = 4
    (Shape(2, 8, 4, 2400), {"wgrad": "wgrad<4>", "nchunk": 4, "tchunk": 256, "time_wgs": 3, "short_last_chunk": True, "bper": 1}),
    (Shape(9, 256, 4, 132), {"wgrad": "wgrad<4>", "nchunk": 1, "bper": 2, "batch_wgs": 5, "short_last_z": True}),
    (Shape(16, 256, 4, 129), {"wgrad": "wgrad<4>", "nchunk": 1, "bper": 4, "batch_wgs": 4, "short_last_z": False}),
    # the layers' own shapes on a pooled scale
    (Shape(2, 256, 4, 129), {"fwd": "fwd<4,64>", "wgrad": "wgrad<4>"}),
    (Shape(2, 64, 16, 513), {"fwd": "fwd_mfma", "wgrad": "wgrad_mfma"}),
]
SHAPES = [s for s, _ in TABLE]
SHAPES_16 = [s for s in SHAPES if s.Mg == 16]
# the weight-gradient rows of the table, for the deterministic-mode check
WGRAD_SPLIT_SHAPES = [Shape(3, 256, 16, 200), Shape(2, 4, 16, 2400), Shape(3, 128, 16, 1500),
                      Shape(2, 8, 4, 2400), Shape(9, 256, 4, 132), Shape(16, 256, 4, 129)]


def sid(s):
    return "B%d-G%d-Mg%d-T%d" % tuple(s)


def test_case_table_reaches_every_branch():
    """The table above against the launchers' rules as plan() restates them, and the branches the file claims to cover."""
    for s, want in TABLE:
        got = plan(s)
        assert {k: got.get(k) for k in want} == want, (s, want, got)
    seen = collections.Counter()
    for s in SHAPES:
        p = plan(s)
        seen.update((p["fwd"], p["dgrad"], p["wgrad"]))
        if s.Mg == 4:
            seen.update(["nchunk>1"] * (p["nchunk"] > 1) + ["bper>1"] * (p["bper"] > 1))
            seen.update(["partial_last_wg"] * p["partial_last_wg"] + ["short_last_z"] * p["short_last_z"])
        else:
            seen.update(["short_last_wg"] * p["short_last_wg"])
    for branch in ("fwd<4,64>", "fwd<4,128>", "fwd<4,256>", "dgrad<4,64>", "dgrad<4,128>", "dgrad<4,256>", "wgrad<4>",
                   "fwd_mfma", "dgrad_mfma", "wgrad_mfma", "nchunk>1", "bper>1", "partial_last_wg", "short_last_z", "short_last_wg"):
        assert seen[branch] > 0, branch
    assert {s.Tin % 4 for s in SHAPES if s.Mg == 4} == {0, 1, 2, 3} and {s.Tin % 4 for s in SHAPES_16} == {0, 1, 2, 3}
    # deterministic mode: one workgroup per group, whatever the shape
    for s in WGRAD_SPLIT_SHAPES:
        p = plan(s, det=True)
        assert p["wgs"] == 1 if s.Mg == 16 else (p["time_wgs"], p["batch_wgs"]) == (1, 1), (s, p)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and float64 references: made once per shape and shared by every test
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(s, rounded=False):
    """x, w, bias, dy, yaux, dw0 (float32, CPU).  rounded: x, w and dy are bf16 numbers (the bias is added in fp32 and yaux is
    only compared with zero: neither goes through the matrix cores)."""
    B, G, Mg, Tin = s
    rng = np.random.default_rng(zlib.crc32(repr(tuple(s)).encode()))
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    x, w, b = t(B, G * CG, Tin), t(G * Mg, CG, K) * (CG * K) ** -0.5, t(G * Mg) * 0.5
    dy, yaux, dw0 = t(B, G * Mg, tout(Tin)), t(B, G * Mg, tout(Tin)), t(G * Mg, CG, K)
    flat = yaux.view(-1)
    flat[0::7] = 0.0   # leaky'(+0) and leaky'(-0) are the slope (aux > 0 ? 1 : slope)
    flat[3::7] = -0.0
    if rounded:
        x, w, dy = (v.bfloat16().float() for v in (x, w, dy))
    return x, w, b, dy, yaux, dw0


def dleaky(yaux):
    return torch.where(yaux > 0, 1.0, SLOPE)


@functools.lru_cache(maxsize=None)
def reference(s, rounded=False):
    """float64: the convolution without bias (`pre`), and dx / dw for dye = dy (TF_NONE) and dye = dy * leaky'(yaux)
    (TF_DLEAKY).  rounded: the bf16 kernels' arithmetic -- operands that are bf16 numbers, and the fp32 product dy * leaky'(yaux)
    rounded to bf16 (nearest even) before it is used."""
    x, w, _, dy, yaux, _ = inputs(s, rounded)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    pre = F.conv1d(xd, wd, None, stride=S, padding=PAD, groups=s.G)
    out = {"pre": pre.detach()}
    for dtf in (TF_NONE, TF_DLEAKY):
        if dtf == TF_NONE:
            dye = dy.double()
        elif rounded:
            dye = (dy * dleaky(yaux).float()).bfloat16().double()
        else:
            dye = dy.double() * dleaky(yaux).double()
        out["dx", dtf], out["dw", dtf] = torch.autograd.grad(pre, (xd, wd), dye, retain_graph=True)
    return out


def ref_forward(s, act, bias, rounded=False):
    y = reference(s, rounded)["pre"]
    if bias:
        y = y + inputs(s, rounded)[2].double().view(1, -1, 1)
    return F.leaky_relu(y, SLOPE) if act == ACT_LEAKY else y


@functools.lru_cache(maxsize=2)
def on_gpu(s, rounded, gpu):
    return tuple(v.to(gpu) for v in inputs(s, rounded))


def rel(got, ref):
    return (got.detach().cpu().double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# the six entry points, called directly
# ---------------------------------------------------------------------------------------------------------------------
def abi_fwd(s, x, w, b, act, bf=False, out=None):
    from vcvits_amd._lib import lib, ptr, stream
    B, G, Mg, Tin = s
    y = torch.full((B, G * Mg, tout(Tin)), float("nan"), device=x.device) if out is None else out  # (an element left unwritten stays NaN)
    fn = lib().vcv_grouped41_fwd_bf16 if bf else lib().vcv_grouped41_fwd
    return fn(ptr(x), ptr(w), ptr(b), ptr(y), B, G, Mg, Tin, tout(Tin), act, SLOPE, stream()), y


def abi_dgrad(s, dy, yaux, w, dtf, bf=False, out=None):
    from vcvits_amd._lib import lib, ptr, stream
    B, G, Mg, Tin = s
    dx = torch.full((B, G * CG, Tin), float("nan"), device=dy.device) if out is None else out
    fn = lib().vcv_grouped41_dgrad_bf16 if bf else lib().vcv_grouped41_dgrad
    return fn(ptr(dy), ptr(yaux), ptr(w), ptr(dx), B, G, Mg, Tin, tout(Tin), dtf, SLOPE, stream()), dx


def abi_wgrad(s, dy, yaux, x, dw, dtf, bf=False):
    """Accumulates onto dw."""
    from vcvits_amd._lib import lib, ptr, stream
    B, G, Mg, Tin = s
    fn = lib().vcv_grouped41_wgrad_bf16 if bf else lib().vcv_grouped41_wgrad
    return fn(ptr(dy), ptr(yaux), ptr(x), ptr(dw), B, G, Mg, Tin, tout(Tin), dtf, SLOPE, stream()), dw


def aux_of(dtf, yaux):
    return yaux if dtf == TF_DLEAKY else None


@contextlib.contextmanager
def deterministic(on=True):
    from vcvits_amd import ops
    old = ops._DETERMINISTIC[0]
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(old)


@contextlib.contextmanager
def fp32_mode():
    from vcvits_amd import ops
    old = ops.compute_dtype()
    ops.set_compute_dtype("f32")
    try:
        yield
    finally:
        ops.set_compute_dtype(old)


_parity = {}


def record(section, line):
    """Keep the measured distances in profiles/grouped41_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "grouped41_parity.txt"), "w") as f:
        f.write("# tests/test_grouped41_gpu.py: max-norm distance of the vcv_grouped41_* entry points from the float64 CPU reference,\n"
                "# relative to max|reference|.  Cases are B-G-Mg-Tin.\n")
        for name in _parity:
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def check(section, tag, errs, tol):
    """Write the figures down first, then assert."""
    record(section, "%-58s %s" % (tag, " ".join("%s=%.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e <= tol, "%s %s: %s off by %.3e (bound %.1e)" % (section, tag, k, e, tol)


ACTS = [(ACT_NONE, "none"), (ACT_LEAKY, "leaky")]
DTFS = [(TF_NONE, "none"), (TF_DLEAKY, "dleaky")]
ids2 = lambda p: p[1]


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward, fp32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS, ids=ids2)
@pytest.mark.parametrize("s", SHAPES, ids=sid)
def test_forward_fp32(gpu, s, act):
    x, w, b, _, _, _ = on_gpu(s, False, gpu)
    errs = {}
    for bias in (True, False):
        st, y = abi_fwd(s, x, w, b if bias else None, act[0])
        assert st == 0, st
        errs["bias" if bias else "nobias"] = rel(y, ref_forward(s, act[0], bias))
    check("forward fp32", "%s %s act=%s" % (sid(s), plan(s)["fwd"], act[1]), errs, TOL)


# ---------------------------------------------------------------------------------------------------------------------
# 2. data gradient, fp32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtf", DTFS, ids=ids2)
@pytest.mark.parametrize("s", SHAPES, ids=sid)
def test_dgrad_fp32(gpu, s, dtf):
    _, w, _, dy, yaux, _ = on_gpu(s, False, gpu)
    st, dx = abi_dgrad(s, dy, aux_of(dtf[0], yaux), w, dtf[0])  # (dx starts as NaN: the kernel overwrites)
    assert st == 0, st
    assert bool(torch.isfinite(dx).all()), "dx has elements the kernel did not write"
    check("data gradient fp32", "%s %s dtf=%s" % (sid(s), plan(s)["dgrad"], dtf[1]), {"dx": rel(dx, reference(s)["dx", dtf[0]])}, TOL)


# ---------------------------------------------------------------------------------------------------------------------
# 3. weight gradient, fp32, default (atomic) mode: onto zeros, and onto an existing gradient
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad_tag(s, det=False):
    p = plan(s, det)
    if s.Mg == 16:
        return "%s %s units=%d wgs=%d" % (sid(s), p["wgrad"], p["nunit"], p["wgs"])
    return "%s %s chunks=%d bper=%d z=%d" % (sid(s), p["wgrad"], p["time_wgs"], p["bper"], p["batch_wgs"])


@pytest.mark.parametrize("dtf", DTFS, ids=ids2)
@pytest.mark.parametrize("s", SHAPES, ids=sid)
def test_wgrad_fp32_atomic(gpu, s, dtf):
    from vcvits_amd._lib import lib
    assert lib().vcv_get_deterministic() == 0
    x, _, _, dy, yaux, dw0 = on_gpu(s, False, gpu)
    ref = reference(s)["dw", dtf[0]]
    st, dw = abi_wgrad(s, dy, aux_of(dtf[0], yaux), x, torch.zeros_like(dw0), dtf[0])
    assert st == 0, st
    st, acc = abi_wgrad(s, dy, aux_of(dtf[0], yaux), x, dw0.clone(), dtf[0])
    assert st == 0, st
    # onto an existing gradient: old value + gradient, the distance still relative to max|gradient|
    old = inputs(s)[5].double()
    onto = (acc.cpu().double() - (old + ref)).abs().max().item() / ref.abs().max().item()
    check("weight gradient fp32, atomics", "%s dtf=%s" % (_wgrad_tag(s), dtf[1]), {"dw": rel(dw, ref), "onto": onto}, TOL_DW)


# ---------------------------------------------------------------------------------------------------------------------
# 4. weight gradient, deterministic mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtf", DTFS, ids=ids2)
@pytest.mark.parametrize("s", WGRAD_SPLIT_SHAPES, ids=sid)
def test_wgrad_fp32_deterministic(gpu, s, dtf):
    from vcvits_amd._lib import lib
    x, _, _, dy, yaux, dw0 = on_gpu(s, False, gpu)
    with deterministic():
        assert lib().vcv_get_deterministic() == 1
        st1, a = abi_wgrad(s, dy, aux_of(dtf[0], yaux), x, torch.zeros_like(dw0), dtf[0])
        st2, b = abi_wgrad(s, dy, aux_of(dtf[0], yaux), x, torch.zeros_like(dw0), dtf[0])
    assert lib().vcv_get_deterministic() == 0
    assert st1 == 0 and st2 == 0
    check("weight gradient fp32, deterministic", "%s dtf=%s" % (_wgrad_tag(s, True), dtf[1]),
          {"dw": rel(a, reference(s)["dw", dtf[0]])}, TOL_DW)
    assert torch.equal(a, b), "two identical deterministic launches differ"


# ---------------------------------------------------------------------------------------------------------------------
# 5. bf16 forms (Mg == 16), called directly: no compute-dtype switch involved
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS, ids=ids2)
@pytest.mark.parametrize("s", SHAPES_16, ids=sid)
def test_forward_bf16(gpu, s, act):
    x, w, b, _, _, _ = on_gpu(s, True, gpu)
    errs = {}
    for bias in (True, False):
        st, y = abi_fwd(s, x, w, b if bias else None, act[0], bf=True)
        assert st == 0, st
        errs["bias" if bias else "nobias"] = rel(y, ref_forward(s, act[0], bias, True))
    check("forward bf16", "%s act=%s" % (sid(s), act[1]), errs, TOL_BF16)


@pytest.mark.parametrize("dtf", DTFS, ids=ids2)
@pytest.mark.parametrize("s", SHAPES_16, ids=sid)
def test_dgrad_bf16(gpu, s, dtf):
    _, w, _, dy, yaux, _ = on_gpu(s, True, gpu)
    st, dx = abi_dgrad(s, dy, aux_of(dtf[0], yaux), w, dtf[0], bf=True)
    assert st == 0, st
    assert bool(torch.isfinite(dx).all()), "dx has elements the kernel did not write"
    check("data gradient bf16", "%s dtf=%s" % (sid(s), dtf[1]), {"dx": rel(dx, reference(s, True)["dx", dtf[0]])}, TOL_BF16)


@pytest.mark.parametrize("dtf", DTFS, ids=ids2)
@pytest.mark.parametrize("s", SHAPES_16, ids=sid)
def test_wgrad_bf16(gpu, s, dtf):
    x, _, _, dy, yaux, dw0 = on_gpu(s, True, gpu)
    ref = reference(s, True)["dw", dtf[0]]
    st, dw = abi_wgrad(s, dy, aux_of(dtf[0], yaux), x, torch.zeros_like(dw0), dtf[0], bf=True)
    assert st == 0, st
    check("weight gradient bf16, atomics", "%s dtf=%s" % (_wgrad_tag(s), dtf[1]), {"dw": rel(dw, ref)}, TOL_BF16)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals: VCV_EINVAL, nothing launched, the output untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    # buffers large enough for any group width tried here, so that a launch that should not happen stays in bounds
    B, G, Tin, MGMAX = 2, 4, 64, 32
    To = tout(Tin)
    g0 = torch.Generator().manual_seed(6)
    x = torch.randn(B, G * CG, Tin, generator=g0).to(gpu)
    w = torch.randn(G * MGMAX, CG, K, generator=g0).to(gpu)
    b = torch.randn(G * MGMAX, generator=g0).to(gpu)
    dy = torch.randn(B, G * MGMAX, To, generator=g0).to(gpu)
    yaux = torch.randn(B, G * MGMAX, To, generator=g0).to(gpu)
    mark = 12345.0
    y, dx, dw = (torch.full(sh, mark, device=gpu) for sh in ((B, G * MGMAX, To), (B, G * CG, Tin), (G * MGMAX, CG, K)))
    tried = []

    def refused(what, st, out):
        torch.cuda.synchronize()
        tried.append(what)
        assert st == EINVAL, "%s returned %d" % (what, st)
        assert bool((out == mark).all()), "%s wrote to its output" % what

    for bf in (False, True):
        for Mg in ((4, 8, 1, 32, 0) if bf else (8, 1, 2, 32, 0)):
            s = Shape(B, G, Mg, Tin)
            refused("fwd bf=%d Mg=%d" % (bf, Mg), abi_fwd(s, x, w, b, ACT_NONE, bf, out=y)[0], y)
            refused("dgrad bf=%d Mg=%d" % (bf, Mg), abi_dgrad(s, dy, None, w, TF_NONE, bf, out=dx)[0], dx)
            refused("wgrad bf=%d Mg=%d" % (bf, Mg), abi_wgrad(s, dy, None, x, dw, TF_NONE, bf)[0], dw)
        for Mg in ((16,) if bf else (4, 16)):
            s = Shape(B, G, Mg, Tin)
            for dtf in (1, 3, 4, 5, 6, -1):  # TF_LEAKY, TF_DRELU, TF_DTANH, TF_DLOGCLAMP, out of range
                refused("dgrad bf=%d Mg=%d dtf=%d" % (bf, Mg, dtf), abi_dgrad(s, dy, yaux, w, dtf, bf, out=dx)[0], dx)
                refused("wgrad bf=%d Mg=%d dtf=%d" % (bf, Mg, dtf), abi_wgrad(s, dy, yaux, x, dw, dtf, bf)[0], dw)
            refused("dgrad bf=%d Mg=%d DLEAKY without yaux" % (bf, Mg), abi_dgrad(s, dy, None, w, TF_DLEAKY, bf, out=dx)[0], dx)
            refused("wgrad bf=%d Mg=%d DLEAKY without yaux" % (bf, Mg), abi_wgrad(s, dy, None, x, dw, TF_DLEAKY, bf)[0], dw)
    # the same buffers are accepted with a supported group width (the refusals above are not a broken call)
    s = Shape(B, G, 16, Tin)
    for bf in (False, True):
        assert abi_fwd(s, x, w, b, ACT_NONE, bf, out=y)[0] == 0
        assert abi_dgrad(s, dy, yaux, w, TF_DLEAKY, bf, out=dx)[0] == 0
        assert abi_wgrad(s, dy, yaux, x, dw, TF_DLEAKY, bf)[0] == 0
    torch.cuda.synchronize()
    assert not bool((y.view(-1)[:B * G * 16 * To] == mark).any()) and not bool((dx == mark).any())
    record("refusals", "%d calls refused with VCV_EINVAL, outputs untouched" % len(tried))


# ---------------------------------------------------------------------------------------------------------------------
# 7. routing: ops.conv_forward / conv_dgrad / conv_wgrad reach these kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [Shape(2, 6, 4, 253), Shape(2, 16, 16, 259)], ids=sid)
def test_python_routing(gpu, s):
    """The bits of the direct ABI call: a launch that the shape test of ops/conv.py sent to the generic kernels instead would
    sum in another order (and move a LAUNCH_COUNTS entry; the grouped-41 launches move none)."""
    from vcvits_amd import ops
    x, w, b, dy, yaux, dw0 = on_gpu(s, False, gpu)
    B, G, Mg, Tin = s
    kw = dict(stride=S, pad=PAD, groups=G)
    with fp32_mode():
        before = dict(ops.LAUNCH_COUNTS)
        for act in (ACT_NONE, ACT_LEAKY):
            for bias in (b, None):
                y = ops.conv_forward(x, w, bias, out_act=act, slope=SLOPE, **kw)
                assert torch.equal(y, abi_fwd(s, x, w, bias, act)[1]), "conv_forward: not vcv_grouped41_fwd's bits"
        dx = ops.conv_dgrad(dy, w, tuple(x.shape), **kw)
        assert torch.equal(dx, abi_dgrad(s, dy, None, w, TF_NONE)[1]), "conv_dgrad: not vcv_grouped41_dgrad's bits"
        dx = ops.conv_dgrad(dy, w, tuple(x.shape), in_tf=TF_DLEAKY, xaux=yaux, slope=SLOPE, **kw)
        assert torch.equal(dx, abi_dgrad(s, dy, yaux, w, TF_DLEAKY)[1]), "conv_dgrad(DLEAKY): not vcv_grouped41_dgrad's bits"
        errs = {}
        for dtf, name in DTFS:
            aux = aux_of(dtf, yaux)
            with deterministic():
                dw = ops.conv_wgrad(dy, x, tuple(w.shape), a_tf=dtf, aaux=aux, slope=SLOPE, **kw)
                direct = abi_wgrad(s, dy, aux, x, torch.zeros_like(dw0), dtf)[1]
            assert torch.equal(dw, direct), "conv_wgrad (deterministic): not vcv_grouped41_wgrad's bits"
            dw = ops.conv_wgrad(dy, x, tuple(w.shape), a_tf=dtf, aaux=aux, slope=SLOPE, **kw)
            errs["dw_" + name] = rel(dw, reference(s)["dw", dtf])
            acc = ops.conv_wgrad(dy, x, tuple(w.shape), out=dw0.clone(), a_tf=dtf, aaux=aux, slope=SLOPE, **kw)
            errs["onto_" + name] = rel(acc.cpu().double() - inputs(s)[5].double(), reference(s)["dw", dtf])
        assert dict(ops.LAUNCH_COUNTS) == before, "a launch went to the generic conv / weight-gradient kernels"
    check("routing through ops", sid(s), errs, TOL_DW)

"""GPU: every kernel path that a SWITCH selects -- deterministic mode (ops.set_deterministic / VCVITS_DETERMINISTIC=1) and the
non-default values of the kernel tuning table (csrc/tuning.h, VCVITS_TUNING=) -- against a plain float64 CPU reference of
the same operation.  The rest of the suite checks the default path; tests/test_determinism_gpu.py only checks that
deterministic mode repeats its bits, which a reproducible but wrong result passes.

References: torch CPU conv1d / conv2d / conv_transpose1d on .double() operands with CPU autograd (bf16 mode: the float64
convolution of the bf16-ROUNDED operands, as tests/test_bf16_gpu.py rounds them), float64 restatements of LayerNorm and
of the relative-position attention, torch.stft in float64.  Tolerances are the ones the default-path test of the same op
uses against the same kind of reference, never wider: 2e-5 max-norm for fp32 conv outputs and gradients
(test_conv_gpu.py), 3e-5 for dw (test_conv_fuzz_gpu.py), 1e-5 on bf16-rounded operands (test_bf16_gpu.py), and the
LayerNorm / STFT / attention / ResBlock-pair files' own bounds.  Every case writes its distance, and the distance of the
default setting on the same inputs, to profiles/switch_parity.txt.

Where two settings are the same arithmetic the results are also compared bit for bit (y and dx; weight and bias
gradients meet in fp32 atomics in the default mode, so their bits vary from run to run whatever the switch):
  xcd_remap, pk_vec   block -> tile mapping / epilogue store width: always the same plan, always bit-equal;
  pk_x4, pk_ws        the staging width and the producer-wave twins can change the channel chunk (BKC) or the split of the
                      reduction (ks), which is a different summation order: bit-equal whenever vcv_conv_pk_plan reports the
                      same (scratch, pack signature) for both settings, which the test reads through a spy;
  pack_tile(_bf16)    the batched re-pack of cached weights gives the bits of the per-launch pack;
  act_grad_vec        float4 vs scalar activation-derivative pass: y / dx / the masked gradient bit-equal (the bias sum
                      inside vcv_act_grad_bias has another order);
  m1_lds              NOT compared bit for bit: short rows reduce R channel sub-rows through LDS and deep channel ranges
                      are split over workgroups that meet in atomics -- neither order is the register kernel's;
  zero_memset         NOT compared bit for bit: what it zeroes is then filled by atomics.

Keys of csrc/tuning.h and where they are exercised here:
  deterministic                               sections 1 and 2 (op level, whole step)
  xcd_remap pk_ws pk_x4 pk_vec                test_pk_switch (and xcd_remap / pk_vec again in test_x3_switch)
  pk_ws_bf16 wgrad_bf16_ws wgrad_finish_vec   test_bf16_switch
  x3_variant x3_v6 x3_js2 x3_old_ks x3_terms  test_x3_forced_variant / test_x3_switch
  x3_all                                      set by ops.set_f32_split(all_shapes=True) in every x3 case here
  wgrad_dma wgrad_tile bias_rows zero_memset  test_wgrad_register_staged / test_wgrad_forced_tile / test_bias_rows_off / test_zero_memset
  c1_chunk m1_lds c1_wgrad_pairs thin_wgrad_wgs act_grad_vec   the thin / streaming tests
  ln_regs stft_wave attn_rows pair_stream     their own tests at the end
  pack_tile pack_tile_bf16                    test_pack_tile_replay
  wgrad_verbose                               diagnostic print; used by test_wgrad_forced_tile to prove which tile ran
  pair_dbg                                    debug output of the fused pair kernel, no arithmetic
  pair_grid                                   tests/test_resblock_pair_gpu.py::test_persistent_workgroups_walk_many_tiles
"""
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

from vcvits_amd import tuning
from vcvits_amd._lib import ACT_LEAKY, ACT_NONE, ACT_TANH, TF_DLEAKY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOPE = 0.1
TOL, TOL_DW, TOL_BF16 = 2e-5, 3e-5, 1e-5
F32_TOLS = {"y": TOL, "dx": TOL, "dw": TOL_DW, "db": TOL}
BF16_TOLS = {"y": TOL_BF16, "dx": TOL_BF16, "dw": TOL_BF16, "db": TOL_BF16}


def _read_state():
    from vcvits_amd import ops
    from vcvits_amd._lib import lib
    keys = {k: tuning.kernel_get(k) for k in tuning.KERNEL_KEYS}
    return keys, {"compute": ops.compute_dtype(), "x3": ops._USE_X3[0], "x3_wgrad": ops._USE_X3_WGRAD[0],
                  "deterministic": ops._DETERMINISTIC[0], "lib_deterministic": lib().vcv_get_deterministic(),
                  "attn_fused": ops._ATTN_FUSED[0]}


try:  # the values at import: the last test of the file compares every switch with them
    KEYS_AT_IMPORT, STATE_AT_IMPORT = _read_state()
except Exception:  # noqa: BLE001  (collected on a machine where the library is not built: the GPU tests do not run there)
    KEYS_AT_IMPORT = STATE_AT_IMPORT = None


# ---------------------------------------------------------------------------------------------------------------------
# 0. helpers
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switched(key, value):
    """One key of the kernel tuning table at `value`; the old value comes back whatever happens inside."""
    old = tuning.kernel_get(key)
    tuning.kernel_set(key, value)
    try:
        yield
    finally:
        tuning.kernel_set(key, old)


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
def compute_dtype(name):
    from vcvits_amd import ops
    old = ops.compute_dtype()
    ops.set_compute_dtype(name)
    try:
        yield
    finally:
        ops.set_compute_dtype(old)


@contextlib.contextmanager
def f32_split(on, terms=None, all_shapes=None, wgrad=None):
    from vcvits_amd import ops
    from vcvits_amd._lib import lib
    old = (ops._USE_X3[0], lib().vcv_conv_x3_get_terms(), lib().vcv_conv_x3_get_all(), ops._USE_X3_WGRAD[0])
    ops.set_f32_split(on, terms=terms, all_shapes=all_shapes, wgrad=wgrad)
    try:
        yield
    finally:
        ops.set_f32_split(old[0], terms=old[1], all_shapes=bool(old[2]), wgrad=old[3])


@contextlib.contextmanager
def x3_variant(variant, js=-1, ks=-1):
    from vcvits_amd._lib import lib
    lib().vcv_conv_x3_set_variant(variant, js, ks)
    try:
        yield
    finally:
        lib().vcv_conv_x3_set_variant(-1, -1, -1)


@contextlib.contextmanager
def wgrad_bf16_force(cand, z=-1):
    from vcvits_amd._lib import lib
    lib().vcv_wgrad_bf16_set_force(cand, z)
    try:
        yield
    finally:
        lib().vcv_wgrad_bf16_set_force(-1, -1)


@contextlib.contextmanager
def wgrad_spy():
    """Which kernel every weight-gradient launch of the MFMA families went to: a list of dicts with `to` = "x3" / "bf16"
    (LAUNCH_COUNTS) or "dma" / "reg" (vcv_conv_wgrad_takes_dma), the group count and whether a slab was handed over.
    The thin and grouped-41 weight gradients never reach ops.conv._launch_wgrad: for them the list stays empty."""
    from vcvits_amd import ops
    from vcvits_amd._lib import lib
    seen = []
    orig = ops.conv._launch_wgrad

    def spy(a):
        dma = lib().vcv_conv_wgrad_takes_dma(ctypes.byref(a))
        before = dict(ops.LAUNCH_COUNTS)
        orig(a)
        to = "x3" if ops.LAUNCH_COUNTS["wgrad_x3"] != before["wgrad_x3"] else \
             "bf16" if ops.LAUNCH_COUNTS["wgrad_bf16"] != before["wgrad_bf16"] else ("dma" if dma else "reg")
        seen.append({"to": to, "G": a.G, "s": a.s, "P": a.P, "slab": bool(a.slab)})

    ops.replace("_launch_wgrad", spy)
    try:
        yield seen
    finally:
        ops.replace("_launch_wgrad", orig)


@contextlib.contextmanager
def conv_spy():
    """(x3 plan, pk plan) of every forward-type launch: (pack words, scratch floats, layout signature) or None where the family
    declines.  Two settings with equal lists run the same tiles, channel chunks and reduction splits."""
    from vcvits_amd import ops
    from vcvits_amd._lib import lib
    seen = []
    orig = ops.conv._launch_conv

    def spy(a, flip_w=None, wt=None):
        rec = []
        for fn in (lib().vcv_conv_x3_plan, lib().vcv_conv_pk_plan):
            plan = (ctypes.c_int64 * 3)()
            rec.append(tuple(plan) if fn(ctypes.byref(a), 1 if flip_w is not None else 0, plan) == 0 else None)
        seen.append(tuple(rec))
        return orig(a, flip_w=flip_w, wt=wt)

    ops.replace("_launch_conv", spy)
    try:
        yield seen
    finally:
        ops.replace("_launch_conv", orig)


_parity = {}


def record(section, line):
    """Keep the measured distances in profiles/switch_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "switch_parity.txt"), "w") as f:
        f.write("# tests/test_switch_parity_gpu.py: max-norm distance from the float64 CPU reference, relative to max|reference|,\n"
                "# of the switched / deterministic path and -- after the bar -- of the library's default setting on the same inputs.\n")
        for name in sorted(_parity):
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def fmt(errs):
    return " ".join("%s=%.2e" % kv for kv in errs.items())


def rel(got, ref):
    ref = ref.double()
    return (got.detach().cpu().double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


def check(section, tag, errs, tols, base=None):
    record(section, "%-58s %s%s" % (tag, fmt(errs), "" if base is None else "  |  " + fmt(base)))
    for k, e in errs.items():
        assert e <= tols[k], "%s %s: %s off by %.3e (bound %.1e)" % (section, tag, k, e, tols[k])


# ---- conv cases: inputs, float64 reference (computed once per case and shared), the GPU run ---------------------------------
Case = collections.namedtuple("Case", "kind B C M T K s p d g P in_leaky act bias res")


def conv(B, C, M, T, K, s, p, d, g, P=1, in_leaky=False, act=ACT_NONE, bias=True, res=False):
    return Case("conv", B, C, M, T, K, s, p, d, g, P, in_leaky, act, bias, res)


def convT(B, C, M, T, K, s, p, in_leaky=True, bias=True):
    return Case("convT", B, C, M, T, K, s, p, 1, 1, 1, in_leaky, ACT_NONE, bias, False)


def cid(c):
    s = "%s-B%d-C%d-M%d-T%d-K%d-s%d-p%d-d%d-g%d" % tuple(c[:10])
    if c.P > 1:
        s += "-P%d" % c.P
    return s + ("-inleaky" if c.in_leaky and c.kind == "conv" else "") + {ACT_NONE: "", ACT_LEAKY: "-leaky", ACT_TANH: "-tanh"}[c.act] + \
        ("" if c.bias else "-nobias") + ("-res" if c.res else "")


def _conv_cpu(c, x, w):
    if c.kind == "convT":
        return F.conv_transpose1d(x, w, None, stride=c.s, padding=c.p)
    if c.P > 1:
        return F.conv2d(x, w, None, stride=(c.s, 1), padding=(c.p, 0), dilation=(c.d, 1), groups=c.g)
    return F.conv1d(x, w, None, stride=c.s, padding=c.p, dilation=c.d, groups=c.g)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """x, w, bias, res, dy of a case (float32, CPU); weights scaled by fan-in as tests/test_conv_gpu.py scales them."""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    tail = (c.T, c.P) if c.P > 1 else (c.T,)
    x = t(c.B, c.C, *tail)
    if c.kind == "convT":
        w = t(c.C, c.M, c.K) * (c.C * c.K / c.s) ** -0.5
    else:
        w = t(c.M, c.C // c.g, c.K, *((1,) if c.P > 1 else ())) * (c.C // c.g * c.K) ** -0.5
    b = t(c.M) * 0.5 if c.bias else None
    with torch.no_grad():
        shape = tuple(_conv_cpu(c, x, w).shape)
    return x, w, b, (t(*shape) if c.res else None), t(*shape)


@functools.lru_cache(maxsize=None)
def reference(c, rounded=False):
    """y, dx, dw, db in float64.  rounded: the operands of the matrix cores (input after its leaky-ReLU, weight, output
    gradient after the activation derivative) rounded to bf16 first, everything else as in fp32 mode."""
    x, w, b, res, gy = inputs(c)
    if rounded:
        xin = (F.leaky_relu(x, SLOPE) if c.in_leaky else x).bfloat16().double()
        wq = w.bfloat16().double()
    else:
        xin = F.leaky_relu(x.double(), SLOPE) if c.in_leaky else x.double()
        wq = w.double()
    xin.requires_grad_(True)
    wq.requires_grad_(True)
    pre = _conv_cpu(c, xin, wq)
    full = pre.detach()
    if b is not None:
        full = full + b.double().view(1, -1, *([1] * (full.dim() - 2)))
    if res is not None:
        full = full + res.double()
    if c.act == ACT_LEAKY:
        y, dact = F.leaky_relu(full, SLOPE), torch.where(full > 0, 1.0, SLOPE).double()
    elif c.act == ACT_TANH:
        y = torch.tanh(full)
        dact = 1.0 - y * y
    else:
        y, dact = full, torch.ones_like(full)
    if rounded:
        g_pre = gy * dact.float()  # (the activation-derivative pass is fp32; its result is what gets rounded)
        g_in, g_pre = g_pre.bfloat16().double(), g_pre.double()
    else:
        g_in = g_pre = gy.double() * dact
    pre.backward(g_in)
    dx = xin.grad
    if c.in_leaky:
        dx = dx * torch.where(x > 0, 1.0, SLOPE).double()
    out = {"y": y, "dx": dx, "dw": wq.grad}
    if b is not None:
        out["db"] = g_pre.sum(dim=[i for i in range(g_pre.dim()) if i != 1])
    return out


def run_gpu(c, gpu):
    from vcvits_amd import ops
    x, w, b, res, gy = inputs(c)
    xg, wg = x.to(gpu).requires_grad_(True), w.to(gpu).requires_grad_(True)
    bg = b.to(gpu).requires_grad_(True) if b is not None else None
    if c.kind == "convT":
        y = ops.conv_transpose1d(xg, wg, bg, stride=c.s, pad=c.p, in_leaky=c.in_leaky, slope=SLOPE)
    else:
        y = ops.conv1d(xg, wg, bg, stride=c.s, pad=c.p, dil=c.d, groups=c.g, in_leaky=c.in_leaky, out_act=c.act, slope=SLOPE,
                       res=res.to(gpu) if res is not None else None)
    y.backward(gy.to(gpu))
    out = {"y": y.detach(), "dx": xg.grad, "dw": wg.grad}
    if bg is not None:
        out["db"] = bg.grad
    return out


def dists(out, ref):
    return {k: rel(out[k], ref[k]) for k in ("y", "dx", "dw", "db") if k in out and k in ref}


MODES = {  # the settings a "default" run of a family is made under
    "lib": lambda: contextlib.nullcontext(),
    "pk": lambda: f32_split(False),
    "x3": lambda: f32_split(True, all_shapes=True),
    "f32wgrad": lambda: f32_split(True, wgrad=False),
    "bf16": lambda: compute_dtype("bf16"),
}
_baselines = {}


def baseline(c, gpu, mode="lib"):
    """The case under the unswitched setting of `mode`: its distances, its outputs and its forward-type launch plans."""
    key = (c, mode)
    if key not in _baselines:
        with MODES[mode](), conv_spy() as plans:
            out = run_gpu(c, gpu)
        _baselines[key] = (dists(out, reference(c, mode == "bf16")), {k: v.detach().cpu() for k, v in out.items()}, list(plans))
    return _baselines[key]


# ---------------------------------------------------------------------------------------------------------------------
# 1. deterministic mode, op level
# ---------------------------------------------------------------------------------------------------------------------
# (case, setting, where the weight gradient must go).  The shapes are the smallest that reach the named branch; the branch is
# asserted through wgrad_spy.  "f32wgrad": the split-operand weight gradient (vcv_wgrad_x3, always slab-combined) is on by
# default and takes K = 5 / K >= 9 launches with more than 32 channels before vcv_conv_wgrad sees them; the wgrad_dma rows
# it would take run with it switched off, and once more with the defaults (-> "x3").
DET_CASES = [
    # wgrad_dma + slab finish, one tile
    (conv(3, 64, 64, 200, 3, 1, 1, 1, 1), "lib", "dma"),
    # wgrad_dma + slab, the reduction split over many (b, q), ragged M / C / T
    (conv(8, 130, 100, 141, 5, 1, 2, 1, 1), "f32wgrad", "dma"),
    (conv(8, 130, 100, 141, 5, 1, 2, 1, 1), "lib", "x3"),
    # wgrad_dma, strided kernel (STR) + slab, period layout
    (conv(2, 32, 128, 67, 5, 3, 2, 1, 1, P=3), "lib", "dma"),
    # rows of 33 frames: the batch is folded into the columns ([1, C, T, B]); U = 33 * 4 = 132 >= 64 -> still wgrad_dma (P = 4)
    (conv(4, 64, 96, 33, 5, 1, 2, 1, 1), "lib", "dma"),
    # ... 15 frames: U = 15 * 4 = 60 < 64 -> the register-staged conv_wgrad_kernel, Z = 1 (the slab is handed over and unused)
    (conv(4, 64, 96, 15, 5, 1, 2, 1, 1), "lib", "reg"),
    # register-staged, grouped (G = 2: no slab, Z = 1)
    (conv(2, 64, 64, 150, 5, 1, 2, 1, 2), "lib", "reg"),
    # vcv_thin_wgrad, C = 1, stride 1: the (channel, tap)-pair kernel is off, one workgroup per (m, c)
    (conv(3, 1, 16, 3000, 15, 1, 7, 1, 1), "lib", "thin"),
    # vcv_thin_wgrad, C = 1, strided, period layout
    (conv(2, 1, 32, 100, 5, 3, 2, 1, 1, P=2), "lib", "thin"),
    # M = 1: vcv_thin_wgrad + vcv_conv_m1_fwd unsplit (no atomic form)
    (conv(64, 1024, 1, 2, 3, 1, 1, 1, 1), "lib", "thin"),
    (conv(3, 40, 1, 1000, 7, 1, 9, 3, 1), "lib", "thin"),
    # vcv_grouped41_wgrad: one workgroup per group, Mg = 4 and Mg = 16, with and without the leaky-ReLU output
    (conv(2, 16, 64, 512, 41, 4, 20, 1, 4), "lib", "g41"),
    (conv(2, 16, 64, 512, 41, 4, 20, 1, 4, act=ACT_LEAKY), "lib", "g41"),
    (conv(2, 64, 256, 260, 41, 4, 20, 1, 16), "lib", "g41"),
    (conv(2, 64, 256, 260, 41, 4, 20, 1, 16, act=ACT_LEAKY), "lib", "g41"),
    # vcv_bias_grad (linear) / vcv_act_grad_bias (leaky) with nseg = 1; the weight gradient is a wgrad_dma launch without dbias
    (conv(2, 32, 48, 700, 7, 1, 3, 1, 1), "lib", "dma"),
    (conv(2, 32, 48, 700, 7, 1, 3, 1, 1, act=ACT_LEAKY), "lib", "dma"),
    # transposed-conv weight gradient (a = leaky(x), b = dy)
    (convT(2, 64, 32, 300, 4, 2, 1), "lib", "dma"),
]


def _det_id(p):
    return cid(p[0]) + ("" if p[1] == "lib" else "-" + p[1]) + "->" + p[2]


def _det_run(c, gpu, mode, rounded, tols, section, want):
    with MODES[mode](), deterministic(), wgrad_spy() as seen:
        a = run_gpu(c, gpu)
        b = run_gpu(c, gpu)
    if want in ("thin", "g41"):
        assert seen == [], seen
    else:
        assert [s["to"] for s in seen] == [want, want], seen
        if c.g == 1:
            assert all(s["slab"] for s in seen), "deterministic mode handed no slab to the weight gradient"
    errs = dists(a, reference(c, rounded))
    base = baseline(c, gpu, "bf16" if rounded else mode)[0]
    check(section, _det_id((c, mode, want)), errs, tols, base)
    # op-level reproducibility: which launcher is at fault when the step-level test (test_determinism_gpu.py) fails
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between two identical deterministic launches" % k


@pytest.mark.parametrize("case", DET_CASES, ids=_det_id)
def test_deterministic_conv_matches_float64(gpu, case):
    c, mode, want = case
    _det_run(c, gpu, mode, False, F32_TOLS, "deterministic fp32", want)


@pytest.mark.parametrize("c", [conv(2, 16, 64, 512, 41, 4, 20, 1, 4, act=ACT_LEAKY), conv(2, 64, 256, 260, 41, 4, 20, 1, 16, act=ACT_LEAKY)],
                         ids=cid)
def test_deterministic_grouped41_wgrad_with_fused_derivative(gpu, c):
    """vcv_grouped41_wgrad with the leaky-ReLU derivative applied while staging dy (a_tf = TF_DLEAKY): the autograd path
    masks dy in a pass of its own, so this form is reached through ops.conv_wgrad only."""
    from vcvits_amd import ops
    x, w, b, _, gy = inputs(c)
    ref = reference(c)
    xg, gyg, yg = x.to(gpu), gy.to(gpu), ref["y"].float().to(gpu)
    with deterministic():
        a = ops.conv_wgrad(gyg, xg, tuple(w.shape), stride=c.s, pad=c.p, groups=c.g, a_tf=TF_DLEAKY, aaux=yg, slope=SLOPE)
        b2 = ops.conv_wgrad(gyg, xg, tuple(w.shape), stride=c.s, pad=c.p, groups=c.g, a_tf=TF_DLEAKY, aaux=yg, slope=SLOPE)
    d = ops.conv_wgrad(gyg, xg, tuple(w.shape), stride=c.s, pad=c.p, groups=c.g, a_tf=TF_DLEAKY, aaux=yg, slope=SLOPE)
    check("deterministic fp32", cid(c) + " conv_wgrad(a_tf=DLEAKY)", {"dw": rel(a, ref["dw"])}, F32_TOLS, {"dw": rel(d, ref["dw"])})
    assert torch.equal(a, b2)


# bf16 mode: the rows of the table whose weight gradient goes to the bf16 MFMA kernel (vcv_wgrad_bf16: always slab-combined;
# what deterministic mode changes there is the Python side -- the bias gradient leaves the launch, a slab is allocated that
# the launch ignores).  The strided period row and the short-row rows get no tile of that kernel (vcv_wgrad_bf16_scratch
# = 0) and run the fp32 code of the table above, as do the thin and grouped rows.
DET_BF16_CASES = [c for c, mode, want in DET_CASES if mode == "lib" and want == "dma" and c.P == 1 and c.T >= 64] + \
                 [conv(8, 130, 100, 141, 5, 1, 2, 1, 1)]


@pytest.mark.parametrize("c", DET_BF16_CASES, ids=cid)
def test_deterministic_conv_bf16_matches_float64_of_rounded_operands(gpu, c):
    from vcvits_amd import ops
    before = dict(ops.LAUNCH_COUNTS)
    _det_run(c, gpu, "bf16", True, BF16_TOLS, "deterministic bf16", "bf16")
    assert ops.LAUNCH_COUNTS["bf16"] >= before["bf16"] + 4, "forward / data gradient did not run on the bf16 kernels"


# ---------------------------------------------------------------------------------------------------------------------
# 2. deterministic mode, one whole step against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_deterministic_vocoder_gan_batch_matches_oracle(gpu):
    """tests/test_training_step_gpu.py::test_vocoder_gan_batch's comparison (both losses, every parameter gradient of the
    generator and discriminator passes against oracle.cpu_step.CpuTrainer, that file's _run and tolerances) with
    deterministic mode on: the Python-side branches of the mode -- the separate bias-gradient pass of conv_wgrad and the
    slab allocation of _launch_wgrad -- inside a real step."""
    import copy

    from oracle.cpu_step import CpuTrainer
    from test_training_step_gpu import _run, small_cfg
    from vcvits_amd import synthetic
    from vcvits_amd.light.vcvits import VocoderGAN
    torch.manual_seed(0)
    cfg = small_cfg()
    module = VocoderGAN(**cfg)
    trainer = CpuTrainer(copy.deepcopy(module.state_dict()), cfg, [2, 3], vocoder_only=True)
    module = module.to(gpu)
    module.configure_optimizers()
    try:
        with deterministic():
            _run(module, trainer, synthetic.vocoder_batch(2, 16, segment_size=4096, seed=3), gpu)
    finally:
        module.optim_g.close()
        module.optim_d.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3a. packed fp32 convs (vcv_conv_pk_*): the split kernel out of the way with ops.set_f32_split(False)
# ---------------------------------------------------------------------------------------------------------------------
PK_CASES = [
    conv(2, 256, 256, 256, 11, 1, 5, 1, 1),                         # 128 x 128 tiles, the channel groups split over workgroups
    # the warp-specialised 128 x 256 twin by default (pk_ws): it needs M >= 128, stride 1, rows longer than 160 and
    # blocks(128, 256) = 16 * 7 * 1 = 112 >= 112 (conv_pk_kernel.h, choose(): the shape above has 4 such blocks and never gets it)
    conv(16, 32, 128, 1792, 3, 1, 1, 1, 1),
    conv(2, 64, 64, 300, 11, 1, 25, 5, 1),
    conv(2, 64, 64, 300, 11, 1, 25, 5, 1, in_leaky=True, res=True),  # input leaky-ReLU and the residual epilogue
    conv(1, 130, 70, 333, 3, 1, 1, 1, 1),                           # ragged everything, odd row length
    # period layout, strided (phased data gradient).  59 rows, not test_conv_gpu.py's 23: the packed kernels want Tout * P >= 96
    # columns (23 rows give 8 * 5 = 40 and every packed family declines)
    conv(2, 128, 512, 59, 5, 3, 2, 1, 1, P=5),
    convT(2, 128, 64, 100, 4, 4, 0),
]
ALWAYS_SAME_PLAN = ("pk_vec", "xcd_remap")
PK_WS_CASE = PK_CASES[1]


def _switch_vs_baseline(c, gpu, mode, key, value, count, section):
    from vcvits_amd import ops
    base_errs, base_out, base_plans = baseline(c, gpu, mode)
    before = ops.LAUNCH_COUNTS[count]
    with MODES[mode](), switched(key, value), conv_spy() as plans:
        out = run_gpu(c, gpu)
    assert ops.LAUNCH_COUNTS[count] > before, "none of this case's launches went to the %s kernels" % count
    check(section, "%s=%d %s (plans %s)" % (key, value, cid(c), "same" if plans == base_plans else "changed"), dists(out, reference(c)),
          F32_TOLS, base_errs)
    return out, base_out, plans == base_plans


@pytest.mark.parametrize("c", PK_CASES, ids=cid)
@pytest.mark.parametrize("key", ["pk_x4", "pk_vec", "pk_ws", "xcd_remap"])
def test_pk_switch(gpu, key, c):
    out, base, same_plan = _switch_vs_baseline(c, gpu, "pk", key, 0, "pk", "packed fp32 convs")
    if key in ALWAYS_SAME_PLAN:
        assert same_plan, "%s changed a launch plan" % key
    if key == "pk_ws" and c == PK_WS_CASE:  # (the one shape whose default plan is the producer-wave twin: another channel chunk without it)
        assert not same_plan, "pk_ws=0 planned what the default plans: the warp-specialised twin was never in play"
    if same_plan:  # same tiles, channel chunks and reduction split: the switch must not change a bit (see the docstring)
        for k in ("y", "dx"):
            assert torch.equal(out[k].cpu(), base[k]), "%s=0 changed bits of %s" % (key, k)


# ---------------------------------------------------------------------------------------------------------------------
# 3b. split-operand convs (vcv_conv_x3_*)
# ---------------------------------------------------------------------------------------------------------------------
X3_A = conv(2, 256, 320, 300, 5, 1, 2, 1, 1)  # fits every variant
X3_B = conv(2, 96, 48, 200, 3, 1, 1, 1, 1)    # 48 output channels: the host refuses the 128- and 256-row variants
X3_VBM = (128, 128, 256, 64, 64, 32, 64)
X3_FORCED = [(X3_A, 0, 1, -1), (X3_A, 0, 2, -1), (X3_A, 1, 1, -1), (X3_A, 1, 2, -1), (X3_A, 2, -1, -1), (X3_A, 3, -1, -1),
             (X3_A, 4, -1, -1), (X3_A, 5, -1, -1), (X3_A, 6, -1, -1),
             (X3_A, 3, -1, 2),  # the channel groups (256 / 16 = 16 >= 4) split over two workgroups per tile
             ] + [(X3_B, v, -1, -1) for v in range(7)]


@pytest.mark.parametrize("p", X3_FORCED, ids=lambda p: "%s-v%d-js%d-ks%d" % (cid(p[0]), p[1], p[2], p[3]))
def test_x3_forced_variant(gpu, p):
    """Every tile variant of the split-operand kernel forced through vcv_conv_x3_set_variant.  choose() refuses a variant on
    the host when the launch has fewer output channels than half a tile + 1 (32 for the 32-row variant): the launch must
    then go to another family, and the result still be right.  (Shape B, 48 channels: variants 0, 1 and 2 are refused for
    the forward launch; variant 6 has 64-row tiles and takes it.  Its stride-1 data gradient has 96 output channels: only
    variant 2 is refused there.)"""
    from vcvits_amd import ops
    c, v, js, ks = p
    x, w, b, _, gy = inputs(c)
    refused = lambda mg: mg < (32 if v == 5 else X3_VBM[v] // 2 + 1)
    with f32_split(True, all_shapes=True), x3_variant(v, js, ks):
        xg, wg, bg = (t.to(gpu).requires_grad_(True) for t in (x, w, b))
        n0 = ops.LAUNCH_COUNTS["x3"]
        y = ops.conv1d(xg, wg, bg, stride=c.s, pad=c.p, dil=c.d)
        n1 = ops.LAUNCH_COUNTS["x3"]
        y.backward(gy.to(gpu))
        n2 = ops.LAUNCH_COUNTS["x3"]
    assert n1 - n0 == (0 if refused(c.M) else 1), "forward: variant %d, %d output channels" % (v, c.M)
    assert n2 - n1 == (0 if refused(c.C) else 1), "data gradient: variant %d, %d output channels" % (v, c.C)
    out = {"y": y.detach(), "dx": xg.grad, "dw": wg.grad, "db": bg.grad}
    check("split-operand convs", "x3_variant=%d js=%d ks=%d %s" % (v, js, ks, cid(c)), dists(out, reference(c)), F32_TOLS,
          baseline(c, gpu, "x3")[0])


# What the plan signature (vcv_conv_x3_plan: pack words, scratch floats, BM, taps per phase, phases) can show of a switch is
# asserted: x3_old_ks changes the scratch, xcd_remap / pk_vec change nothing.  It carries neither the column width of the tile nor
# the taps per stage, so for x3_js2 and x3_v6 the planner is asked which variant the test's shape reaches (_x3_choice).
# x3_js2 = 0 acts on variants 0 / 1 only.  X3_A's forward (320 output channels, U = 300) is planned as variant 2 (256 x 128) and
# does not read the switch; its data gradient (256 output channels) is planned as variant 0 (128 x 256) and loses its second tap
# per stage under it: the switch is checked through dx.
X3_SWITCHES = [
    ("x3_js2", 0, X3_A), ("x3_terms", 9, X3_A), ("pk_vec", 0, X3_A), ("xcd_remap", 0, X3_A),
    # fewer than 192 tiles and 96 / 16 = 6 channel groups: the round-3 rule splits them three ways, the default rule two ways
    # (the plans differ: asserted; on the issue's (2, 512, 128, 100, 5) both rules pick 16)
    ("x3_old_ks", 1, conv(2, 96, 512, 1300, 3, 1, 1, 1, 1)),
]


@pytest.mark.parametrize("p", X3_SWITCHES, ids=lambda p: "%s=%d-%s" % (p[0], p[1], cid(p[2])))
def test_x3_switch(gpu, p):
    key, value, c = p
    out, base, same_plan = _switch_vs_baseline(c, gpu, "x3", key, value, "x3", "split-operand convs")
    if key in ALWAYS_SAME_PLAN:
        assert same_plan
        for k in ("y", "dx"):
            assert torch.equal(out[k].cpu(), base[k]), "%s=0 changed bits of %s" % (key, k)
    if key == "x3_old_ks":
        assert not same_plan, "x3_old_ks=1 planned the same channel-group split as the default rule"


def _x3_choice(B, Mg, U, v6=True):
    """The tile variant conv_x3.hip's choose() plans for a stride-1, one-phase launch of Mg output channels and U columns, as
    vcv_conv_plan_describe reports it (host-only; 64 input channels and 3 taps: every variant's LDS image fits)."""
    from vcvits_amd._lib import VcvConvArgs, lib
    a = VcvConvArgs()
    a.B, a.G, a.Cg, a.Mg, a.Tin, a.Tout, a.P, a.K = B, 1, 64, Mg, U, U, 1, 3
    a.s, a.dj, a.off, a.os, a.oo, a.phases, a.Q, a.alpha = 1, 1, -1, 1, 0, 1, U, 1.0
    words = (ctypes.c_int32 * 16)()
    with f32_split(True, all_shapes=True), switched("x3_v6", 1 if v6 else 0):
        assert lib().vcv_conv_plan_describe(ctypes.byref(a), 3, 0, words) == 0
    return words[0]


def test_x3_choice_of_the_switch_shapes():
    """The shapes of the x3_js2 / x3_v6 cases reach the variants those switches act on (see X3_SWITCHES)."""
    assert _x3_choice(X3_A.B, X3_A.M, X3_A.T) == 2 and _x3_choice(X3_A.B, X3_A.C, X3_A.T) == 0
    assert _x3_choice(8, 64, 11777) == 6 and _x3_choice(8, 64, 11777, v6=False) == 4  # (64 x 128: eff 0.958 against 64 x 256's 0.719)
    assert _x3_choice(8, 64, 11776 - 512) != 6  # (one column tile fewer: blocks(64, 512) = 8 * 23 = 184 < 192)


def test_x3_v6_off(gpu):
    """x3_v6 = 0 on a launch the default plan gives the 64 x 512 tile: 48 <= M < 96, blocks(64, 256) = 8 * 47 = 376 > 256,
    blocks(64, 512) = 8 * 24 = 192 >= 192 and eff(64, 512) = 0.719 >= eff(64, 256) - 0.02 = 0.715 (conv_x3.hip, choose()).
    Forward only (the data gradient has the same shape)."""
    from vcvits_amd import ops
    B, C, M, T, K = 8, 64, 64, 11777, 3
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32))
    w = torch.from_numpy(rng.standard_normal((M, C, K)).astype(np.float32)) * (C * K) ** -0.5
    ref = F.conv1d(x.double(), w.double(), padding=1)
    xg, wg = x.to(gpu), w.to(gpu)
    with f32_split(True, all_shapes=True):
        n0 = ops.LAUNCH_COUNTS["x3"]
        y1 = ops.conv_forward(xg, wg, pad=1)
        with switched("x3_v6", 0):
            y0 = ops.conv_forward(xg, wg, pad=1)
        assert ops.LAUNCH_COUNTS["x3"] == n0 + 2
    check("split-operand convs", "x3_v6=0 conv-B8-C64-M64-T11777-K3 (forward)", {"y": rel(y0, ref)}, F32_TOLS, {"y": rel(y1, ref)})


# ---------------------------------------------------------------------------------------------------------------------
# 3c. MFMA weight gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [conv(3, 64, 64, 200, 3, 1, 1, 1, 1), conv(8, 130, 100, 141, 5, 1, 2, 1, 1),
                               conv(2, 32, 128, 67, 5, 3, 2, 1, 1, P=3)], ids=cid)
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_wgrad_register_staged(gpu, c, det):
    """wgrad_dma = 0: the register-staged conv_wgrad_kernel on the shapes the LDS-DMA kernel takes by default (it is the
    general path for the shapes that kernel declines), with the bias gradient by its own pass."""
    with MODES["f32wgrad"](), switched("wgrad_dma", 0), deterministic(det), wgrad_spy() as seen:
        out = run_gpu(c, gpu)
    assert [s["to"] for s in seen] == ["reg"], seen
    check("weight gradients", "wgrad_dma=0 %s %s" % ("deterministic" if det else "", cid(c)), dists(out, reference(c)), F32_TOLS,
          baseline(c, gpu, "f32wgrad")[0])


WG_TILES = ((128, 256), (128, 128), (128, 64), (64, 256), (64, 128), (64, 64), (32, 128))  # wgrad_dma.hip, WG_TILES


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "slab"])
@pytest.mark.parametrize("cand", range(7))
def test_wgrad_forced_tile(gpu, capfd, cand, det):
    """wgrad_tile = 0..6.  The launcher memoises its plan per launch shape, so every candidate (and the slab form of it) has a
    shape of its own that no other test uses; M = 160 admits every tile (Mg >= BM / 2 + 1).  wgrad_verbose prints each
    plan that is evaluated: with a forced tile exactly that one (the only proof that the force took effect)."""
    from vcvits_amd import ops
    B, C, M, K, T = 2, 96, 160, 5, 211 + cand + (10 if det else 0)
    rng = np.random.default_rng(1000 + T)
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    x, dy = t(B, C, T), t(B, M, T)
    wz = torch.zeros(M, C, K, dtype=torch.float64, requires_grad=True)
    ref = torch.autograd.grad(F.conv1d(x.double(), wz, None, padding=2), wz, dy.double())[0]
    xg, dyg = x.to(gpu), dy.to(gpu)
    torch.cuda.synchronize()
    capfd.readouterr()
    with MODES["f32wgrad"](), deterministic(det), switched("wgrad_verbose", 1), switched("wgrad_tile", cand), wgrad_spy() as seen:
        dbias = torch.zeros(M, device=gpu)
        got = ops.conv_wgrad(dyg, xg, (M, C, K), pad=2, dbias=dbias)
        again = ops.conv_wgrad(dyg, xg, (M, C, K), pad=2)
        again2 = ops.conv_wgrad(dyg, xg, (M, C, K), pad=2)
        acc = again.clone()  # accumulate onto an existing gradient with a scale (the epilogue's / the slab finish's alpha)
        ops.conv_wgrad(dyg, xg, (M, C, K), pad=2, out=acc, alpha=0.5)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    tiles = [ln.split(" tile ")[1].split(":")[0] for ln in err.splitlines() if ln.startswith("wgrad plan ")]
    # (two plans: the launch with the bias sums and the one without are two cache keys)
    assert tiles and set(tiles) == {"%dx%d" % WG_TILES[cand]}, (cand, tiles, err[-400:])
    assert [s["to"] for s in seen] == ["dma"] * 4 and all(s["slab"] == det for s in seen), seen
    d = ops.conv_wgrad(dyg, xg, (M, C, K), pad=2)  # (no force: the memoised forced plan again, or, after a slab launch, the cost model's own plan)
    check("weight gradients", "wgrad_tile=%d %s conv_wgrad-B2-C96-M160-T%d-K5" % (cand, "slab" if det else "atomics", T),
          {"dw": rel(got, ref), "db": rel(dbias, dy.double().sum(dim=(0, 2)))}, F32_TOLS, {"dw": rel(d, ref)})
    assert rel(again, ref) <= TOL_DW and rel(acc, 1.5 * ref) <= TOL_DW, (rel(again, ref), rel(acc, 1.5 * ref))
    if det:
        assert torch.equal(again, again2), "the slab combine is not bit-reproducible"


@pytest.mark.parametrize("c", [conv(3, 64, 64, 200, 3, 1, 1, 1, 1), conv(2, 32, 48, 700, 7, 1, 3, 1, 1, act=ACT_LEAKY),
                               conv(2, 1, 32, 700, 5, 3, 2, 1, 1, P=37)], ids=cid)
def test_zero_memset(gpu, c):
    """zero_memset = 1: vcv_zero_async goes through hipMemsetAsync instead of the fill kernel.  (The weight-gradient
    accumulators of ops.conv_wgrad are torch.zeros, which the switch does not touch; inside the library the helper zeroes
    the split bias-gradient sums, the LayerNorm parameter gradients, the attention table gradients and the STFT input
    gradient: test_zero_memset_users.)"""
    with switched("zero_memset", 1):
        out = run_gpu(c, gpu)
    check("weight gradients", "zero_memset=1 %s" % cid(c), dists(out, reference(c)), F32_TOLS, baseline(c, gpu)[0])


def test_zero_memset_users(gpu):
    from vcvits_amd import ops
    rng = np.random.default_rng(21)
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    # vcv_bias_grad split over nseg = min(1024 / C, units / 8) = 4 segments (16 rows of two 1024-float pieces), not accumulating
    dy = t(16, 24, 1100)
    ref = dy.double().sum(dim=(0, 2))
    base = rel(ops.bias_grad(dy.to(gpu)), ref)
    with switched("zero_memset", 1):
        got = rel(ops.bias_grad(dy.to(gpu)), ref)
    check("weight gradients", "zero_memset=1 bias_grad-B16-C24-T1100", {"db": got}, F32_TOLS, {"db": base})
    # generic LayerNorm backward (C = 96): dgamma / dbeta are zeroed, then filled by atomics
    base = _layernorm_errs(gpu, (2, 96, 50), True)
    with switched("zero_memset", 1):
        errs = _layernorm_errs(gpu, (2, 96, 50), True)
    check("weight gradients", "zero_memset=1 layernorm_c-B2-C96-T50", errs, LN_TOLS, base)
    # STFT magnitude backward with reflect padding: dy is zeroed, then filled by atomics
    base = _stft_errs(gpu, 2048, 512, 2048, 5120, True, 2)
    with switched("zero_memset", 1):
        errs = _stft_errs(gpu, 2048, 512, 2048, 5120, True, 2)
    check("weight gradients", "zero_memset=1 stft_mag-2048/512-T5120-reflect", errs, STFT_TOLS, base)


BF16_SHAPES = [conv(2, 128, 128, 512, 5, 1, 2, 1, 1), conv(2, 130, 100, 333, 5, 1, 2, 1, 1)]


@pytest.mark.parametrize("p", [(k, v, c) for k, v in (("wgrad_bf16_ws", 0), ("wgrad_finish_vec", 0), ("pk_ws_bf16", 1)) for c in BF16_SHAPES]
                         # C = 130 selects the scalar finish by itself (C % 4 != 0): a ragged shape with C % 4 == 0 for wgrad_finish_vec
                         + [("wgrad_finish_vec", 0, conv(2, 132, 100, 333, 5, 1, 2, 1, 1)),
                            # the producer-wave twin is planned for blocks(128, 256) >= 112 only (see PK_CASES): the two shapes above
                            # keep their plan under pk_ws_bf16 = 1, this one changes kernels
                            ("pk_ws_bf16", 1, conv(16, 32, 128, 1792, 3, 1, 1, 1, 1))],
                         ids=lambda p: "%s=%d-%s" % (p[0], p[1], cid(p[2])))
def test_bf16_switch(gpu, p):
    from vcvits_amd import ops
    key, value, c = p
    base = baseline(c, gpu, "bf16")[0]
    before = dict(ops.LAUNCH_COUNTS)
    with compute_dtype("bf16"), switched(key, value):
        out = run_gpu(c, gpu)
    assert ops.LAUNCH_COUNTS["wgrad_bf16"] == before["wgrad_bf16"] + 1 and ops.LAUNCH_COUNTS["bf16"] == before["bf16"] + 2
    check("bf16 mode", "%s=%d %s" % (key, value, cid(c)), dists(out, reference(c, True)), BF16_TOLS, base)


@pytest.mark.parametrize("cand", range(6))
def test_wgrad_bf16_forced_candidate(gpu, cand):
    """vcv_wgrad_bf16_set_force(cand, -1): each (WM, WC, WU) tile of the bf16 weight gradient on a shape that fits them all
    (128 output and 128 input channels: bm <= Mg and bc <= Cg for every candidate).  Under a force pick() looks at that candidate
    alone, and where it does not fit vcv_wgrad_bf16_scratch returns 0: ops.conv._launch_wgrad then goes to vcv_conv_wgrad and
    LAUNCH_COUNTS["wgrad_bf16"] stays -- so the counter moving is the proof that the forced candidate ran."""
    from vcvits_amd import ops
    c = BF16_SHAPES[0]
    x, w, _, _, gy = inputs(c)
    ref = reference(c, True)
    before = ops.LAUNCH_COUNTS["wgrad_bf16"]
    with compute_dtype("bf16"), wgrad_bf16_force(cand):
        got = ops.conv_wgrad(gy.to(gpu), x.to(gpu), tuple(w.shape), pad=c.p)
        again = ops.conv_wgrad(gy.to(gpu), x.to(gpu), tuple(w.shape), pad=c.p)
    assert ops.LAUNCH_COUNTS["wgrad_bf16"] == before + 2, "candidate %d was not launched" % cand
    check("bf16 mode", "wgrad_bf16 candidate %d %s" % (cand, cid(c)), {"dw": rel(got, ref["dw"])}, BF16_TOLS,
          {"dw": baseline(c, gpu, "bf16")[0]["dw"]})
    assert torch.equal(got, again)


# ---------------------------------------------------------------------------------------------------------------------
# 3d. thin / streaming kernels
# ---------------------------------------------------------------------------------------------------------------------
def _simple_switch(gpu, section, key, value, c, tols=F32_TOLS, note=""):
    base = baseline(c, gpu)
    with switched(key, value):
        out = run_gpu(c, gpu)
    check(section, "%s=%d %s%s" % (key, value, note, cid(c)), dists(out, reference(c)), tols, base[0])
    return out, base[1]


@pytest.mark.parametrize("c", [conv(2, 48, 64, 50, 5, 1, 2, 1, 1), conv(3, 32, 32, 1000, 7, 1, 3, 1, 1)], ids=cid)
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_bias_rows_off(gpu, c, det):
    """bias_rows = 0: short rows on the segmented vcv_bias_grad kernel (the general path for T > 1024).  In the default mode
    the bias sums of these two shapes are collected inside the weight-gradient launch, so the kernel under test runs in
    deterministic mode (ops/conv.py: the bias gradient leaves the launch) and for the folded short rows."""
    with deterministic(det):
        _simple_switch(gpu, "thin / streaming", "bias_rows", 0, c, note="deterministic " if det else "")


@pytest.mark.parametrize("c", [conv(2, 1, 40, 257, 5, 1, 2, 1, 1), conv(2, 1, 17, 300, 15, 1, 7, 1, 1)], ids=cid)
@pytest.mark.parametrize("chunk", [1, 4, 16, 64])
def test_c1_chunk(gpu, c, chunk):
    """c1_chunk: output channels per workgroup of vcv_conv_c1_fwd.  A chunk larger than M (64 > 40, 64 > 17) is clamped: the
    launcher caps it at C1_MMAX = 64 = the LDS weight table, the grid has ceil(M / chunk) = 1 chunk and the kernel clamps its
    channel count to M - m0, so neither the weight reads nor the stores leave the M rows.  Same arithmetic per output:
    bit-equal to the default chunking."""
    out, base = _simple_switch(gpu, "thin / streaming", "c1_chunk", chunk, c)
    assert torch.equal(out["y"].cpu(), base["y"]), "c1_chunk=%d changed bits of y" % chunk


M1_SHAPES = [(3, 48, 1, 70, 5, 1, 4, 2, 1), (64, 1024, 1, 2, 3, 1, 1, 1, 1), (2, 32, 1, 8192, 7, 1, 3, 1, 1)]


@pytest.mark.parametrize("c", [conv(*s, **kw) for s in M1_SHAPES for kw in ({}, {"in_leaky": True, "act": ACT_TANH})], ids=cid)
def test_m1_lds_off(gpu, c):
    """m1_lds = 0: the register kernel conv_m1_fwd_kernel (the path of every strided one-output-channel conv) on stride-1
    shapes, plain and with the input leaky-ReLU + tanh output of the generator's last layer."""
    _simple_switch(gpu, "thin / streaming", "m1_lds", 0, c)


@pytest.mark.parametrize("c", [conv(3, 1, 16, 3000, 15, 1, 7, 1, 1), conv(2, 1, 17, 300, 15, 1, 7, 1, 1)], ids=cid)
def test_c1_wgrad_pairs_off(gpu, c):
    _simple_switch(gpu, "thin / streaming", "c1_wgrad_pairs", 0, c)


@pytest.mark.parametrize("c", [conv(2, 1024, 1, 24, 3, 1, 1, 1, 1), conv(2, 1, 32, 700, 5, 3, 2, 1, 1, P=37)], ids=cid)
@pytest.mark.parametrize("wgs", [1, 7, 100000])
def test_thin_wgrad_wgs(gpu, c, wgs):
    """thin_wgrad_wgs: the workgroup count vcv_thin_wgrad aims at.  The position split is capped at U / 1024 and floored at 1
    on the host, so 1 and 100000 are both legal (1: no split; 100000: 8 pieces of the 8658 positions of the period case)."""
    _simple_switch(gpu, "thin / streaming", "thin_wgrad_wgs", wgs, c)


@pytest.mark.parametrize("c", [conv(2, 32, 48, T, 3, 1, 1, 1, 1, act=ACT_LEAKY, bias=bias) for T in (64, 67, 68) for bias in (True, False)],
                         ids=cid)
def test_act_grad_vec_off(gpu, c):
    """act_grad_vec = 0: the scalar activation-derivative passes (vcv_act_grad without a bias, vcv_act_grad_bias with one) at
    a row length the float4 form takes (T % 4 == 0) and one it does not.  T = 64 is folded into the column dimension (rows
    of <= 64 frames) and never reaches vcv_act_grad_bias; T = 68 is the shortest unfolded row with T % 4 == 0.  The masked
    gradient is the same per element, so y and dx keep their bits."""
    out, base = _simple_switch(gpu, "thin / streaming", "act_grad_vec", 0, c)
    for k in ("y", "dx"):
        assert torch.equal(out[k].cpu(), base[k]), "act_grad_vec=0 changed bits of %s" % k


def test_act_grad_vec_off_mel_log(gpu):
    """ops.mel_log's backward: the log-clamp derivative (TF_DLOGCLAMP) as a scalar pass, [2, 1025, 40] -> 80 mel bins."""
    from vcvits_amd import ops
    rng = np.random.default_rng(40)
    spec = torch.from_numpy(np.abs(rng.standard_normal((2, 1025, 40))).astype(np.float32) + 0.01)
    mel = torch.from_numpy(np.abs(rng.standard_normal((80, 1025))).astype(np.float32) / 1025)
    gy = torch.from_numpy(rng.standard_normal((2, 80, 40)).astype(np.float32))
    sr = spec.double().requires_grad_(True)
    ref = torch.log(torch.clamp(torch.matmul(mel.double(), sr), min=1e-5))
    ref.backward(gy.double())

    def run():
        sg = spec.to(gpu).requires_grad_(True)
        y = ops.mel_log(sg, mel.to(gpu), 1e-5)
        y.backward(gy.to(gpu))
        return y.detach(), sg.grad

    y1, d1 = run()
    with switched("act_grad_vec", 0):
        y0, d0 = run()
    check("thin / streaming", "act_grad_vec=0 mel_log-B2-F1025-T40", {"y": rel(y0, ref.detach()), "dx": rel(d0, sr.grad)}, F32_TOLS,
          {"y": rel(y1, ref.detach()), "dx": rel(d1, sr.grad)})
    assert torch.equal(d0, d1) and torch.equal(y0, y1)


# ---- LayerNorm over channels ---------------------------------------------------------------------------------------------
LN_TOLS = {k: 2e-5 for k in ("out", "dx", "dy", "dgamma", "dbeta")}  # tests/test_layernorm_gpu.py


@functools.lru_cache(maxsize=None)
def _layernorm_case(shape, with_y):
    B, C, T = shape
    rng = np.random.default_rng(B * 1000 + C + T + (7 if with_y else 0))
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    x, y, ga, be, gy = t(B, C, T), (t(B, C, T) if with_y else None), t(C), t(C), t(B, C, T)
    xd, gd, bd = (v.double().requires_grad_(True) for v in (x, ga, be))
    yd = y.double().requires_grad_(True) if with_y else None
    inp = (xd + yd if with_y else xd).transpose(1, 2)
    mu = inp.mean(-1, keepdim=True)
    var = ((inp - mu) ** 2).mean(-1, keepdim=True)
    ref = ((inp - mu) / torch.sqrt(var + 1e-5) * gd + bd).transpose(1, 2)
    ref.backward(gy.double())
    refs = {"out": ref.detach(), "dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad}
    if with_y:
        refs["dy"] = yd.grad
    return (x, y, ga, be, gy), refs


def _layernorm_errs(gpu, shape, with_y):
    from vcvits_amd import ops
    (x, y, ga, be, gy), refs = _layernorm_case(shape, with_y)
    xg, gg, bg = (v.to(gpu).requires_grad_(True) for v in (x, ga, be))
    yg = y.to(gpu).requires_grad_(True) if with_y else None
    out = ops.layernorm_c(xg, yg, gg, bg)
    out.backward(gy.to(gpu))
    got = {"out": out, "dx": xg.grad, "dgamma": gg.grad, "dbeta": bg.grad}
    if with_y:
        got["dy"] = yg.grad
    return {k: rel(got[k], refs[k]) for k in got}


@pytest.mark.parametrize("shape", [(3, 256, 37), (2, 128, 64), (16, 128, 204)], ids=lambda s: "B%d-C%d-T%d" % s)
@pytest.mark.parametrize("with_y", [True, False])
def test_ln_regs_off(gpu, shape, with_y):
    """ln_regs = 0: the generic LayerNorm kernels -- the ones every width other than 128 / 256 runs on -- at 128 and 256
    channels, against the float64 LayerNorm over C."""
    base = _layernorm_errs(gpu, shape, with_y)
    with switched("ln_regs", 0):
        errs = _layernorm_errs(gpu, shape, with_y)
    check("thin / streaming", "ln_regs=0 layernorm_c-B%d-C%d-T%d%s" % (shape + ("+y" if with_y else "",)), errs, LN_TOLS, base)


@pytest.mark.parametrize("regs", [1, 0])
def test_layernorm_bwd_both_entry_points(gpu, regs):
    """vcv_layernorm_c_bwd (library-owned workspace) and vcv_layernorm_c_bwd_ws (caller's workspace) on one case: the same
    kernels, so with ln_regs = 1 (partial rows summed in index order) the same bits; with ln_regs = 0 both are the atomics
    form and agree with the float64 reference."""
    from vcvits_amd._lib import check as ck, lib, ptr, stream
    shape = (3, 256, 37)
    B, C, T = shape
    (x, y, ga, be, gy), refs = _layernorm_case(shape, True)
    xg, yg, gg, bg, gyg = (v.to(gpu) for v in (x, y, ga, be, gy))
    new = lambda like: torch.empty_like(like)
    with switched("ln_regs", regs):
        out, mean, rstd = new(xg), torch.empty(B, T, device=gpu), torch.empty(B, T, device=gpu)
        ck(lib().vcv_layernorm_c_fwd(ptr(xg), ptr(yg), ptr(gg), ptr(bg), ptr(out), ptr(mean), ptr(rstd), B, C, T, 1e-5, stream()), "fwd")
        dx1, dg1, db1, dx2, dg2, db2 = new(xg), new(gg), new(gg), new(xg), new(gg), new(gg)
        n = lib().vcv_layernorm_c_bwd_scratch(B, C, T)
        assert (n > 0) == bool(regs)
        ws = torch.empty(max(n, 1), device=gpu)
        ck(lib().vcv_layernorm_c_bwd_ws(ptr(xg), ptr(yg), ptr(gg), ptr(mean), ptr(rstd), ptr(gyg), ptr(dx1), ptr(dg1), ptr(db1), B, C, T,
                                        ptr(ws) if n else None, n, stream()), "bwd_ws")
        ck(lib().vcv_layernorm_c_bwd(ptr(xg), ptr(yg), ptr(gg), ptr(mean), ptr(rstd), ptr(gyg), ptr(dx2), ptr(dg2), ptr(db2), B, C, T,
                                     stream()), "bwd")
        torch.cuda.synchronize()
    e1 = {"dx": rel(dx1, refs["dx"]), "dgamma": rel(dg1, refs["dgamma"]), "dbeta": rel(db1, refs["dbeta"])}
    e2 = {"dx": rel(dx2, refs["dx"]), "dgamma": rel(dg2, refs["dgamma"]), "dbeta": rel(db2, refs["dbeta"])}
    check("thin / streaming", "ln_regs=%d vcv_layernorm_c_bwd_ws B3-C256-T37 (| vcv_layernorm_c_bwd)" % regs, e1, LN_TOLS, e2)
    assert all(v <= 2e-5 for v in e2.values()), e2
    assert torch.equal(dx1, dx2)
    if regs:
        assert torch.equal(dg1, dg2) and torch.equal(db1, db2)


# ---- STFT magnitude ------------------------------------------------------------------------------------------------------
STFT_TOLS = {"spec": 1e-5, "dy": 1e-4}  # tests/test_stft_sizes.py


@functools.lru_cache(maxsize=None)
def _stft_case(n_fft, hop, win, T, reflect, B, backward=True):
    rng = np.random.default_rng(n_fft + hop + T + B + (1 if reflect else 0))
    y = torch.from_numpy((rng.standard_normal((B, T)) * 0.3).astype(np.float32))
    yd = y.double().requires_grad_(backward)
    pad = (n_fft - hop) // 2
    yp = F.pad(yd.unsqueeze(1), (pad, pad), mode="reflect" if reflect else "constant").squeeze(1)
    s = torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=torch.float64), center=False,
                   return_complex=True)
    ref = torch.sqrt(s.real ** 2 + s.imag ** 2 + 1e-6)
    r = torch.from_numpy(rng.standard_normal(tuple(ref.shape)).astype(np.float32))
    if backward:
        (ref * r.double()).sum().backward()
    return y, r, ref.detach(), yd.grad


def _stft_errs(gpu, n_fft, hop, win, T, reflect, B, backward=True):
    from vcvits_amd import ops
    y, r, ref, dref = _stft_case(n_fft, hop, win, T, reflect, B, backward)
    yg = y.to(gpu).requires_grad_(backward)
    out = ops.stft_mag(yg, n_fft, hop, (n_fft - hop) // 2, reflect=reflect, win_length=win)
    errs = {"spec": rel(out, ref)}
    if backward:
        (out * r.to(gpu)).sum().backward()
        errs["dy"] = rel(yg.grad, dref)
    return errs


# stft.hip:764: the switch governs the FORWARD magnitude launch of n_fft = 2048 only, in its three frame-count regimes (<= 1024
# frames: one frame per workgroup, <= 4096: four, more: 4 x 4); the backward kernels and every other n_fft (stft_generic.hip)
# do not read it -- the two generic sizes run once to show that the switch leaves them alone
@pytest.mark.parametrize("p", [(2048, 512, 2048, 5120, 2, True), (2048, 512, 1200, 6000, 3, True), (2048, 512, 2048, 180000, 3, False),
                               (2048, 512, 2048, 270000, 8, False), (1024, 256, 1024, 4096, 3, True), (128, 32, 128, 777, 3, True)],
                         ids=lambda p: "%d-%d-%d-T%d-B%d" % p[:5])
@pytest.mark.parametrize("reflect", [True, False], ids=["reflect", "zero"])
def test_stft_wave_off(gpu, p, reflect):
    n_fft, hop, win, T, B, backward = p
    base = _stft_errs(gpu, n_fft, hop, win, T, reflect, B, backward)
    with switched("stft_wave", 0):
        errs = _stft_errs(gpu, n_fft, hop, win, T, reflect, B, backward)
    check("thin / streaming", "stft_wave=0 stft_mag-%d/%d/%d-T%d-B%d-%s" % (n_fft, hop, win, T, B, "reflect" if reflect else "zero"),
          errs, STFT_TOLS, base)


# ---- relative-position attention -----------------------------------------------------------------------------------------
ATTN_NAMES = ("out", "attn", "dq", "dk", "dv", "dembk", "dembv")


def _attn_inputs(gpu, B, H, dk, T, w):
    rng = np.random.default_rng(100 + T)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    q, k, v, gy = t(B, H * dk, T), t(B, H * dk, T), t(B, H * dk, T), t(B, H * dk, T)
    ek, ev = t(1, 2 * w + 1, dk) * dk ** -0.5, t(1, 2 * w + 1, dk) * dk ** -0.5
    mask = torch.ones(B, T)
    mask[B - 1, T - T // 5:] = 0.0  # ragged
    mask[0, T // 3] = 0.0            # an interior hole: a masked query row and a masked key column
    return q, k, v, ek, ev, mask, gy


def _attn_float64(q, k, v, ek, ev, mask, gy, H, w):
    """oracle.vits_oracle.rel_attention's arithmetic (explicit band indexing, masked_fill(-1e4), softmax) in float64."""
    q, k, v, ek, ev = (t.double().requires_grad_(True) for t in (q, k, v, ek, ev))
    B, C, T = q.shape
    dk = C // H
    qh, kh, vh = (t.view(B, H, dk, T).transpose(2, 3) for t in (q, k, v))
    qs = qh / dk ** 0.5
    off = torch.arange(T).unsqueeze(0) - torch.arange(T).unsqueeze(1) + w
    band = ((off >= 0) & (off <= 2 * w)).double()
    offc = off.clamp(0, 2 * w)
    scores = qs @ kh.transpose(-2, -1) + torch.gather(qs @ ek[0].t(), 3, offc.expand(B, H, T, T)) * band
    am = (mask.unsqueeze(2) * mask.unsqueeze(1)).unsqueeze(1)
    p = torch.softmax(scores.masked_fill(am == 0, -1e4), dim=-1)
    pw = torch.stack([torch.diagonal(F.pad(p, (w, w)), offset=r, dim1=2, dim2=3)[..., :T] for r in range(2 * w + 1)], dim=-1)
    out = (p @ vh + pw @ ev[0]).transpose(2, 3).reshape(B, C, T)
    out.backward(gy.double())
    return [out.detach(), p.detach(), q.grad, k.grad, v.grad, ek.grad, ev.grad]


def _attn_gpu(gpu, ins, H, w, p, fused=True):
    from vcvits_amd import ops
    q, k, v, ek, ev, mask, gy = ins
    old = ops._ATTN_FUSED[0]
    ops._ATTN_FUSED[0] = fused
    try:
        ops.set_seed_state(77)
        ts = [t.to(gpu).requires_grad_(True) for t in (q, k, v, ek, ev)]
        before = ops.LAUNCH_COUNTS["attn_fused"]
        out, attn = ops.rel_attention(ts[0], ts[1], ts[2], ts[3], ts[4], mask.to(gpu), H, w, p, training=True, want_attn=True)
        assert ops.LAUNCH_COUNTS["attn_fused"] - before == (1 if fused else 0)
        out.backward(gy.to(gpu))
    finally:
        ops._ATTN_FUSED[0] = old
    return [out.detach(), attn.detach()] + [t.grad for t in ts]


@pytest.mark.parametrize("case", [(2, 2, 32, 31, 4), (2, 2, 64, 129, 1), (1, 2, 32, 256, 4)], ids=lambda c: "B%d-H%d-dk%d-T%d-w%d" % c)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attn_rows_off(gpu, case, p):
    """attn_rows = 0: the workgroup-per-tile fused attention kernels (the path of every T > 256) at T <= 256, forward and
    backward, ragged mask with an interior hole.  p = 0: against the float64 restatement of the oracle's arithmetic at
    tests/test_attention_full_gpu.py's bounds (1e-4, 2e-4 for the two relative tables); p = 0.1: against the unfused path
    with the same counter-based masks at tests/test_attention_fused_gpu.py's 2e-5."""
    B, H, dk, T, w = case
    ins = _attn_inputs(gpu, B, H, dk, T, w)
    if p == 0.0:
        ref = _attn_float64(*ins, H, w)
        tols = {n: (2e-4 if n.startswith("demb") else 1e-4) for n in ATTN_NAMES}
    else:
        ref = [t.cpu() for t in _attn_gpu(gpu, ins, H, w, p, fused=False)]
        tols = {n: 2e-5 for n in ATTN_NAMES}
    base = dict(zip(ATTN_NAMES, (rel(a, b) for a, b in zip(_attn_gpu(gpu, ins, H, w, p), ref))))
    with switched("attn_rows", 0):
        got = _attn_gpu(gpu, ins, H, w, p)
    assert all(torch.isfinite(t).all() for t in got)
    errs = dict(zip(ATTN_NAMES, (rel(a, b) for a, b in zip(got, ref))))
    check("thin / streaming", "attn_rows=0 rel_attention-B%d-H%d-dk%d-T%d-w%d-p%g" % (case + (p,)), errs, tols, base)
    if p > 0:
        frac = float((got[1] == 0).float().mean())
        assert 0.5 * p < frac < 1.0, frac


# ---- the fused ResBlock pair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dil", [(7, 3), (11, 5)])
def test_pair_stream_off(gpu, K, dil):
    """pair_stream = 0: the fused pair kernel declines 64 channels x K >= 7 (and keeps the rest), its entry point refuses the
    launch instead of running it, and the ResBlock falls back to two vcv_conv_bf16io_* launches per pair whose result is
    within tests/test_resblock_pair_gpu.py's bound of that file's CPU reference."""
    from test_resblock_pair_gpu import SLOPE as PSLOPE, _cpu_reference, _inputs
    from vcvits_amd import ops
    from vcvits_amd._lib import ACT_LEAKY as LEAKY
    from vcvits_amd.model.modules import ResBlock1
    C, T, B = 64, 760, 2
    x, w1, b1, w2, b2 = _inputs(B, C, K, T, seed=C * 100 + K * 10 + dil)
    xg, w1g, b1g, w2g, b2g = (t.to(gpu) for t in (x, w1, b1, w2, b2))
    ref = _cpu_reference(x, w1, b1, w2, b2, dil)
    scale, rms = ref.abs().max().item(), ref.pow(2).mean().sqrt().item()
    block = ResBlock1(C, K, (1, 3, 5)).to(gpu).eval()
    with compute_dtype("bf16"), torch.no_grad():
        assert ops.resblock_pair_supported(xg, w1g, w2g, dil)
        fused = ops.resblock_pair_x16(xg, w1g, b1g, w2g, b2g, dil, slope=PSLOPE)
        acc_fused = block.forward_x16(xg, None, 1.0 / 3)
        with switched("pair_stream", 0):
            assert not ops.resblock_pair_supported(xg, w1g, w2g, dil)
            w3 = torch.zeros(C, C, 3, device=gpu)
            assert ops.resblock_pair_supported(xg, w3, w3, dil)  # K = 3 keeps its weights resident: not streamed
            assert ops.resblock_pair_supported(xg[:, :32].contiguous(), w1g[:32, :32].contiguous(), w2g[:32, :32].contiguous(), dil)
            with pytest.raises(RuntimeError):
                ops.resblock_pair_x16(xg, w1g, b1g, w2g, b2g, dil, slope=PSLOPE)
            before = dict(ops.LAUNCH_COUNTS)
            acc = block.forward_x16(xg, None, 1.0 / 3)
            assert ops.LAUNCH_COUNTS.get("pair_fused", 0) == before.get("pair_fused", 0), "the block still used the fused pair"
            assert ops.LAUNCH_COUNTS["bf16io"] == before["bf16io"] + 6
            xt = ops.conv_forward_x16(xg, w1g, b1g, pad=(K - 1) * dil // 2, dil=dil, in_leaky=True, out_act=LEAKY, slope=PSLOPE,
                                      out_dtype=torch.bfloat16)
            y2 = ops.conv_forward_x16(xt, w2g, b2g, pad=(K - 1) // 2, dil=1, res=xg, out_dtype=torch.float16)
    err = (y2.float().cpu() - ref).abs()
    e_f = (fused.float().cpu() - ref).abs()
    record("thin / streaming", "%-58s max=%.2e rms=%.2e  |  max=%.2e rms=%.2e" % (
        "pair_stream=0 pair-C64-K%d-d%d-T760 (two launches | fused)" % (K, dil), err.max().item() / scale,
        err.pow(2).mean().sqrt().item() / rms, e_f.max().item() / scale, e_f.pow(2).mean().sqrt().item() / rms))
    assert err.max().item() <= 6e-3 * scale and err.pow(2).mean().sqrt().item() <= 6e-4 * rms
    # the whole block (three pairs, stage-mean epilogue): two launches per pair against the fused pairs, that file's bound (i)
    d = (acc.float() - acc_fused.float()).abs().max().item()
    assert d <= 6e-3 * max(acc_fused.float().abs().max().item(), 1.0), d


# ---- batched re-pack of cached weights -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,key", [("x3", "pack_tile"), ("bf16", "pack_tile_bf16"), ("bf16", "pack_tile")])
def test_pack_tile_replay(gpu, mode, key):
    """pack_tile / pack_tile_bf16 = 0: the thread-per-item pack kernel inside vcv_pack_many.  Those keys act on the BATCHED
    re-pack only (every pack of a weight-normed tree re-made in one launch after its parameters changed; a per-launch pack
    uses pack_x3_kernel / pack_pk_kernel whatever the switch), so the test goes through ops.weight_norm_many: first use packs
    per launch and records the job, a version bump of v re-normalises and replays the job through vcv_pack_many.  The
    replayed pack must give the bits of the per-launch pack, tiled or not, and the float64 result."""
    from vcvits_amd import ops
    c = conv(2, 128, 128, 300, 5, 1, 2, 1, 1, bias=False)
    x, w, _, _, _ = inputs(c)
    v = w.to(gpu)
    g = v.flatten(1).norm(dim=1).view(-1, 1, 1).contiguous()  # weight_norm(v, |v|) == v up to fp32 rounding
    xg = x.to(gpu)
    tol = TOL_BF16 if mode == "bf16" else TOL
    with MODES[mode](), torch.no_grad():
        (w0,) = ops.weight_norm_many([v], [g])
        wd = w0.cpu().bfloat16().double() if mode == "bf16" else w0.cpu().double()
        xd = x.bfloat16().double() if mode == "bf16" else x.double()
        ref = F.conv1d(xd, wd, padding=c.p)
        y_lazy = ops.conv_forward(xg, w0, pad=c.p)
        ys = {}
        for value in (1, 0):
            with switched(key, value):
                v.add_(0.0)  # (same values, new version: the cached effective weights and their packs are dropped)
                before = ops.LAUNCH_COUNTS.get("pack_many", 0)
                (w1,) = ops.weight_norm_many([v], [g])
                assert ops.LAUNCH_COUNTS.get("pack_many", 0) == before + 1, "the packs were not re-made by vcv_pack_many"
                n0 = ops.LAUNCH_COUNTS[mode]
                ys[value] = ops.conv_forward(xg, w1, pad=c.p)
                assert ops.LAUNCH_COUNTS[mode] == n0 + 1, "the forward did not run on the %s kernels" % mode
    check("weight packs", "%s=0 (%s) replayed pack %s" % (key, mode, cid(c)), {"y": rel(ys[0], ref)}, {"y": tol}, {"y": rel(ys[1], ref)})
    assert torch.equal(ys[1], y_lazy), "the tiled batched pack differs from the per-launch pack"
    assert torch.equal(ys[0], y_lazy), "%s=0: the thread-per-item batched pack differs from the per-launch pack" % key


# ---------------------------------------------------------------------------------------------------------------------
# a host-side guard the m1_lds review turned up
# ---------------------------------------------------------------------------------------------------------------------
def test_one_output_channel_conv_with_more_than_16_taps(gpu):
    """The register kernel of vcv_conv_m1_fwd unrolls 16 taps; its launcher took any K and silently dropped the taps from the
    17th on for launches the LDS-staged kernel does not take (stride > 1, m1_lds = 0).  Such launches now go to the GEMM
    kernels (ops/conv.py) and the entry point refuses them (VCV_EINVAL)."""
    from vcvits_amd._lib import check as ck, lib, ptr, stream
    c = conv(2, 32, 1, 300, 17, 2, 8, 1, 1)
    out = run_gpu(c, gpu)
    check("thin / streaming", cid(c), dists(out, reference(c)), F32_TOLS)
    x, w, b, _, _ = inputs(c)
    y = torch.empty(2, 1, 150, device=gpu)
    xg, wg, bg = x.to(gpu), w.to(gpu), b.to(gpu)
    with pytest.raises(RuntimeError):
        ck(lib().vcv_conv_m1_fwd(ptr(xg), ptr(wg), ptr(bg), ptr(y), 2, 32, 300, 150, 1, 17, 2, 1, 8, 0, ACT_NONE, SLOPE, stream()),
           "vcv_conv_m1_fwd")


# ---------------------------------------------------------------------------------------------------------------------
# last: nothing leaked
# ---------------------------------------------------------------------------------------------------------------------
def test_every_switch_is_back_at_its_default(gpu):
    assert KEYS_AT_IMPORT is not None, "the library could not be read when this file was imported"
    keys, state = _read_state()
    assert keys == KEYS_AT_IMPORT, {k: (v, KEYS_AT_IMPORT[k]) for k, v in keys.items() if v != KEYS_AT_IMPORT[k]}
    assert state == STATE_AT_IMPORT, (state, STATE_AT_IMPORT)

"""The split-operand form of the LDS-DMA weight-gradient kernel (csrc/wgrad_dma.hip, VcvWgradArgs.split_terms = 6: fp32
fragments split into three bf16 terms each in registers, six bf16 MFMA products) against the float64 CPU reference of the same
operation (tests/wgrad_f64.py).

vcv_conv_wgrad is called THROUGH THE C ABI with a hand-filled VcvWgradArgs, vcv_conv_x3_set_all(1) admitting every shape (the
setting and the number of terms come back in `finally`); before every launch the host-only query vcv_conv_wgrad_split_terms
must say that the launch runs in the arithmetic the test means.  test_routing_through_ops then checks what ops.conv_wgrad
hands over under the Python switches.

Conventions of tests/test_wgrad_mfma_abi_gpu.py: dw, dbias and the slab are views between 1024 sentinel floats on each side
(the slab pre-filled with NaN); distances are max|got - ref| / max|ref|; bounds TOL_DW = 3e-5, TOL_DB = 2e-5.  Every distance
is written to profiles/wgrad_dma_split_parity.txt next to d32, the distance of the float32 CPU run of the reference from its
float64 run.

kind = "exact": operands are integers in [-8, 8], `b` through leaky-ReLU with slope 0.5, alpha = 0.5, dw and dbias preloaded
with integers: every partial sum is a multiple of 1/4 below 2^22 (test_case_table asserts it), any order is exact and the
result must be BIT-EQUAL to float64 cast to float32.

The term probe: `a` has one nonzero position per row, so every dw element is ONE product, which must come out bit for bit:
12 x 12 significant bits need the planes (0,0) (0,1) (1,0) (1,1); 24 bits times a power of two need (2,0), the mirror (0,2).
A missing or mispaired term plane fails there, where the 3e-5 bound alone would let it through.

Slab mode (deterministic combine) is launched twice and must give the same bits.  No test shape is the workload's own."""
import collections
import contextlib
import ctypes
import functools
import os
import re
import zlib

import numpy as np
import pytest
import torch

import wgrad_f64 as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
TOL_DW, TOL_DB = 3e-5, 2e-5
GUARD, SENT = 1024, 12345.0
KINDS = ("normal", "exact")
WG_TILES = ((128, 256), (128, 128), (128, 64), (64, 256), (64, 128), (64, 64), (32, 128))  # wgrad_dma.hip, WG_TILES
PLAN_LINE = re.compile(r"^wgrad plan M\d+ C\d+ K\d+ U\d+ s\d+ tile (\d+x\d+): occ \d+ tiles \d+ total \d+ Z \d+ cost [\d.]+ us lds \d+( terms 6)?$")

Case = collections.namedtuple("Case", "grp B Mg Cg Ta Tb P K s dj off")


def conv_tb(Ta, K, s, pad, dil=1):
    """input rows of the Conv whose output has Ta rows (no rows left over)"""
    return (Ta - 1) * s + (K - 1) * dil + 1 - 2 * pad


def convT_tb(Ta, K, s, pad):
    return (Ta - 1) * s - 2 * pad + K


def cid(c):
    return "%s-B%d-M%d-C%d-Ta%d-Tb%d-P%d-K%d-s%d-dj%d-off%d" % tuple(c)


# every tile candidate: a ragged last m-tile, N = 480 (no multiple of a tile width), a last stage of 13 positions
TILE = Case("tile", 2, 160, 96, 141, 141, 1, 5, 1, 1, -2)
# the strided kernel: period layouts at stride 3 (narrow and the widest period), one row at stride 2
STRIDED = [Case("strided", 2, 128, 32, 67, conv_tb(67, 5, 3, 2), 3, 5, 3, 1, -2),
           Case("strided", 3, 64, 64, 3, conv_tb(3, 5, 3, 2), 37, 5, 3, 1, -2),
           Case("strided", 2, 64, 64, 43, conv_tb(43, 5, 2, 2), 3, 5, 2, 1, -2)]
# wide periods at unit stride (the layout of the 1024-channel period layers)
WIDE = [Case("wide", 3, 64, 64, 6, 6, 37, 5, 1, 1, -2), Case("wide", 2, 64, 64, 10, 10, 13, 5, 1, 1, -2)]
# tap geometry
TAPS = [Case("taps", 2, 64, 96, 130, 130, 1, 1, 1, 1, 0)]
TAPS += [Case("taps", 2, 64, 64, 130, conv_tb(130, K, 1, K // 2), 1, K, 1, 1, -(K // 2)) for K in (3, 7, 11, 16)]
TAPS.append(Case("taps", 2, 64, 64, 130, conv_tb(130, 3, 1, 5, 5), 1, 3, 1, 5, -5))       # dilation 5, pad 5
TAPS.append(Case("taps", 2, 64, 32, 130, convT_tb(130, 4, 2, 1), 1, 4, 2, 1, -1))         # ConvTranspose roles: a = x, b = dy
TAPS.append(Case("taps", 2, 64, 64, 130, conv_tb(130, 5, 1, 2) - 2, 1, 5, 1, 1, -2))      # Tb two rows short: taps fall outside
OPTS = Case("opts", 2, 64, 64, 130, 130, 1, 3, 1, 1, -1)
SWEEP = [TILE] + STRIDED + WIDE + TAPS + [OPTS]
PROBES = (Case("probe", 2, 64, 32, 130, 130, 1, 3, 1, 1, -1), Case("probe", 2, 128, 32, 67, conv_tb(67, 5, 3, 2), 3, 5, 3, 1, -2))
ROUTED = Case("routed", 2, 64, 64, 200, 200, 1, 7, 1, 1, -3)  # K 7: vcv_wgrad_x3 declines it under the default setting


def dma_eligible(c):
    """wgrad_dma_eligible of csrc/wgrad_dma.hip for the plain options of this file"""
    return c.Mg >= 32 and c.Cg * c.K >= 96 and c.Ta * c.P >= 64 and 1 <= c.s <= 8


def test_case_table():
    """Host only: every case is one wgrad_dma_kernel takes, the exact pass stays exact, and the table holds what the
    docstring says it holds."""
    for c in SWEEP + list(PROBES) + [ROUTED]:
        assert dma_eligible(c), c
        assert 8 * 8 * c.B * c.Ta * c.P < (1 << 24) // 4, c
    assert TILE.Mg % 128 and TILE.Mg % 64 and TILE.Mg % 32 == 0 and TILE.Mg >= 128 // 2 + 1
    assert all((TILE.Cg * TILE.K) % bn for _, bn in WG_TILES) and TILE.Ta % 64 == 13
    assert {c.s for c in STRIDED} == {2, 3} and {c.P for c in STRIDED} == {3, 37}
    assert {c.K for c in TAPS} == {1, 3, 4, 5, 7, 11, 16} and any(c.dj == 5 and c.off == -5 for c in TAPS)
    assert any(c.Tb == conv_tb(c.Ta, c.K, c.s, -c.off, c.dj) - 2 for c in TAPS)


def test_abi_field():
    """split_terms is the LAST field of VcvWgradArgs and a fresh struct holds 0 there (= fp32-input MFMA, what every caller
    that does not know the field gets)."""
    from vcvits_amd._lib import VcvWgradArgs
    assert VcvWgradArgs._fields_[-1][0] == "split_terms" and VcvWgradArgs().split_terms == 0
    assert VcvWgradArgs.split_terms.offset == VcvWgradArgs.slab_floats.offset + 8
    assert ctypes.sizeof(VcvWgradArgs) == VcvWgradArgs.split_terms.offset + 8  # (int32 + tail padding of an 8-aligned struct)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and float64 references: made once per (case, kind) and shared
# ---------------------------------------------------------------------------------------------------------------------
EXACT = dict(alpha=0.5, b_tf=W.TF_LEAKY, slope=0.5)


@functools.lru_cache(maxsize=None)
def inputs(c, kind):
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    if kind == "exact":
        t = lambda *sh: torch.from_numpy(rng.integers(-8, 9, sh).astype(np.float32))
    else:
        t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    return t(c.B, c.Mg, c.Ta, c.P), t(c.B, c.Cg, c.Tb, c.P), t(c.Mg, c.Cg, c.K), t(c.Mg)


@functools.lru_cache(maxsize=None)
def reference(c, kind, a_tf=W.TF_NONE, b_tf=W.TF_NONE, slope=0.1):
    """(float64 dw, float64 dbias, d32 of dw, d32 of dbias): without alpha and preloads."""
    a, b, _, _ = inputs(c, kind)
    dw = W.wgrad(a, b, c.K, c.s, c.dj, c.off, a_tf, b_tf, slope)
    dw32 = W.wgrad(a, b, c.K, c.s, c.dj, c.off, a_tf, b_tf, slope, dtype=torch.float32)
    db = W.dbias(a)
    return dw, db, W.dist(dw32, dw), W.dist(W.dbias(a, torch.float32), db)


@functools.lru_cache(maxsize=4)
def on_gpu(c, kind, gpu):
    return tuple(t.to(gpu) for t in inputs(c, kind))


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


@contextlib.contextmanager
def all_shapes(terms=6):
    from vcvits_amd._lib import lib
    L = lib()
    old = (L.vcv_conv_x3_get_terms(), L.vcv_conv_x3_get_all())
    try:
        assert L.vcv_conv_x3_set_terms(terms) == 0 and L.vcv_conv_x3_set_all(1) == 0
        yield
    finally:
        L.vcv_conv_x3_set_terms(old[0])
        L.vcv_conv_x3_set_all(old[1])


@contextlib.contextmanager
def switched(key, value):
    from vcvits_amd import tuning
    old = tuning.kernel_get(key)
    tuning.kernel_set(key, value)
    try:
        yield
    finally:
        tuning.kernel_set(key, old)


Out = collections.namedtuple("Out", "status dw db terms")


def abi(gpu, c, tensors, *, split=6, alpha=1.0, a_tf=W.TF_NONE, b_tf=W.TF_NONE, slope=0.1, preload=False, want_db=False, slab=False):
    """One call of vcv_conv_wgrad -> Out(status, dw, dbias or None, what vcv_conv_wgrad_split_terms said); the sentinels around
    dw, dbias and the slab are checked here."""
    from vcvits_amd._lib import VcvWgradArgs, lib, stream
    a, b, pre_dw, pre_db = tensors
    dw = Guarded((c.Mg, c.Cg, c.K), gpu, pre_dw if preload else 0.0)
    db = Guarded((c.Mg,), gpu, pre_db if preload else 0.0) if want_db else None
    nw = c.Mg * c.Cg * c.K
    sl = Guarded((6 * nw,), gpu, float("nan")) if slab else None
    A = VcvWgradArgs()
    A.a, A.b, A.dw, A.dbias = a.data_ptr(), b.data_ptr(), dw.t.data_ptr(), db.t.data_ptr() if db else None
    A.B, A.G, A.Cg, A.Mg, A.Ta, A.Tb, A.P, A.K = c.B, 1, c.Cg, c.Mg, c.Ta, c.Tb, c.P, c.K
    A.s, A.dj, A.off, A.a_tf, A.b_tf, A.transpose_out, A.alpha, A.slope = c.s, c.dj, c.off, a_tf, b_tf, 0, alpha, slope
    if slab:
        A.slab, A.slab_floats = sl.t.data_ptr(), 6 * nw
    A.split_terms = split
    assert lib().vcv_conv_wgrad_takes_dma(ctypes.byref(A)) == 1, cid(c)
    terms = lib().vcv_conv_wgrad_split_terms(ctypes.byref(A))
    st = lib().vcv_conv_wgrad(ctypes.byref(A), stream())
    torch.cuda.synchronize()
    assert dw.intact(), "a write outside dw"
    assert db is None or db.intact(), "a write outside dbias"
    assert sl is None or sl.intact(), "a write outside the slab"
    return Out(st, dw.t, db.t if db else None, terms)


_parity = {}


def record(section, line):
    """Keep the measured distances in profiles/wgrad_dma_split_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "wgrad_dma_split_parity.txt"), "w") as f:
        f.write("# tests/test_wgrad_dma_split_gpu.py: max-norm distance of vcv_conv_wgrad with split_terms = 6 (wgrad_dma_kernel, six bf16\n"
                "# product terms) from the float64 CPU reference (tests/wgrad_f64.py), relative to max|reference|; d32 is the distance of\n"
                "# the float32 CPU run of the reference from its float64 run.  Bounds: dw 3e-5, dbias 2e-5.  Cases are\n"
                "# group-B-Mg-Cg-Ta-Tb-P-K-s-dj-off.  The exact pass and the term probe (bit-equal to float64) have no distances.\n")
        for name in _parity:
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def run_and_check(gpu, c, kind, section, tag="", slab=False, **kw):
    """One case in the split form: the library says six terms, the float64 reference is met within the bounds (normal) or
    bit for bit (exact), slab launches repeat bit for bit.  In the exact pass alpha / b_tf / slope / preload are EXACT's
    unless given.  -> dw"""
    opts = dict(kw)
    if kind == "exact":
        for k, v in dict(EXACT, preload=True).items():
            opts.setdefault(k, v)
    alpha, preload = opts.get("alpha", 1.0), opts.get("preload", False)
    a_tf, b_tf, slope = opts.get("a_tf", W.TF_NONE), opts.get("b_tf", W.TF_NONE), opts.get("slope", 0.1)
    want_db = opts.setdefault("want_db", a_tf == W.TF_NONE)
    _, _, pre_dw, pre_db = inputs(c, kind)
    with all_shapes():
        r = abi(gpu, c, on_gpu(c, kind, gpu), slab=slab, **opts)
        r2 = abi(gpu, c, on_gpu(c, kind, gpu), slab=slab, **opts) if slab else None
    assert r.terms == 6, "%s: the library does not run the split form (%d)" % (cid(c), r.terms)
    assert r.status == 0, r.status
    if slab:
        assert r2.status == 0 and torch.equal(r.dw, r2.dw), "%s %s: the slab combine is not bit-reproducible" % (cid(c), tag)
    dw64, db64, d32, d32b = reference(c, kind, a_tf, b_tf, slope)
    if preload:
        dw64, db64 = pre_dw.double() + float(np.float32(alpha)) * dw64, pre_db.double() + db64
    else:
        dw64 = float(np.float32(alpha)) * dw64
    if kind == "exact":
        assert bool((dw64.float().double() == dw64).all())
        assert torch.equal(r.dw.cpu(), dw64.float()), "%s %s: dw is not the float64 reference's bits (distance %.3e)" % (
            cid(c), tag, W.dist(r.dw, dw64))
        if want_db:
            assert torch.equal(r.db.cpu(), db64.float()), "%s %s: dbias is not exact (distance %.3e)" % (cid(c), tag, W.dist(r.db, db64))
        return r.dw
    e = W.dist(r.dw, dw64)
    eb = W.dist(r.db, db64) if want_db else None
    record(section, "%-52s %-28s dw=%.1e%s  | d32 dw=%.1e db=%.1e" % (cid(c), tag, e, "" if eb is None else " db=%.1e" % eb, d32, d32b))
    assert e <= TOL_DW, "%s %s: dw off by %.3e (bound %.1e)" % (cid(c), tag, e, TOL_DW)
    assert eb is None or eb <= TOL_DB, "%s %s: dbias off by %.3e (bound %.1e)" % (cid(c), tag, eb, TOL_DB)
    return r.dw


# ---------------------------------------------------------------------------------------------------------------------
# every tile candidate
# ---------------------------------------------------------------------------------------------------------------------
_planned = set()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slab", [False, True], ids=["atomics", "slab"])
@pytest.mark.parametrize("cand", range(7))
def test_every_tile(gpu, capfd, cand, slab, kind):
    """wgrad_tile = 0..6 in the split form, combined with atomics and through slabs.  wgrad_verbose prints each plan that is
    evaluated (plans are memoised per shape, arithmetic and forced tile): the first launch of a (candidate, mode) must print
    exactly the forced tile with the split form's mark."""
    capfd.readouterr()
    with switched("wgrad_verbose", 1), switched("wgrad_tile", cand):
        run_and_check(gpu, TILE, kind, "every tile candidate", "tile=%dx%d %s" % (WG_TILES[cand] + ("slab" if slab else "atomics",)), slab=slab,
                      want_db=not slab)  # (a caller that hands over a slab sums the bias itself: include/vcvits_hip.h)
    lines = [PLAN_LINE.match(ln) for ln in capfd.readouterr().err.splitlines() if ln.startswith("wgrad plan ")]
    assert all(lines), "a plan line test_switch_parity_gpu.py could not parse"
    assert {m.group(1) for m in lines} <= {"%dx%d" % WG_TILES[cand]} and all(m.group(2) for m in lines), [m.group(0) for m in lines]
    if (cand, slab, EXACT["b_tf"] if kind == "exact" else 0) not in _planned:
        assert lines, "no plan was evaluated for a shape launched for the first time"
        _planned.add((cand, slab, EXACT["b_tf"] if kind == "exact" else 0))


# ---------------------------------------------------------------------------------------------------------------------
# strided kernel, wide periods, tap geometry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", STRIDED + WIDE + TAPS, ids=cid)
def test_parity(gpu, c, kind):
    """The strided form at strides 3 and 2, wide periods at unit stride and the tap geometries, with the bias row sums
    collected in the same launch; once with atomics and once through slabs."""
    sec = {"strided": "strided kernel", "wide": "wide period at unit stride", "taps": "tap geometry"}[c.grp]
    run_and_check(gpu, c, kind, sec, "atomics")
    run_and_check(gpu, c, kind, sec, "slab", slab=True, want_db=False)


# ---------------------------------------------------------------------------------------------------------------------
# transforms and options
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind_slope", [("normal", 0.1), ("exact", 0.5)], ids=lambda ks: "%s-slope%g" % ks)
@pytest.mark.parametrize("tf", [(1, 0), (0, 1), (1, 1)], ids=["a", "b", "ab"])
def test_operand_leaky_relu(gpu, tf, kind_slope):
    """a_tf / b_tf = LEAKY in the three combinations the kernel has (slope 0.1; the exact pass 0.5 -- 0.1 times an integer has
    more than 24 bits), on a plain row and on a strided period row."""
    kind, slope = kind_slope
    for c in (OPTS, STRIDED[0]):
        run_and_check(gpu, c, kind, "transforms and options", "a_tf=%d b_tf=%d slope=%g" % (tf[0], tf[1], slope), a_tf=tf[0], b_tf=tf[1],
                      slope=slope)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_alpha_onto_a_preloaded_dw(gpu, kind):
    """alpha = 0.5 onto a preloaded dw (and the bias sums onto a preloaded dbias), with atomics and through slabs."""
    run_and_check(gpu, OPTS, kind, "transforms and options", "alpha=0.5 preload", alpha=0.5, preload=True)
    run_and_check(gpu, OPTS, kind, "transforms and options", "alpha=0.5 preload slab", alpha=0.5, preload=True, slab=True, want_db=False)
    run_and_check(gpu, STRIDED[0], kind, "transforms and options", "alpha=0.5 preload", alpha=0.5, preload=True)


# ---------------------------------------------------------------------------------------------------------------------
# term probe
# ---------------------------------------------------------------------------------------------------------------------
def _bits(rng, shape, nbits):
    """numbers with exactly `nbits` significant bits (top and bottom bit set), random sign, exponents -2 .. 2"""
    mant = rng.integers(1 << (nbits - 1), 1 << nbits, shape) | 1
    if nbits == 1:
        mant = np.ones(shape, dtype=np.int64)
    v = mant.astype(np.float64) * np.exp2(rng.integers(-2, 3, shape) - (nbits - 1)) * rng.choice([-1.0, 1.0], shape)
    assert bool((v.astype(np.float32).astype(np.float64) == v).all())
    return torch.from_numpy(v.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [(12, 12), (24, 1), (1, 24)], ids=["12x12", "24x1", "1x24"])
@pytest.mark.parametrize("c", PROBES, ids=cid)
def test_term_probe(gpu, c, bits):
    """One nonzero position per row of `a`: every dw element is a single product of at most 24 significant bits and must be
    that product's bits.  12 x 12 bits: terms (0,0) (0,1) (1,0) (1,1); 24 x 1: (2,0) and (1,0); 1 x 24: (0,2) and (0,1)."""
    rng = np.random.default_rng(zlib.crc32(repr((tuple(c), bits)).encode()))
    a = torch.zeros(c.B, c.Mg, c.Ta, c.P)
    vals = _bits(rng, (c.Mg,), bits[0])
    for m in range(c.Mg):
        a[rng.integers(c.B), m, rng.integers(c.Ta), rng.integers(c.P)] = vals[m]
    b = _bits(rng, (c.B, c.Cg, c.Tb, c.P), bits[1])
    ref = W.wgrad(a, b, c.K, c.s, c.dj, c.off)
    assert bool((ref.float().double() == ref).all()) and bool((ref != 0).any())
    for slab in (False, True):
        with all_shapes():
            r = abi(gpu, c, (a.to(gpu), b.to(gpu), None, None), slab=slab)
        assert r.status == 0 and r.terms == 6
        assert torch.equal(r.dw.cpu(), ref.float()), "%s %dx%d bits %s: a product term is missing or mispaired (distance %.3e)" % (
            cid(c), bits[0], bits[1], "slab" if slab else "atomics", W.dist(r.dw, ref))


# ---------------------------------------------------------------------------------------------------------------------
# refusals and switches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_switches_keep_the_fp32_body(gpu, capfd):
    """split_terms = 0, wgrad_dma_split = 0 and nine-term mode each run the fp32-input body: the library says 0 terms, the slab
    results have the same bits as each other (and other bits than the split form's), and the plan line of the shape carries
    no split mark; with the key off the plan memoised for split_terms = 0 is reused (nothing is planned again)."""
    c = Case("switch", 2, 96, 64, 173, 173, 1, 3, 1, 1, -1)
    rng = np.random.default_rng(7)
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    a, b = t(c.B, c.Mg, c.Ta, c.P), t(c.B, c.Cg, c.Tb, c.P)
    ts = (a.to(gpu), b.to(gpu), None, None)
    ref = W.wgrad(a, b, c.K, c.s, c.dj, c.off)
    capfd.readouterr()
    with switched("wgrad_verbose", 1):
        with all_shapes():
            r0 = abi(gpu, c, ts, split=0, slab=True)
            l0 = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("wgrad plan ")]
            with switched("wgrad_dma_split", 0):
                rk = abi(gpu, c, ts, split=6, slab=True)
            lk = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("wgrad plan ")]
            r6 = abi(gpu, c, ts, split=6, slab=True)
            l6 = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("wgrad plan ")]
        with all_shapes(terms=9):
            r9 = abi(gpu, c, ts, split=6, slab=True)
    assert [r.status for r in (r0, rk, r6, r9)] == [0] * 4
    assert (r0.terms, rk.terms, r6.terms, r9.terms) == (0, 0, 6, 0)
    assert l0 and all(PLAN_LINE.match(ln) and not ln.endswith(" terms 6") for ln in l0), l0
    assert lk == [], lk
    assert l6 and all(PLAN_LINE.match(ln) and ln.endswith(" terms 6") for ln in l6), l6
    assert torch.equal(r0.dw, rk.dw) and torch.equal(r0.dw, r9.dw)
    assert not torch.equal(r0.dw, r6.dw), "split_terms = 6 gave the fp32-input body's bits"
    for name, r in (("split_terms=0", r0), ("split_terms=6", r6)):
        e = W.dist(r.dw, ref)
        record("refusals and switches", "%-52s %-28s dw=%.1e" % (cid(c), name, e))
        assert e <= TOL_DW, (name, e)


@pytest.mark.gpu
@pytest.mark.parametrize("terms", [1, 3, 5, 7, 9, -6, 1 << 20])
def test_other_term_counts_are_refused(gpu, terms):
    """Anything other than 0 or 6 in the field is VCV_EINVAL, and nothing is written."""
    c = OPTS
    with all_shapes():
        r = abi(gpu, c, on_gpu(c, "normal", gpu), split=terms, want_db=True)
    assert r.status == EINVAL, r.status
    assert not bool(r.dw.any()) and not bool(r.db.any()), "a refused call wrote to an output"


# ---------------------------------------------------------------------------------------------------------------------
# routing through ops
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def ops_state():
    """Every Python switch and library setting the routing reads comes back."""
    from vcvits_amd import ops
    from vcvits_amd._lib import lib
    old = (ops.compute_dtype(), ops._USE_X3[0], lib().vcv_conv_x3_get_terms(), lib().vcv_conv_x3_get_all(), ops._USE_X3_WGRAD[0])
    try:
        yield ops
    finally:
        ops.set_compute_dtype(old[0])
        ops.set_f32_split(old[1], terms=old[2], all_shapes=bool(old[3]), wgrad=old[4])


@contextlib.contextmanager
def wgrad_spy():
    """What ops.conv._launch_wgrad handed to the library: split_terms, and whether the launch went to vcv_conv_wgrad."""
    from vcvits_amd import ops
    seen = []
    orig = ops.conv._launch_wgrad

    def spy(a):
        before = ops.LAUNCH_COUNTS["wgrad"]
        orig(a)
        seen.append({"split_terms": a.split_terms, "conv_wgrad": ops.LAUNCH_COUNTS["wgrad"] != before})

    ops.replace("_launch_wgrad", spy)
    try:
        yield seen
    finally:
        ops.replace("_launch_wgrad", orig)


@pytest.mark.gpu
def test_routing_through_ops(gpu):
    """On a shape vcv_wgrad_x3 declines (K 7), ops.conv_wgrad under the default setting hands split_terms = 6 to
    vcv_conv_wgrad; under set_f32_split(True, wgrad=False), set_f32_split(False), nine terms and bf16 mode it hands over 0.
    Every result meets float64 at its bound."""
    c = ROUTED
    a, b, _, _ = inputs(c, "normal")
    ag, bg = a[..., 0].contiguous().to(gpu), b[..., 0].contiguous().to(gpu)
    ref = reference(c, "normal")[0]
    modes = (("default", lambda ops: ops.set_f32_split(True, terms=6, all_shapes=False, wgrad=True), 6, True),
             ("wgrad=False", lambda ops: ops.set_f32_split(True, terms=6, all_shapes=False, wgrad=False), 0, True),
             ("split off", lambda ops: ops.set_f32_split(False), 0, True),
             ("nine terms", lambda ops: ops.set_f32_split(True, terms=9, all_shapes=False, wgrad=True), 0, True),
             ("bf16", lambda ops: ops.set_compute_dtype("bf16"), 0, None))
    for name, setup, want, to_conv_wgrad in modes:
        with ops_state() as ops, wgrad_spy() as seen:
            ops.set_compute_dtype("f32")
            setup(ops)
            got = ops.conv_wgrad(ag, bg, (c.Mg, c.Cg, c.K), stride=c.s, pad=-c.off, dil=c.dj)
            torch.cuda.synchronize()
        assert len(seen) == 1 and seen[0]["split_terms"] == want, (name, seen)
        assert to_conv_wgrad is None or seen[0]["conv_wgrad"] == to_conv_wgrad, (name, seen)
        if name != "bf16":  # (bf16 mode rounds the operands: tests/test_wgrad_mfma_abi_gpu.py holds it to its own reference)
            e = W.dist(got, ref)
            record("routing through ops", "%-52s %-28s split_terms=%d dw=%.1e" % (cid(c), name, seen[0]["split_terms"], e))
            assert e <= TOL_DW, (name, e)

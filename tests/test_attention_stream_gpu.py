"""The streamed relative-position attention (csrc/attention_stream.hip behind vcv_rel_attn_stream_fwd) at the edges of its
tiling, against a float64 CPU reference, and its routing in ops.rel_attention.

The kernel is called THROUGH THE C ABI, as tests/test_attention_abi_gpu.py calls the fused kernels, so the routing cannot send
a case elsewhere; test_routing_* then check what ops.rel_attention sends where.

Reference: tests/attention_rows_f64.py (the output for a list of query rows; tests/test_attention_stream_cpu.py pins it to
tests/attention_f64.py) on float64 copies of the float32 inputs: every row up to T = 4,099, about 60 rows at T = 20,000.
Distances are max|a - b| / max|b|.  Bound, the policy of tests/test_attention_abi_gpu.py unchanged: max(16 * d32, 2e-6) capped
at 1e-4, where d32 is the distance of the FLOAT32 CPU run of the reference from its float64 run for the same case and rows.

The tiling the edges of the case table assume: 128 queries per workgroup, 32 per wave, key tiles of 32.
Every distance is appended to profiles/attention_parity.txt.
"""
import collections
import contextlib
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import attention_f64 as A
import attention_rows_f64 as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
FACTOR, FLOOR, CAP = 16, 2e-6, 1e-4
GUARD, SENT = 1024, 12345.0
QB, QW, KT = 128, 32, 32  # queries per workgroup, per wave; keys per tile

Case = collections.namedtuple("Case", "B H dk T w mask")

CASES = [
    Case(1, 1, 32, 1, 4, "ones"),              # one query, one key
    Case(2, 1, 32, 5, 7, "ragged"),            # T <= w: band clipped on both sides
    Case(2, 2, 64, 32, 0, "hole"),             # w = 0, an exact key tile
    Case(2, 1, 64, 33, 4, "ragged"),           # one key in the second tile
    Case(1, 2, 32, 128, 4, "ones"),            # exactly one workgroup
    Case(2, 1, 32, 129, 7, "ragged+hole"),     # one query in the second workgroup; the band crosses wave and workgroup
    Case(3, 1, 64, 257, 4, "mixed"),           # ones | ragged | all zero: an all-masked batch row is uniform over T
    Case(2, 2, 64, 897, 4, "ragged+hole"),     # first T routed by default
    Case(1, 2, 32, 1030, 4, "head40"),         # keys 0..39 masked: the running max starts at -1e4 and is rescaled
    Case(2, 1, 64, 4099, 7, "ragged"),         # many tiles, odd tail
    Case(1, 2, 32, 20000, 4, "ragged+hole"),   # long; compared on ~60 rows
]
ROUTED, MIN_T_CASE, LONG = CASES[7], CASES[6], CASES[10]


def cid(c):
    return "B%d-H%d-dk%d-T%d-w%d-%s" % tuple(c)


def make_mask(c):
    B, T = c.B, c.T
    m = torch.ones(B, T)
    if c.mask == "mixed":  # element 0 all ones, element 1 ragged, element 2 all zero
        m[1, T - T // 5:] = 0.0
        m[2, :] = 0.0
        return m
    if c.mask == "head40":
        m[0, :40] = 0.0
        return m
    if "ragged" in c.mask:
        m[B - 1, T - T // 5:] = 0.0
    if "hole" in c.mask:
        m[0, T // 3] = 0.0
    return m


def rows_of(c):
    """Every row, or at T = 20,000 the rows at the tile, band and mask edges plus 40 random ones."""
    T, w = c.T, c.w
    if T <= 4099:
        return list(range(T))
    edges = {0, 1, w, 31, 32, T // 3 - 1, T // 3, T // 3 + 1, T - T // 5 - 1, T - T // 5} | set(range(T - 33, T))
    rng = np.random.default_rng(T)
    return sorted(edges | set(int(r) for r in rng.integers(0, T, size=40)))


def test_case_table_reaches_every_edge():
    """CPU: the table above against the tiling it assumes."""
    cdiv = lambda a, b: -(-a // b)
    T = [c.T for c in CASES]
    assert 1 in T and KT in T and KT + 1 in T and QB in T and QB + 1 in T and 897 in T
    assert any(c.T <= c.w for c in CASES) and any(c.w == 0 for c in CASES) and any(c.w == 7 for c in CASES)
    assert {c.dk for c in CASES} == {32, 64}
    assert any(c.T % KT not in (0, 1) and cdiv(c.T, KT) > 100 for c in CASES)          # many tiles, odd tail
    assert any(not bool(make_mask(c)[b].any()) for c in CASES for b in range(c.B))      # an all-masked batch row
    assert any(not bool(make_mask(c)[0, :KT].any()) and bool(make_mask(c)[0, KT + 8:].all()) for c in CASES)  # a masked first tile
    c = CASES[5]   # the band of the last query of workgroup 0 reaches into workgroup 1, and the other way round
    assert c.T > QB and c.w > 0 and 2 * c.w + 1 <= 16
    assert all(c.B * c.H <= 4 for c in CASES)
    r = rows_of(LONG)
    assert 55 <= len(r) <= 100 and {0, 1, LONG.w, 31, 32, LONG.T - 33, LONG.T - 1} <= set(r)
    m = make_mask(LONG)[0]
    assert any(m[i] != m[i + 1] for i in r if i + 1 < LONG.T)  # rows on both sides of a mask edge


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references: made once per case and shared
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(c):
    """q, k, v, embk, embv, mask (float32, CPU): standard normal, q scaled by 2 (rows are not near-uniform), the tables by
    dk^-0.5."""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    C = c.H * c.dk
    q, k, v = 2.0 * t(c.B, C, c.T), t(c.B, C, c.T), t(c.B, C, c.T)
    ek, ev = t(1, 2 * c.w + 1, c.dk) * c.dk ** -0.5, t(1, 2 * c.w + 1, c.dk) * c.dk ** -0.5
    return q, k, v, ek, ev, make_mask(c)


def _rows_chunked(c, dtype):
    rows = rows_of(c)
    return torch.cat([AR.rel_attention_rows(*inputs(c), rows[i:i + 1024], dtype=dtype) for i in range(0, len(rows), 1024)], dim=2)


@functools.lru_cache(maxsize=None)
def reference(c):
    """(float64 out[:, :, rows], d32)"""
    r64 = _rows_chunked(c, torch.float64)
    return r64, A.dist(_rows_chunked(c, torch.float32), r64)


def bound(d32):
    return min(max(FACTOR * d32, FLOOR), CAP)


@functools.lru_cache(maxsize=2)
def on_gpu(c, gpu):
    return tuple(t.to(gpu) for t in inputs(c))


class Guarded:
    """n floats pre-filled with NaN (an element left unwritten stays NaN) between two runs of GUARD sentinel floats."""

    def __init__(self, shape, device):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device=device)
        self.buf[:GUARD] = SENT
        self.buf[GUARD + n:] = SENT
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        n = self.t.numel()
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + n:] == SENT).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())


def abi_fwd(c, ins):
    """-> status, out (Guarded)"""
    from vcvits_amd._lib import lib, ptr, stream
    q, k, v, ek, ev, mask = ins
    out = Guarded((c.B, c.H * c.dk, c.T), k.device)
    st = lib().vcv_rel_attn_stream_fwd(ptr(q) if q is not None else None, ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(mask), ptr(out.t),
                                       c.B, c.H, c.dk, c.T, c.w, c.dk ** -0.5, stream())
    return st, out


@contextlib.contextmanager
def compute_mode(mode):
    from vcvits_amd import ops
    old = ops.compute_dtype()
    ops.set_compute_dtype(mode)
    try:
        yield
    finally:
        ops.set_compute_dtype(old)


MARK = "# ---- tests/test_attention_stream_gpu.py"
_lines = []


def record(line):
    """Append to profiles/attention_parity.txt: what the file held before this module's block, then every line measured so far."""
    print(line)
    if line not in _lines:
        _lines.append(line)
    path = os.path.join(ROOT, "profiles", "attention_parity.txt")
    head = open(path).read() if os.path.exists(path) else ""
    head = head.split(MARK)[0].rstrip("\n")
    with open(path, "w") as f:
        f.write(head + "\n\n" + MARK + ": vcv_rel_attn_stream_fwd (keys and values streamed) against tests/attention_rows_f64.py,\n"
                "# as out=kernel/d32/bound over the rows compared.  Cases are B-H-dk-T-window-mask.\n\n[streamed forward]\n")
        f.write("\n".join(_lines) + "\n")


def check(tag, got, ref, d32, bnd=None):
    """Write the figure down first, then assert."""
    err, bnd = A.dist(got, ref), bound(d32) if bnd is None else bnd
    record("%-58s out=%.1e/%.1e/%.1e" % (tag, err, d32, bnd))
    assert err <= bnd, "%s: out off by %.3e (d32 %.3e, bound %.3e)" % (tag, err, d32, bnd)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel at the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_forward(gpu, c):
    ins = on_gpu(c, gpu)
    ref, d32 = reference(c)
    st, out = abi_fwd(c, ins)
    assert st == 0, st
    assert out.intact(), "a write outside the buffer"
    assert not bool(torch.isnan(out.t).any()), "out has elements the kernel did not write"
    st, again = abi_fwd(c, ins)
    assert st == 0 and torch.equal(out.t, again.t), "out differs between two identical launches"
    rows = rows_of(c)
    check("%s rows=%d" % (cid(c), len(rows)), out.t[:, :, rows], ref, d32)
    m = make_mask(c)
    for b in range(c.B):
        if not bool(m[b].any()):  # an all-masked batch row: uniform over all T keys, whatever q and k hold
            v, ev = inputs(c)[2][b].double(), inputs(c)[4][0].double()
            key = torch.arange(c.T).unsqueeze(1) + torch.arange(2 * c.w + 1).unsqueeze(0) - c.w   # [T, 2w+1]
            band = ((key >= 0) & (key < c.T)).double() @ ev / c.T                                  # [T, dk]
            want = v.view(c.H, c.dk, c.T).mean(2, keepdim=True) + band.t().unsqueeze(0)            # [H, dk, T]
            err = (out.t[b].cpu().double() - want.reshape(c.H * c.dk, c.T)).abs().max().item() / ref.abs().max().item()
            assert err <= bound(d32), "an all-masked row is not uniform over T (%.2e, on the scale of the case's reference)" % err


@pytest.mark.gpu
@pytest.mark.parametrize("c", [CASES[5], CASES[6]], ids=cid)
def test_batch_row_alone_has_the_same_bits(gpu, c):
    ins = on_gpu(c, gpu)
    st, out = abi_fwd(c, ins)
    assert st == 0
    q, k, v, ek, ev, mask = ins
    for b in range(c.B):
        one = c._replace(B=1)
        st, alone = abi_fwd(one, (q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), ek, ev, mask[b:b + 1].contiguous()))
        assert st == 0 and alone.intact()
        assert torch.equal(alone.t[0], out.t[b]), "batch row %d differs from the same row computed alone" % b


@pytest.mark.gpu
def test_refusals(gpu):
    """Argument checks: VCV_EINVAL, nothing launched, the output untouched.  Every buffer has the size the shape asks for."""
    from vcvits_amd._lib import lib
    tried = []

    def attempt(B, H, dk, T, w, null_q=False, expect=EINVAL):
        c = Case(B, H, dk, T, w, "ones")
        g0 = torch.Generator().manual_seed(9)
        q, k, v = (torch.randn(B, H * dk, T, generator=g0).to(gpu) for _ in range(3))
        ek, ev = (torch.randn(1, 2 * w + 1, dk, generator=g0).to(gpu) for _ in range(2))
        what = "B%d-H%d-dk%d-T%d-w%d%s" % (B, H, dk, T, w, " null q" if null_q else "")
        if not null_q:
            assert lib().vcv_rel_attn_stream_supported(B, H, dk, T, w) == expect, "supported " + what
        st, out = abi_fwd(c, (None if null_q else q, k, v, ek, ev, torch.ones(B, T, device=gpu)))
        torch.cuda.synchronize()
        assert st == expect, "%s returned %d" % (what, st)
        if expect == EINVAL:
            assert out.untouched(), "%s wrote to the output" % what
        else:
            assert out.intact() and not bool(torch.isnan(out.t).any())
        tried.append(what)

    attempt(1, 1, 48, 40, 4)       # a head width the kernel is not built for
    attempt(1, 1, 7, 40, 4)        # an odd one
    attempt(1, 1, 32, 40, 8)       # 2 w + 1 = 17 relative positions
    attempt(1, 1, 32, 40, 4, null_q=True)
    attempt(65536, 1, 32, 1, 4)    # B * H past the grid's y limit
    attempt(1, 1, 32, 40, 4, expect=0)  # the same buffers' shape is accepted when nothing is wrong with the call
    record("%d calls refused with VCV_EINVAL, output untouched: %s" % (len(tried) - 1, "; ".join(tried[:-1])))
    # the fused entry point keeps its limit
    assert lib().vcv_rel_attn_supported(1, 1, 64, 897, 4) == EINVAL and lib().vcv_rel_attn_supported(1, 1, 64, 896, 4) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. routing: ops.rel_attention
# ---------------------------------------------------------------------------------------------------------------------
def _through_ops(c, ins, grad=False, requires_grad=False, want_attn=False, training=False, pdrop=0.0):
    """-> out, attn, (streamed launches, fused launches)"""
    from vcvits_amd import ops
    q, k, v, ek, ev, mask = ins
    if requires_grad:
        q, k, v, ek, ev = (t.clone().requires_grad_(True) for t in (q, k, v, ek, ev))
    before = (ops.LAUNCH_COUNTS["attn_stream"], ops.LAUNCH_COUNTS["attn_fused"])
    with torch.set_grad_enabled(grad):
        out, attn = ops.rel_attention(q, k, v, ek, ev, mask, c.H, c.w, pdrop, training=training, want_attn=want_attn)
    return out, attn, (ops.LAUNCH_COUNTS["attn_stream"] - before[0], ops.LAUNCH_COUNTS["attn_fused"] - before[1])


@pytest.mark.gpu
def test_routing_first_streamed_length(gpu):
    """T = 897 under no_grad without `attn`: one streamed launch, no fused one, the bits of the direct call.  With gradients,
    with `attn`, or with dropout: where the call went before (no streamed launch)."""
    from vcvits_amd import ops
    c = ROUTED
    ins = on_gpu(c, gpu)
    assert ops._ATTN_STREAM_MIN_T[0] == 897
    with compute_mode("f32"):
        out, attn, n = _through_ops(c, ins)
        assert n == (1, 0) and attn is None, n
        st, direct = abi_fwd(c, ins)
        assert st == 0 and torch.equal(out, direct.t), "ops.rel_attention: not vcv_rel_attn_stream_fwd's bits"
        # inference_mode is no_grad for this purpose
        with torch.inference_mode():
            o2, _, n = _through_ops(c, ins)
        assert n == (1, 0) and torch.equal(o2, out)
        # tensors that require grad under no_grad still stream; with grad mode on they do not
        _, _, n = _through_ops(c, ins, grad=False, requires_grad=True)
        assert n == (1, 0), n
        ref, d32 = reference(c)
        for kw in (dict(grad=True, requires_grad=True), dict(want_attn=True), dict(training=True, pdrop=0.1)):
            o3, a3, n = _through_ops(c, ins, **kw)
            assert n[0] == 0, "a streamed launch with %s" % (kw,)
            if "pdrop" not in kw:
                assert A.dist(o3, ref) <= bound(d32)
            if kw.get("want_attn"):
                assert a3 is not None and tuple(a3.shape) == (c.B, c.H, c.T, c.T)
        # grad mode on but nothing requires grad: streamed
        _, _, n = _through_ops(c, ins, grad=True)
        assert n == (1, 0), n
    record("routing %s: ops.rel_attention == vcv_rel_attn_stream_fwd bit for bit under no_grad; grad / attn / dropout: not streamed" % cid(c))


@pytest.mark.gpu
def test_routing_below_the_threshold_and_moved_threshold(gpu):
    from vcvits_amd import ops
    with compute_mode("f32"):
        c = Case(1, 2, 32, 896, 4, "ragged+hole")
        _, _, n = _through_ops(c, on_gpu(c, gpu))
        assert n == (0, 1), "T = 896 by default: %s" % (n,)
        c = MIN_T_CASE
        ins = on_gpu(c, gpu)
        ref, d32 = reference(c)
        _, _, n = _through_ops(c, ins)
        assert n == (0, 1), n
        old = ops._ATTN_STREAM_MIN_T[0]
        ops._ATTN_STREAM_MIN_T[0] = 1
        try:
            out, attn, n = _through_ops(c, ins)
            assert n == (1, 0) and attn is None, n
            check("routing MIN_T=1 %s" % cid(c), out, ref, d32)
            ops._ATTN_STREAM_MIN_T[0] = 0  # never
            _, _, n = _through_ops(ROUTED, on_gpu(ROUTED, gpu))
            assert n[0] == 0, n
        finally:
            ops._ATTN_STREAM_MIN_T[0] = old


@pytest.mark.gpu
def test_routing_bf16_mode_has_the_same_bits(gpu):
    """The streamed kernel is mode-independent (fp32-input MFMA in both compute modes)."""
    c = ROUTED
    ins = on_gpu(c, gpu)
    with compute_mode("f32"):
        a, _, n = _through_ops(c, ins)
        assert n == (1, 0)
    with compute_mode("bf16"):
        b, _, n = _through_ops(c, ins)
        assert n == (1, 0)
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_memory_is_linear_in_T(gpu):
    """B = 1, H = 2, dk = 32, T = 4096 under no_grad without `attn`: the call allocates its output and little else (the
    three-launch path allocated two [2, 4096, 4096] float tensors, 268 MB, where q is 1 MB)."""
    c = Case(1, 2, 32, 4096, 4, "ragged+hole")
    ins = tuple(t.to(gpu) for t in inputs(c))
    with compute_mode("f32"):
        _through_ops(c, ins)  # (code objects, lazy allocations of the first call)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.max_memory_allocated()
        out, _, n = _through_ops(c, ins)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    limit = 2 * ins[0].numel() * 4 + (1 << 20)
    record("memory %s: peak %d bytes over the call (limit %d; q is %d bytes)" % (cid(c), peak, limit, ins[0].numel() * 4))
    assert peak <= limit, (peak, limit)
    assert n == (1, 0)
    del out


# ---------------------------------------------------------------------------------------------------------------------
# 3. the encoder end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_encoder_end_to_end(gpu):
    """TransformerEncoder(64, 128, 2 heads, 2 layers, k = 3) in eval() under no_grad at B = 2, T = 1000, lengths [1000, 700]
    against the oracle on the float64 state_dict; bound: the oracle's float32 run against its float64 run, factor 16, cap 1e-4."""
    from golden_util import fill_state_dict, keys_shapes_of
    from oracle import vits_oracle as O
    from vcvits_amd import ops
    from vcvits_amd.model.transformer.relative_attention_transformer import TransformerEncoder
    n_layers = 2
    m = TransformerEncoder(64, 128, n_heads=2, n_layers=n_layers, kernel_size=3)
    sd = fill_state_dict(keys_shapes_of(m), 11)
    m.load_state_dict(sd)
    m = m.to(gpu).eval()
    B, T = 2, 1000
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 64, T)).astype(np.float32))
    xm = O.sequence_mask(torch.tensor([1000, 700]), T).unsqueeze(1).float()
    run = lambda dt: O.transformer_encoder_forward({"t." + k: v.to(dt) for k, v in sd.items()}, "t", x.to(dt), xm.to(dt), 2, n_layers, 3)
    r64 = run(torch.float64)
    d32 = A.dist(run(torch.float32), r64)
    before = (ops.LAUNCH_COUNTS["attn_stream"], ops.LAUNCH_COUNTS["attn_fused"])
    with compute_mode("f32"), torch.no_grad():
        y = m(x.to(gpu), xm.to(gpu))
    assert ops.LAUNCH_COUNTS["attn_stream"] - before[0] == n_layers and ops.LAUNCH_COUNTS["attn_fused"] == before[1]
    assert bool(torch.isfinite(y).all())
    check("encoder 64/128 H2 L2 k3 B2 T1000 lengths 1000,700", y, r64, d32)

"""The bf16-operand streamed attention kernels (csrc/attention_stream_bf16.hip) at the edges of their tiling, through the C ABI
with guard bands around the output, and their routing behind VCVITS_ATTN_STREAM_BF16 in bf16 compute mode.

References: tests/attention_f64.py (relative-position) and a float64 softmax((scale q)^T k) v with a key bound per row (HuBERT,
the expression of tests/test_hubert_gpu.py), on float64 copies of the inputs.

Bound 1, inputs that are bf16 numbers already (q, k, v rounded on the host, the tables fp32): the scores are exact up to fp32
accumulation, so the only bf16 rounding is that of each probability as the operand of the second product, at most 2^-9
relative, after the row sum was formed; rescale factors and v are exact.  Elementwise
    |out - ref| <= 2^-8 * (P_ref @ |v|) + slack,    slack = bound(d32) * max|ref|,
bound() and d32 (the float32 CPU run of the reference against its float64 run) as in tests/test_attention_stream_gpu.py: the
bound of tests/test_attention_abi_gpu.py::test_bf16_mode.
Bound 2, general fp32 inputs: rel_l2(gpu, f64) <= 2 * rel_l2(restatement, f64), the restatement being the reference's text in
float32 on q, k, v rounded to bf16 with the probabilities rounded to bf16 before the second product (tests/test_hubert_gpu.py's
2 x rule).  Both distances of every case go to profiles/attn_stream_bf16_parity.txt.
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
import hubert_f64 as R
import test_attention_stream_gpu as SG
import test_hubert_gpu as HG
import test_hubert_lengths_gpu as HL
from test_attention_stream_cpu import _mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
Case = SG.Case
HCase = collections.namedtuple("HCase", "B H d T")

REL = [
    Case(1, 1, 32, 1, 4, "ones"),            # one query, one key
    Case(2, 1, 64, 5, 7, "ragged"),          # T <= w
    Case(2, 2, 32, 31, 4, "hole"),           # one tile - 1
    Case(2, 2, 64, 32, 0, "hole"),           # one tile, w = 0
    Case(2, 1, 32, 33, 4, "ragged"),         # one tile + 1
    Case(2, 1, 64, 97, 7, "zero"),           # an all-zero batch row
    Case(2, 1, 32, 129, 7, "ragged+hole"),   # two query blocks: the band crosses waves and blocks, all three carries live
    Case(2, 2, 64, 130, 4, "ragged+hole"),
    Case(1, 2, 32, 161, 4, "head"),          # keys 0 .. 79 masked: the running max starts at -1e4 and is rescaled away
]
HUB = [HCase(3, 2, 64, 1), HCase(3, 1, 80, 33), HCase(3, 1, 64, 33), HCase(3, 2, 64, 129), HCase(3, 1, 80, 129),
       HCase(3, 1, 64, 200), HCase(3, 2, 80, 200)]


def hid(c):
    return "B%d-H%d-d%d-T%d" % tuple(c)


def lengths_of(c):
    """full, 1, mid-tile"""
    return [c.T, 1, min(c.T, c.T // 2 + 3)]


def test_case_tables():
    """CPU: the tables above against what they are meant to reach."""
    assert {c.T for c in REL} >= {1, 5, 31, 32, 33, 97, 129, 130, 161} and {c.dk for c in REL} == {32, 64}
    assert any(c.T <= c.w for c in REL) and any(c.w == 0 for c in REL) and sum(c.H == 2 for c in REL) >= 2
    assert any(not bool(_mask(c.mask, c.B, c.T)[b].any()) for c in REL for b in range(c.B))
    c = REL[-1]
    m = _mask(c.mask, c.B, c.T)[0]
    assert not bool(m[:64].any()) and bool(m[c.T // 2:].all())  # two whole key tiles masked before the first live key
    assert {c.T for c in HUB} == {1, 33, 129, 200} and {c.d for c in HUB} == {64, 80}
    for c in HUB:
        n = lengths_of(c)
        assert n[0] == c.T and n[1] == 1 and 1 <= n[2] <= c.T and (c.T < 32 or n[2] % 32 != 0)


def bf(t):
    return t.bfloat16().float()


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references: made once per case and shared, never modified
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rel_inputs(c, rounded):
    rng = np.random.default_rng(zlib.crc32(repr(("bf16",) + tuple(c)).encode()))
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    C = c.H * c.dk
    q, k, v = 2.0 * t(c.B, C, c.T), t(c.B, C, c.T), t(c.B, C, c.T)
    ek, ev = t(1, 2 * c.w + 1, c.dk) * c.dk ** -0.5, t(1, 2 * c.w + 1, c.dk) * c.dk ** -0.5
    if rounded:
        q, k, v = bf(q), bf(k), bf(v)
    return q, k, v, ek, ev, _mask(c.mask, c.B, c.T)


@functools.lru_cache(maxsize=None)
def rel_reference(c, rounded):
    """(float64 out, reach = P_ref @ |v| in the layout of out, d32)"""
    ins = rel_inputs(c, rounded)
    r = A.rel_attention(*ins)
    B, H, dk, T = c.B, c.H, c.dk, c.T
    va = ins[2].double().view(B, H, dk, T).transpose(2, 3).abs()
    reach = (r.P.view(B, H, T, T) @ va).transpose(2, 3).reshape(B, H * dk, T)
    return r.out, reach, A.dist(A.rel_attention(*ins, dtype=torch.float32).out, r.out)


@functools.lru_cache(maxsize=None)
def rel_restatement(c):
    """The reference's text in float32 on q, k, v rounded to bf16; the probabilities enter the value product rounded to bf16
    (the band-value product keeps them as they are, as in the kernel): out + (bf16(P) - P) @ v."""
    q, k, v, ek, ev, mask = rel_inputs(c, False)
    r = A.rel_attention(bf(q), bf(k), bf(v), ek, ev, mask, dtype=torch.float32)
    B, H, dk, T = c.B, c.H, c.dk, c.T
    P = r.P.view(B, H, T, T)
    dv = (bf(P) - P) @ bf(v).view(B, H, dk, T).transpose(2, 3)
    return r.out + dv.transpose(2, 3).reshape(B, H * dk, T)


@functools.lru_cache(maxsize=None)
def hub_inputs(c, rounded):
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(c)).encode()))
    qkv = torch.randn(c.B, 3 * c.H * c.d, c.T, generator=g, dtype=torch.float64).to(torch.float32)
    qkv[:, :c.H * c.d] *= 3.0  # rows that are not near-uniform
    return bf(qkv) if rounded else qkv


def hub_attention(qkv, c, n, dtype, round_p=False):
    """softmax((d^-0.5 q)^T k) v per head over the keys s < n[b]; 0 for the queries at or behind n[b].  -> out, P"""
    q, k, v = (t.to(dtype).reshape(c.B, c.H, c.d, c.T) for t in qkv.chunk(3, dim=1))
    live = torch.arange(c.T)[None, :] < torch.tensor(n)[:, None]                       # [B, T]
    s = torch.einsum("bhdt,bhds->bhts", q, k) * c.d ** -0.5
    P = torch.softmax(s.masked_fill(~live[:, None, None, :], float("-inf")), dim=-1)
    out = torch.einsum("bhts,bhds->bhdt", bf(P) if round_p else P, v) * live[:, None, None, :]
    return out.reshape(c.B, c.H * c.d, c.T), P * live[:, None, :, None]


@functools.lru_cache(maxsize=None)
def hub_reference(c, rounded, with_lengths):
    qkv = hub_inputs(c, rounded)
    n = lengths_of(c) if with_lengths else [c.T] * c.B
    out, P = hub_attention(qkv, c, n, torch.float64)
    va = qkv.chunk(3, dim=1)[2].double().reshape(c.B, c.H, c.d, c.T).abs()
    reach = torch.einsum("bhts,bhds->bhdt", P, va).reshape(c.B, c.H * c.d, c.T)
    return out, reach, A.dist(hub_attention(qkv, c, n, torch.float32)[0], out)


MARK = "# tests/test_attention_stream_bf16_gpu.py"
_lines = collections.OrderedDict()


def record(section, line):
    """Keep the printed figures in profiles/attn_stream_bf16_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _lines.setdefault(section, [])
    if line not in _lines[section]:
        _lines[section].append(line)
    with open(os.path.join(ROOT, "profiles", "attn_stream_bf16_parity.txt"), "w") as f:
        f.write(MARK + ": the bf16-operand streamed attention kernels (vcv_rel_attn_stream_fwd_bf16, vcv_hubert_attn_fwd[_len]_bf16)\n"
                "# against float64.  bound 1 (bf16-valued q, k, v): worst = max |out - ref| / (2^-8 P_ref|v| + slack), asserted <= 1.\n"
                "# bound 2 (fp32 q, k, v): relative L2 from float64 of the GPU and of the restatement with bf16 operands, asserted\n"
                "# gpu <= 2 * restatement.  Rel-pos cases are B-H-dk-T-window-mask, HuBERT cases B-H-d-T.\n")
        for name, lines in _lines.items():
            f.write("\n[%s]\n" % name)
            f.write("\n".join(lines) + "\n")


def rel_abi(c, ins, entry="vcv_rel_attn_stream_fwd_bf16"):
    from vcvits_amd._lib import lib, ptr, stream
    q, k, v, ek, ev, mask = ins
    out = SG.Guarded((c.B, c.H * c.dk, c.T), k.device)
    st = getattr(lib(), entry)(ptr(q) if q is not None else None, ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(mask), ptr(out.t),
                               c.B, c.H, c.dk, c.T, c.w, c.dk ** -0.5, stream())
    return st, out


def hub_abi(c, qkv, n=None, ldb=None, bf16=True):
    """q, k, v as slices of the fused projection (ldb = 3 * H * d * T)"""
    import ctypes
    from vcvits_amd._lib import lib, ptr, stream
    E = c.H * c.d
    out = SG.Guarded((c.B, E, c.T), qkv.device)
    q = ptr(qkv)
    k, v = ctypes.c_void_p(q.value + 4 * E * c.T), ctypes.c_void_p(q.value + 8 * E * c.T)
    ldb = 3 * E * c.T if ldb is None else ldb
    sfx = "_bf16" if bf16 else ""
    if n is None:
        st = getattr(lib(), "vcv_hubert_attn_fwd" + sfx)(q, k, v, ptr(out.t), c.B, c.H, c.d, c.T, ldb, c.d ** -0.5, stream())
    else:
        st = getattr(lib(), "vcv_hubert_attn_fwd_len" + sfx)(q, k, v, ptr(out.t), c.B, c.H, c.d, c.T, ldb, c.d ** -0.5, ptr(n), stream())
    return st, out


def check_bound1(section, tag, got, ref, reach, d32):
    slack = SG.bound(d32) * ref.abs().max().item()
    err = (got.cpu().double() - ref).abs()
    worst = (err / (2.0 ** -8 * reach + slack)).max().item()
    record(section, "%-40s worst=%.3f  max-norm distance=%.1e  d32=%.1e" % (tag, worst, A.dist(got, ref), d32))
    assert worst <= 1.0, "%s: |out - ref| is %.3f of 2^-8 P|v| + slack" % (tag, worst)


def check_bound2(section, tag, got, rest, ref):
    d_gpu, d_ref = R.rel_l2(got.cpu(), ref), R.rel_l2(rest, ref)
    record(section, "%-40s gpu %.3e   bf16-operand restatement %.3e   ratio %.2f" % (tag, d_gpu, d_ref, d_gpu / max(d_ref, 1e-300)))
    assert d_gpu <= 2.0 * d_ref, "%s: gpu %.3e > 2 x %.3e" % (tag, d_gpu, d_ref)


def clean_twice(run):
    """status 0, guard bands intact, every element written, no NaN, and the same bits from the same call twice"""
    st, out = run()
    assert st == 0, st
    assert out.intact(), "a write outside the buffer"
    assert not bool(torch.isnan(out.t).any()), "NaN, or elements the kernel did not write"
    st, again = run()
    assert st == 0 and torch.equal(out.t, again.t), "out differs between two identical launches"
    return out.t


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels at the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", REL, ids=SG.cid)
def test_rel_bf16_valued_inputs(gpu, c):
    ins = tuple(t.to(gpu) for t in rel_inputs(c, True))
    ref, reach, d32 = rel_reference(c, True)
    got = clean_twice(lambda: rel_abi(c, ins))
    check_bound1("rel-pos, bound 1", SG.cid(c), got, ref, reach, d32)
    # a masked query is the uniform average over all T keys (the masked ones included) plus its band of embv / T
    q, k, v, ek, ev, mask = rel_inputs(c, True)
    key = torch.arange(c.T).unsqueeze(1) + torch.arange(2 * c.w + 1).unsqueeze(0) - c.w        # [T, 2w+1]
    band = ((key >= 0) & (key < c.T)).double() @ ev[0].double() / c.T                           # [T, dk]
    vh = v.double().view(c.B, c.H, c.dk, c.T)
    want = (vh.mean(3, keepdim=True) + band.t()[None, None]).reshape(c.B, c.H * c.dk, c.T)
    room = 2.0 ** -8 * vh.abs().mean(3, keepdim=True).expand(-1, -1, -1, c.T).reshape(c.B, c.H * c.dk, c.T) \
        + SG.bound(d32) * ref.abs().max().item()
    dead = (mask == 0)[:, None, :].expand(-1, c.H * c.dk, -1)
    if bool(dead.any()):
        over = ((got.cpu().double() - want).abs() / room)[dead].max().item()
        assert over <= 1.0, "a masked query is not uniform over T (%.3f of the bound)" % over


@pytest.mark.gpu
@pytest.mark.parametrize("c", REL, ids=SG.cid)
def test_rel_fp32_inputs(gpu, c):
    ins = tuple(t.to(gpu) for t in rel_inputs(c, False))
    ref = rel_reference(c, False)[0]
    got = clean_twice(lambda: rel_abi(c, ins))
    check_bound2("rel-pos, bound 2", SG.cid(c), got, rel_restatement(c), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("with_lengths", [False, True], ids=["all", "lengths"])
@pytest.mark.parametrize("c", HUB, ids=hid)
def test_hubert_bf16_valued_inputs(gpu, c, with_lengths):
    qkv = hub_inputs(c, True).to(gpu)
    n = torch.tensor(lengths_of(c), dtype=torch.int32, device=gpu) if with_lengths else None
    ref, reach, d32 = hub_reference(c, True, with_lengths)
    got = clean_twice(lambda: hub_abi(c, qkv, n))
    check_bound1("HuBERT, bound 1", hid(c) + (" lengths" if with_lengths else ""), got, ref, reach, d32)
    if with_lengths:
        for b, nb in enumerate(lengths_of(c)):
            assert nb == c.T or bool((got[b, :, nb:] == 0).all()), "row %d: a query behind its end is not exact 0" % b
        # what lies behind a row's end is never used: NaN there changes no bit
        dirty = hub_inputs(c, True).clone()
        for b, nb in enumerate(lengths_of(c)):
            dirty[b, :, nb:] = float("nan")
        st, out = hub_abi(c, dirty.to(gpu), n)
        assert st == 0 and out.intact() and torch.equal(out.t, got)


@pytest.mark.gpu
@pytest.mark.parametrize("with_lengths", [False, True], ids=["all", "lengths"])
@pytest.mark.parametrize("c", HUB, ids=hid)
def test_hubert_fp32_inputs(gpu, c, with_lengths):
    qkv = hub_inputs(c, False)
    nl = lengths_of(c) if with_lengths else [c.T] * c.B
    n = torch.tensor(nl, dtype=torch.int32, device=gpu) if with_lengths else None
    ref = hub_reference(c, False, with_lengths)[0]
    rest = hub_attention(bf(qkv), c, nl, torch.float32, round_p=True)[0]
    got = clean_twice(lambda: hub_abi(c, qkv.to(gpu), n))
    check_bound2("HuBERT, bound 2", hid(c) + (" lengths" if with_lengths else ""), got, rest, ref)


@pytest.mark.gpu
def test_refusals(gpu):
    """VCV_EINVAL, nothing launched, the output untouched; the accepted call of the same buffers writes all of it."""
    from vcvits_amd._lib import lib
    for B, H, dk, T, w, null_q, expect in ((1, 1, 48, 40, 4, False, EINVAL), (1, 1, 32, 40, 8, False, EINVAL), (1, 1, 32, 40, 4, True, EINVAL),
                                           (65536, 1, 32, 1, 4, False, EINVAL), (1, 1, 32, 40, 4, False, 0)):
        c = Case(B, H, dk, T, w, "ones")
        g0 = torch.Generator().manual_seed(9)
        q, k, v = (torch.randn(B, H * dk, T, generator=g0).to(gpu) for _ in range(3))
        ek, ev = (torch.randn(1, 2 * w + 1, dk, generator=g0).to(gpu) for _ in range(2))
        st, out = rel_abi(c, (None if null_q else q, k, v, ek, ev, torch.ones(B, T, device=gpu)))
        torch.cuda.synchronize()
        assert st == expect, (tuple(c), null_q, st)
        assert out.untouched() if expect == EINVAL else (out.intact() and not bool(torch.isnan(out.t).any())), tuple(c)
    for c, ldb, expect in ((HCase(1, 1, 48, 40), None, EINVAL), (HCase(2, 1, 64, 40), 64 * 40 - 1, EINVAL), (HCase(2, 1, 80, 40), None, 0)):
        for n in (None, torch.full((c.B,), c.T, dtype=torch.int32, device=gpu)):
            qkv = torch.randn(c.B, 3 * c.H * c.d, c.T, generator=torch.Generator().manual_seed(4)).to(gpu)
            st, out = hub_abi(c, qkv, n, ldb)
            torch.cuda.synchronize()
            assert st == expect, (tuple(c), ldb, st)
            assert out.untouched() if expect == EINVAL else (out.intact() and not bool(torch.isnan(out.t).any())), tuple(c)


# ---------------------------------------------------------------------------------------------------------------------
# 2. routing
# ---------------------------------------------------------------------------------------------------------------------
KEYS = ("attn_stream_bf16", "attn_stream", "attn_fused")


@contextlib.contextmanager
def switch(value, mode):
    from vcvits_amd import ops
    old = ops._ATTN_STREAM_BF16[0]
    ops._ATTN_STREAM_BF16[0] = value
    try:
        with SG.compute_mode(mode):
            yield
    finally:
        ops._ATTN_STREAM_BF16[0] = old


def counted(fn):
    """-> fn(), launches counted under KEYS"""
    from vcvits_amd import ops
    before = [ops.LAUNCH_COUNTS[k] for k in KEYS]
    r = fn()
    return r, tuple(ops.LAUNCH_COUNTS[k] - b for k, b in zip(KEYS, before))


def through_ops(c, ins, grad=False):
    from vcvits_amd import ops
    q, k, v, ek, ev, mask = ins
    if grad:
        q, k, v, ek, ev = (t.clone().requires_grad_(True) for t in (q, k, v, ek, ev))
    with torch.set_grad_enabled(grad):
        out, attn = ops.rel_attention(q, k, v, ek, ev, mask, c.H, c.w, 0.0, training=False, want_attn=False)
    return out.detach()


@pytest.mark.gpu
def test_routing_rel(gpu):
    from vcvits_amd import ops
    assert ops._ATTN_STREAM_BF16[0] == 0, "the switch is off by default"
    c = Case(1, 2, 32, 900, 4, "ragged+hole")
    ins = tuple(t.to(gpu) for t in rel_inputs(c, False))
    with switch(0, "f32"):
        base, n = counted(lambda: through_ops(c, ins))
        assert n == (0, 1, 0), n
    for sw, mode in ((0, "bf16"), (1, "f32")):  # either alone: the fp32-operand kernel, its counter, its bits
        with switch(sw, mode):
            out, n = counted(lambda: through_ops(c, ins))
            assert n == (0, 1, 0) and torch.equal(out, base), (sw, mode, n)
    with switch(1, "bf16"):
        out, n = counted(lambda: through_ops(c, ins))
        assert n == (1, 0, 0), n
        st, direct = rel_abi(c, ins)
        assert st == 0 and direct.intact() and torch.equal(out, direct.t), "ops.rel_attention: not vcv_rel_attn_stream_fwd_bf16's bits"
        assert not torch.equal(out, base)
        with torch.inference_mode():
            o2, n = counted(lambda: through_ops(c, ins))
        assert n == (1, 0, 0) and torch.equal(o2, out)
        # one frame below the streamed threshold: the fused kernel, as today
        c896 = c._replace(T=896)
        _, n = counted(lambda: through_ops(c896, tuple(t.to(gpu) for t in rel_inputs(c896, False))))
        assert n == (0, 0, 1), n
        # with gradients: today's path (no streamed forward of either kind)
        _, n = counted(lambda: through_ops(c, ins, grad=True))
        assert n[0] == 0 and n[1] == 0, n
    ref = rel_reference(c, False)[0]
    check_bound2("routing", "rel_attention " + SG.cid(c), out, rel_restatement(c), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [HCase(3, 2, 64, 129), HCase(3, 1, 80, 33)], ids=hid)
def test_routing_hubert(gpu, c):
    from vcvits_amd import ops
    qkv = hub_inputs(c, False).to(gpu)
    q, k, v = (t.contiguous() for t in qkv.chunk(3, dim=1))
    n = torch.tensor(lengths_of(c), dtype=torch.int32, device=gpu)
    for lengths in (None, n):
        with switch(0, "f32"):
            base, cnt = counted(lambda: ops.hubert_attention_qkv(qkv, c.H, lengths=lengths))
            assert cnt == (0, 0, 0)
            st, direct = hub_abi(c, qkv, lengths, bf16=False)
            assert st == 0 and torch.equal(base, direct.t)
        for sw, mode in ((0, "bf16"), (1, "f32")):
            with switch(sw, mode):
                out, cnt = counted(lambda: ops.hubert_attention_qkv(qkv, c.H, lengths=lengths))
                assert cnt == (0, 0, 0) and torch.equal(out, base), (sw, mode)
                assert torch.equal(ops.hubert_attention(q, k, v, c.H, lengths=lengths), base)
        with switch(1, "bf16"):
            out, cnt = counted(lambda: ops.hubert_attention_qkv(qkv, c.H, lengths=lengths))
            assert cnt == (1, 0, 0), cnt
            st, direct = hub_abi(c, qkv, lengths)
            assert st == 0 and direct.intact() and torch.equal(out, direct.t)
            sep, cnt = counted(lambda: ops.hubert_attention(q, k, v, c.H, lengths=lengths))
            assert cnt == (1, 0, 0) and torch.equal(sep, out) and not torch.equal(out, base)


@pytest.mark.gpu
def test_encoder_end_to_end(gpu):
    """TransformerEncoder(64, 128, 2 heads, 2 layers, k = 3) in eval() under no_grad at B = 2, T = 900, lengths [900, 700], bf16
    mode with the switch on: two bf16-operand launches, and within 2 x the distance from the float64 oracle of the oracle's
    float32 text under torch.autocast("cpu", torch.bfloat16)."""
    from golden_util import fill_state_dict, keys_shapes_of
    from oracle import vits_oracle as O
    from vcvits_amd.model.transformer.relative_attention_transformer import TransformerEncoder
    n_layers = 2
    m = TransformerEncoder(64, 128, n_heads=2, n_layers=n_layers, kernel_size=3)
    sd = fill_state_dict(keys_shapes_of(m), 11)
    m.load_state_dict(sd)
    m = m.to(gpu).eval()
    B, T = 2, 900
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 64, T)).astype(np.float32))
    xm = O.sequence_mask(torch.tensor([900, 700]), T).unsqueeze(1).float()
    run = lambda dt: O.transformer_encoder_forward({"t." + k: v.to(dt) for k, v in sd.items()}, "t", x.to(dt), xm.to(dt), 2, n_layers, 3)
    with torch.no_grad():
        r64 = run(torch.float64)
        with torch.autocast("cpu", torch.bfloat16):
            rbf = run(torch.float32).double()
    with switch(1, "bf16"), torch.no_grad():
        y, n = counted(lambda: m(x.to(gpu), xm.to(gpu)))
    assert n == (n_layers, 0, 0), n
    assert bool(torch.isfinite(y).all())
    check_bound2("encoder", "encoder 64/128 H2 L2 k3 B2 T900 lengths 900,700", y, rbf, r64)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the HuBERT extractor end to end: the small configurations and the rule of tests/test_hubert_gpu.py and
#    tests/test_hubert_lengths_gpu.py, with their cached models, inputs and references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant,frames", [("A", 130), ("B", 37)])
def test_hubert_extractor(gpu, variant, frames):
    ref = HG._ref(variant, 3, frames, None, "f64")
    rbf = HG._ref(variant, 3, frames, None, "bf16")
    with switch(1, "bf16"):
        (out, pm), n = counted(lambda: HG._model(variant, gpu).extract_features(HG._source(3, frames).to(gpu)))
    assert pm is None and n == (HG.VARIANTS[variant]["layers"], 0, 0), n
    assert bool(torch.isfinite(out).all())
    check_bound2("HuBERT extractor", "%s B=3 T'=%d" % (variant, frames), out, rbf, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["A", "B"])
def test_hubert_extractor_with_lengths(gpu, variant):
    """the six rows of tests/test_hubert_lengths_gpu.py in one padded batch, each against the restatement of the row alone"""
    lens, frames = HL.BATCHES["six"]
    with switch(1, "bf16"):
        (out, pm), n = counted(lambda: HL._model(variant, gpu).extract_features(HL._source("six").to(gpu), lengths=list(lens)))
    assert n == (HL.VARIANTS[variant]["layers"], 0, 0), n
    out = out.cpu()
    assert bool(torch.isfinite(out).all())
    failures = []
    for b, f in enumerate(frames):
        assert f == max(frames) or out[b, f:].abs().max().item() == 0.0, "row %d has values behind its end" % b
        ref, rbf = HL._ref(variant, "six", b, None, "f64"), HL._ref(variant, "six", b, None, "bf16")
        try:
            check_bound2("HuBERT extractor, lengths", "%s six row %d T'=%d" % (variant, b, f), out[b, :f], rbf, ref)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures

"""CPU side of the streamed training attention (csrc/attention_stream_grad.hip): declarations, argument checks (which launch
nothing), the workspace size, the routing switch, the resources of the built kernels, and the conditions the GPU tests rest
on: the case table reaches every edge of the tiling, the reference's own float32 error leaves room under the caps, and the
(max, sum) restatement that `stats` is compared with is the softmax of tests/attention_f64.py.
"""
import os

import pytest
import torch

import attention_f64 as A
import attention_stream_grad_cases as G
from test_attention_stream_cpu import _kernel_notes

EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
ENTRIES = ("vcv_rel_attn_stream_train_fwd", "vcv_rel_attn_stream_bwd_workspace", "vcv_rel_attn_stream_bwd")


def test_entry_points_are_declared():
    from vcvits_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vcvits_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and name in _lib._ARGTYPES and hasattr(L, name)
        assert name + "(" in hdr
    block = hdr[hdr.index("attention_stream_grad.hip"):hdr.index("vcv_rel_attn_stream_bwd(")]
    assert block.count("relative_attention_transformer.py:150-182") >= 2 and "autograd" in block


def test_argument_checks_and_workspace_size():
    """Everything below returns on the host before any launch: every pointer is null or never dereferenced."""
    from vcvits_amd import _lib
    L = _lib.lib()
    fwd = lambda ptrs, B, H, dk, T, w, p: L.vcv_rel_attn_stream_train_fwd(*ptrs, B, H, dk, T, w, 1.0, p, 1, None)
    bwd = lambda ptrs, B, H, dk, T, w, p: L.vcv_rel_attn_stream_bwd(*ptrs, B, H, dk, T, w, 1.0, p, 1, None)
    assert fwd([None] * 8, 1, 1, 32, 40, 4, 0.0) == EINVAL and bwd([None] * 15, 1, 1, 32, 40, 4, 0.0) == EINVAL  # null pointers
    one = 64  # a non-null address that is never read: the shape or pdrop is refused first
    for B, H, dk, T, w in ((1, 1, 48, 40, 4), (1, 1, 16, 40, 4), (1, 1, 32, 40, 8), (1, 1, 32, 0, 4), (0, 1, 32, 40, 4),
                           (65536, 1, 32, 40, 4), (1, 1, 32, 40, -1)):
        assert L.vcv_rel_attn_stream_supported(B, H, dk, T, w) == EINVAL
        assert fwd([one] * 8, B, H, dk, T, w, 0.0) == EINVAL and bwd([one] * 15, B, H, dk, T, w, 0.0) == EINVAL
        assert L.vcv_rel_attn_stream_bwd_workspace(B, H, dk, T, w) < 0
    for p in (1.0, 1.5, -0.1, float("nan")):
        assert fwd([one] * 8, 1, 1, 32, 40, 4, p) == EINVAL and bwd([one] * 15, 1, 1, 32, 40, 4, p) == EINVAL
    for i in range(8):  # each pointer on its own
        assert fwd([None if j == i else one for j in range(8)], 1, 1, 32, 40, 4, 0.0) == EINVAL
    for i in range(15):
        assert bwd([None if j == i else one for j in range(15)], 1, 1, 32, 40, 4, 0.0) == EINVAL
    # the workspace is linear in T
    ws = L.vcv_rel_attn_stream_bwd_workspace
    for B, H, dk, w in ((1, 2, 32, 4), (16, 4, 64, 4), (2, 1, 64, 7), (1, 1, 32, 0)):
        const = B * H * 2 * (2 * w + 1) * dk  # one block's partial tables per head
        for T in (1, 5, 127, 128, 129, 1000, 15000, 1 << 20):
            a, b = ws(B, H, dk, T, w), ws(B, H, dk, 2 * T, w)
            assert 0 < a and b <= 2 * a + const, (B, H, dk, w, T, a, b)
            assert a <= B * H * T * (1 + 2 * (2 * w + 1) + dk) + const  # no more than a few tensors the size of q
    assert ws(1, 2, 32, 15000, 4) * 4 < 8 * (2 * 32 * 15000 * 4)


def test_switch_and_counter_are_declared():
    from vcvits_amd import ops, tuning
    assert ops.LAUNCH_COUNTS["attn_stream_grad"] >= 0
    kind, default, doc, _ = tuning.REGISTRY["VCVITS_ATTN_STREAM_GRAD_MIN_T"]
    assert kind == "int" and default == 0 and doc
    assert ops._ATTN_STREAM_GRAD_MIN_T is ops.attention._ATTN_STREAM_GRAD_MIN_T  # one list, shared by reference
    if "VCVITS_ATTN_STREAM_GRAD_MIN_T" not in os.environ:
        assert ops._ATTN_STREAM_GRAD_MIN_T[0] == 0
    assert any("VCVITS_ATTN_STREAM_GRAD_MIN_T" in line for line in tuning.table())


def test_kernels_use_no_scratch_memory(tmp_path):
    """The new object's kernels, read from the code object's notes (no GPU): no scratch, no spills, static LDS <= 64 KB."""
    from vcvits_amd import build_ext
    build_ext.build(verbose=False)
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    notes = _kernel_notes("attention_stream_grad", tmp_path)
    mine = {n: f for n, f in notes.items() if "rel_attn_stream" in n}
    for stem in ("train_fwd_kernelILi32E", "train_fwd_kernelILi64E", "bwd_q_kernelILi32E", "bwd_q_kernelILi64E",
                 "bwd_kv_kernelILi32E", "bwd_kv_kernelILi64E", "demb_reduce_kernel"):
        assert sum(stem in n for n in mine) == 1, (stem, sorted(mine))
    assert len(mine) == 7, sorted(mine)
    for name, f in notes.items():
        print(name, f)
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] <= 64 * 1024, (name, f)
        assert f["vgpr_count"] <= 512, (name, f)


def test_case_table_reaches_every_edge():
    cdiv = lambda a, b: -(-a // b)
    C = G.CASES
    T = [c.T for c in C]
    assert 1 in T and G.KT in T and G.KT + 1 in T and G.QB in T and G.QB + 1 in T and 897 in T
    assert any(c.T <= c.w for c in C) and any(c.w == 0 for c in C) and any(c.w == 7 for c in C)
    assert {c.dk for c in C} == {32, 64}
    assert any(c.T % G.KT not in (0, 1) and cdiv(c.T, G.KT) == 33 for c in C)                   # 33 tiles, odd tail
    assert any(not bool(G.make_mask(c)[b].any()) for c in C for b in range(c.B))                 # an all-masked batch row
    assert any(not bool(G.make_mask(c)[0, :G.KT].any()) and bool(G.make_mask(c)[0, G.KT + 8:].all()) for c in C)
    c = G.C129  # the band of the last lane of workgroup 0 reaches into workgroup 1, and the other way round
    assert c.T > G.QB and c.w > 0 and 2 * c.w + 1 <= 16
    assert not bool(G.make_mask(G.C257)[2].any())
    assert all(c.B * c.H <= 4 for c in C)
    ps = {}
    for c, p, seed in G.RUNS:
        ps.setdefault(c, set()).add(p)
    assert all(ps[c] >= {0.0, 0.1} for c in C) and sum(0.5 in s for s in ps.values()) == 2
    assert (G.C129, 0.1, G.BIG_SEED) in G.RUNS and G.BIG_SEED > 1 << 63
    assert len({s for _, _, s in G.RUNS}) == len(C) + 1


@pytest.mark.parametrize("run", G.RUNS, ids=G.run_id)
def test_reference_error_leaves_room_under_the_caps(run):
    """The condition on the inputs: 16 * d32 <= cap for every tensor, so no cap binds from the reference's side."""
    c, p, seed = run
    ref, d32, (m64, l64), ds = G.reference(c, p, seed)
    for n in ("out",) + G.GRADS:
        print("%s %s 16*d32 = %.2e (cap %.0e)" % (G.run_id(run), n, G.FACTOR * d32[n], G.cap(n)))
        assert G.FACTOR * d32[n] <= G.cap(n), (n, d32[n])
    print("%s stats 16*d32 = %.2e" % (G.run_id(run), G.FACTOR * ds))
    assert G.FACTOR * ds <= G.CAP
    if c.T == 1:
        for n in ("dq", "dk", "dembk"):
            assert not bool(getattr(ref, n).any())
    m = G.make_mask(c)
    for b in range(c.B):
        if not bool(m[b].any()):  # an all-masked batch row passes no gradient into q and k
            assert not bool(ref.dq[b].any()) and not bool(ref.dk[b].any())
            assert bool((m64.view(c.B, c.H, c.T)[b] == -1e4).all()) and bool((l64.view(c.B, c.H, c.T)[b] == c.T).all())


@pytest.mark.parametrize("c", G.CASES, ids=G.cid)
def test_max_and_sum_are_the_softmax_of_the_reference(c):
    """exp(s - m) / l is P of tests/attention_f64.py and m + log l is torch.logsumexp, in float64."""
    q, k, v, ek, ev, mask, dO = G.inputs(c)
    s, m, l = G.row_stats(q, k, ek, mask)
    assert s.dtype == torch.float64
    P = A.rel_attention(q, k, v, ek, ev, mask).P
    assert A.dist(torch.exp(s - m.unsqueeze(2)) / l.unsqueeze(2), P) <= 1e-14
    lse = torch.logsumexp(s, dim=2)
    assert torch.expm1(G.lse64(m, l) - lse).abs().max().item() <= 1e-12
    # a masked query row is exact in float32 too: m = -1e4, l = T
    _, m32, l32 = G.row_stats(q, k, ek, mask, torch.float32)
    dead = (G.make_mask(c) == 0).repeat_interleave(c.H, 0)
    assert bool((m32[dead] == -1e4).all()) and bool((l32[dead] == c.T).all())

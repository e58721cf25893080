"""Training through the streamed relative-position attention (csrc/attention_stream_grad.hip behind
vcv_rel_attn_stream_train_fwd / vcv_rel_attn_stream_bwd) at the edges of its tiling against a float64 CPU reference with the
same dropout mask, and its routing in ops.rel_attention behind VCVITS_ATTN_STREAM_GRAD_MIN_T.

Tests 1-4 call the kernels THROUGH THE C ABI, so the routing cannot send a case elsewhere; 5-7 go through ops.
Cases, inputs, reference and bound: tests/attention_stream_grad_cases.py (tests/test_attention_stream_grad_cpu.py asserts what
they rest on).  Every distance is appended to profiles/attention_parity.txt under this module's own marker.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import attention_f64 as A
import attention_stream_grad_cases as G
import test_attention_stream_gpu as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
Guarded, compute_mode, cid = SG.Guarded, SG.compute_mode, G.cid

MARK = "# ---- tests/test_attention_stream_grad_gpu.py"
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
        f.write(head + "\n\n" + MARK + ": vcv_rel_attn_stream_train_fwd / vcv_rel_attn_stream_bwd (nothing of size T x T) against\n"
                "# tests/attention_f64.py with the same keep mask, as tensor=kernel/d32/bound.  Cases are B-H-dk-T-window-mask-p.\n\n"
                "[streamed training]\n")
        f.write("\n".join(_lines) + "\n")


def check(tag, got, ref, d32, names, zero_scale=None):
    """Write the figures down first, then assert."""
    errs = {n: A.dist(got[n], getattr(ref, n)) for n in names}
    for n in names:
        if zero_scale is not None and not bool(getattr(ref, n).any()):
            errs[n] = got[n].detach().cpu().double().abs().max().item() / zero_scale
    bounds = {n: G.bound(n, d32[n]) for n in names}
    record("%-52s %s" % (tag, " ".join("%s=%.1e/%.1e/%.1e" % (n, errs[n], d32[n], bounds[n]) for n in names)))
    for n in names:
        assert errs[n] <= bounds[n], "%s: %s off by %.3e (d32 %.3e, bound %.3e)" % (tag, n, errs[n], d32[n], bounds[n])
    return errs


_dev = {}


def on_gpu(c, gpu):
    if c not in _dev:
        if len(_dev) >= 2:
            _dev.pop(next(iter(_dev)))
        _dev[c] = tuple(t.to(gpu) for t in G.inputs(c))
    return _dev[c]


def abi_fwd(c, ins, p, seed, null_stats=False):
    """-> status, out, stats (Guarded)"""
    from vcvits_amd._lib import lib, ptr, stream
    q, k, v, ek, ev, mask = ins[:6]
    out = Guarded((c.B, c.H * c.dk, c.T), k.device)
    stats = Guarded((c.B * c.H, c.T, 2), k.device)
    st = lib().vcv_rel_attn_stream_train_fwd(ptr(q), ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(mask), ptr(out.t),
                                             None if null_stats else ptr(stats.t), c.B, c.H, c.dk, c.T, c.w, c.dk ** -0.5, p, seed,
                                             stream())
    return st, out, stats


def abi_bwd(c, ins, out, stats, p, seed):
    """-> status, {dq, dk, dv, dembk, dembv: Guarded}, workspace (Guarded, exactly the documented size)"""
    from vcvits_amd._lib import lib, ptr, stream
    q, k, v, ek, ev, mask, dO = ins
    dev = k.device
    g = {n: Guarded(tuple(t.shape), dev) for n, t in (("dq", q), ("dk", k), ("dv", v), ("dembk", ek), ("dembv", ev))}
    n_ws = lib().vcv_rel_attn_stream_bwd_workspace(c.B, c.H, c.dk, c.T, c.w)
    ws = Guarded((max(n_ws, 1),), dev)
    st = lib().vcv_rel_attn_stream_bwd(ptr(q), ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(mask), ptr(out), ptr(stats), ptr(dO), ptr(ws.t),
                                       ptr(g["dq"].t), ptr(g["dk"].t), ptr(g["dv"].t), ptr(g["dembk"].t), ptr(g["dembv"].t),
                                       c.B, c.H, c.dk, c.T, c.w, c.dk ** -0.5, p, seed, stream())
    return st, g, ws


# ---------------------------------------------------------------------------------------------------------------------
# 1. the training forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("run", G.RUNS, ids=G.run_id)
def test_train_forward(gpu, run):
    c, p, seed = run
    ins = on_gpu(c, gpu)
    ref, d32, (m64, l64), ds32 = G.reference(c, p, seed)
    st, out, stats = abi_fwd(c, ins, p, seed)
    assert st == 0, st
    for name, gd in (("out", out), ("stats", stats)):
        assert gd.intact(), "%s: a write outside the buffer" % name
        assert not bool(torch.isnan(gd.t).any()), "%s has elements the kernel did not write" % name
    st, out2, stats2 = abi_fwd(c, ins, p, seed)
    assert st == 0 and torch.equal(out.t, out2.t) and torch.equal(stats.t, stats2.t), "two identical launches differ"
    check("forward %s" % G.run_id(run), {"out": out.t}, ref, d32, ("out",))
    err = G.stats_dist(stats.t[:, :, 0], stats.t[:, :, 1], m64, l64)
    bnd = min(max(G.FACTOR * ds32, G.FLOOR), G.CAP)
    record("%-52s stats=%.1e/%.1e/%.1e" % ("forward %s" % G.run_id(run), err, ds32, bnd))
    assert err <= bnd, "stats: m + log l off by %.3e (d32 %.3e, bound %.3e)" % (err, ds32, bnd)
    dead = (G.make_mask(c) == 0).repeat_interleave(c.H, 0)
    s = stats.t.cpu()
    assert bool((s[:, :, 0][dead] == -1e4).all()) and bool((s[:, :, 1][dead] == c.T).all()), "a masked query row is not (-1e4, T)"
    if p == 0:
        st, plain = SG.abi_fwd(c, ins[:6])
        assert st == 0
        same = torch.equal(plain.t, out.t)
        record("%-52s out %s vcv_rel_attn_stream_fwd's bits (distance %.1e)" % (
            "forward %s" % G.run_id(run), "has" if same else "has NOT", A.dist(out.t, plain.t)))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the backward pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("run", G.RUNS, ids=G.run_id)
def test_backward(gpu, run):
    c, p, seed = run
    ins = on_gpu(c, gpu)
    ref, d32, _, _ = G.reference(c, p, seed)
    st, out, stats = abi_fwd(c, ins, p, seed)
    assert st == 0, st
    runs = []
    for _ in range(2):
        st, g, ws = abi_bwd(c, ins, out.t, stats.t, p, seed)
        assert st == 0, st
        assert ws.intact(), "a write outside the documented workspace"
        for n in G.GRADS:
            assert g[n].intact(), "%s: a write outside the buffer" % n
            assert not bool(torch.isnan(g[n].t).any()), "%s has elements the kernels did not write (or read an unwritten workspace word)" % n
        runs.append({n: g[n].t for n in G.GRADS})
    check("backward %s" % G.run_id(run), runs[0], ref, d32, G.GRADS, zero_scale=G.cancel_scale(c, ref) if c.T == 1 else None)
    for n in G.GRADS:  # one writer per element, sums in index order: every tensor, every mode
        assert torch.equal(runs[0][n], runs[1][n]), "%s differs between two identical launches" % n
    m = G.make_mask(c)
    for b in range(c.B):
        if not bool(m[b].any()):  # an all-masked batch row: no gradient into q and k; dv = (uniform, dropped weights)^T dO
            assert not bool(runs[0]["dq"][b].any()) and not bool(runs[0]["dk"][b].any()), "dq / dk of an all-masked batch row"
            dO = G.inputs(c)[6][b].double().view(c.H, c.dk, c.T)
            keep = G.keep_of(c, p, seed)
            wgt = torch.full((c.H, c.T, c.T), 1.0 / c.T, dtype=torch.float64)
            if keep is not None:
                wgt = wgt * keep[b * c.H:(b + 1) * c.H].double() * A.inv_keep(p)
            want = torch.einsum("hdi,hij->hdj", dO, wgt).reshape(c.H * c.dk, c.T)
            err = (runs[0]["dv"][b].cpu().double() - want).abs().max().item() / ref.dv.abs().max().item()
            record("%-52s dv of the all-masked batch row against uniform weights: %.1e" % ("backward %s" % G.run_id(run), err))
            assert err <= G.bound("dv", d32["dv"]), err


# ---------------------------------------------------------------------------------------------------------------------
# 3. a batch row alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", [G.C129, G.C257], ids=cid)
def test_batch_row_alone_has_the_same_bits(gpu, c):
    ins = on_gpu(c, gpu)
    st, out, stats = abi_fwd(c, ins, 0.0, 0)
    assert st == 0
    st, g, _ = abi_bwd(c, ins, out.t, stats.t, 0.0, 0)
    assert st == 0
    q, k, v, ek, ev, mask, dO = ins
    for b in range(c.B):
        one = c._replace(B=1)
        ins1 = tuple(t[b:b + 1].contiguous() for t in (q, k, v)) + (ek, ev, mask[b:b + 1].contiguous(), dO[b:b + 1].contiguous())
        st, o1, s1 = abi_fwd(one, ins1, 0.0, 0)
        assert st == 0 and torch.equal(o1.t[0], out.t[b])
        st, g1, ws1 = abi_bwd(one, ins1, o1.t, s1.t, 0.0, 0)
        assert st == 0 and ws1.intact()
        for n in ("dq", "dk", "dv"):
            assert torch.equal(g1[n].t[0], g[n].t[b]), "%s of batch row %d differs from the same row computed alone" % (n, b)


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu):
    """VCV_EINVAL, nothing launched, every output untouched; the same buffers are accepted when nothing is wrong."""
    tried = []

    def attempt(B, H, dk, T, w, p=0.0, null_stats=False, expect=EINVAL):
        c = G.Case(B, H, dk, T, w, "ones")
        g0 = torch.Generator().manual_seed(9)
        q, k, v, dO = (torch.randn(B, H * dk, T, generator=g0).to(gpu) for _ in range(4))
        ek, ev = (torch.randn(1, 2 * w + 1, dk, generator=g0).to(gpu) for _ in range(2))
        ins = (q, k, v, ek, ev, torch.ones(B, T, device=gpu), dO)
        what = "B%d-H%d-dk%d-T%d-w%d-p%g%s" % (B, H, dk, T, w, p, " null stats" if null_stats else "")
        st, out, stats = abi_fwd(c, ins, p, 3, null_stats)
        torch.cuda.synchronize()
        assert st == expect, "forward %s returned %d" % (what, st)
        if expect == EINVAL:
            assert out.untouched() and stats.untouched(), "forward %s wrote to an output" % what
            out_in, stats_in = torch.zeros_like(q), torch.ones(B * H, T, 2, device=gpu)
        else:
            assert out.intact() and stats.intact() and not bool(torch.isnan(out.t).any()) and not bool(torch.isnan(stats.t).any())
            out_in, stats_in = out.t, stats.t
        if null_stats:
            from vcvits_amd._lib import lib, ptr, stream
            g = {n: Guarded(tuple(t.shape), gpu) for n, t in (("dq", q), ("dk", k), ("dv", v), ("dembk", ek), ("dembv", ev))}
            ws = Guarded((lib().vcv_rel_attn_stream_bwd_workspace(B, H, dk, T, w),), gpu)
            st = lib().vcv_rel_attn_stream_bwd(ptr(q), ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(ins[5]), ptr(out_in), None, ptr(dO),
                                               ptr(ws.t), ptr(g["dq"].t), ptr(g["dk"].t), ptr(g["dv"].t), ptr(g["dembk"].t),
                                               ptr(g["dembv"].t), B, H, dk, T, w, dk ** -0.5, p, 3, stream())
        else:
            st, g, ws = abi_bwd(c, ins, out_in, stats_in, p, 3)
        torch.cuda.synchronize()
        assert st == expect, "backward %s returned %d" % (what, st)
        if expect == EINVAL:
            assert ws.untouched() and all(t.untouched() for t in g.values()), "backward %s wrote to an output" % what
        else:
            assert ws.intact() and all(t.intact() and not bool(torch.isnan(t.t).any()) for t in g.values())
        tried.append(what)

    attempt(1, 1, 48, 40, 4)            # a head width the kernels are not built for
    attempt(1, 1, 32, 40, 8)            # 2 w + 1 = 17 relative positions
    attempt(1, 1, 32, 40, 4, null_stats=True)
    attempt(65536, 1, 32, 1, 4)         # B * H past the grid's y limit
    attempt(1, 1, 32, 40, 4, p=1.0)     # pdrop outside [0, 1)
    attempt(1, 1, 32, 40, 4, p=0.5, expect=0)  # the same buffers' shape is accepted when nothing is wrong with the call
    record("%d calls refused with VCV_EINVAL, outputs untouched: %s" % (len(tried) - 1, "; ".join(tried[:-1])))


# ---------------------------------------------------------------------------------------------------------------------
# 5. routing: ops.rel_attention
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def grad_min_t(value):
    from vcvits_amd import ops
    old = ops._ATTN_STREAM_GRAD_MIN_T[0]
    ops._ATTN_STREAM_GRAD_MIN_T[0] = value
    try:
        yield
    finally:
        ops._ATTN_STREAM_GRAD_MIN_T[0] = old


COUNTERS = ("attn_stream_grad", "attn_stream", "attn_fused")


def through_ops(c, ins, grad=True, want_attn=False, training=False, pdrop=0.0):
    """-> out, attn, leaves (q, k, v, embk, embv with requires_grad when `grad`), launches per counter, seed drawn (or None)"""
    from vcvits_amd import ops
    q, k, v, ek, ev, mask = ins[:6]
    leaves = tuple(t.clone().requires_grad_(grad) for t in (q, k, v, ek, ev))
    before = [ops.LAUNCH_COUNTS[n] for n in COUNTERS]
    old, ops.DROPOUT_TRACE[0] = ops.DROPOUT_TRACE[0], []
    try:
        with torch.set_grad_enabled(grad):
            out, attn = ops.rel_attention(*leaves, mask, c.H, c.w, pdrop, training=training, want_attn=want_attn)
        trace = ops.DROPOUT_TRACE[0]
    finally:
        ops.DROPOUT_TRACE[0] = old
    seed = trace[0][2] if trace else None
    return out, attn, leaves, tuple(ops.LAUNCH_COUNTS[n] - b for n, b in zip(COUNTERS, before)), seed


@pytest.mark.gpu
def test_routing_default_switch_does_not_stream(gpu):
    from vcvits_amd import ops
    c = G.CASES[7]  # T = 897
    assert ops._ATTN_STREAM_GRAD_MIN_T[0] == 0
    with compute_mode("f32"):
        before = ops.LAUNCH_COUNTS["attn_stream_grad"]
        out, _, leaves, n, _ = through_ops(c, on_gpu(c, gpu))
        assert n[0] == 0 and n[1] == 0, n
        out.backward(on_gpu(c, gpu)[6])
        assert ops.LAUNCH_COUNTS["attn_stream_grad"] == before and leaves[0].grad is not None


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_routing_with_the_switch_on(gpu, p):
    c = G.C257
    ins = on_gpu(c, gpu)
    dO = ins[6]
    with compute_mode("f32"), grad_min_t(1):
        out, attn, leaves, n, seed = through_ops(c, ins, training=p > 0, pdrop=p)
        assert n == (1, 0, 0) and attn is None, n
        assert (seed is not None) == (p > 0)
        seed = seed or 0
        out.backward(dO)
        got = dict(zip(G.GRADS, (t.grad for t in leaves)))
        st, o, s = abi_fwd(c, ins, p, seed)
        assert st == 0 and torch.equal(out, o.t), "ops.rel_attention: not vcv_rel_attn_stream_train_fwd's bits"
        st, g, _ = abi_bwd(c, ins, o.t, s.t, p, seed)
        assert st == 0
        for name in G.GRADS:
            assert torch.equal(got[name], g[name].t), "ops.rel_attention: %s is not vcv_rel_attn_stream_bwd's bits" % name
        ref, d32, _, _ = G.reference(c, p, seed)
        got["out"] = out
        check("routing MIN_T=1 %s p=%g" % (cid(c), p), got, ref, d32, ("out",) + G.GRADS)
        # what keeps its path
        _, a2, _, n, _ = through_ops(c, ins, want_attn=True, training=p > 0, pdrop=p)
        assert n[0] == 0 and a2 is not None and tuple(a2.shape) == (c.B, c.H, c.T, c.T), n
        if p == 0:  # a no-grad call keeps the inference kernel: the fused one at this T, the streamed one once it reaches down here
            from vcvits_amd import ops
            _, _, _, n, _ = through_ops(c, ins, grad=False)
            assert n == (0, 0, 1), n
            old, ops._ATTN_STREAM_MIN_T[0] = ops._ATTN_STREAM_MIN_T[0], 1
            try:
                _, _, _, n, _ = through_ops(c, ins, grad=False)
            finally:
                ops._ATTN_STREAM_MIN_T[0] = old
            assert n == (0, 1, 0), "a no-grad call moves only attn_stream: %s" % (n,)
    with compute_mode("bf16"), grad_min_t(1):  # fp32 matrix instructions in both compute modes
        out_b, _, leaves_b, n, seed_b = through_ops(c, ins, training=p > 0, pdrop=p)
        assert n == (1, 0, 0), n
        if p == 0:
            out_b.backward(dO)
            assert torch.equal(out_b, out)
            for name, t in zip(G.GRADS, leaves_b):
                assert torch.equal(t.grad, got[name]), "%s: bf16 mode differs from f32 mode" % name
        else:  # another seed was drawn: compare with the direct call at that seed
            st, o, s = abi_fwd(c, ins, p, seed_b)
            assert st == 0 and torch.equal(out_b, o.t)


# ---------------------------------------------------------------------------------------------------------------------
# 6. memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_memory_is_linear_in_T(gpu):
    """B 1, H 2, dk 32, T 4096, p = 0.1, forward + backward: out, stats, three gradients, their hand-over to .grad and the
    workspace.  One T x T tensor would be 128 x bytes(q)."""
    c = G.Case(1, 2, 32, 4096, 4, "ragged+hole")
    ins = tuple(t.to(gpu) for t in SG.inputs(c))
    g = torch.randn(c.B, c.H * c.dk, c.T, device=gpu)

    from vcvits_amd import ops

    def step(leaves):
        before = [ops.LAUNCH_COUNTS[n] for n in COUNTERS]
        out, _ = ops.rel_attention(*leaves, ins[5], c.H, c.w, 0.1, training=True, want_attn=False)
        out.backward(g)
        return tuple(ops.LAUNCH_COUNTS[n] - b for n, b in zip(COUNTERS, before))

    fresh = lambda: tuple(t.clone().requires_grad_(True) for t in ins[:5])
    with compute_mode("f32"), grad_min_t(1):
        step(fresh())  # (code objects, lazy allocations of the first call)
        leaves = fresh()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        n = step(leaves)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    bq = ins[0].numel() * 4
    limit = 8 * bq + (1 << 20)
    record("memory %s p=0.1 forward + backward: peak %d bytes (limit %d; q is %d bytes, one T x T tensor %d)" % (
        cid(c), peak, limit, bq, c.B * c.H * c.T * c.T * 4))
    assert n == (1, 0, 0), n
    assert peak <= limit, (peak, limit)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the encoder end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_encoder_end_to_end(gpu):
    """TransformerEncoder(64, 128, 2 heads, 2 layers, k = 3, p_dropout = 0) in train() at B = 2, T = 1000, lengths [1000, 700]:
    y, dx and every parameter gradient of (y * g).sum() against float64 autograd of the oracle; bound: the project's fp32 bar
    of 1e-4 (the oracle's own float32 run is <= 1.3e-6 from float64 on every tensor)."""
    from golden_util import fill_state_dict, keys_shapes_of
    from oracle import vits_oracle as O
    from vcvits_amd import ops
    from vcvits_amd.model.transformer.relative_attention_transformer import TransformerEncoder
    n_layers, BAR = 2, 1e-4
    m = TransformerEncoder(64, 128, n_heads=2, n_layers=n_layers, kernel_size=3, p_dropout=0.)
    sd = fill_state_dict(keys_shapes_of(m), 11)
    m.load_state_dict(sd)
    m = m.to(gpu).train()
    B, T = 2, 1000
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((B, 64, T)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((B, 64, T)).astype(np.float32))
    xm = O.sequence_mask(torch.tensor([1000, 700]), T).unsqueeze(1).float()
    # float64 autograd of the oracle
    names = [k for k, _ in m.named_parameters()]
    P64 = {"t." + k: v.double().clone().requires_grad_(k in names) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    y64 = O.transformer_encoder_forward(P64, "t", x64, xm.double(), 2, n_layers, 3)
    (y64 * g.double()).sum().backward()
    # the model on the streamed training kernels
    xg = x.to(gpu).requires_grad_(True)
    before = ops.LAUNCH_COUNTS["attn_stream_grad"]
    with compute_mode("f32"), grad_min_t(1):
        y = m(xg, xm.to(gpu))
        (y * g.to(gpu)).sum().backward()
    assert ops.LAUNCH_COUNTS["attn_stream_grad"] - before == n_layers
    errs = {"y": A.dist(y, y64), "dx": A.dist(xg.grad, x64.grad)}
    for k, prm in m.named_parameters():
        assert prm.grad is not None, k
        ref = P64["t." + k].grad
        if k.endswith("conv_k.bias"):  # zero mathematically (softmax shift invariance): measured against d conv_q.bias
            scale = P64["t." + k.replace("conv_k", "conv_q")].grad.abs().max().item()
            errs[k] = (prm.grad.cpu().double() - ref).abs().max().item() / scale
        else:
            errs[k] = A.dist(prm.grad, ref)
    worst = max(errs, key=errs.get)
    record("encoder 64/128 H2 L2 k3 B2 T1000 lengths 1000,700 train(): y=%.1e dx=%.1e worst parameter gradient %s=%.1e (bar %.0e)" % (
        errs["y"], errs["dx"], worst, errs[worst], BAR))
    for k, e in errs.items():
        assert e <= BAR, "%s off by %.3e" % (k, e)

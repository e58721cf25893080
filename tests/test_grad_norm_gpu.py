"""GPU: gradient norms of segments of the flat gradient buffer and clipping by global norm.

  A  vcv_grad_sqnorm through the launcher: one-hot buffers at every position where the kernel changes lane, vector, workgroup
     or the head / tail path; segment tables with misaligned bounds, empty segments and NaN outside every segment; normal data
     against math.fsum (exact); bit-reproducibility; NaN; the clip coefficient.
  B  vcv_adamw_clip / vcv_adamw_dev_clip against torch.optim.AdamW in float64 after clip_grad_norm_, and their bits at
     coef = 1.0f against vcv_adamw / vcv_adamw_dev.
  C  FlatAdamW(max_grad_norm, norm_segments) on three parameters, one of them without a gradient.
  D  the training module at reduced widths, B = 2 (in a child pytest process, as tests/test_graphed_gpu.py runs its
     whole-batch graphs).
  E  two ranks on one GPU (gloo), after tests/test_ddp_two_procs_one_gpu.py.

Bounds.  A sum of m non-negative fp64 terms, in ANY order, is within (m - 1) * 2^-53 < m * 2^-52 of the exact sum relative to
it, and the square of an fp32 value is exact in fp64: `sq` is held to m * 2^-52 of math.fsum, m the segment's length.  `norm`
is sqrt (correctly rounded in fp64) rounded to fp32: at most 1 fp32 ulp from float32(sqrt(exact)).  The AdamW comparisons use
tests/test_elementwise_gpu.py::test_adamw's measure (max |diff| over max |reference|) and its bound, 1e-6."""
import copy
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = 4096   # floats one workgroup of the reduction's first stage covers per pass: 256 threads x 4 float4 loads x 4 floats
MAXB = 1024   # workgroups per segment (the grid cap): past UNIT * MAXB floats a workgroup loops
N_LOOP = UNIT * MAXB + 7


def _cmp(name, got, ref, tol):
    """tests/test_elementwise_gpu.py::_cmp, restated."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref.double()).abs().max().item() / scale
    print("%s: rel err %.3e" % (name, err))
    assert err <= tol, "%s: rel err %.3e" % (name, err)


def _ulps(a, b):
    """Distance in fp32 ulps between two non-negative finite fp32 values."""
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


class _Sq:
    """One workspace / record / table per segment count; the workspace is filled with NaN before every call (a partial that
    stage one did not write in THIS call must not reach a sum)."""

    def __init__(self, gpu):
        self.gpu, self.state = gpu, {}

    def __call__(self, buf, table, max_norm=0.0):
        from vcvits_amd import ops
        S = len(table)
        if S not in self.state:
            self.state[S] = (torch.empty(S * ops.GRAD_SQNORM_WS_PER_SEGMENT, device=self.gpu, dtype=torch.float64),
                             torch.empty((ops.grad_sqnorm_record_bytes(S) + 7) // 8 * 8, device=self.gpu, dtype=torch.uint8))
        ws, rec = self.state[S]
        n = buf.numel()
        for lo, hi in table:
            assert 0 <= lo <= n and 0 <= hi <= n, (lo, hi, n)  # (the kernel trusts the table)
        segs = torch.tensor([v for r in table for v in r], dtype=torch.int64).to(self.gpu)
        ws.fill_(float("nan"))
        rec.fill_(0xFF)
        ops.grad_sqnorm(buf, segs, S, ws, rec, max_norm)
        raw = rec.cpu().numpy().tobytes()
        return {"sq": np.frombuffer(raw, np.float64, S, 0), "norm": np.frombuffer(raw, np.float32, S, 8 * S),
                "total": np.frombuffer(raw, np.float32, 1, 12 * S)[0], "coef": np.frombuffer(raw, np.float32, 1, 12 * S + 4)[0],
                "raw": raw[:12 * S + 8]}


@pytest.fixture(scope="module")
def sq(gpu):
    return _Sq(gpu)


def _positions(n, lo, hi, base_mis):
    """Element indices of [lo, hi) at 0, at the end and on both sides of every change of path: the scalar head (up to the first
    16-byte boundary; `base_mis` = floats the buffer itself starts past one), float4 lanes, waves, the four loads of a
    thread, workgroups, a workgroup's second pass, and the scalar tail."""
    head = (4 - (lo + base_mis) % 4) % 4
    body = lo + min(head, hi - lo)
    n4 = (hi - body) // 4
    tail = body + 4 * n4
    ks = {lo, hi - 1, lo + 1, hi - 2}
    for base in (lo, body):
        for d in (0, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, UNIT - 1, UNIT, UNIT + 1, 2 * UNIT - 1, 2 * UNIT,
                  UNIT * MAXB - 1, UNIT * MAXB, UNIT * MAXB + 1, UNIT * MAXB + 4):
            ks.update((base + d, base - 1 + d))
    for d in (-5, -4, -1, 0, 1, 2, 3):
        ks.add(tail + d)
    return sorted(k for k in ks if lo <= k < hi)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 262145, N_LOOP])
def test_sqnorm_one_hot(gpu, sq, n):
    """n zeros and a single 3.0 at position k: exactly 9.0 in the owning segment and 0.0 elsewhere -- whole buffer as one
    segment, cut in two at a misaligned element, and from a buffer that itself starts 4 bytes past a 16-byte boundary."""
    big = torch.zeros(n + 1, device=gpu, dtype=torch.float32)
    cut = n // 3 + (1 if (n // 3) % 4 == 0 else 0)  # (never a multiple of 4 once n >= 3)
    cases = [(big[:n], [(0, n)], 0)]
    if n >= 3:
        cases.append((big[:n], [(0, cut), (cut, n)], 0))
    if n in (5, 257, 1025, 262145):
        cases.append((big[1:], [(0, n)], 1))
    calls = 0
    for buf, table, mis in cases:
        for si, (lo, hi) in enumerate(table):
            for k in _positions(n, lo, hi, mis):
                buf[k] = 3.0
                r = sq(buf, table)
                buf[k] = 0.0
                calls += 1
                want = [9.0 if j == si else 0.0 for j in range(len(table))]
                assert r["sq"].tolist() == want, (n, table, mis, k, r["sq"].tolist())
                assert r["norm"].tolist() == [3.0 if j == si else 0.0 for j in range(len(table))], (n, table, k, r["norm"])
                assert r["total"] == 3.0 and r["coef"] == 1.0, (n, table, k, r["total"], r["coef"])
    print("n=%d: %d launches checked" % (n, calls))


def _exact(x64, lo, hi):
    return math.fsum((x64[lo:hi] * x64[lo:hi]).tolist()) if hi > lo else 0.0


def _check_against_fsum(r, x64, table, tag):
    exact = [_exact(x64, lo, hi) for lo, hi in table]
    for s, (lo, hi) in enumerate(table):
        m = max(hi - lo, 0)
        rel = abs(r["sq"][s] - exact[s]) / exact[s] if exact[s] else abs(r["sq"][s])
        u = _ulps(r["norm"][s], np.float32(math.sqrt(exact[s])))
        print("%s seg %d [%d, %d): sq rel err %.3e (bound %.3e), norm %d ulp" % (tag, s, lo, hi, rel, m * 2.0 ** -52, u))
        assert rel <= m * 2.0 ** -52, (tag, s, rel)
        assert u <= 1, (tag, s, r["norm"][s], math.sqrt(exact[s]))
    tot = np.float32(math.sqrt(math.fsum(exact)))
    assert _ulps(r["total"], tot) <= 1, (tag, r["total"], tot)


TABLES = [
    [(1, 4998)],                                            # S = 1, lo % 4 = 1
    [(2, 1027), (1029, 4093)],                              # S = 2, lo % 4 = 2 and 1, a gap between them
    [(3, 1030), (1030, 1030), (1031, 4999)],                # S = 3, lo % 4 = 3, an empty segment, lo % 4 = 3
    [(7, 7)],                                               # nothing but an empty segment
    [(2501, 4999), (5, 2498)],                              # not in buffer order
    [(6, 6), (9, 10), (10, 13), (13, 17), (4100, 4100), (17, 4100), (4101, 4102), (4500, 4999)],  # S = 8
]


@pytest.mark.parametrize("ti", range(len(TABLES)))
def test_sqnorm_segment_tables(gpu, sq, ti):
    """Misaligned bounds, empty segments, segments that do not cover the buffer: every element outside them is NaN, and no
    NaN may reach a sum."""
    table = TABLES[ti]
    n = 5000
    x = torch.randn(n, generator=torch.Generator().manual_seed(40 + ti))
    covered = torch.zeros(n, dtype=torch.bool)
    for lo, hi in table:
        covered[lo:hi] = True
    assert not bool(covered.all())
    x[~covered] = float("nan")
    r = sq(x.to(gpu), table)
    assert np.isfinite(r["sq"]).all() and np.isfinite(r["norm"]).all() and np.isfinite(r["total"]), r
    for s, (lo, hi) in enumerate(table):
        if hi <= lo:
            assert r["sq"][s] == 0.0 and r["norm"][s] == 0.0
    _check_against_fsum(r, x.double().numpy(), table, "table %d" % ti)


def test_sqnorm_rejects_more_than_eight_segments(gpu, sq):
    with pytest.raises(ValueError):
        sq(torch.zeros(64, device=gpu), [(i, i + 1) for i in range(9)])


@pytest.fixture(scope="module")
def normal_data(gpu):
    n = 1000003
    x = torch.randn(n, generator=torch.Generator().manual_seed(7)) * 0.37
    table = [(0, 333335), (333335, 666671), (666671, n)]
    return x.to(gpu), x.double().numpy(), table


def test_sqnorm_normal_data_against_fsum(gpu, sq, normal_data):
    xg, x64, table = normal_data
    _check_against_fsum(sq(xg, table), x64, table, "normal")


def test_sqnorm_two_calls_give_identical_bits(gpu, sq, normal_data):
    xg, _x64, table = normal_data
    a = sq(xg, table, 3.0)
    b = sq(xg, table, 3.0)
    assert a["raw"] == b["raw"]


def test_sqnorm_nan_propagates(gpu, sq):
    x = torch.randn(3000, generator=torch.Generator().manual_seed(1))
    x[1234] = float("nan")
    r = sq(x.to(gpu), [(0, 1000), (1000, 3000)], 1.0)
    assert np.isfinite(r["sq"][0]) and np.isnan(r["sq"][1]) and np.isnan(r["norm"][1])
    assert np.isnan(r["total"]) and np.isnan(r["coef"])
    r = sq(x.to(gpu), [(0, 1000), (1000, 3000)], 0.0)  # clipping off: the coefficient does not depend on the data
    assert np.isnan(r["total"]) and r["coef"] == 1.0
    x[1234] = float("inf")
    r = sq(x.to(gpu), [(0, 3000)], 1.0)
    assert np.isinf(r["total"]) and r["coef"] == 0.0  # (torch: max_norm / inf = 0)


def test_sqnorm_clip_coefficient(gpu, sq):
    x = torch.randn(4099, generator=torch.Generator().manual_seed(2))
    xg = x.to(gpu)
    table = [(0, 1001), (1001, 4099)]
    total = sq(xg, table)["total"]
    assert total > 1.0
    assert sq(xg, table, float(total) * 1.5)["coef"] == 1.0           # a norm below max_norm
    assert sq(torch.zeros_like(xg), table, 1e-3)["coef"] == 1.0        # an all-zero gradient: 1e-3 / 1e-6 clamps to 1
    for off in (0.0, -1.0, float("inf"), float("nan")):                # clipping off
        r = sq(xg, table, off)
        assert r["coef"] == 1.0 and r["total"] == total
    for max_norm in (float(total) / 2, 0.37, 1e-4):                     # the norm is 2 x max_norm, and two more
        r = sq(xg, table, max_norm)
        want = np.float32(max_norm) / (r["total"] + np.float32(1e-6))   # torch's formula, every operation in fp32
        assert isinstance(want, np.float32) and r["coef"] == want and r["coef"] < 1.0, (max_norm, r["coef"], want)
    half = sq(xg, table, float(total) / 2)["coef"]
    assert abs(float(half) - 0.5) < 1e-6


# ---- B: the _clip AdamW entries -------------------------------------------------------------------------------------
HYP = dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-9, wd=0.01)


def _torch_adamw_f64(p0, grads, max_norm):
    """torch.optim.AdamW on the CPU in float64, clip_grad_norm_ before every step; `grads`: one list per step."""
    pr = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([pr], lr=HYP["lr"], betas=HYP["betas"], eps=HYP["eps"], weight_decay=HYP["wd"])
    for g in grads:
        pr.grad = g.double().clone()
        torch.nn.utils.clip_grad_norm_([pr], max_norm)
        opt.step()
    return pr.detach()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_adamw_clip_against_torch_f64(gpu, sq, n, form):
    from vcvits_amd import ops
    gen = torch.Generator().manual_seed(6 + n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    max_norm = 0.5 * float(grads[0].double().norm())  # half the first gradient's norm
    ref = _torch_adamw_f64(p0, grads, max_norm)
    p, m, v = p0.to(gpu), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    st = _Sq(gpu)
    st(torch.zeros(4, device=gpu), [(0, 4)])  # (allocates the workspace and the record)
    ws, rec = st.state[1]
    segs = torch.tensor([0, n], dtype=torch.int64).to(gpu)
    coef = rec[16:20].view(torch.float32)[0]
    hyper = torch.zeros(2, device=gpu, dtype=torch.int32)
    for step, g in enumerate(grads, 1):
        gg = g.to(gpu)
        keep = gg.clone()
        ops.grad_sqnorm(gg, segs, 1, ws, rec, max_norm)
        assert step > 1 or float(coef) < 1.0
        if form == "host":
            ops.adamw_step_clip(p, gg, m, v, HYP["lr"], HYP["betas"], HYP["eps"], HYP["wd"], step, coef)
        else:
            ops.set_hyper(hyper, HYP["lr"], step - 1)
            ops.adamw_step_dev_clip(p, gg, m, v, HYP["betas"], HYP["eps"], HYP["wd"], hyper, 1, coef)
        assert torch.equal(gg, keep)  # the gradient is read, never written
    _cmp("adamw_clip[%s, n=%d]" % (form, n), p, ref, tol=1e-6)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_adamw_clip_with_unit_coefficient_is_the_plain_step(gpu, n):
    from vcvits_amd import ops
    gen = torch.Generator().manual_seed(60 + n)
    one = torch.ones((), device=gpu)
    hyper = torch.zeros(2, device=gpu, dtype=torch.int32)
    state = [torch.randn(n, generator=gen).to(gpu), torch.randn(n, generator=gen).to(gpu) * 0.1,
             (torch.randn(n, generator=gen) ** 2).to(gpu) * 0.01]
    for form in ("host", "dev"):
        a, b = [t.clone() for t in state], [t.clone() for t in state]
        for step in range(1, 4):
            g = torch.randn(n, generator=gen).to(gpu)
            keep = g.clone()
            if form == "host":
                ops.adamw_step(a[0], g, a[1], a[2], HYP["lr"], HYP["betas"], HYP["eps"], HYP["wd"], step)
                ops.adamw_step_clip(b[0], g, b[1], b[2], HYP["lr"], HYP["betas"], HYP["eps"], HYP["wd"], step, one)
            else:
                ops.set_hyper(hyper, HYP["lr"], step - 1)
                ops.adamw_step_dev(a[0], g, a[1], a[2], HYP["betas"], HYP["eps"], HYP["wd"], hyper, 1)
                ops.adamw_step_dev_clip(b[0], g, b[1], b[2], HYP["betas"], HYP["eps"], HYP["wd"], hyper, 1, one)
            assert torch.equal(g, keep)
            for name, x, y in zip("pmv", a, b):
                assert torch.equal(x, y), (form, n, step, name, float((x - y).abs().max()))
        assert not torch.equal(a[0], state[0])


# ---- C: FlatAdamW ---------------------------------------------------------------------------------------------------
def _torch_params_f64(p0s, grad_steps, max_norm, lr, betas, eps):
    """torch.optim.AdamW (float64, CPU) over several parameters; grad_steps: per step one list of gradients, None = the
    parameter received none (torch skips it); clip_grad_norm_ over all of them before each step."""
    prs = [torch.nn.Parameter(p.double().clone()) for p in p0s]
    opt = torch.optim.AdamW(prs, lr=lr, betas=betas, eps=eps, weight_decay=0.01)
    norms = []
    for grads in grad_steps:
        for pr, g in zip(prs, grads):
            pr.grad = None if g is None else g.double().clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(prs, max_norm if max_norm is not None else float("inf"))))
        opt.step()
    return [pr.detach() for pr in prs], norms


@pytest.mark.parametrize("segments", ["default", "named"])
def test_flat_adamw_clipped_step(gpu, segments):
    from vcvits_amd.light.optim import FlatAdamW
    gen = torch.Generator().manual_seed(17)
    shapes = [(7,), (64, 5), (1,)]
    p0s = [torch.randn(*s, generator=gen) for s in shapes]
    ws = [[torch.randn(*s, generator=gen) for s in shapes] for _ in range(3)]
    a, b, c = [torch.nn.Parameter(p.clone().to(gpu)) for p in p0s]
    lr, betas, eps = 2e-4, (0.8, 0.99), 1e-9
    # b (64 x 5, the middle of the buffer) receives no gradient: the step is two launches around it
    exact = math.sqrt(math.fsum((torch.cat([ws[0][0].flatten(), ws[0][2].flatten()]).double() ** 2).tolist()))
    max_norm = 0.5 * exact
    kw = {} if segments == "default" else {"norm_segments": [("ab", [a, b]), ("c", [c])]}
    opt = FlatAdamW([a, b, c], lr, betas=betas, eps=eps, max_grad_norm=max_norm, **kw)
    assert opt.offsets == [0, 1, 321]
    ref, ref_norms = _torch_params_f64(p0s, [[w[0], None, w[2]] for w in ws], max_norm, lr, betas, eps)
    for step, w in enumerate(ws):
        opt.zero_grad()
        loss = (a * w[0].to(gpu)).sum() + (c * w[2].to(gpu)).sum()
        loss.backward()
        keep = opt.grad.clone()
        opt.step()
        assert torch.equal(opt.grad, keep)  # the flat gradient buffer keeps the unclipped gradient
        got = {k: np.float32(v.item()) for k, v in opt.grad_norms().items()}
        sq_a = math.fsum((w[0].double() ** 2).flatten().tolist())
        sq_c = math.fsum((w[2].double() ** 2).flatten().tolist())
        assert _ulps(got["total"], np.float32(math.sqrt(sq_a + sq_c))) <= 1 and abs(got["total"] - ref_norms[step]) <= 1e-6 * ref_norms[step]
        if segments == "default":
            assert set(got) == {"all", "total", "coef"} and got["all"] == got["total"]
        else:
            assert set(got) == {"ab", "c", "total", "coef"}
            assert _ulps(got["ab"], np.float32(math.sqrt(sq_a))) <= 1 and _ulps(got["c"], np.float32(math.sqrt(sq_c))) <= 1
        assert got["coef"] == np.float32(max_norm) / (got["total"] + np.float32(1e-6)) and got["coef"] < 1.0
    for name, p, r in zip("abc", (a, b, c), ref):
        _cmp("flat_adamw_clip[%s] %s" % (segments, name), p, r, tol=1e-6)
    # the parameter without a gradient is skipped as before: not decayed, no moments, no step count
    assert torch.equal(b.detach().cpu(), p0s[1]) and opt._pstep == [3, 0, 3]
    assert float(opt.exp_avg[1:321].abs().max()) == 0.0 and float(opt.exp_avg_sq[1:321].abs().max()) == 0.0
    assert set(opt.state_dict()) == {"step", "lr", "exp_avg", "exp_avg_sq", "param_steps"}
    # switched off again, the step is the one it always was
    opt.max_grad_norm = None
    assert not opt.norms_enabled()
    opt.close()


def test_flat_adamw_norms_without_clipping(gpu):
    """log_norms alone: the norms are written, the coefficient is exactly 1, and the parameters get the bits of the plain
    step."""
    from vcvits_amd.light.optim import FlatAdamW
    gen = torch.Generator().manual_seed(18)
    p0 = torch.randn(1000, generator=gen)
    w = torch.randn(1000, generator=gen)
    res = []
    for log in (False, True):
        p = torch.nn.Parameter(p0.clone().to(gpu))
        opt = FlatAdamW([p], 2e-4, betas=(0.8, 0.99), eps=1e-9)
        opt.log_norms = log
        for _ in range(2):
            opt.zero_grad()
            (p * w.to(gpu)).sum().backward()
            opt.step()
        if log:
            n = opt.grad_norms()
            assert float(n["coef"]) == 1.0 and _ulps(n["all"].item(), np.float32(math.sqrt(math.fsum((w.double() ** 2).tolist())))) <= 1
        res.append(p.detach().clone())
        opt.close()
    assert torch.equal(res[0], res[1])


# ---- D: VCVITS (child process) ----------------------------------------------------------------------------------------
IN_CHILD = os.environ.get("VCVITS_GRAD_NORM_TESTS_CHILD") == "1"
module_tests = pytest.mark.skipif(not IN_CHILD, reason="runs inside test_module_tests_in_child_process")
N_MODULE_TESTS = 7


def test_module_tests_in_child_process(gpu):
    """A GPU fault in a graph replay kills the process: the module tests run in a child pytest, as tests/test_graphed_gpu.py's."""
    if IN_CHILD:
        pytest.skip("this is the child")
    env = dict(os.environ, VCVITS_GRAD_NORM_TESTS_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_module_"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900,
                       cwd=os.path.dirname(HERE))
    out = r.stdout.decode(errors="replace")
    print(out[-6000:])
    assert r.returncode == 0, out[-6000:]
    assert "%d passed" % N_MODULE_TESTS in out, out[-1500:]


def _module_class():
    """The VCVITS of tests/test_graphed_gpu.py's reduced-width B = 2 workload: the GAN step on the decoder (VocoderGAN), the
    module whose step deterministic mode makes bit-reproducible (tests/test_determinism_gpu.py) -- which is what lets the
    tests below ask for equal BITS (that test pins the vocoder step only; nothing pins the full SynthesizerSVC step's bits).
    The loss VALUES are summed with float atomics in every mode: they are compared as tests/test_graphed_gpu.py compares
    them, to 2e-5; parameters, norms and coefficients bit for bit."""
    from vcvits_amd.light.vcvits import VocoderGAN
    return VocoderGAN


def _cfg():
    from vcvits_amd import configs
    cfg = configs.base()
    cfg["model"].update({"inter_channels": 16, "upsample_initial_channel": 32, "multi_period_discriminator_periods": [2, 3]})
    cfg["data"]["n_mel_channels"] = 40
    cfg["train"]["segment_size"] = 4096
    return cfg


def _batches(cfg, gpu):
    from vcvits_amd import synthetic
    return [{k: v.to(gpu) for k, v in synthetic.vocoder_batch(2, 16, segment_size=4096, seed=3 + i).items()} for i in range(2)]


_RUNS = {}
N_BATCHES = 4  # recorded runs: two eager sightings, the capture at the third, replays at the third and the fourth


def _run(gpu, name, clip=None, log=False, recorded=False, probe_first=False, clip_each=None):
    """One module from the shared initial state through N_BATCHES batches (batch 0, 1, 0, 1) in deterministic mode; cached.
    clip_each = (max norm of optim_g, max norm of optim_d): written through Lightning's hook, one value per optimizer."""
    if name in _RUNS:
        return _RUNS[name]
    from vcvits_amd import ops
    from vcvits_amd.light import graphed
    VCVITS = _module_class()
    cfg = _cfg()
    if "sd" not in _RUNS:
        torch.manual_seed(11)
        _RUNS["sd"] = copy.deepcopy(VCVITS(**cfg).state_dict())
        _RUNS["batches"] = _batches(cfg, gpu)
    if clip is not None:
        cfg["trainer"] = {"gradient_clip_val": clip, "gradient_clip_algorithm": "norm"}
    cfg["train"]["log_grad_norms"] = log
    res = {"outs": [], "params": [], "probe": {}}
    ops.set_deterministic(True)
    graphed.set_batch_enabled(recorded)
    try:
        torch.manual_seed(12)
        mod = VCVITS(**cfg)
        mod.load_state_dict(_RUNS["sd"])
        mod = mod.to(gpu)
        mod.configure_optimizers()
        if clip_each is not None:
            mod.configure_gradient_clipping(mod.optim_g, 0, gradient_clip_val=clip_each[0], gradient_clip_algorithm="norm")
            mod.configure_gradient_clipping(mod.optim_d, 1, gradient_clip_val=clip_each[1], gradient_clip_algorithm="norm")
        res["p0"] = (mod.optim_g.flat.detach().cpu().clone(), mod.optim_d.flat.detach().cpu().clone())

        def probe(idx, opt):
            res["probe"][idx] = {"grad": opt.grad.detach().cpu().clone(), "touched": bytes(opt._touched)}

        for i in range(N_BATCHES):
            out = mod.fit_batch(_RUNS["batches"][i % 2], after_backward=probe if (probe_first and i == 0) else None)
            res["outs"].append({k: v.detach().cpu().clone() for k, v in out.items()})
            res["params"].append((mod.optim_g.flat.detach().cpu().clone(), mod.optim_d.flat.detach().cpu().clone()))
            if i == 0:
                res["d_total"] = float(mod.optim_d.grad_norms()["total"]) if mod.optim_d.norms_enabled() else None
        res["scalars"] = mod.training_scalars()
        bg = mod.__dict__.get("_batch_graph")
        res["replays"], res["captures"], res["failed"] = (bg.replays, bg.captures, bg.failed) if bg is not None else (0, 0, None)
        # element ranges of the three networks in the two flat buffers, from the parameters themselves (not from the
        # optimizers' segment tables: this is what catches a wrong segment boundary)
        res["ranges"] = {}
        for net, opt in (("net_g", mod.optim_g), ("net_period_d", mod.optim_d), ("net_scale_d", mod.optim_d)):
            ids = {id(p) for p in getattr(mod, net).parameters()}
            res["ranges"][net] = [(opt.offsets[i], opt.offsets[i] + p.numel()) for i, p in enumerate(opt.params) if id(p) in ids]
        res["param_ranges"] = {k: [(o.offsets[i], o.offsets[i] + p.numel()) for i, p in enumerate(o.params)]
                               for k, o in (("g", mod.optim_g), ("d", mod.optim_d))}
        res["hyper"] = dict(lr=mod.optim_g.lr, betas=mod.optim_g.betas, eps=mod.optim_g.eps)
        mod.optim_g.close()
        mod.optim_d.close()
        mod.drop_graphs()
    finally:
        graphed.set_batch_enabled(True)
        ops.set_deterministic(False)
    if recorded:
        assert res["failed"] is False and res["captures"] == 1 and res["replays"] == N_BATCHES - 2, (res["failed"], res["captures"], res["replays"])
    else:
        assert res["replays"] == 0
    _RUNS[name] = res
    return res


def _probe_run(gpu):
    """Norms on, no clipping, eager, the first batch probed: the unclipped gradients and norms of batch 0."""
    return _run(gpu, "probe", log=True, probe_first=True)


def _clip_values(gpu):
    r = _probe_run(gpu)
    return 0.5 * float(r["outs"][0]["grad_norm_g"]), 0.5 * r["d_total"]


def _bits_equal(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        same = torch.equal(x, y)
        print("%s[%d]: %s%s" % (what, i, "bit-equal" if same else "DIFFERENT", "" if same else
                                " (%d of %d elements, max |diff| %.3e)" % (int((x != y).sum()), x.numel(), float((x - y).abs().max()))))
    for x, y in zip(a, b):
        assert torch.equal(x, y), what


@module_tests
def test_module_options_off_returns_losses_only(gpu):
    for recorded in (False, True):
        r = _run(gpu, "off_rec" if recorded else "off_eager", recorded=recorded)
        for out in r["outs"]:
            assert set(out) == {"g", "d"}, sorted(out)


@module_tests
@pytest.mark.parametrize("recorded", [False, True])
def test_module_huge_clip_value_changes_no_bit(gpu, recorded):
    """gradient_clip_val = 1e30: the norm launch and the `_clip` steps run with coef = 1.0f; the parameters after every batch
    have the bits of a run without the option."""
    tag = "rec" if recorded else "eager"
    off = _run(gpu, "off_" + tag, recorded=recorded)
    on = _run(gpu, "huge_" + tag, clip=1e30, recorded=recorded)
    assert set(on["outs"][-1]) == {"g", "d", "grad_norm_g", "grad_norm_p_d", "grad_norm_s_d", "clip_coef_g", "clip_coef_d"}
    for out in on["outs"]:
        assert float(out["clip_coef_g"]) == 1.0 and float(out["clip_coef_d"]) == 1.0 and float(out["grad_norm_g"]) > 0
    for k in range(2):
        _bits_equal([p[k] for p in off["params"]], [p[k] for p in on["params"]], "huge clip %s, optimizer %d, batch" % (tag, k))


def _f64_first_step(r, key, idx, max_norm):
    """torch.optim.AdamW in float64 on the CPU, one step from the run's initial parameters on the gradient the probe captured
    (per parameter; those that received no gradient have .grad None), after clip_grad_norm_(max_norm)."""
    p0, pr = r["p0"][idx], r["probe"][idx]
    ranges = r["param_ranges"][key]
    h = r["hyper"]
    p0s = [p0[lo:hi] for lo, hi in ranges]
    grads = [pr["grad"][lo:hi] if pr["touched"][i] else None for i, (lo, hi) in enumerate(ranges)]
    ref, norms = _torch_params_f64(p0s, [grads], max_norm, h["lr"], h["betas"], h["eps"])
    return torch.cat([x.flatten() for x in ref]), norms[0]


@module_tests
def test_module_clipped_replays_equal_eager_and_the_f64_restatement(gpu):
    cg, cd = _clip_values(gpu)
    eager = _run(gpu, "clip_eager", log=True, clip_each=(cg, cd), probe_first=True)
    rec = _run(gpu, "clip_rec", log=True, clip_each=(cg, cd), recorded=True)
    # clipping is active on the first batch, at about one half
    c0 = eager["outs"][0]
    print("clip values %.6g / %.6g; first batch coefficients %.6f / %.6f" % (cg, cd, float(c0["clip_coef_g"]), float(c0["clip_coef_d"])))
    assert abs(float(c0["clip_coef_g"]) - 0.5) < 1e-3 and abs(float(c0["clip_coef_d"]) - 0.5) < 0.1
    # the first step against float64, from the gradient the probe captured in this very run
    for key, idx, max_norm in (("g", 0, cg), ("d", 1, cd)):
        ref, norm = _f64_first_step(eager, key, idx, max_norm)
        assert norm > max_norm
        _cmp("first clipped step, optimizer %s" % key, eager["params"][0][idx], ref, tol=1e-6)
    # replayed batches (the third and the fourth) are the eager ones, bit for bit: parameters, norms, coefficients
    for k in range(2):
        _bits_equal([p[k] for p in eager["params"]], [p[k] for p in rec["params"]], "clipped, optimizer %d, batch" % k)
    for i, (a, b) in enumerate(zip(eager["outs"], rec["outs"])):
        assert set(a) == set(b)
        for name in sorted(a):
            if name in ("g", "d"):  # (loss values: float atomics in every mode, _module_class)
                assert abs(float(a[name]) - float(b[name])) <= 2e-5 * abs(float(a[name])), (i, name, float(a[name]), float(b[name]))
            else:
                assert torch.equal(a[name], b[name]), (i, name, float(a[name]), float(b[name]))
    assert not torch.equal(eager["params"][0][0], _run(gpu, "off_eager")["params"][0][0])  # (and clipping moved the step)


@module_tests
def test_module_norms_are_the_fsum_norms_of_the_captured_gradient(gpu):
    """Over net_g, net_period_d and net_scale_d, each to 1 fp32 ulp: a wrong segment boundary moves a norm by far more."""
    r = _probe_run(gpu)
    out = r["outs"][0]
    assert set(out) == {"g", "d", "grad_norm_g", "grad_norm_p_d", "grad_norm_s_d"}  # (norms on, clipping off: no coefficients)
    for net, idx, name in (("net_g", 0, "grad_norm_g"), ("net_period_d", 1, "grad_norm_p_d"), ("net_scale_d", 1, "grad_norm_s_d")):
        g = r["probe"][idx]["grad"].double()
        exact = math.sqrt(math.fsum(torch.cat([g[lo:hi] for lo, hi in r["ranges"][net]]).pow(2).tolist()))
        u = _ulps(out[name].item(), np.float32(exact))
        print("%s = %.9g, fsum %.9g: %d ulp (%d elements)" % (name, float(out[name]), exact, u, sum(hi - lo for lo, hi in r["ranges"][net])))
        assert exact > 0 and u <= 1, (name, float(out[name]), exact)
    assert float(out["grad_norm_p_d"]) != float(out["grad_norm_s_d"])


@module_tests
def test_module_one_graph_returns_each_batch_its_own_norms(gpu):
    """Batches 0 and 1 (one shape, different data) through ONE recorded graph: the third and fourth batch are replays, their
    norm triples differ from each other and are the eager run's bits."""
    eager = _run(gpu, "log_eager", log=True)
    rec = _run(gpu, "log_rec", log=True, recorded=True)
    names = ("grad_norm_g", "grad_norm_p_d", "grad_norm_s_d")
    t2, t3 = [tuple(float(rec["outs"][i][n]) for n in names) for i in (2, 3)]
    print("replayed norm triples:", t2, t3)
    assert all(a != b for a, b in zip(t2, t3)), (t2, t3)
    for i in range(N_BATCHES):
        for n in names:
            assert torch.equal(eager["outs"][i][n], rec["outs"][i][n]), (i, n, float(eager["outs"][i][n]), float(rec["outs"][i][n]))
    # norms on, clipping off: the parameters keep the bits of the run without either option
    off = _run(gpu, "off_rec", recorded=True)
    for k in range(2):
        _bits_equal([p[k] for p in off["params"]], [p[k] for p in rec["params"]], "log only, optimizer %d, batch" % k)


@module_tests
def test_module_training_scalars_after_a_replayed_batch(gpu):
    """Every name of the reference's two scalar_dicts (vits/light/vcvits.py:123-130, 167-171), as Python floats."""
    rec = _run(gpu, "log_rec", log=True, recorded=True)
    s = rec["scalars"]
    want = ["loss/g/total", "learning_rate", "grad_norm_g", "loss/g/p_fm", "loss/g/s_fm", "loss/g/p_gen", "loss/g/s_gen",
            "loss/g/loss_mel", "loss/d/total", "grad_norm_p_d", "grad_norm_s_d"]
    want += ["loss/d_p_%s/%d" % (k, i) for k in "rg" for i in range(2)]   # two periods
    want += ["loss/d_s_%s/%d" % (k, i) for k in "rg" for i in range(3)]   # three scales
    missing = [k for k in want if k not in s]
    assert not missing, (missing, sorted(s))
    assert all(isinstance(v, float) and math.isfinite(v) for v in s.values()), s
    last = rec["outs"][-1]
    assert s["grad_norm_g"] == float(last["grad_norm_g"]) and s["loss/g/total"] == float(last["g"]) and s["loss/d/total"] == float(last["d"])
    d_terms = sum(v for k, v in s.items() if k.startswith("loss/d_"))
    assert abs(d_terms - s["loss/d/total"]) <= 1e-5 * abs(s["loss/d/total"])
    # without the options the scalars are still there, the norms are not
    off = _run(gpu, "off_rec", recorded=True)["scalars"]
    assert "grad_norm_g" not in off and "loss/d_p_r/0" in off and "loss/g/total" in off and "learning_rate" in off


# ---- E: two ranks on one GPU ------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, path):
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "GLOO_SOCKET_IFNAME": "lo"})
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vcvits_amd import configs, ops, synthetic
    from vcvits_amd.light.vcvits import VocoderGAN
    ops.set_deterministic(True)
    cfg = configs.base()
    cfg["model"].update({"inter_channels": 16, "upsample_initial_channel": 32, "multi_period_discriminator_periods": [2, 3]})
    cfg["data"]["n_mel_channels"] = 40
    cfg["train"]["segment_size"] = 4096
    cfg["train"]["log_grad_norms"] = True
    cfg["trainer"] = {"gradient_clip_val": 1e-2}  # far below either optimizer's gradient norm at initialisation
    torch.manual_seed(5)
    module = VocoderGAN(**cfg).to(dev)
    module.configure_optimizers()
    assert module.optim_g._ddp and module.optim_g.world == world
    outs = []
    for i in range(2):
        batch = {k: v.to(dev) for k, v in synthetic.vocoder_batch(2, 16, segment_size=4096, seed=10 * i + rank).items()}  # per rank
        out = module.fit_batch(batch)
        outs.append({k: v.detach().cpu().clone() for k, v in out.items()})
    torch.save(dict(outs=outs, g=module.optim_g.flat.cpu(), d=module.optim_d.flat.cpu()), path)
    dist.barrier()
    from vcvits_amd.light.optim import shutdown_flag_groups
    shutdown_flag_groups()
    dist.destroy_process_group()


def test_two_ranks_clip_by_the_same_coefficient(gpu, tmp_path):
    """Each rank its own data, clipping on below the norm: the norm is taken after the all-reduce, so norms, coefficients and
    parameters are bit-identical across the ranks after two batches (the losses are each rank's own)."""
    port = _free_port()
    procs, paths = [], []
    for rank in range(2):
        path = str(tmp_path / ("rank%d.pt" % rank))
        paths.append(path)
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), str(rank), "2", str(port), path],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise AssertionError("a rank hung (ranks out of step with their collectives?)")
        outs.append(o)
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    a, b = [torch.load(p, weights_only=False) for p in paths]
    assert torch.equal(a["g"], b["g"]) and torch.equal(a["d"], b["d"])
    for x, y in zip(a["outs"], b["outs"]):
        for name in ("grad_norm_g", "grad_norm_p_d", "grad_norm_s_d", "clip_coef_g", "clip_coef_d"):
            assert torch.equal(x[name], y[name]), (name, float(x[name]), float(y[name]))
        assert float(x["clip_coef_g"]) < 1.0 and float(x["clip_coef_d"]) < 1.0
        assert float(x["g"]) != float(y["g"])  # different data on the two ranks


if __name__ == "__main__":
    _worker(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])

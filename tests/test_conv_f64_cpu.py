"""tests/conv_f64.py (the float64 restatement of VcvConvArgs that tests/test_conv_epilogue_abi_gpu.py measures the kernels
against) pinned to torch's float64 CPU convolutions and to torch autograd, on the roles ops/conv.py builds: Conv1d, the
period Conv2d((k, 1)), ConvTranspose1d as one phase per output residue, and their data gradients (a_mode 1 with a negative tap
step, the flipped-weight form, the phased strided form, out_tf as the derivative of the activation the gradient flows into).
No GPU, no library."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_f64 as C

TOL = 1e-12


def _t(rng, *sh):
    return torch.from_numpy(rng.standard_normal(sh))


def _rng(shape):
    return np.random.default_rng(zlib.crc32(repr(shape).encode()))


def _out_len(T, K, s, pad, dil):
    return (T + 2 * pad - dil * (K - 1) - 1) // s + 1


def _fconv(x, w, s, pad, dil, groups=1):
    """x [B, C, T, P], w [M, C/g, K] -> float64 [B, M, Tout, P] by torch"""
    if x.shape[3] == 1:
        return F.conv1d(x[..., 0], w, None, s, pad, dil, groups).unsqueeze(-1)
    return F.conv2d(x, w.unsqueeze(-1), None, (s, 1), (pad, 0), (dil, 1), groups)


FWD = [(2, 5, 7, 40, 1, 3, 1, 1, 1, 1), (2, 6, 4, 33, 1, 5, 2, 2, 1, 1), (1, 3, 5, 50, 1, 4, 3, 1, 2, 1), (2, 4, 6, 41, 1, 11, 1, 5, 5, 1),
       (2, 5, 3, 17, 3, 5, 3, 2, 1, 1), (3, 4, 4, 9, 13, 5, 1, 2, 1, 1), (2, 3, 4, 20, 2, 2, 2, 0, 3, 1), (2, 8, 12, 37, 1, 41, 4, 20, 1, 4),
       (2, 6, 9, 30, 1, 3, 1, 1, 1, 3), (1, 4, 4, 12, 5, 1, 1, 0, 1, 2)]


@pytest.mark.parametrize("shape", FWD, ids=lambda s: "B%d-C%d-M%d-T%d-P%d-K%d-s%d-pad%d-dil%d-G%d" % s)
def test_forward_is_conv1d_and_period_conv2d(shape):
    B, Cin, M, T, P, K, s, pad, dil, G = shape
    rng = _rng(shape)
    x, w = _t(rng, B, Cin, T, P), _t(rng, M, Cin // G, K)
    Tout = _out_len(T, K, s, pad, dil)
    g = C.geom(B, G, Cin // G, M // G, T, Tout, P, K, s, dil, -pad)
    prior = _t(rng, B, M, Tout, P)
    y, S = C.conv(g, x, w, prior)
    ref = _fconv(x, w, s, pad, dil, G)
    assert C.dist(y, ref) <= TOL
    assert C.dist(S, _fconv(x.abs(), w.abs(), s, pad, dil, G)) <= TOL
    # fewer positions than output rows: the rows past Q keep the prior, S is zero there
    if Tout > 3:
        y2, S2 = C.conv(g._replace(Q=Tout - 3), x, w, prior)
        assert C.dist(y2[:, :, :Tout - 3], ref[:, :, :Tout - 3]) <= TOL and torch.equal(y2[:, :, Tout - 3:], prior[:, :, Tout - 3:])
        assert not bool(S2[:, :, Tout - 3:].any())
    # more positions than rows (Q > Tout) and a negative row offset: nothing outside [0, Tout) is written
    # (q = 0 goes to row -1, q = Tout + 1 to row Tout; q = Tout reads zeros past the input)
    y3, _ = C.conv(g._replace(Q=Tout + 2, oo=-1), x, w, prior)
    assert C.dist(y3, _fconv(F.pad(x, (0, 0, 0, 3 * s)), w, s, pad, dil, G)[:, :, 1:Tout + 1]) <= TOL


CONVT = [(2, 5, 7, 30, 4, 2, 1), (2, 4, 3, 25, 7, 3, 2), (1, 3, 6, 40, 16, 8, 4), (2, 4, 4, 31, 3, 1, 1), (2, 3, 5, 19, 8, 4, 2), (1, 4, 3, 11, 5, 3, 0)]


@pytest.mark.parametrize("shape", CONVT, ids=lambda s: "B%d-Cin%d-Cout%d-T%d-K%d-s%d-pad%d" % s)
def test_phased_launch_is_conv_transpose1d(shape):
    """a_mode 1, s 1, dj -1, os = phases = stride, oo = -pad: one phase per output residue; Q covers every residue's rows, so
    some (q, r) fall outside [0, Tout) at both ends and must not be written."""
    B, Cin, Cout, T, K, s, pad = shape
    rng = _rng(shape)
    x, w = _t(rng, B, Cin, T, 1), _t(rng, Cin, Cout, K)
    Tout = (T - 1) * s - 2 * pad + K
    Q = (Tout - 1 + pad) // s + 1
    g = C.geom(B, 1, Cin, Cout, T, Tout, 1, K, 1, -1, 0, s, -pad, s, Q, 1)
    prior = torch.full((B, Cout, Tout, 1), 7.0, dtype=torch.float64)
    y, _ = C.conv(g, x, w, prior)
    assert C.dist(y[..., 0], F.conv_transpose1d(x[..., 0], w, None, s, pad)) <= TOL
    rows = torch.arange(Q).view(-1, 1) * s - pad + torch.arange(s).view(1, -1)
    if pad > 0:
        assert bool((rows < 0).any())  # (the first residues of q = 0 lie above the tensor)


DGRAD = [(2, 5, 7, 40, 1, 3, 1, 1, 1), (2, 6, 4, 33, 1, 5, 2, 2, 1), (1, 3, 5, 50, 1, 4, 3, 1, 1), (2, 4, 6, 41, 1, 11, 1, 5, 5), (2, 5, 3, 17, 3, 5, 3, 2, 1),
         (3, 4, 4, 9, 13, 5, 1, 2, 1), (2, 4, 4, 21, 2, 5, 4, 2, 1)]


def _dgrad_geom(B, Cin, M, T, P, K, s, pad, dil, form):
    Tout = _out_len(T, K, s, pad, dil)
    if form == "flip":
        return C.geom(B, 1, M, Cin, Tout, T, P, K, 1, dil, pad - (K - 1) * dil, Q=T), 1
    if s == 1:
        return C.geom(B, 1, M, Cin, Tout, T, P, K, 1, -dil, pad, Q=T, a_mode=1), 0
    return C.geom(B, 1, M, Cin, Tout, T, P, K, 1, -1, 0, s, -pad, s, (T - 1 + pad) // s + 1, 1), 0


@pytest.mark.parametrize("shape", DGRAD, ids=lambda s: "B%d-C%d-M%d-T%d-P%d-K%d-s%d-pad%d-dil%d" % s)
def test_data_gradient_forms_are_autograd(shape):
    """a_mode 1 with dj = -dil (stride 1), the phased form (stride > 1), the flipped-weight form (stride 1), each with and
    without out_tf as the derivative of the activation in front of the conv (oaux = what that derivative is a function of)."""
    B, Cin, M, T, P, K, s, pad, dil = shape
    rng = _rng(shape)
    x0 = _t(rng, B, Cin, T, P).requires_grad_()
    w = _t(rng, M, Cin, K)
    dy = _t(rng, B, M, _out_len(T, K, s, pad, dil), P)
    prior = torch.zeros(B, Cin, T, P, dtype=torch.float64)
    sl = C.f32(0.1)
    for form in ("a_mode1",) + (("flip",) if s == 1 else ()):
        g, flip = _dgrad_geom(B, Cin, M, T, P, K, s, pad, dil, form)
        ref = torch.autograd.grad(_fconv(x0, w, s, pad, dil), x0, dy)[0]
        assert C.dist(C.conv(g, dy, w, prior, flip=flip)[0], ref) <= TOL, form
        for tf, fwd, aux_of in ((C.TF_DLEAKY, lambda t: F.leaky_relu(t, sl), "in"), (C.TF_DRELU, torch.relu, "out"), (C.TF_DTANH, torch.tanh, "out")):
            h = fwd(x0)
            ref = torch.autograd.grad(_fconv(h, w, s, pad, dil), x0, dy)[0]
            got = C.conv(g, dy, w, prior, flip=flip, out_tf=tf, oaux=(x0 if aux_of == "in" else h).detach(), slope=0.1)[0]
            assert C.dist(got, ref) <= TOL, (form, tf)


def test_input_transforms():
    """The six in_tf values: tf(x) is what a plain convolution of the transformed tensor sees; the derivative masks are the
    autograd derivatives of the activations whose OUTPUT (leaky: input or output, same sign) is xaux."""
    rng = _rng("in_tf")
    B, Cin, M, T, K = 2, 4, 3, 30, 3
    x, w, z = _t(rng, B, Cin, T, 1), _t(rng, M, Cin, K), _t(rng, B, Cin, T, 1).requires_grad_()
    g = C.geom(B, 1, Cin, M, T, T, 1, K, 1, 1, -1)
    prior = torch.zeros(B, M, T, 1, dtype=torch.float64)
    sl, clamp = C.f32(0.1), C.f32(0.5)
    assert C.dist(C.conv(g, x, w, prior, in_tf=C.TF_LEAKY, slope=0.1)[0], _fconv(F.leaky_relu(x, sl), w, 1, 1, 1)) <= TOL
    for tf, fwd, slope in ((C.TF_DLEAKY, lambda t: F.leaky_relu(t, sl), 0.1), (C.TF_DRELU, torch.relu, 0.1), (C.TF_DTANH, torch.tanh, 0.1),
                           (C.TF_DLOGCLAMP, lambda t: torch.log(torch.clamp(t + 1.0, min=clamp)), 0.5)):
        h = fwd(z)
        dact = torch.autograd.grad(h, z, x)[0]  # x * act'(z)
        got = C.conv(g, x, w, prior, in_tf=tf, xaux=h.detach(), slope=slope)[0]
        assert C.dist(got, _fconv(dact, w, 1, 1, 1)) <= TOL, tf
    with pytest.raises(ValueError):
        C.conv(g, x, w, prior, in_tf=6, xaux=x)


@pytest.mark.parametrize("act", [C.ACT_NONE, C.ACT_LEAKY, C.ACT_RELU, C.ACT_TANH, C.ACT_LOGCLAMP])
@pytest.mark.parametrize("out_tf", C.OUT_TFS)
def test_epilogue_order(act, out_tf):
    """v = alpha*acc + bias; act; dact(oaux); + res; * mask; + y -- composed by hand from torch operations; S is the sum of
    magnitudes of everything added; a float32 run of the same text is close and not identical."""
    rng = _rng(("epi", act, out_tf))
    B, Cin, M, T, P, K = 2, 5, 4, 21, 3, 3
    x, w = _t(rng, B, Cin, T, P), _t(rng, M, Cin, K)
    bias, res, prior, oaux = _t(rng, M), _t(rng, B, M, T, P), _t(rng, B, M, T, P), torch.tanh(_t(rng, B, M, T, P))
    mask = torch.from_numpy((rng.random((B, T)) > 0.3).astype(np.float64))
    g = C.geom(B, 1, Cin, M, T, T, P, K, 1, 1, -1)
    slope = 0.75 if act == C.ACT_LOGCLAMP else 0.1
    sl, al = C.f32(slope), C.f32(0.3)
    kw = dict(bias=bias, res=res, mask=mask, oaux=oaux, out_act=act, out_tf=out_tf, alpha=0.3, slope=slope)
    acc = _fconv(x, w, 1, 1, 1)
    v = al * acc + bias.view(1, M, 1, 1)
    v = [v, F.leaky_relu(v, sl), torch.relu(v), torch.tanh(v), torch.log(torch.clamp(v, min=sl))][act]
    v = v * {0: 1.0, 2: torch.where(oaux > 0, 1.0, sl), 3: (oaux > 0).double(), 4: 1 - oaux * oaux}[out_tf]
    v = (v + res) * mask.view(B, 1, T, 1)
    Sref = abs(al) * _fconv(x.abs(), w.abs(), 1, 1, 1) + bias.abs().view(1, M, 1, 1) + res.abs()
    for accumulate in (False, True):
        y, S = C.conv(g, x, w, prior, accumulate=accumulate, **kw)
        assert C.dist(y, v + prior if accumulate else v) <= TOL
        assert C.dist(S, Sref + prior.abs() if accumulate else Sref) <= TOL
        masked = (mask == 0).view(B, 1, T, 1).expand_as(y)
        assert torch.equal(y[masked], prior[masked] if accumulate else torch.zeros_like(y[masked]))
    y32, _ = C.conv(g, x.float(), w.float(), prior.float(), bias=bias.float(), res=res.float(), mask=mask.float(), oaux=oaux.float(),
                    out_act=act, out_tf=out_tf, alpha=0.3, slope=slope, dtype=torch.float32)
    y64, _ = C.conv(g, x.float(), w.float(), prior.float(), bias=bias.float(), res=res.float(), mask=mask.float(), oaux=oaux.float(),
                    out_act=act, out_tf=out_tf, alpha=0.3, slope=slope)
    assert y32.dtype == torch.float32 and 0 < C.dist(y32, y64) < 1e-5
    for bad in (C.TF_LEAKY, C.TF_DLOGCLAMP, 6, -1):
        with pytest.raises(ValueError):
            C.conv(g, x, w, prior, out_tf=bad, oaux=oaux)


def test_rounded_operands_and_gamma():
    rng = _rng("rounded")
    B, Cin, M, T, K = 2, 6, 4, 25, 3
    x, w = _t(rng, B, Cin, T, 1).float(), _t(rng, M, Cin, K).float()
    g = C.geom(B, 1, Cin, M, T, T, 1, K, 1, 1, -1)
    prior = torch.zeros(B, M, T, 1)
    rb = lambda t: t.bfloat16().double()
    xl = torch.maximum(x, x * torch.tensor(0.1, dtype=torch.float32))
    got = C.conv(g, x, w, prior, in_tf=C.TF_LEAKY, slope=0.1, rounded=True)[0]
    assert torch.equal(got, _fconv(rb(xl), rb(w), 1, 1, 1))
    assert C.gamma(100) == pytest.approx(100 * 2.0 ** -24, rel=1e-4) and C.gamma(1) > 2.0 ** -24


THIN_DGRAD = [(2, 1, 5, 40, 1, 5, 3, 2, 2), (2, 1, 33, 23, 3, 15, 2, 7, 2), (1, 1, 16, 50, 1, 16, 3, 0, 1), (2, 3, 4, 31, 2, 4, 2, 3, 3),
              (2, 1, 7, 29, 1, 1, 3, 0, 2), (2, 1, 6, 30, 1, 5, 1, 2, 2)]


@pytest.mark.parametrize("shape", THIN_DGRAD, ids=lambda s: "B%d-C%d-M%d-T%d-P%d-K%d-s%d-pad%d-dil%d" % s)
def test_strided_dilated_data_gradient_is_autograd(shape):
    """conv_f64.dgrad (stride and dilation together: vcv_conv_c1_dgrad takes both) is the float64 autograd data gradient, its S
    the same gradient of the magnitudes; rows of x past the last one a tap reaches come back as exact zeros with S = 0; and
    where one VcvConvArgs launch expresses the gradient (stride 1, or dilation 1) conv() gives the same numbers."""
    B, Cin, M, T, P, K, s, pad, dil = shape
    rng = _rng(shape)
    Tout = _out_len(T, K, s, pad, dil)
    last = (Tout - 1) * s + (K - 1) * dil - pad  # the last row of x a tap reaches
    T = max(T, last + 1) + 4  # (four rows no output touches)
    x0 = _t(rng, B, Cin, T, P).requires_grad_()
    w = _t(rng, M, Cin, K)
    dy = _t(rng, B, M, Tout, P)
    y = _fconv(x0, w, s, pad, dil)[:, :, :Tout]
    ref = torch.autograd.grad(y, x0, dy)[0]
    got, S = C.dgrad(dy, w, T, s, dil, pad)
    assert C.dist(got, ref) <= TOL
    xa = x0.detach().clone().requires_grad_()
    Sref = torch.autograd.grad(_fconv(xa, w.abs(), s, pad, dil)[:, :, :Tout], xa, dy.abs())[0]
    assert C.dist(S, Sref) <= TOL
    assert last < T - 1 and not bool(got[:, :, last + 1:].any()) and not bool(S[:, :, last + 1:].any())
    prior = torch.zeros(B, Cin, T, P, dtype=torch.float64)
    if s == 1:
        g = C.geom(B, 1, M, Cin, Tout, T, P, K, 1, -dil, pad, Q=T, a_mode=1)
        assert C.dist(C.conv(g, dy, w, prior)[0], got) <= TOL
    elif dil == 1:
        g = C.geom(B, 1, M, Cin, Tout, T, P, K, 1, -1, 0, s, -pad, s, (T - 1 + pad) // s + 1, 1)
        assert C.dist(C.conv(g, dy, w, prior)[0], got) <= TOL


@pytest.mark.parametrize("K", [4, 5])
def test_single_channel_taps_reversed_and_masked(K):
    """The forms vcv_conv_c1_fwd_flip runs: Cg = 1 with flip = 1 is the convolution with every weight row read backwards
    (A(m, 0, k) = w[m, K-1-k]; [1, M, K] and [M, 1, K] are the same memory), and with pad' = (K-1)*dil - pad that is the
    autograd data gradient of a one-OUTPUT-channel conv; out_tf DLEAKY on top is the derivative of the leaky-ReLU in front."""
    rng = _rng(("c1flip", K))
    B, M, T, P, dil, pad = 2, 6, 21, 2, 2, 3
    w = _t(rng, 1, M, K)  # the forward conv's weight [1, C = M, K]
    x0 = _t(rng, B, M, T, P).requires_grad_()
    Tout = _out_len(T, K, 1, pad, dil)
    dy = _t(rng, B, 1, Tout, P)
    prior = torch.zeros(B, M, T, P, dtype=torch.float64)
    g = C.geom(B, 1, 1, M, Tout, T, P, K, 1, dil, pad - (K - 1) * dil)
    got = C.conv(g, dy, w, prior, flip=1)[0]
    assert C.dist(got, torch.autograd.grad(_fconv(x0, w, 1, pad, dil), x0, dy)[0]) <= TOL
    assert C.dist(got, _fconv(dy, w.flip(2).reshape(M, 1, K), 1, (K - 1) * dil - pad, dil)) <= TOL
    sl = C.f32(0.1)
    ref = torch.autograd.grad(_fconv(F.leaky_relu(x0, sl), w, 1, pad, dil), x0, dy)[0]
    assert C.dist(C.conv(g, dy, w, prior, flip=1, out_tf=C.TF_DLEAKY, oaux=x0.detach(), slope=0.1)[0], ref) <= TOL


def test_one_output_channel_with_more_or_fewer_rows_than_the_formula():
    """vcv_conv_m1_fwd is handed Tout: fewer rows than Tin + 2*pad - dil*(K-1) are the first rows of the convolution, more read
    zeros past the input (the bias and the activation still apply)."""
    rng = _rng("m1rows")
    B, Cin, T, P, K, pad = 2, 17, 30, 2, 3, 1
    x, w, bias = _t(rng, B, Cin, T, P), _t(rng, 1, Cin, K), _t(rng, 1)
    full = torch.tanh(_fconv(F.pad(F.leaky_relu(x, C.f32(0.1)), (0, 0, 0, 2)), w, 1, pad, 1) + bias.view(1, 1, 1, 1))
    for Tout in (T - 3, T + 2):
        g = C.geom(B, 1, Cin, 1, T, Tout, P, K, 1, 1, -pad)
        y, _ = C.conv(g, x, w, torch.zeros(B, 1, Tout, P, dtype=torch.float64), bias=bias, in_tf=C.TF_LEAKY, out_act=C.ACT_TANH, slope=0.1)
        assert C.dist(y, full[:, :, :Tout]) <= TOL

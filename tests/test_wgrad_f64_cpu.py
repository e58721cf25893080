"""tests/wgrad_f64.py's operand transforms (the ones vcv_thin_wgrad takes and the MFMA weight gradient refuses) pinned to torch
autograd in float64: each derivative transform is the derivative of the activation whose output (leaky-ReLU: input or output,
same sign) is the aux tensor.  The plain formula is pinned in tests/test_wgrad_mfma_abi_gpu.py.  No GPU, no library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_f64 as W

TOL = 1e-12


def _t(rng, *sh):
    return torch.from_numpy(rng.standard_normal(sh))


def _acts(sl, clamp):
    return {W.TF_DLEAKY: (lambda t: F.leaky_relu(t, sl), 0.1), W.TF_DRELU: (torch.relu, 0.1), W.TF_DTANH: (torch.tanh, 0.1),
            W.TF_DLOGCLAMP: (lambda t: torch.log(torch.clamp(t + 1.0, min=clamp)), 0.5)}


@pytest.mark.parametrize("tf", [W.TF_DLEAKY, W.TF_DRELU, W.TF_DTANH, W.TF_DLOGCLAMP])
@pytest.mark.parametrize("side", ["a", "b"])
def test_derivative_transforms_are_autograd(tf, side):
    """tf on `a` (the gradient that flows back into an activation BEHIND the conv) and on `b` (the chain rule through an
    activation in FRONT of a conv whose roles are swapped): tf(v) = v * act'(z), aux = act(z)."""
    rng = np.random.default_rng(17 * tf + (side == "b"))
    B, M, Cin, Ta, P, K, s, dil, pad = 2, 3, 4, 19, 2, 3, 2, 2, 1
    Tb = (Ta - 1) * s + dil * (K - 1) + 1 - 2 * pad
    a, b = _t(rng, B, M, Ta, P), _t(rng, B, Cin, Tb, P)
    sl32, cl32 = float(np.float32(0.1)), float(np.float32(0.5))
    fwd, slope = _acts(sl32, cl32)[tf]
    v = a if side == "a" else b
    z = _t(rng, *v.shape).requires_grad_()
    h = fwd(z)
    tv = torch.autograd.grad(h, z, v)[0]  # v * act'(z)
    kw = dict(a_tf=tf, aaux=h.detach()) if side == "a" else dict(b_tf=tf, baux=h.detach())
    got = W.wgrad(a, b, K, s, dil, -pad, slope=slope, **kw)
    ref = W.wgrad(tv, b, K, s, dil, -pad) if side == "a" else W.wgrad(a, tv, K, s, dil, -pad)
    assert W.dist(got, ref) <= TOL
    mag = W.wgrad_mag(a, b, K, s, dil, -pad, slope=slope, **kw)
    ref = W.wgrad(tv.abs(), b.abs(), K, s, dil, -pad) if side == "a" else W.wgrad(a.abs(), tv.abs(), K, s, dil, -pad)
    assert W.dist(mag, ref) <= TOL and bool((mag >= got.abs() - 1e-12).all())


def test_transformed_weight_gradient_is_the_conv_weight_gradient():
    """End to end on the role ops.conv_wgrad builds for a discriminator layer: y = conv(leaky(x)), the loss reads tanh(y):
    a = dL/dtanh with DTANH of aux = tanh(y), b = x with LEAKY."""
    rng = np.random.default_rng(3)
    B, Cin, T, P, K, s, pad = 2, 5, 23, 3, 5, 3, 2
    sl = float(np.float32(0.1))
    x = _t(rng, B, Cin, T, P)
    w = _t(rng, 1, Cin, K, 1).requires_grad_()
    y = F.conv2d(F.leaky_relu(x, sl), w, None, (s, 1), (pad, 0))
    out = torch.tanh(y)
    g = _t(rng, *out.shape)
    ref = torch.autograd.grad(out, w, g)[0][..., 0]
    got = W.wgrad(g, x, K, s, 1, -pad, a_tf=W.TF_DTANH, aaux=out.detach(), b_tf=W.TF_LEAKY, slope=0.1)
    assert W.dist(got, ref) <= TOL


def test_derivative_transform_needs_its_aux():
    a, b = torch.zeros(1, 1, 4, 1), torch.zeros(1, 1, 4, 1)
    with pytest.raises(AttributeError):
        W.wgrad(a, b, 1, 1, 1, 0, a_tf=W.TF_DLEAKY)
    with pytest.raises(ValueError):
        W.wgrad(a, b, 1, 1, 1, 0, a_tf=6, aaux=a)

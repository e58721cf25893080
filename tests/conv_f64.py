"""Restatement of the conv family's forward formula and fused epilogue at the C ABI (test oracle only).

The formula of include/vcvits_hip.h (VcvConvArgs), by explicit index gather -- no torch.nn.functional.conv*:

    y[b, g*Mg + m, q*os + oo (+ r), p] = epilogue(alpha * sum_{c < Cg, j < J} A(m, c, kw0 + j*kws) *
                                                          tf(x[b, g*Cg + c, q*s + j*dj + off, p]))

with rows of x outside [0, Tin) read as zero and rows of y outside [0, Tout) not written;
    phases <= 1: J = K, kw0 = 0, kws = 1;   phases > 1: residue r < phases uses the taps kw = r + j*phases (< K);
    a_mode 0: A(m, c, k) = w[(g*Mg + m), c, k];   a_mode 1: A(m, c, k) = w[(g*Cg + c), m, k];
    flip (the packed families' stride-1 data gradient of a conv with weight w [Cg, Mg, K]): A(m, c, k) = w[c, m, K-1-k];
    epilogue: v = alpha*acc + bias[m]; v = act(v); v *= dact(oaux) (out_tf); v += res; v *= mask[b, row];
              if (accumulate) v += y; y = v.

conv() takes the preloaded y and returns the whole expected y (an element the contract does not write keeps its value)
in the dtype it is asked for, so the same text is the float64 yardstick and the float32 reference computation, and S, the
float64 sum of magnitudes behind every element, |alpha| * sum |A| |tf(x)| + |bias| + |res| + |y prior| (the prior only where
it is accumulated onto; 0 where nothing is written), which scales the element-wise rounding bound of the tests.
rounded=True rounds A and tf(x) to bf16 (the leaky-ReLU formed in float32 as the kernel forms it: fmaxf(f, f * slope))
before the sum, as vcv_conv_bf16_* does; the epilogue operands stay as they are.

Shares no code with vcvits_amd."""
import collections
import math

import torch

ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_TANH, ACT_LOGCLAMP = 0, 1, 2, 3, 4  # include/vcvits_hip.h
TF_NONE, TF_LEAKY, TF_DLEAKY, TF_DRELU, TF_DTANH, TF_DLOGCLAMP = 0, 1, 2, 3, 4, 5
OUT_TFS = (TF_NONE, TF_DLEAKY, TF_DRELU, TF_DTANH)  # the out_tf values of the contract

Geom = collections.namedtuple("Geom", "B G Cg Mg Tin Tout P K s dj off os oo phases Q a_mode", defaults=(1, 0, 1, None, 0))


def geom(B, G, Cg, Mg, Tin, Tout, P, K, s, dj, off, os=1, oo=0, phases=1, Q=None, a_mode=0):
    return Geom(B, G, Cg, Mg, Tin, Tout, P, K, s, dj, off, os, oo, phases, Tout if Q is None else Q, a_mode)


def f32(v):
    """the float32 NUMBER the library is handed for a float argument (0.1 is not a float32)"""
    return float(torch.tensor(v, dtype=torch.float32))


def bf16_round(t):
    return t.float().bfloat16().float()


def in_transform(x, tf, xaux, slope, rounded, dtype):
    """tf(x) as the kernel's MFMA sees it."""
    x = x.detach().cpu()
    sl = f32(slope)
    if rounded:
        assert tf in (TF_NONE, TF_LEAKY)
        x = x.float()
        if tf == TF_LEAKY:
            x = torch.maximum(x, x * torch.tensor(slope, dtype=torch.float32))
        return bf16_round(x).to(dtype)
    x = x.to(dtype)
    if tf == TF_NONE:
        return x
    if tf == TF_LEAKY:
        return torch.where(x > 0, x, x * sl)
    a = xaux.detach().cpu().to(dtype)
    if tf == TF_DLEAKY:
        return x * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, sl))
    if tf == TF_DRELU:
        return torch.where(a > 0, x, torch.zeros_like(x))
    if tf == TF_DTANH:
        return x * (1 - a * a)
    if tf == TF_DLOGCLAMP:
        return torch.where(a > math.log(sl), x * torch.exp(-a), torch.zeros_like(x))
    raise ValueError("in_tf %r" % (tf,))


def activation(v, act, slope):
    sl = f32(slope)
    if act == ACT_NONE:
        return v
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * sl)
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_LOGCLAMP:
        return torch.log(torch.clamp(v, min=sl))
    raise ValueError("out_act %r" % (act,))


def out_transform(v, tf, a, slope):
    if tf == TF_NONE:
        return v
    if tf == TF_DLEAKY:
        return v * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, f32(slope)))
    if tf == TF_DRELU:
        return torch.where(a > 0, v, torch.zeros_like(v))
    if tf == TF_DTANH:
        return v * (1 - a * a)
    raise ValueError("out_tf %r is outside the contract" % (tf,))


def weights(w, g, flip, rounded, dtype):
    """A as [G, Mg, Cg, K] in `dtype`."""
    w = w.detach().cpu()
    w = bf16_round(w) if rounded else w
    w = w.to(dtype)
    if flip:
        assert g.G == 1 and g.a_mode == 0
        return w.reshape(g.Cg, g.Mg, g.K).permute(1, 0, 2).flip(2).unsqueeze(0)
    if g.a_mode == 0:
        return w.reshape(g.G, g.Mg, g.Cg, g.K)
    return w.reshape(g.G, g.Cg, g.Mg, g.K).permute(0, 2, 1, 3)


def conv(g, x, w, y_prior, *, flip=0, bias=None, res=None, mask=None, xaux=None, oaux=None, in_tf=TF_NONE, out_act=ACT_NONE,
         out_tf=TF_NONE, accumulate=False, alpha=1.0, slope=0.1, rounded=False, dtype=torch.float64):
    """x [B, G*Cg, Tin, P], w as a_mode / flip say, y_prior [B, G*Mg, Tout, P] -> (y [B, G*Mg, Tout, P] in `dtype`, S float64)."""
    B, G, Cg, Mg, P, Q = g.B, g.G, g.Cg, g.Mg, g.P, g.Q
    assert tuple(x.shape) == (B, G * Cg, g.Tin, P) and tuple(y_prior.shape) == (B, G * Mg, g.Tout, P)
    tx = in_transform(x, in_tf, xaux, slope, rounded, dtype).reshape(B, G, Cg, g.Tin, P)
    A = weights(w, g, flip, rounded, dtype)
    y = y_prior.detach().cpu().to(dtype).clone().reshape(B, G, Mg, g.Tout, P)
    S = torch.zeros(B, G, Mg, g.Tout, P, dtype=torch.float64)
    cpu = lambda t: None if t is None else t.detach().cpu().to(dtype)
    like_y = lambda t: None if t is None else cpu(t).reshape(B, G, Mg, g.Tout, P)
    bias_, res_, oaux_, mask_ = cpu(bias), like_y(res), like_y(oaux), cpu(mask)
    al = f32(alpha)
    q = torch.arange(Q)
    nph = g.phases if g.phases > 1 else 1
    for r in range(nph):
        kw0, kws = (r, nph) if nph > 1 else (0, 1)
        J = (max(0, g.K - r) + nph - 1) // nph if nph > 1 else g.K
        acc = torch.zeros(B, G, Mg, Q, P, dtype=dtype)
        mag = torch.zeros(B, G, Mg, Q, P, dtype=torch.float64)
        for j in range(J):
            rows = q * g.s + j * g.dj + g.off
            ok = (rows >= 0) & (rows < g.Tin)
            if not bool(ok.any()):
                continue
            xk = tx[:, :, :, rows.clamp(0, g.Tin - 1), :] * ok.to(dtype).view(1, 1, 1, Q, 1)  # [B, G, Cg, Q, P]
            Ak = A[:, :, :, kw0 + j * kws]  # [G, Mg, Cg]
            acc += torch.einsum("gmc,bgcqp->bgmqp", Ak, xk)
            mag += torch.einsum("gmc,bgcqp->bgmqp", Ak.double().abs(), xk.double().abs())
        trow = q * g.os + g.oo + r
        keep = (trow >= 0) & (trow < g.Tout)
        if not bool(keep.any()):
            continue
        qi, ti = q[keep], trow[keep]
        v = al * acc[:, :, :, qi, :]
        s_ = abs(al) * mag[:, :, :, qi, :]
        if bias_ is not None:
            v = v + bias_.view(1, G, Mg, 1, 1)
            s_ = s_ + bias_.double().abs().view(1, G, Mg, 1, 1)
        v = activation(v, out_act, slope)
        if out_tf != TF_NONE:
            v = out_transform(v, out_tf, oaux_[:, :, :, ti, :], slope)
        if res_ is not None:
            v = v + res_[:, :, :, ti, :]
            s_ = s_ + res_[:, :, :, ti, :].double().abs()
        if mask_ is not None:
            v = v * mask_[:, ti].view(B, 1, 1, -1, 1)
        if accumulate:
            v = v + y[:, :, :, ti, :]
            s_ = s_ + y[:, :, :, ti, :].double().abs()
        y[:, :, :, ti, :] = v
        S[:, :, :, ti, :] = s_
    return y.reshape(B, G * Mg, g.Tout, P), S.reshape(B, G * Mg, g.Tout, P)


def dgrad(dy, w, Tin, s, dil, pad, dtype=torch.float64):
    """The data gradient of a conv with ANY stride and dilation together, which no single VcvConvArgs launch expresses (the
    a_mode-1 form wants stride 1, the phased form dilation 1): dy [B, M, Tout, P], w [M, C, K] ->
        dx[b, c, t, p] = sum_{m, k, q: q*s + k*dil - pad == t} w[m, c, k] * dy[b, m, q, p]     (dx [B, C, Tin, P] in `dtype`),
    and S, the float64 sum of magnitudes behind every element (0 on a row no tap reaches).  By explicit scatter."""
    dy_ = dy.detach().cpu().to(dtype)
    w_ = w.detach().cpu().to(dtype)
    B, M, Tout, P = dy_.shape
    Cin, K = w_.shape[1], w_.shape[2]
    dx = torch.zeros(B, Cin, Tin, P, dtype=dtype)
    S = torch.zeros(B, Cin, Tin, P, dtype=torch.float64)
    q = torch.arange(Tout)
    for k in range(K):
        t = q * s + k * dil - pad
        ok = (t >= 0) & (t < Tin)
        if not bool(ok.any()):
            continue
        dx[:, :, t[ok], :] += torch.einsum("mc,bmqp->bcqp", w_[:, :, k], dy_[:, :, q[ok], :])
        S[:, :, t[ok], :] += torch.einsum("mc,bmqp->bcqp", w_[:, :, k].double().abs(), dy_[:, :, q[ok], :].double().abs())
    return dx, S


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-24: the relative bound on an fp32 sum of n terms in any order (Higham, Accuracy and
    Stability of Numerical Algorithms, section 3.1)."""
    u = 2.0 ** -24
    return n * u / (1 - n * u)


def dist(got, ref):
    """max|got - ref| / max|ref|"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)

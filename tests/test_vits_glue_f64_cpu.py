"""The references of tests/vits_glue_f64.py, pinned on the CPU (no GPU, no library): every hand-written gradient against torch
autograd in float64 on the model's own formulas (modules.py:147-175, posterior_encoder.py:36-38, modules.py:317-336,
losses.py:40-55, modules.py:19-31), the float32 nearest index map against F.interpolate, slicing against a Python loop, and the
case table of tests/test_vits_glue_abi_gpu.py: its "float32 map" pairs really need float32, its exact pass really is exact."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import test_vits_glue_abi_gpu as G
import vits_glue_f64 as V

B, H, T = 3, 5, 37


def rnd(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape))


def holes(seed, b=B, t=T):
    m = torch.from_numpy(np.random.default_rng(seed).choice([0.0, 0.5, 1.0], (b, t)))
    m[:, 1] = 0.0
    return m


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * (1 + b.abs().max().item()), (a - b).abs().max().item()


def test_wn_gate():
    for g_w, goff in ((None, 0), (2 * H, 0), (6 * H, 2 * H), (6 * H, 4 * H)):
        xin, dacts = rnd(1, B, 2 * H, T).requires_grad_(True), rnd(2, B, H, T)
        g = rnd(3, B, g_w, 1).requires_grad_(True) if g_w else None
        pre = xin if g is None else xin + g[:, goff:goff + 2 * H]
        a, b = torch.chunk(pre, 2, 1)  # commons.py:99-106
        acts = torch.tanh(a) * torch.sigmoid(b)
        close(V.wn_gate(xin.detach(), None if g is None else g.detach()[..., 0], goff), acts.detach())
        acts.backward(dacts)
        dxin = V.wn_gate_bwd(xin.detach(), None if g is None else g.detach()[..., 0], goff, dacts)
        close(dxin, xin.grad)
        if g is not None:  # the conditioning gradient: the row sums of dxin, in this layer's slice, as _WnGateFn.backward asks for them
            dg = V.row_sum(dxin, B * 2 * H, T, 2 * H, g_w, goff, torch.zeros(B, g_w))
            close(dg, g.grad[..., 0])


def test_row_sum_keeps_the_other_words():
    x, prior = rnd(4, 30, 7), rnd(5, 3, 30)
    out = V.row_sum(x, 30, 7, 10, 30, 10, prior)
    assert torch.equal(out[:, :10], prior[:, :10]) and torch.equal(out[:, 20:], prior[:, 20:])
    close(out[:, 10:20], x.sum(1).view(3, 10))
    assert V.row_sum(x.float(), 30, 7, 10, 30, 10, prior.float(), torch.float32).dtype == torch.float32


def test_wn_res_skip():
    mask = holes(6)
    for last in (0, 1):
        for with_out in (0, 1):
            x, rs = rnd(7, B, H, T).requires_grad_(True), rnd(8, B, H if last else 2 * H, T).requires_grad_(True)
            out = rnd(9, B, H, T).requires_grad_(True) if with_out else None
            o0 = out if with_out else torch.zeros(B, H, T, dtype=torch.float64)
            if last:  # modules.py:168-174
                want_x, want_o = None, o0 + rs
            else:
                want_x, want_o = (x + rs[:, :H]) * mask.unsqueeze(1), o0 + rs[:, H:]
            xn, on = V.wn_res_skip(x.detach(), out.detach() if with_out else None, rs.detach(), mask, last)
            close(on, want_o.detach())
            assert (xn is None) == bool(last)
            if last:
                continue
            close(xn, want_x.detach())
            for dxn, don in ((rnd(10, B, H, T), None), (None, rnd(11, B, H, T)), (rnd(10, B, H, T), rnd(11, B, H, T))):
                for v in (x, rs):
                    v.grad = None
                z = torch.zeros(B, H, T, dtype=torch.float64)
                torch.autograd.backward((want_x, want_o), (z if dxn is None else dxn, z if don is None else don), retain_graph=True)
                drs, dx = V.wn_res_skip_bwd(dxn, don, mask, (B, H, T))
                close(drs, rs.grad)
                close(dx, x.grad)


def test_split_sample():
    mask = holes(12)
    mk = mask.unsqueeze(1)
    for with_eps in (0, 1):
        stats = (0.3 * rnd(13, B, 2 * H, T)).requires_grad_(True)
        eps = rnd(14, B, H, T) if with_eps else None
        m, logs = torch.split(stats * mk, H, dim=1)  # posterior_encoder.py:36-38
        z = (m + eps * torch.exp(logs)) * mk if with_eps else None
        gm, gl, gz = V.split_sample(stats.detach(), eps, mask)
        close(gm, m.detach())
        close(gl, logs.detach())
        assert (gz is None) == (not with_eps)
        if with_eps:
            close(gz, z.detach())
        for dm, dl, dz in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)):
            stats.grad = None
            d = [rnd(15 + i, B, H, T) if on else None for i, on in enumerate((dm, dl, dz))]
            outs = [(m, d[0]), (logs, d[1])] + ([(z, d[2])] if with_eps else [])
            outs = [(o, g) for o, g in outs if g is not None]
            torch.autograd.backward([o for o, _ in outs], [g for _, g in outs], retain_graph=True)
            close(V.split_sample_bwd(d[0], d[1], d[2], eps, logs.detach(), mask, (B, H, T)), stats.grad)  # (dz is ignored without eps)


def test_coupling_and_round_trip():
    mask = holes(18)
    for reverse in (0, 1):
        x1, m, dy = rnd(19, B, H, T).requires_grad_(True), rnd(20, B, H, T).requires_grad_(True), rnd(21, B, H, T)
        mk = mask.unsqueeze(1)
        want = (x1 - m) * mk if reverse else m + x1 * mk  # modules.py:327-336
        close(V.coupling(x1.detach(), m.detach(), mask, reverse), want.detach())
        want.backward(dy)
        a, b = x1.detach().clone().requires_grad_(True), m.detach().clone().requires_grad_(True)
        V.coupling(a, b, mask, reverse).backward(dy)
        close(a.grad, x1.grad)
        close(b.grad, m.grad)
    x1, m = rnd(19, B, H, T), rnd(20, B, H, T)
    close(V.coupling(V.coupling(x1, m, mask, 0), m, mask, 1), x1 * mask.unsqueeze(1) ** 2)


def test_prior_sample():
    m, logs, noise = rnd(22, B, H, T), 0.3 * rnd(23, B, H, T), rnd(24, B, H, T)
    close(V.prior_sample(m, logs, noise, 0.667), m + noise * torch.exp(logs) * 0.667)  # synthesizer_svc.py:104


def test_kl():
    mask = holes(25)
    mask[-1] = 0.0
    leaves = [rnd(26, B, H, T), rnd(27, B, H, T), rnd(28, B, H, T), 0.3 * rnd(29, B, H, T)]
    zp, lq, mp, lp = (v.requires_grad_(True) for v in leaves)
    kl = lp - lq - 0.5 + 0.5 * ((zp - mp) ** 2) * torch.exp(-2.0 * lp)  # losses.py:40-55
    mk = mask.unsqueeze(1)
    loss = torch.sum(kl * mk) / torch.sum(mk)
    num, den = V.kl(zp.detach(), lq.detach(), mp.detach(), lp.detach(), mask)
    close(num / den, loss.detach())
    assert den.item() == mask.sum().item()
    gout = torch.tensor(0.37, dtype=torch.float64)
    loss.backward(gout)
    got = V.kl_bwd(zp.detach(), mp.detach(), lp.detach(), mask, gout, den)
    for g, leaf in zip(got, (zp, lq, mp, lp)):
        close(g, leaf.grad)


def test_layernorm_c():
    for C, with_y in ((1, 1), (2, 0), (5, 1), (33, 0)):
        x, ga, be, dout = rnd(30, B, C, T).requires_grad_(True), rnd(31, C).requires_grad_(True), rnd(32, C).requires_grad_(True), rnd(33, B, C, T)
        y = rnd(34, B, C, T).requires_grad_(True) if with_y else None
        v = x + y if with_y else x
        want = F.layer_norm(v.transpose(1, -1), (C,), ga, be, 1e-5).transpose(1, -1)  # modules.py:19-31
        out, mean, rstd = V.layernorm_c(x.detach(), y.detach() if with_y else None, ga.detach(), be.detach(), 1e-5)
        close(out, want.detach(), 1e-10)
        close(mean, v.detach().mean(1))
        close(rstd, 1.0 / torch.sqrt(v.detach().var(1, unbiased=False) + 1e-5), 1e-10)
        want.backward(dout)
        dx, dgamma, dbeta = V.layernorm_c_bwd(x.detach(), y.detach() if with_y else None, ga.detach(), dout, 1e-5)
        close(dx, x.grad, 1e-9)
        close(dgamma, ga.grad, 1e-10)
        close(dbeta, be.grad)
        if with_y:
            close(dx, y.grad, 1e-9)


def interp(Tin, Tout):
    return F.interpolate(torch.arange(Tin, dtype=torch.float32).view(1, 1, Tin), size=Tout, mode="nearest").view(-1).long()


def nearest_pairs():
    """every (Tin, Tout) whose index map the GPU table computes, the raw sizes included"""
    pairs = set()
    for c in G.TABLE:
        if c.entry in ("nearest_fwd", "nearest_bwd"):
            pairs.add((c.p["Tin"], c.p["Tout"]))
        if c.entry in ("raw_fwd", "raw_bwd"):
            tir = c.p["raw"][0] if c.p["raw"][0] > 0 else c.p["Tin"]
            if c.p["raw"][1] > 0 and tir <= c.p["Tin"]:
                pairs.add((tir, c.p["raw"][1]))
    return sorted(pairs)


def test_nearest_index_is_torchs():
    """for every pair the GPU table uses, and for every Tin < 260, Tout < 700"""
    assert len(nearest_pairs()) >= 10
    for Tin, Tout in nearest_pairs():
        assert torch.equal(V.nearest_index(Tin, Tout), interp(Tin, Tout)), (Tin, Tout)
    differ = 0
    for Tin in range(1, 260):
        x = torch.arange(Tin, dtype=torch.float32).view(1, 1, Tin)
        for Tout in range(1, 700):
            idx = V.nearest_index(Tin, Tout)
            assert torch.equal(idx, F.interpolate(x, size=Tout, mode="nearest").view(-1).long()), (Tin, Tout)
            differ += int(not torch.equal(idx, torch.arange(Tout) * Tin // Tout))
    assert differ == 4300  # the pairs at which an index map in integer or double arithmetic would move a frame


def test_nearest_table_pairs_need_the_float32_map():
    """Every pair of the GPU table marked "float32 map" differs from the exact rational map to * Tin // Tout (and from the same
    formula in double), so a kernel that computed the index in integer or double arithmetic fails on it."""
    marked = [c for c in G.TABLE if c.p.get("f32map")]
    assert {c.entry for c in marked} == {"nearest_fwd", "nearest_bwd", "raw_fwd", "raw_bwd"}
    for c in marked:
        Tin, Tout = c.p["raw"] if "raw" in c.p else (c.p["Tin"], c.p["Tout"])
        idx = V.nearest_index(Tin, Tout)
        to = torch.arange(Tout)
        assert not torch.equal(idx, to * Tin // Tout), c.name
        assert not torch.equal(idx, torch.floor(to.double() * (Tin / Tout)).long().clamp(max=Tin - 1)), c.name
        # ... and on the data of the case: the two maps read different frames of x / add dy into different frames of dx
        t = G.inputs("%s-%s" % (c.entry, c.name), "exact")
        src = t["x"] if "x" in t else t["dy"]
        assert src.shape[-1] == (c.p["Tin"] if "x" in t else c.p["Tout"])
    for c in G.TABLE:
        if c.entry in ("nearest_fwd", "nearest_bwd") and not c.p["f32map"]:
            assert torch.equal(V.nearest_index(c.p["Tin"], c.p["Tout"]), torch.arange(c.p["Tout"]) * c.p["Tin"] // c.p["Tout"]), c.name


def test_nearest_and_raw():
    x = rnd(35, 3, 40)
    close(V.nearest(x, 100), F.interpolate(x.unsqueeze(0), size=100, mode="nearest")[0])
    dy = rnd(36, 3, 100)
    a = x.clone().requires_grad_(True)
    F.interpolate(a.unsqueeze(0), size=100, mode="nearest")[0].backward(dy)
    close(V.nearest_bwd(dy, 40), a.grad)
    # raw sizes: the map of (33, 82) on the first 33 / 82 frames, zeros beyond; (0, .) reads Tin itself
    y = V.nearest_raw(x, 100, (33, 82))
    close(y[:, :82], F.interpolate(x[:, :33].unsqueeze(0), size=82, mode="nearest")[0])
    assert bool((y[:, 82:] == 0).all())
    dx = V.nearest_raw_bwd(dy, 40, (33, 82))
    a = x.clone().requires_grad_(True)
    F.interpolate(a[:, :33].unsqueeze(0), size=82, mode="nearest")[0].backward(dy[:, :82])
    close(dx, a.grad)
    assert bool((dx[:, 33:] == 0).all())
    close(V.nearest_raw(x, 100, (0, 100)), V.nearest(x, 100))
    close(V.nearest_raw(x, 100, (-3, 100)), V.nearest(x, 100))
    assert bool((V.nearest_raw(x, 100, (33, 0)) == 0).all()) and bool((V.nearest_raw(x, 100, (41, 100)) == 0).all())
    assert bool((V.nearest_raw_bwd(dy, 40, (33, 0)) == 0).all()) and bool((V.nearest_raw_bwd(dy, 40, (41, 100)) == 0).all())


def test_slice():
    for p in G.SLICES:
        Bn, Cn, Tn, S, mul, ids = p["B"], p["H"], p["T"], p["S"], p["mul"], torch.tensor(p["ids"])
        x, dy = rnd(37, Bn, Cn, Tn), rnd(38, Bn, Cn, S)
        want, dx = torch.zeros(Bn, Cn, S, dtype=torch.float64), torch.zeros(Bn, Cn, Tn, dtype=torch.float64)
        for b in range(Bn):  # commons.py:48-54: x[b, :, i : i + S], zero padded
            for s in range(S):
                t = int(ids[b]) * mul + s
                if 0 <= t < Tn:
                    want[b, :, s] = x[b, :, t]
                    dx[b, :, t] = dy[b, :, s]
        assert torch.equal(V.slice(x, ids, mul, S), want)
        assert torch.equal(V.slice_bwd(dy, ids, mul, Tn), dx)
    x = rnd(37, 2, 3, 40)
    assert torch.equal(V.slice(x, torch.tensor([3, 36]), 1, 4), torch.stack([x[0, :, 3:7], x[1, :, 36:40]]))


def test_dropout_is_the_attention_hash():
    import attention_f64 as A
    x = rnd(39, 1000)
    for p in (0.0, 0.1, 0.5):
        y = V.dropout(x, G.f32(p), 0x1234ABCD)
        keep = torch.from_numpy(A.keep_mask(0x1234ABCD, 1000, G.f32(p)))
        assert torch.equal(y, torch.where(keep, x * A.inv_keep(G.f32(p)), torch.zeros_like(x)))
        assert abs(keep.double().mean().item() - (1 - p)) < 0.05
    assert bool((V.dropout(x, 0.0, 7) == x).all())


def test_exact_pass_is_exact():
    """From the case table alone: every result and every partial sum of the exact pass is a multiple of its quantum (a power of
    two) and below 2^24 quanta, so it is a float32 number whatever the order of the additions, atomics included; and on the
    generated operands themselves: the float64 reference of every exact case is a float32 number and a multiple of its quantum."""
    n = 0
    for c in G.TABLE:
        if c.entry in G.NO_EXACT:
            continue
        budget = G.exact_budget(c)
        if budget is None:
            assert c.entry == "dropout"
            continue
        for q, bound in budget:
            assert math.log2(q) == int(math.log2(q)), c.name
            assert bound < (1 << 24) * q, "%s %s: sums up to %g in steps of %g" % (c.entry, c.name, bound, q)
        if c.name == "n2097408":
            continue  # (its operands are 40 MB: the budget above is what holds it; the smaller KL cases run the same generator)
        q, top = min(b[0] for b in budget), max(b[1] for b in budget)
        for label, (y64, _, _, _) in G.reference("%s-%s" % (c.entry, c.name), "exact").items():
            assert bool((y64.float().double() == y64).all()), (c.name, label)
            assert bool(((y64 / q) == torch.round(y64 / q)).all()) and y64.abs().max().item() <= top, (c.entry, c.name, label)
        n += 1
    assert n > 100

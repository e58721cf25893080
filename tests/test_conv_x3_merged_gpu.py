"""GPU: the merged-phase form of the split-operand conv kernel (conv_x3_merged_kernel: one workgroup computes every output
residue of a phased launch -- strided data gradients, transposed-conv forwards -- from one staged input span) against the
per-residue form (tuning key x3_merge_phases = 0) and against float64 torch CPU.

Per output element the merged form does the additions of the per-residue form in the same order (channel groups outer, taps
inner, small terms first), so the two must agree BIT FOR BIT, for six and nine terms; both are fp32 arithmetic, within the
project's fp32 kernel bound of 2e-5 max-norm of the float64 result (test_conv_x3_gpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vcvits_amd import tuning
from vcvits_amd._lib import TF_DLEAKY, TF_LEAKY

pytestmark = pytest.mark.gpu

SLOPE = 0.1
TOL = 2e-5


def _case(name, C=32, M=48, H=100, P=3, K=5, s=3, pad=2, B=2, leaky=False, res=False, b0=0):
    return dict(name=name, C=C, M=M, H=H, P=P, K=K, s=s, pad=pad, B=B, leaky=leaky, res=res, b0=b0)


# strided data gradients in the period layout [B, C, H, P]: conv C -> M, the gradient has M reduction channels and C rows
DGRAD_CASES = [
    _case("H100", H=100), _case("H101", H=101), _case("H102", H=102),   # every Tin mod stride; U ~ 102: one ragged column tile
    _case("chtail", M=44),                                               # 44 reduction channels: a channel tail in the third group
    _case("mtail-H100", C=40, M=64, H=100), _case("mtail-H101", C=40, M=64, H=101), _case("mtail-H102", C=40, M=64, H=102),
    _case("B1", B=1), _case("B3", B=3),
    _case("K3", K=3, pad=1),                                             # one tap per residue
    _case("K7", K=7, pad=3),                                             # 3, 2, 2 taps
    _case("K2", K=2, pad=0),                                             # residue 2 has no taps: zeros plus the epilogue operands
    _case("K2-res-leaky", K=2, pad=0, leaky=True, res=True),
    _case("s2K4", K=4, s=2, pad=1),                                      # two residues
    _case("s2K4-M128", C=128, M=64, K=4, s=2, pad=1),                    # 128 rows: the 128 x 128 tile, two residues
    _case("C128", C=128, M=48),                                          # 128 rows: the 128 x 128 tile, three residues
    _case("C100", C=100, M=64),                                          # ... with an m-tail
    _case("C64", C=64, M=48),                                            # 64 rows: the 64 x 256 tile
    _case("leaky", leaky=True),                                          # out_tf = DLEAKY with oaux
    _case("res", res=True),                                              # residual gradient (ResGradLink)
    _case("leaky-res", C=40, M=64, leaky=True, res=True),
    _case("b0", B=4, b0=2),                                              # batch slice, as the G step uses
    _case("P37", H=20, P=37),                                            # wide rows, several rows per tile, two column tiles
    _case("P37-C128", C=128, H=20, P=37),
]


def rel64(a, b):
    return (a.detach().cpu().double() - b).abs().max().item() / (b.abs().max().item() + 1e-300)


def _both_forms(run):
    """run() under x3_merge_phases = 1 and 0, for 6 and 9 terms -> {(terms, merged): result}; every run must be taken by the
    split kernel.  The switch is read when the launch is planned; cached plans / packs are dropped after each flip."""
    from vcvits_amd import ops
    old = tuning.kernel_get("x3_merge_phases")
    out = {}
    try:
        for terms in (6, 9):
            ops.set_f32_split(True, terms=terms, all_shapes=True)
            for merged in (1, 0):
                tuning.kernel_set("x3_merge_phases", merged)
                ops.invalidate_weights()
                before = ops.LAUNCH_COUNTS["x3"]
                out[(terms, merged)] = run()
                assert ops.LAUNCH_COUNTS["x3"] == before + 1, "the split kernel did not take this launch"
    finally:
        tuning.kernel_set("x3_merge_phases", old)
        ops.invalidate_weights()
        ops.set_f32_split(True, terms=6, all_shapes=False)
    return out


def _check(out, ref, name):
    for terms in (6, 9):
        m, s = out[(terms, 1)], out[(terms, 0)]
        em, es = rel64(m, ref), rel64(s, ref)
        print("%s terms=%d merged_vs_f64=%.3g per_residue_vs_f64=%.3g bit_equal=%s" % (name, terms, em, es, torch.equal(m, s)))
        assert torch.equal(m, s), "%s, %d terms: merged and per-residue launches differ (max %g)" % (
            name, terms, (m - s).abs().max().item())
        assert em < TOL and es < TOL, (name, terms, em, es)


@pytest.mark.parametrize("c", DGRAD_CASES, ids=lambda c: c["name"])
def test_merged_strided_dgrad(gpu, c):
    from vcvits_amd import ops
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    B, C, M, H, P, K, s, pad = (c[k] for k in ("B", "C", "M", "H", "P", "K", "s", "pad"))
    x, w = t(B, C, H, P), t(M, C, K, 1) * (C * K) ** -0.5
    xr = x.double().requires_grad_(True)
    yr = F.conv2d(F.leaky_relu(xr, SLOPE) if c["leaky"] else xr, w.double(), None, stride=(s, 1), padding=(pad, 0))
    dy = t(*yr.shape)
    yr.backward(dy.double())
    ref = xr.grad
    res = t(B, C, H, P) if c["res"] else None
    if res is not None:
        ref = ref + res.double()
    b0 = c["b0"]
    ref = ref[b0:]
    xg, wg, dyg = x.to(gpu), w.to(gpu), dy.to(gpu)
    resg = res.to(gpu) if res is not None else None
    kw = {}
    if c["leaky"]:
        kw.update(out_tf=TF_DLEAKY, oaux=xg[b0:], slope=SLOPE)
    if resg is not None:
        kw["res"] = resg[b0:]

    def run():
        dx = torch.full((B, C, H, P), float("nan"), device=gpu)
        ops.conv_dgrad(dyg[b0:], wg, (B - b0, C, H, P), stride=s, pad=pad, out=dx[b0:], **kw)
        assert torch.isnan(dx[:b0]).all()
        return dx[b0:].cpu()

    _check(_both_forms(run), ref, c["name"])


@pytest.mark.parametrize("s,K,pad,leaky", [(2, 4, 1, False), (3, 7, 2, True), (2, 4, 1, True), (3, 7, 2, False)])
@pytest.mark.parametrize("C,M", [(48, 40), (128, 64), (64, 128)])
def test_merged_transposed_forward(gpu, C, M, s, K, pad, leaky):
    """conv_transpose1d forwards (P = 1, T = 130): 32-, 64- and 128-row tiles, bias, input leaky-ReLU."""
    from vcvits_amd import ops
    rng = np.random.default_rng(C * 1000 + M * 10 + s)
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    B, T = 2, 130
    x, w, b = t(B, C, T), t(C, M, K) * (C * K / s) ** -0.5, t(M) * 0.1
    xin = F.leaky_relu(x.double(), SLOPE) if leaky else x.double()
    ref = F.conv_transpose1d(xin, w.double(), b.double(), stride=s, padding=pad)
    xg, wg, bg = x.to(gpu), w.to(gpu), b.to(gpu)
    kw = dict(in_tf=TF_LEAKY, slope=SLOPE) if leaky else {}

    def run():
        return ops.convT_forward(xg, wg, bg, stride=s, pad=pad, **kw).cpu()

    _check(_both_forms(run), ref, "convT-C%d-M%d-s%d-K%d" % (C, M, s, K))


def test_merged_key_is_in_the_tuning_table():
    """x3_merge_phases is a key of the kernel tuning table, default on."""
    assert "x3_merge_phases" in tuning.KERNEL_KEYS
    assert tuning.kernel_get("x3_merge_phases") == 1

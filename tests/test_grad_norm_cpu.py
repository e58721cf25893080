"""CPU side of the gradient norms / clipping by global norm (csrc/elementwise.hip: vcv_grad_sqnorm, vcv_adamw_clip,
vcv_adamw_dev_clip; light/optim.py: FlatAdamW(max_grad_norm, norm_segments); light/vcvits.py: the two options): the
declarations, the argument checks that return before any launch, option parsing and its errors, the segment table's
contiguity rule, and the resources of the built kernels."""
import os

import pytest
import torch
from torch import nn

from test_attention_stream_cpu import _kernel_notes

EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
ENTRIES = ("vcv_grad_sqnorm", "vcv_adamw_clip", "vcv_adamw_dev_clip")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared():
    from vcvits_amd import _lib, ops
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "vcvits_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and name in _lib._ARGTYPES and hasattr(L, name)
        assert "int " + name + "(" in hdr
    # the `_clip` entries are the plain ones plus one pointer in front of the stream
    assert _lib._ARGTYPES["vcv_adamw_clip"] == _lib._ARGTYPES["vcv_adamw"][:-1] + [_lib._P, _lib._P]
    assert _lib._ARGTYPES["vcv_adamw_dev_clip"] == _lib._ARGTYPES["vcv_adamw_dev"][:-1] + [_lib._P, _lib._P]
    for name in ("grad_sqnorm", "adamw_step_clip", "adamw_step_dev_clip"):
        assert callable(getattr(ops, name))
    assert ops.grad_sqnorm_record_bytes(1) == 20 and ops.grad_sqnorm_record_bytes(3) == 44


def test_argument_checks_launch_nothing():
    """Everything below returns on the host before any launch: every pointer is null or never dereferenced."""
    from vcvits_amd import _lib
    L = _lib.lib()
    one = 64  # a non-null, 8-byte-aligned address that is never read
    sq = lambda ptrs, S: L.vcv_grad_sqnorm(ptrs[0], ptrs[1], S, ptrs[2], ptrs[3], 1.0, None)
    for i in range(4):
        assert sq([None if j == i else one for j in range(4)], 1) == EINVAL
    for S in (0, -1, 9, 1 << 20):
        assert sq([one] * 4, S) == EINVAL
    assert sq([66, one, one, one], 1) == EINVAL and sq([one, one, 68, one], 1) == EINVAL  # misaligned buffer / workspace
    clip = lambda ptrs, n, step: L.vcv_adamw_clip(*ptrs[:4], n, 1e-3, 0.9, 0.99, 1e-8, 0.01, step, ptrs[4], None)
    dev = lambda ptrs, n, base: L.vcv_adamw_dev_clip(*ptrs[:4], n, 0.9, 0.99, 1e-8, 0.01, ptrs[4], base, ptrs[5], None)
    for i in range(5):
        assert clip([None if j == i else one for j in range(5)], 4, 1) == EINVAL
    for i in range(6):
        assert dev([None if j == i else one for j in range(6)], 4, 1) == EINVAL
    assert clip([one] * 5, 0, 1) == EINVAL and clip([one] * 5, 4, 0) == EINVAL
    assert dev([one] * 6, 0, 1) == EINVAL and dev([one] * 6, 4, 0) == EINVAL


def test_ops_refuse_cpu_tensors():
    from vcvits_amd import ops
    f = torch.zeros(8)
    with pytest.raises(RuntimeError):
        ops.grad_sqnorm(f, torch.zeros(2, dtype=torch.int64), 1, torch.zeros(1024, dtype=torch.float64),
                        torch.zeros(24, dtype=torch.uint8), 1.0)
    with pytest.raises(RuntimeError):
        ops.adamw_step_clip(f, f, f, f, 1e-3, (0.9, 0.99), 1e-8, 0.01, 1, torch.ones(()))
    with pytest.raises(RuntimeError):
        ops.adamw_step_dev_clip(f, f, f, f, (0.9, 0.99), 1e-8, 0.01, torch.zeros(2, dtype=torch.int32), 1, torch.ones(()))


def test_clip_option_parsing():
    from vcvits_amd.light.vcvits import parse_gradient_clip
    assert parse_gradient_clip(None) is None and parse_gradient_clip(0) is None and parse_gradient_clip(0.0, "norm") is None
    assert parse_gradient_clip(0.5) == 0.5 and parse_gradient_clip("2", "norm") == 2.0 and parse_gradient_clip(1e30) == 1e30
    for bad in (-1, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            parse_gradient_clip(bad)
    with pytest.raises(NotImplementedError):
        parse_gradient_clip(1.0, "value")
    with pytest.raises(NotImplementedError):
        parse_gradient_clip(None, "value")
    with pytest.raises(ValueError):
        parse_gradient_clip(1.0, "median")


def _small_cfg():
    from vcvits_amd import configs
    cfg = configs.base()
    cfg["model"].update({"inter_channels": 16, "upsample_initial_channel": 32, "multi_period_discriminator_periods": [2, 3]})
    cfg["data"]["n_mel_channels"] = 40
    cfg["train"]["segment_size"] = 4096
    return cfg


def test_module_options_and_errors():
    """hparams.trainer.gradient_clip_val / gradient_clip_algorithm and hparams.train.log_grad_norms: absent, None and 0 are
    off; a negative value and the algorithm "value" fail when the module is built; the optimizers receive the values."""
    from vcvits_amd.light.vcvits import VocoderGAN
    cfg = _small_cfg()
    m = VocoderGAN(**cfg)
    assert m._norm_options() == (None, False)
    m.configure_optimizers()
    for o in (m.optim_g, m.optim_d):
        assert o.max_grad_norm is None and o.log_norms is False and not o.norms_enabled()
        assert o._norm_state is None  # nothing allocated, nothing launched
    assert m.optim_g._norm_names == ["net_g"] and m.optim_d._norm_names == ["net_period_d", "net_scale_d"]
    # the two discriminators' ranges tile optim_d's buffer, the scale discriminator first (reverse registration order)
    (plo, phi), (slo, shi) = m.optim_d._norm_ranges
    assert slo == 0 and shi == plo and phi == m.optim_d.numel
    assert shi == sum(p.numel() for p in m.net_scale_d.parameters())
    assert m.optim_g._norm_ranges == [(0, m.optim_g.numel)]
    for val in (None, 0, 0.0):
        cfg2 = _small_cfg()
        cfg2["trainer"] = {"gradient_clip_val": val, "gradient_clip_algorithm": "norm"}
        assert VocoderGAN(**cfg2)._norm_options() == (None, False)
    cfg2 = _small_cfg()
    cfg2["trainer"] = {"gradient_clip_val": 0.75}
    cfg2["train"]["log_grad_norms"] = True
    m2 = VocoderGAN(**cfg2)
    assert m2._norm_options() == (0.75, True)
    m2.configure_optimizers()
    assert m2.optim_g.max_grad_norm == 0.75 and m2.optim_d.max_grad_norm == 0.75 and m2.optim_g.log_norms and m2.optim_d.log_norms
    assert "max_grad_norm" not in m2.optim_g.state_dict() and set(m2.optim_g.state_dict()) == set(m.optim_g.state_dict())
    for trainer, err in (({"gradient_clip_val": -0.5}, ValueError), ({"gradient_clip_val": 1.0, "gradient_clip_algorithm": "value"}, NotImplementedError)):
        cfg3 = _small_cfg()
        cfg3["trainer"] = trainer
        with pytest.raises(err):
            VocoderGAN(**cfg3)
    # Lightning's hook writes the optimizer's setting
    m.configure_gradient_clipping(m.optim_d, 1, gradient_clip_val=2.0, gradient_clip_algorithm="norm")
    assert m.optim_d.max_grad_norm == 2.0 and m.optim_g.max_grad_norm is None
    m.configure_gradient_clipping(m.optim_d, 1, gradient_clip_val=None)
    assert m.optim_d.max_grad_norm is None
    # positional calls without optimizer_idx (Lightning 2.x's signature): (optimizer, clip value, algorithm)
    m.configure_gradient_clipping(m.optim_d, 1, "norm")
    assert m.optim_d.max_grad_norm == 1.0
    m.configure_gradient_clipping(m.optim_d, 0.25, "norm")
    assert m.optim_d.max_grad_norm == 0.25
    m.configure_gradient_clipping(m.optim_d, 1, 3.0, "norm")  # (Lightning 1.x, positional)
    assert m.optim_d.max_grad_norm == 3.0
    m.configure_gradient_clipping(m.optim_d, None)
    assert m.optim_d.max_grad_norm is None
    with pytest.raises(NotImplementedError):
        m.configure_gradient_clipping(m.optim_g, 0, gradient_clip_val=1.0, gradient_clip_algorithm="value")
    with pytest.raises(ValueError):
        m.configure_gradient_clipping(m.optim_g, 0, gradient_clip_val=-1.0)
    for o in (m.optim_g, m.optim_d, m2.optim_g, m2.optim_d):
        o.close()


def test_norm_segments_must_be_contiguous_ranges():
    from vcvits_amd.light.optim import FlatAdamW
    a, b, c = nn.Parameter(torch.randn(7)), nn.Parameter(torch.randn(64, 5)), nn.Parameter(torch.randn(1))
    o = FlatAdamW([a, b, c], 1e-3, norm_segments=[("ab", [a, b]), ("c", [c])])
    assert o.offsets == [0, 1, 321]  # stored in reverse registration order: c, b, a
    assert o._norm_names == ["ab", "c"] and o._norm_ranges == [(1, 328), (0, 1)]
    o.close()
    o = FlatAdamW([a, b, c], 1e-3)
    assert o._norm_names == ["all"] and o._norm_ranges == [(0, 328)] and o.max_grad_norm is None
    with pytest.raises(RuntimeError):
        o.grad_norms()
    o.close()
    other = nn.Parameter(torch.randn(2))
    for bad in ([("ac", [a, c]), ("b", [b])],          # a and c are not neighbours in the buffer
                [("a", [a])],                           # leaves parameters out: the total would not be the optimizer's norm
                [("ab", [a, b]), ("bc", [b, c])],       # overlap
                [("ab", [a, b]), ("ab", [c])],          # repeated name
                [("total", [a, b, c])],                 # reserved name
                [("x", [a, b, c, other])],              # a parameter of another optimizer
                [("x", [a, b, c]), ("y", [])]):         # empty group
        with pytest.raises(ValueError):
            FlatAdamW([a, b, c], 1e-3, norm_segments=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            FlatAdamW([a, b, c], 1e-3, max_grad_norm=bad)
    o = FlatAdamW([a, b, c], 1e-3, max_grad_norm=0)
    assert o.max_grad_norm is None
    o.close()


def test_kernels_use_no_scratch_memory(tmp_path):
    """The four new kernels, read from the built object (no GPU): no scratch, no spills; the reduction's stage one keeps only
    the block reduction's four doubles in LDS, the finishing stage at most 64 KB."""
    from vcvits_amd import build_ext
    build_ext.build(verbose=False)
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    notes = _kernel_notes("elementwise", tmp_path)
    mine = {}
    for stem in ("grad_sqnorm_partial_kernel", "grad_sqnorm_finish_kernel", "adamw_clip_kernel", "adamw_dev_clip_kernel"):
        hit = [n for n in notes if stem in n]
        assert len(hit) == 1, (stem, sorted(notes))
        mine[stem] = notes[hit[0]]
    for name, f in mine.items():
        print(name, f)
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] <= 64 * 1024, (name, f)
    assert mine["grad_sqnorm_partial_kernel"]["group_segment_fixed_size"] == 32
    assert mine["adamw_clip_kernel"]["group_segment_fixed_size"] == 0

"""CPU side of the streamed relative-position attention (csrc/attention_stream.hip):

  * tests/attention_rows_f64.py (the output for a list of query rows, the only reference that fits at T = 20,000) is pinned
    to tests/attention_f64.py at small T: equal in float64;
  * the new kernels keep their arrays in registers (no scratch), read from the built object;
  * the argument checks of the two entry points, which launch nothing, and the declarations that go with the kernel
    (exports, launch counter, the routing threshold in the tuning registry).
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attention_f64 as A
import attention_rows_f64 as AR

EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)


def _mask(kind, B, T):
    m = torch.ones(B, T)
    if "ragged" in kind:
        m[B - 1, T - max(T // 5, 1):] = 0.0
    if "hole" in kind:
        m[0, T // 3] = 0.0
    if "zero" in kind:
        m[B - 1, :] = 0.0
    if "head" in kind:  # the first keys masked
        m[0, :T // 2] = 0.0
    return m


SMALL = [  # B, H, dk, T, w, mask
    (1, 1, 8, 1, 4, "ones"),
    (2, 1, 8, 5, 7, "ragged"),          # T <= w
    (2, 2, 16, 32, 0, "hole"),          # w = 0
    (2, 1, 32, 33, 4, "ragged"),
    (3, 2, 8, 70, 4, "ragged+hole"),
    (2, 1, 16, 97, 7, "zero"),          # an all-zero batch row
    (2, 2, 8, 130, 3, "head+ragged"),
]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "B%d-H%d-dk%d-T%d-w%d-%s" % c)
def test_rows_restatement_equals_the_full_reference(case):
    B, H, dk, T, w, kind = case
    rng = np.random.default_rng(T * 131 + w)
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    q, k, v = 2.0 * t(B, H * dk, T), t(B, H * dk, T), t(B, H * dk, T)
    ek, ev = t(1, 2 * w + 1, dk) * dk ** -0.5, t(1, 2 * w + 1, dk) * dk ** -0.5
    mask = _mask(kind, B, T)
    full = A.rel_attention(q, k, v, ek, ev, mask).out
    assert full.dtype == torch.float64
    every = AR.rel_attention_rows(q, k, v, ek, ev, mask, list(range(T)))
    assert every.dtype == torch.float64 and every.shape == full.shape
    assert A.dist(every, full) == 0.0, A.dist(every, full)
    # a subset, out of order: the columns of the full output, in that order
    rows = sorted({0, T - 1, T // 2, min(w, T - 1), T // 3})[::-1]
    some = AR.rel_attention_rows(q, k, v, ek, ev, mask, rows)
    assert some.shape == (B, H * dk, len(rows))
    assert A.dist(some, full[:, :, rows]) <= 1e-15, A.dist(some, full[:, :, rows])
    # the float32 run of the same text stays a float32 computation, at float32 distance
    r32 = AR.rel_attention_rows(q, k, v, ek, ev, mask, rows, dtype=torch.float32)
    assert r32.dtype == torch.float32 and A.dist(r32, some) <= 1e-5


def _kernel_notes(stem, tmp_path):
    """{kernel name: {metadata field: int}} of the gfx950 code object inside csrc/<stem>.o."""
    from vcvits_amd import build_ext
    llvm = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(build_ext.CSRC, stem + ".o")
    fat, co = str(tmp_path / (stem + ".fat")), str(tmp_path / (stem + ".co"))
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for entry in re.split(r"\n\s+- \.", notes):  # one list item per kernel
        name = re.search(r"\.?name:\s+(\S+)", entry)
        if name and "private_segment_fixed_size" in entry:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.?(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def test_stream_kernels_use_no_scratch_memory(tmp_path):
    """The six instances that stand on csrc/attn_stream_tile.h, read from the built objects (no GPU): no scratch and no
    spills anywhere in the two files, the static LDS of each instance, and the register budgets: at most 168 for the rel-pos
    dk = 32 kernel (three workgroups of four waves per CU: 512 registers per SIMD lane / 3, in granules of 8), at most 256
    (what one wave can address without spilling) for the others."""
    from vcvits_amd import build_ext
    build_ext.build(verbose=False)
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    stream, hubert = _kernel_notes("attention_stream", tmp_path), _kernel_notes("hubert", tmp_path)
    for name, f in list(stream.items()) + list(hubert.items()):
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] <= 64 * 1024, (name, f)  # static LDS: no attribute call in the launcher
    want = {"rel_attn_stream_fwd_kernelILi32E": (30976, 168), "rel_attn_stream_fwd_kernelILi64E": (43392, 256),
            "hubert_attn_fwd_kernelILi64ELb0E": (16640, 256), "hubert_attn_fwd_kernelILi64ELb1E": (16640, 256),
            "hubert_attn_fwd_kernelILi80ELb0E": (22912, 256), "hubert_attn_fwd_kernelILi80ELb1E": (22912, 256)}
    attn = {n: f for n, f in list(stream.items()) + list(hubert.items()) if "attn" in n}
    assert len(attn) == 6, sorted(attn)
    for key, (lds, regs) in want.items():
        (name, f), = [(n, f) for n, f in attn.items() if key in n]
        print(name, f)
        assert f["group_segment_fixed_size"] == lds, (name, f)
        assert f["vgpr_count"] <= regs, (name, f)  # unified count: vector and accumulation registers


def test_entry_points_are_declared_and_check_their_arguments():
    """Header, library and _lib.EXPORTS carry the two entry points; the argument checks run on the host and launch nothing,
    so they can be exercised without a GPU (every pointer below is null or never dereferenced)."""
    from vcvits_amd import _lib
    L = _lib.lib()
    assert "vcv_rel_attn_stream_supported" in _lib.EXPORTS and "vcv_rel_attn_stream_fwd" in _lib.EXPORTS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vcvits_hip.h")).read()
    assert "vcv_rel_attn_stream_fwd(" in hdr and "relative_attention_transformer.py:150-182" in hdr
    ok = L.vcv_rel_attn_stream_supported
    for dk in (32, 64):
        for T in (1, 896, 897, 20000, 1 << 20):
            assert ok(1, 2, dk, T, 4) == 0
    assert ok(1, 1, 32, 10, 0) == 0 and ok(1, 1, 32, 10, 7) == 0 and ok(65535, 1, 32, 10, 4) == 0 and ok(255, 257, 32, 10, 4) == 0
    for B, H, dk, T, w in ((1, 1, 48, 40, 4), (1, 1, 7, 40, 4), (1, 1, 16, 40, 4), (1, 1, 32, 40, 8), (1, 1, 32, 0, 4),
                           (0, 1, 32, 40, 4), (1, 0, 32, 40, 4), (1, 1, 32, 40, -1), (65536, 1, 32, 40, 4), (256, 256, 64, 40, 4)):
        assert ok(B, H, dk, T, w) == EINVAL, (B, H, dk, T, w)
        assert L.vcv_rel_attn_stream_fwd(None, None, None, None, None, None, None, B, H, dk, T, w, 1.0, None) == EINVAL
    assert L.vcv_rel_attn_stream_fwd(None, None, None, None, None, None, None, 1, 1, 32, 40, 4, 1.0, None) == EINVAL  # null pointers
    # the fused kernels' limits are where they were
    assert L.vcv_rel_attn_supported(1, 1, 64, 896, 4) == 0 and L.vcv_rel_attn_supported(1, 1, 64, 897, 4) == EINVAL


def test_routing_switch_and_counter_are_declared():
    from vcvits_amd import ops, tuning
    assert ops.LAUNCH_COUNTS["attn_stream"] >= 0
    kind, default, doc, _ = tuning.REGISTRY["VCVITS_ATTN_STREAM_MIN_T"]
    assert kind == "int" and default == 897 and doc
    assert ops._ATTN_STREAM_MIN_T is ops.attention._ATTN_STREAM_MIN_T  # one list, shared by reference
    assert any("VCVITS_ATTN_STREAM_MIN_T" in line for line in tuning.table())

"""CPU side of the bf16-operand streamed attention kernels (csrc/attention_stream_bf16.hip on csrc/attn_stream_tile.h):

  * the three entry points are declared (header, library, _lib.EXPORTS), the switch is in the tuning registry with default 0,
    the launch counter exists;
  * their argument checks, which run on the host and launch nothing;
  * the six instances keep their arrays in registers (no scratch, no spills), their static LDS sizes, and register counts
    no higher than the fp32 instance of the same shape is held to (tests/test_attention_stream_cpu.py), read from the built
    object;
  * the fragment map of the second product, in numpy: which key a reduction element of the bf16 MFMA is.
"""
import ctypes
import os

import numpy as np
import pytest

from test_attention_stream_cpu import _kernel_notes

EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vcv_rel_attn_stream_fwd_bf16", "vcv_hubert_attn_fwd_bf16", "vcv_hubert_attn_fwd_len_bf16")


def test_entries_switch_and_counter_are_declared():
    from vcvits_amd import _lib, ops, tuning
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "vcvits_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and name + "(" in hdr, name
        assert getattr(L, name) is not None
        assert _lib._ARGTYPES[name] == _lib._ARGTYPES[name[:-len("_bf16")]], name  # the signature of the fp32 twin
    kind, default, doc, _ = tuning.REGISTRY["VCVITS_ATTN_STREAM_BF16"]
    assert default == 0 and default is not True and doc
    assert ops._ATTN_STREAM_BF16 is ops.attention._ATTN_STREAM_BF16 and len(ops._ATTN_STREAM_BF16) == 1  # one list, shared
    assert any("VCVITS_ATTN_STREAM_BF16" in line for line in tuning.table())
    assert ops.LAUNCH_COUNTS["attn_stream_bf16"] >= 0 and ops.LAUNCH_COUNTS is ops.hubert.LAUNCH_COUNTS
    # the switch alone routes nothing: the compute dtype must be bf16 too
    old, mode = ops._ATTN_STREAM_BF16[0], ops.compute_dtype()
    try:
        for sw in (0, 1):
            for dt in ("f32", "bf16"):
                ops._ATTN_STREAM_BF16[0] = sw
                ops.set_compute_dtype(dt)
                assert ops.attn_stream_bf16() == (sw == 1 and dt == "bf16")
    finally:
        ops._ATTN_STREAM_BF16[0] = old
        ops.set_compute_dtype(mode)


def test_entries_check_their_arguments():
    """VCV_EINVAL before any launch: there is no GPU here, so a call that reached a launch would return VCV_EHIP.  The
    pointers are null or the address of a host buffer that a refused call never dereferences."""
    from vcvits_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rel = L.vcv_rel_attn_stream_fwd_bf16
    assert rel(None, None, None, None, None, None, None, 1, 1, 32, 40, 4, 1.0, None) == EINVAL
    for hole in range(7):  # each pointer null in turn, the shape a supported one
        args = [None if i == hole else p for i in range(7)]
        assert rel(*args, 1, 1, 32, 40, 4, 1.0, None) == EINVAL, hole
    for B, H, dk, T, w in ((1, 1, 48, 40, 4), (1, 1, 32, 40, 8), (1, 1, 32, 0, 4), (65536, 1, 32, 40, 4), (256, 256, 64, 40, 4),
                           (0, 1, 32, 40, 4), (1, 1, 32, 40, -1), (1, 1, 80, 40, 4)):
        assert L.vcv_rel_attn_stream_supported(B, H, dk, T, w) == EINVAL
        assert rel(p, p, p, p, p, p, p, B, H, dk, T, w, 1.0, None) == EINVAL, (B, H, dk, T, w)

    hub, hub_len = L.vcv_hubert_attn_fwd_bf16, L.vcv_hubert_attn_fwd_len_bf16
    ld = lambda H, dk, T: H * dk * T
    for hole in range(4):
        args = [None if i == hole else p for i in range(4)]
        assert hub(*args, 1, 2, 64, 40, ld(2, 64, 40), 0.125, None) == EINVAL, hole
        assert hub_len(*args, 1, 2, 64, 40, ld(2, 64, 40), 0.125, p, None) == EINVAL, hole
    assert hub_len(p, p, p, p, 1, 2, 64, 40, ld(2, 64, 40), 0.125, None, None) == EINVAL  # null frames
    for B, H, dk, T in ((1, 1, 48, 40), (1, 1, 32, 40), (1, 2, 64, 0), (65536, 1, 64, 40), (256, 256, 80, 40), (0, 1, 64, 40)):
        assert L.vcv_hubert_attn_supported(B, H, dk, T) != 0
        assert hub(p, p, p, p, B, H, dk, T, ld(H, dk, max(T, 1)), 0.125, None) == EINVAL, (B, H, dk, T)
        assert hub_len(p, p, p, p, B, H, dk, T, ld(H, dk, max(T, 1)), 0.125, p, None) == EINVAL, (B, H, dk, T)
    for dk in (64, 80):  # ldb one float short of a batch row
        assert L.vcv_hubert_attn_supported(2, 3, dk, 40) == 0
        assert hub(p, p, p, p, 2, 3, dk, 40, ld(3, dk, 40) - 1, 0.125, None) == EINVAL
        assert hub_len(p, p, p, p, 2, 3, dk, 40, ld(3, dk, 40) - 1, 0.125, p, None) == EINVAL


# kernel name fragment -> (static LDS bytes, the register budget of the fp32 instance of the same shape).  This build: 156 / 212
# registers for rel-pos dk = 32 / 64, 156 / 204 for HuBERT d = 64 / 80 (the header of csrc/attention_stream_bf16.hip quotes them).
WANT = {"rel_attn_stream_fwd_bf16_kernelILi32E": (27520, 168), "rel_attn_stream_fwd_bf16_kernelILi64E": (35968, 256),
        "hubert_attn_fwd_bf16_kernelILi64ELb0E": (9216, 256), "hubert_attn_fwd_bf16_kernelILi64ELb1E": (9216, 256),
        "hubert_attn_fwd_bf16_kernelILi80ELb0E": (12544, 256), "hubert_attn_fwd_bf16_kernelILi80ELb1E": (12544, 256)}


def test_bf16_stream_kernels_resources(tmp_path):
    """The six instances of csrc/attention_stream_bf16.hip, read from the built object (no GPU): no scratch, no spills, static
    LDS within 64 KB and equal to the sizes the file's header states, and registers within the budget of the fp32 instance of
    the same shape: 168 for rel-pos dk = 32 (three workgroups of four waves per CU), 256 for the others.  The counts of this
    build are printed; the file's header quotes them."""
    from vcvits_amd import build_ext
    build_ext.build(verbose=False)
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    notes = {n: f for n, f in _kernel_notes("attention_stream_bf16", tmp_path).items() if "attn" in n}  # (common.h's zeroing kernel aside)
    assert len(notes) == 6 and all("_bf16_kernel" in n for n in notes), sorted(notes)
    for name, f in notes.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] <= 64 * 1024, (name, f)
    for key, (lds, budget) in WANT.items():
        (name, f), = [(n, f) for n, f in notes.items() if key in n]
        print(name, f)
        assert f["group_segment_fixed_size"] == lds, (name, f)
        assert f["vgpr_count"] <= budget, (name, f)  # unified count: vector and accumulation registers
    # the LDS sizes from the strides the header of csrc/attn_stream_tile.h states: K [32][D + 8] and V [rows][36] in bf16
    kv = lambda D, rows: 2 * (32 * (D + 8) + rows * 36)
    band = lambda D: 4 * (32 + 2 * 16 * D + 2 * 128 * 18)  # the mask tile, two tables, rel and the band probabilities
    assert (kv(32, 32) + band(32), kv(64, 64) + band(64), kv(64, 64), kv(80, 96)) == (27520, 35968, 9216, 12544)


def acc_row(e, h):
    """common.h: the row of accumulator element e of lane half h in a 32 x 32 MFMA result"""
    return (e & 3) + 8 * (e >> 2) + 4 * h


def test_fragment_map_of_the_second_product():
    """tile_pv_bf16: registers 8 m .. 8 m + 7 of S (lane half hf) are the B fragment of MFMA m, so reduction element
    8 hf + e of MFMA m is key acc_row(8 m + e, hf).  The map covers each of the 32 keys exactly once, it is the two 4-key runs
    the A fragment reads from the value tile, and a 32x32x16 MFMA evaluated with it on ASYMMETRIC integer data is V P^T."""
    key = np.array([[[acc_row(8 * m + e, hf) for e in range(8)] for hf in range(2)] for m in range(2)])  # [m][hf][e]
    assert sorted(key.reshape(-1).tolist()) == list(range(32))
    for m in range(2):
        assert sorted(key[m].reshape(-1).tolist()) == list(range(16 * m, 16 * m + 16))  # MFMA m sums the keys 16 m .. 16 m + 15
        for hf in range(2):
            lo, hi = 16 * m + 4 * hf, 16 * m + 8 + 4 * hf  # the two 8-byte reads of tile_pv_bf16
            assert key[m, hf].tolist() == list(range(lo, lo + 4)) + list(range(hi, hi + 4))
            assert lo % 4 == 0 and hi + 4 <= 32
    # reduction index k = 8 hf + e of the instruction: A[row][k] from lane (row, hf) element e, B[k][col] likewise
    rng = np.random.default_rng(3)
    V = rng.integers(-8, 9, size=(32, 32)).astype(np.float64)  # [channel][key]
    P = rng.integers(0, 17, size=(32, 32)).astype(np.float64)  # [query][key]: S^T register r of lane (query, hf) is key acc_row(r, hf)
    assert not np.array_equal(V, V.T) and not np.array_equal(P, P.T)
    O = np.zeros((32, 32))
    for m in range(2):
        A = np.zeros((32, 16))
        Bm = np.zeros((16, 32))
        for hf in range(2):
            for e in range(8):
                A[:, 8 * hf + e] = V[:, key[m, hf, e]]          # what the lane (channel, hf) reads from Vs
                Bm[8 * hf + e, :] = P[:, acc_row(8 * m + e, hf)]  # register 8 m + e of the lane (query, hf)
        O += A @ Bm
    assert np.array_equal(O, V @ P.T)
    # a map in natural key order (element e = key 16 m + 8 hf + e) pairs the operands wrongly
    wrong = np.array([[[16 * m + 8 * hf + e for e in range(8)] for hf in range(2)] for m in range(2)])
    assert not np.array_equal(wrong, key)


def test_fragment_map_of_the_scores():
    """tile_scores_bf16 / tile_load_q_bf16: element e of step i of lane half hf is channel 16 i + 8 hf + e on both operands, and
    qf[8 i + e] holds it; over (i, hf, e) every channel of D = 32, 64, 80 appears once."""
    for D in (32, 64, 80):
        ch = [16 * (j >> 3) + 8 * hf + (j & 7) for hf in range(2) for j in range(D // 2)]
        assert sorted(ch) == list(range(D))
        # the staging thread (key, group g) writes channels g * D / 8 .. + D / 8 - 1: all of them over the 8 groups
        assert sorted(g * (D // 8) + i for g in range(8) for i in range(D // 8)) == list(range(D))
        assert (D // 2 + 4) % 8 == 4  # the key tile's row stride in dwords: 16 keys distinct mod 16 fill the 64 banks once

"""CPU: the pitch step of the reference's data path -- estimate_pitch's import surface and argument errors, pYIN's derived
constants and host tables, the pyin kernels' code objects, and the float64 oracle (tests/pyin_f64.py) on clean tones,
silence and noise."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pyin_f64 as P


def test_estimate_pitch_resolves_at_the_reference_import_path():
    from vits.data.audio import coarse_f0, estimate_pitch, normalize_pitch  # infer.py:10, preprocess.py:9
    from vits.data import pitch_classes
    assert callable(estimate_pitch) and callable(normalize_pitch) and callable(coarse_f0) and callable(pitch_classes)


def test_argument_errors_before_any_device_work():
    from vits.data.audio import estimate_pitch, pitch_classes
    x = np.zeros(4000, dtype=np.float32)
    with pytest.raises(ValueError):
        estimate_pitch(x, 16000, 2048, 2048, 320, method="crepe")
    with pytest.raises(NotImplementedError):
        estimate_pitch(x, 16000, 2048, 2048, 320, n_formants=2)
    with pytest.raises(NotImplementedError):
        estimate_pitch(x, 16000, 1024, 1024, 320)  # the kernels are laid out for frame_length 2048
    with pytest.raises(ValueError):
        estimate_pitch(np.zeros(319, dtype=np.float32), 16000, 2048, 2048, 320)  # N + 2 pad < frame_length
    with pytest.raises(ValueError):
        estimate_pitch(np.zeros((2, 4000), dtype=np.float32), 16000, 2048, 2048, 320)
    bad = x.copy()
    bad[7] = np.inf
    with pytest.raises(ValueError):
        estimate_pitch(bad, 16000, 2048, 2048, 320)
    with pytest.raises(NotImplementedError):
        pitch_classes(torch.zeros(1, 4000), [4000], 16000, 2048, 1024)


def test_pyin_ops_refuse_cpu_tensors():
    from vcvits_amd import ops
    with pytest.raises(RuntimeError, match="not on the GPU"):
        ops.pyin(torch.zeros(1, 4000))


def test_normalize_pitch():
    from vits.data.audio import normalize_pitch
    p = torch.tensor([[0.0, 100.0, 200.0]])
    out = normalize_pitch(p, torch.tensor([100.0]), torch.tensor([50.0]))
    assert out is p and out.tolist() == [[0.0, 0.0, 2.0]]


def test_derived_constants():
    from vcvits_amd.ops import pitch
    assert P.FMIN == 65.40639132514966 and P.FMAX == 2093.004522404789
    assert pitch.PYIN_FMIN == P.FMIN and pitch.PYIN_FMAX == P.FMAX
    c = P.consts()
    assert (c["win"], c["min_period"], c["max_period"], c["n_pitch_bins"], c["width"]) == (1024, 7, 245, 601, 91)
    k = pitch.pyin_consts()
    assert (k["win_length"], k["min_period"], k["max_period"], k["n_lags"], k["n_bins"], k["n_states"],
            k["transition_width"]) == (1024, 7, 245, 239, 601, 1202, 91)
    assert round(35.92 * 12 * 320 / 16000) == 9
    assert pitch.PYIN_LOG_TINY == -708.3964185322641 == float(np.log(P.TINY))
    for n in (320, 321, 639, 640, 865, 160000):
        assert pitch.pyin_n_frames(n) == 1 + (n + 2 * 864 - 2048) // 320 == 1 + (n - 320) // 320
        assert P.frames(np.zeros(n, np.float32), 864).shape[0] == pitch.pyin_n_frames(n)


def test_oracle_reflect_padding_is_numpys():
    for n in range(2, 3001):
        y = np.arange(n, dtype=np.float32)
        assert np.array_equal(np.pad(y, (864, 864), mode="reflect"), y[P.reflect_index(np.arange(n + 1728), n, 864)]), n


def test_host_tables_match_the_oracles_dense_matrices():
    from vcvits_amd.data.audio import coarse_f0
    from vcvits_amd.ops import pitch
    t = pitch.pyin_host_tables()
    c = P.consts()
    lt, lpi = P.viterbi_tables(c)
    nb = 601
    for d in range(91):
        for s, off in ((0, 0), (1, nb)):
            for j in (0, 1, 44, 45, 46, 300, 554, 555, 556, 600):
                i = j + d - 45
                if 0 <= i < nb:
                    assert t["band"][s, d, j] == lt[off + i, j]
                    assert t["band"][s, d, j] == lt[(nb - off) + i, nb + j]  # the unvoiced targets see the same band
    assert np.array_equal(t["log_p_init"], lpi)
    thr, beta = P.tables()
    assert np.array_equal(t["thresholds"], thr) and np.array_equal(t["beta_probs"], beta)
    f = (P.FMIN * 2 ** (np.arange(nb) / 120)).astype(np.float32)
    assert np.array_equal(t["f0_table"][:nb], f) and t["f0_table"][nb] == 0
    assert np.array_equal(t["class_table"], coarse_f0(torch.from_numpy(t["f0_table"].copy())).numpy())


def _tone(f, dur=0.6, sr=16000):
    t = np.arange(int(dur * sr)) / sr
    return (0.3 * np.sin(2 * np.pi * f * t) + 0.1 * np.sin(4 * np.pi * f * t + 1)).astype(np.float32)


@pytest.mark.parametrize("f", [110.0, 220.0, 440.0, 880.0])
def test_oracle_tracks_clean_tones(f):
    f0, voiced, vp = P.pyin(_tone(f))
    assert voiced[1:].all()
    assert np.abs(12 * np.log2(f0[1:] / f)).max() <= 0.1


@pytest.mark.parametrize("f", [1500.0, 2000.0])
def test_oracle_high_tones_voiced_frames_in_tune(f):
    f0, voiced, vp = P.pyin(_tone(f))
    assert voiced.any()
    assert np.abs(12 * np.log2(f0[voiced] / f)).max() <= 0.1


def test_oracle_silence_and_noise_are_unvoiced():
    assert not P.pyin(np.zeros(9600, dtype=np.float32))[1].any()
    noise = (0.1 * np.random.default_rng(0).standard_normal(9600)).astype(np.float32)
    assert not P.pyin(noise)[1].any()


def test_pyin_kernels_use_no_scratch_memory(tmp_path):
    """csrc/pyin.hip keeps its arrays in registers and LDS (`.private_segment_fixed_size: 0` for every kernel), as
    test_abi_and_host.py checks for the MFMA files.  Reads the device code out of the built object (no GPU)."""
    from vcvits_amd import build_ext
    build_ext.build(verbose=False)
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    obj = os.path.join(build_ext.CSRC, "pyin.o")
    fat, co = str(tmp_path / "pyin.fat"), str(tmp_path / "pyin.co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    for k in ("pyin_yin_kernel", "pyin_obs_kernel", "pyin_viterbi_kernel"):
        assert k in notes, k
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    assert len(sizes) >= 3 and max(sizes) == 0, sizes

"""CPU: what the resampling / pitch-shift kernels rest on, established over the restatement (tests/audio_fx_f64.py) -- the
band of the sinc filter bank, the reachability of the GPU tests' bounds by the reference's own float32 arithmetic -- plus the
host-side WAV reader, the reference's import paths and the no-CPU-fallback rule."""
import math
import struct
import wave

import numpy as np
import pytest
import torch

import audio_fx_f64 as R

DENSE_RATIOS = [(48000, 16000), (44100, 16000), (22050, 16000), (16000, 48000), (16000, 44100)]
COPRIME_RATIOS = [(16951, 16000), (15101, 16000)]


def _phases(n, count=1000, seed=0):
    return np.sort(np.random.default_rng(seed).choice(n, size=count, replace=False))


@pytest.mark.parametrize("orig,new", DENSE_RATIOS + COPRIME_RATIOS)
def test_taps_outside_the_band_are_zero_and_the_band_fits(orig, new):
    """Every float32 tap with |t| >= 6 before clamping is exactly 0, the taps with |t| < 6 are contiguous and at most W of
    them: the table of n * W taps holds everything the dense bank does."""
    from vcvits_amd import ops
    c = ops.resample_consts(orig, new)
    o, n, base, width = R.ratio(orig, new)
    assert (c["o"], c["n"], c["base"], c["width"], c["n_taps"]) == (o, n, base, width, 2 * width + o)
    assert c["W"] == R.band_bound(orig, new)
    phases = None if (orig, new) in DENSE_RATIOS else _phases(n)
    kern, w, raw = R.sinc_kernel(orig, new, None, phases)
    kern = kern[:, 0]
    assert w == width and kern.dtype == torch.float32 and raw.dtype == torch.float64
    outside = raw.abs() >= R.LOWPASS_WIDTH
    assert bool((kern[outside] == 0).all())
    first, count = R.band_of(raw)
    inside = ~outside
    span = torch.arange(raw.shape[1])[None, :]
    assert bool((inside == ((span >= first[:, None]) & (span < (first + count)[:, None]))).all())  # contiguous
    assert int(count.min()) >= 1 and int(count.max()) <= c["W"], (int(count.max()), c["W"])
    # formed in float32 (functional.resample's bank) the same taps are not exactly zero, but far below any rounding
    k32, _, raw32 = R.sinc_kernel(orig, new, torch.float32, np.arange(n) if phases is None else phases)
    far = raw32.abs() >= R.LOWPASS_WIDTH
    assert float(k32[:, 0][far].abs().max()) < 1e-20
    print("%d -> %d: width %d, %d taps per dense row, band %d..%d of W = %d" % (orig, new, width, raw.shape[1],
                                                                              int(count.min()), int(count.max()), c["W"]))


@pytest.mark.parametrize("orig,new", DENSE_RATIOS + COPRIME_RATIOS)
def test_float32_convolution_meets_the_chain_bound(orig, new):
    """The reference's own arithmetic (float32 taps, float32 conv1d) is within (W + 1) * 2^-24 * sum |tap| |x| of the float64
    convolution of the same taps: the bound the GPU test holds the kernel to is reachable."""
    W = R.band_bound(orig, new)
    worst = 0.0
    for name, x in R.signals(orig, seconds=0.25, seed=1).items():
        y64, a = R.resample(x, orig, new, dtype=torch.float64, kernel_dtype=None, terms=True)
        y32 = R.resample(x, orig, new, dtype=torch.float32, kernel_dtype=None)
        o, n, _, _ = R.ratio(orig, new)
        assert y32.shape[0] == int(math.ceil(n * len(x) / o))
        bound = (W + 1) * 2.0 ** -24 * a
        ratio = float(((y32.double() - y64).abs() / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool(((y32.double() - y64).abs() <= bound).all()), (name, ratio)
    print("%d -> %d: float32 conv1d uses at most %.3f of the bound" % (orig, new, worst))


def test_banded_and_dense_restatement_agree():
    x = R.signals(22050, seconds=0.2, seed=2)["vowel"]
    for orig, new in ((22050, 16000), (16000, 44100)):
        d = R.resample(x, orig, new, dense=True)
        b = R.resample(x, orig, new, dense=False)
        assert d.shape == b.shape and float((d - b).abs().max()) < 1e-14


def test_host_constants():
    from vcvits_amd import ops
    assert ops.resample_out_len(16000, 48000, 16000) == 5334 and ops.resample_out_len(3, 16000, 48000) == 9
    c = ops.resample_consts(48000, 16000)
    assert (c["o"], c["n"], c["width"]) == (3, 1, 19) and c["W"] <= 38
    assert ops.resample_consts(16951, 16000)["W"] * 16000 * 4 < 1.2e6  # about 1 MB, never the 2 GB dense bank
    p = ops.pitch_shift_consts(16000, 16000, 1)
    assert p["orig_freq"] == 16951 and p["len_stretch"] == int(round(16000 / p["rate"]))
    assert ops.phase_vocoder_frames(126, p["rate"]) == len(R.time_steps(126, p["rate"]))
    with pytest.raises(ValueError):
        ops.resample_consts(0, 16000)


def _write_wav(path, data, rate, width):
    """data int [T, C] of `width`-byte samples, through the standard library's wave module."""
    with wave.open(str(path), "wb") as f:
        f.setnchannels(data.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        if width == 3:
            raw = b"".join(int(v).to_bytes(3, "little", signed=True) for v in data.reshape(-1))
        else:
            raw = data.astype({2: "<i2", 4: "<i4"}[width]).tobytes()
        f.writeframes(raw)


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("channels", [1, 2])
def test_wav_reader_scales_as_torchaudio_load(tmp_path, width, channels):
    from vits.utils import load_wav_to_torch
    rng = np.random.default_rng(width * 10 + channels)
    full = 2 ** (8 * width - 1)
    data = rng.integers(-full, full, size=(777, channels), dtype=np.int64)
    data[0], data[1] = -full, full - 1
    path = tmp_path / "a.wav"
    _write_wav(path, data, 44100 if channels == 1 else 48000, width)
    audio, rate = load_wav_to_torch(str(path))
    assert rate == (44100 if channels == 1 else 48000)
    assert audio.dtype == torch.float32 and tuple(audio.shape) == (777,)
    scaled = (data.astype(np.float64) / full).astype(np.float32)  # one rounding, as int -> float32 then a power of two
    want = torch.mean(torch.from_numpy(scaled.T.copy()), dim=0)
    assert torch.equal(audio, want)


def test_wav_reader_float32_and_refusals(tmp_path):
    from vcvits_amd.utils import load_wav_to_torch
    x = np.random.default_rng(3).standard_normal((100, 2)).astype("<f4")
    body = x.tobytes()
    fmt = struct.pack("<HHIIHH", 3, 2, 22050, 22050 * 8, 8, 32)
    riff = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    path = tmp_path / "f.wav"
    path.write_bytes(b"RIFF" + struct.pack("<I", len(riff)) + riff)
    audio, rate = load_wav_to_torch(str(path))
    assert rate == 22050 and torch.equal(audio, torch.mean(torch.from_numpy(x.T.copy()), dim=0))
    flac = tmp_path / "a.flac"
    flac.write_bytes(b"fLaC" + bytes(64))
    with pytest.raises(ValueError, match="not a RIFF/WAVE file"):
        load_wav_to_torch(str(flac))
    eight = tmp_path / "u8.wav"
    with wave.open(str(eight), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(1)
        f.setframerate(8000)
        f.writeframes(bytes(range(100)))
    with pytest.raises(ValueError, match="only WAV PCM 16 / 24 / 32-bit"):
        load_wav_to_torch(str(eight))


def test_reference_names_resolve_and_nothing_falls_back_to_the_cpu():
    from vits.data.audio import get_pitch, infer_inputs, load_audio, shift_audio
    from vits.utils import load_wav_to_torch
    import vcvits_amd.data.audio as A
    import vcvits_amd.utils as U
    assert load_audio is A.load_audio and shift_audio is A.shift_audio and get_pitch is A.get_pitch
    assert infer_inputs is A.infer_inputs and load_wav_to_torch is U.load_wav_to_torch is A.load_wav_to_torch
    x = torch.randn(4000)
    assert shift_audio(x, 16000, 0) is x
    from vcvits_amd import ops
    with pytest.raises(RuntimeError, match="not on the GPU"):
        ops.resample(x, 48000, 16000)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        ops.pitch_shift(x, 16000, 2)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        ops.phase_vocoder(torch.zeros(257, 10, dtype=torch.complex64), 0.9, 128)


def test_restated_pitch_shift_moves_the_pitch():
    """The GPU test's pitch assertion holds for the float64 restatement run through the float64 pYIN restatement: a 220 Hz
    tone shifted by +4 semitones tracks within one pYIN bin (10 cents) of 220 * 2 ** (4 / 12)."""
    import pyin_f64 as P
    sr, n_steps = 16000, 4
    y = R.pitch_shift(R.tone(sr, 220.0, seconds=1.0), sr, n_steps).numpy().astype(np.float32)
    f0, voiced = P.pyin(y)[:2]
    f0, voiced = np.asarray(f0)[3:-3], np.asarray(voiced)[3:-3]
    assert voiced.mean() > 0.9
    cents = 1200 * np.log2(np.median(f0[voiced]) / (220.0 * 2 ** (n_steps / 12)))
    print("restated pitch shift +%d: median f0 off by %.2f cents" % (n_steps, cents))
    assert abs(cents) <= 10.0

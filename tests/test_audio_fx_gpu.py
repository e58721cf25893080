"""GPU: sinc resampling, phase vocoder and pitch shift (csrc/audio_fx.hip) against the restatement of torchaudio
(tests/audio_fx_f64.py) on seeded synthetic signals -- the tap table, the resampler, the vocoder fed the restatement's own
spectrogram, pitch shift end to end, the pitch it produces, batch invariance and determinism, and the public surface
(load_audio / shift_audio / get_pitch / infer_inputs, the dataset's hooks).

Bounds: see each test.  Where the reference's float32 arithmetic is itself noisy (the vocoder's phase), the kernel is held
to twice the float32 restatement's own distance from the float64 run; both distances go to profiles/audio_fx_parity.txt."""
import math
import os
import wave

import numpy as np
import pytest
import torch

import audio_fx_f64 as R

pytestmark = pytest.mark.gpu

SR = 16000
RATIOS = [(48000, 16000), (44100, 16000), (22050, 16000), (16000, 48000), (16000, 44100), (16951, 16000), (15101, 16000)]
STEPS = [-12, -5, -1, 1, 7, 12]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_parity = {}


def _record(section, lines):
    """Keep the printed figures in profiles/audio_fx_parity.txt (rewritten with every section measured so far)."""
    for ln in lines[len(_parity.get(section, ())):]:
        print(ln)
    _parity[section] = list(lines)
    with open(os.path.join(ROOT, "profiles", "audio_fx_parity.txt"), "w") as f:
        f.write("# tests/test_audio_fx_gpu.py: distances from the float64 restatement (tests/audio_fx_f64.py), GPU kernels\n"
                "# next to the float32 restatement (the reference's own arithmetic).  Asserted: gpu <= 2 * ref32.\n")
        for name in sorted(_parity):
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def _ref_band(orig, new):
    """The restated float32 bank restricted to its band, for every phase: (first tap with |t| < 6 [n], taps [n, W], zero
    past the bank's last tap).  Each phase is evaluated on a window that starts before its band."""
    o, n, base, width = R.ratio(orig, new)
    W, K = R.band_bound(orig, new), 2 * width + o
    p = torch.arange(n)
    k0 = torch.floor(width + o * p.to(torch.float64) / n - R.LOWPASS_WIDTH * o / base).to(torch.int64) - 3
    k = k0[:, None] + torch.arange(W + 8)[None, :]
    valid = (k >= 0) & (k < K)
    kern, raw = R.sinc_taps(orig, new, p[:, None], k.clamp(0, K - 1), None)
    inside = valid & (raw.abs() < R.LOWPASS_WIDTH)
    pos = torch.argmax(inside.to(torch.int8), dim=1)
    rows = torch.arange(n)
    assert bool(inside.any(dim=1).all())
    assert bool(((pos > 0) | (k[:, 0] <= 0)).all()), "a window starts inside its band"
    assert bool((~inside[:, -1] | (k[:, -1] >= K - 1)).all()), "a window ends inside its band"
    first = k[rows, pos]
    idx = pos[:, None] + torch.arange(W)[None, :]
    assert int(idx.max()) < k.shape[1]
    taps = torch.where(valid.gather(1, idx), kern.gather(1, idx), torch.zeros((), dtype=torch.float32))
    return first, taps


@pytest.mark.parametrize("orig,new", RATIOS)
def test_tap_table(gpu, orig, new):
    """First-tap indices equal; |tap - ref| <= 2^-23 |ref| + 1e-14 (one float32 ulp for a flipped rounding of two float64
    evaluations that differ in the last place, plus the absolute error of sin near its zeros)."""
    from vcvits_amd import ops
    c, first, taps = ops.resample_table(gpu, orig, new)
    rfirst, rtaps = _ref_band(orig, new)
    assert tuple(taps.shape) == (c["W"], c["n"]) and tuple(first.shape) == (c["n"],)
    assert torch.equal(first.cpu().to(torch.int64), rfirst)
    got = taps.cpu().t().double()
    want = rtaps.double()
    err = (got - want).abs()
    differ = float((got != want).double().mean())
    print("%d -> %d: %d x %d taps, %.4f %% not bit-identical, largest |tap - ref| %.3e"
          % (orig, new, c["n"], c["W"], 100 * differ, float(err.max())))
    assert bool((err <= 2.0 ** -23 * want.abs() + 1e-14).all())


def _ragged(orig, seed):
    sig = list(R.signals(orig, seconds=0.25, seed=seed).values())
    full = len(sig[0])
    lens = [full, full - 137, full // 2 + 1, 1000]
    x = torch.zeros(len(sig), full)
    for i, (s, n) in enumerate(zip(sig, lens)):
        x[i, :n] = torch.from_numpy(s[:n])
    return x, lens


@pytest.mark.parametrize("orig,new", RATIOS)
def test_resample_against_float64_convolution(gpu, orig, new):
    """|y_gpu - y64| <= (W + 1) * 2^-24 * sum_k |tap_k| |x_k| per sample, y64 the float64 convolution of the same float32
    taps (the standard bound of a length-W FMA chain); zeros past each row's own length; output lengths exact."""
    from vcvits_amd import ops
    x, lens = _ragged(orig, seed=3)
    y = ops.resample(x.to(gpu), orig, new, lengths=lens).cpu()
    o, n, _, _ = R.ratio(orig, new)
    W = R.band_bound(orig, new)
    assert tuple(y.shape) == (len(lens), int(math.ceil(n * x.shape[1] / o)))
    worst = 0.0
    for i, ln in enumerate(lens):
        y64, a = R.resample(x[i, :ln], orig, new, dtype=torch.float64, kernel_dtype=None, terms=True)
        m = y64.shape[0]
        assert m == int(math.ceil(n * ln / o))
        assert not bool(y[i, m:].any())
        bound = (W + 1) * 2.0 ** -24 * a
        err = (y[i, :m].double() - y64).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (i, worst)
    print("%d -> %d: the kernel uses at most %.3f of the bound" % (orig, new, worst))


def _rate(n_steps):
    return 2.0 ** (-float(n_steps) / 12)


@pytest.fixture(scope="module")
def utterances():
    sig = R.signals(SR, seconds=1.0, seed=5)
    names = sorted(sig)
    return names, torch.stack([torch.from_numpy(sig[k]) for k in names])


def test_phase_vocoder_on_the_restated_spectrogram(gpu, utterances):
    """F' exact; magnitudes within 8 * 2^-24 * (|S0| + |S1|) of the float64 vocoder on the same float32 spectrogram; the
    magnitude-weighted phase distance d = sum mag |e^{i phi} - e^{i phi64}| per utterance satisfies d_gpu <= 2 * d_ref32."""
    from vcvits_amd import ops
    names, wavs = utterances
    hop = 128
    spec = R.stft(wavs, 512, torch.float32)  # complex64 [B, 257, F]
    assert spec.dtype == torch.complex64
    dev = spec.to(gpu)
    lines = []
    for n_steps in STEPS:
        rate = _rate(n_steps)
        out = ops.phase_vocoder(dev, rate, hop).cpu()
        adv = lambda dt: torch.linspace(0, math.pi * hop, 257, dtype=dt)[..., None]  # noqa: E731
        mag64, ph64 = R.phase_vocoder(spec, rate, adv(torch.float64), torch.float64, parts=True)
        mag32, ph32 = R.phase_vocoder(spec, rate, adv(torch.float32), torch.float32, parts=True)
        assert out.shape == mag64.shape and out.shape[-1] == len(R.time_steps(spec.shape[-1], rate))
        ts = R.time_steps(spec.shape[-1], rate)
        padded = torch.nn.functional.pad(spec, [0, 2]).abs().double()
        s0, s1 = padded.index_select(-1, ts.long()), padded.index_select(-1, (ts + 1).long())
        re, im = out.real.double(), out.imag.double()
        mag = torch.sqrt(re * re + im * im)
        assert bool(((mag - mag64).abs() <= 8 * 2.0 ** -24 * (s0 + s1)).all())
        unit64 = torch.polar(torch.ones_like(ph64), ph64)
        unit_gpu = torch.complex(re, im) / mag.clamp_min(1e-300)
        unit32 = torch.polar(torch.ones_like(ph64), ph32.double())
        d_gpu = (mag64 * (unit_gpu - unit64).abs()).sum(dim=(1, 2))
        d_ref = (mag64 * (unit32 - unit64).abs()).sum(dim=(1, 2))
        for i, name in enumerate(names):
            lines.append("n_steps %+3d %-6s d_gpu %.4e  d_ref32 %.4e  (sum of magnitudes %.4e)"
                         % (n_steps, name, float(d_gpu[i]), float(d_ref[i]), float(mag64[i].sum())))
        _record("phase vocoder: magnitude-weighted phase distance", lines)
        assert bool((d_gpu <= 2 * d_ref).all()), (n_steps, d_gpu.tolist(), d_ref.tolist())


def test_pitch_shift_end_to_end(gpu, utterances):
    """Relative RMS error against the float64 restatement: e_gpu <= 2 * e_ref32; output shape = input shape."""
    from vcvits_amd import ops
    names, wavs = utterances
    lines = []
    for n_steps in STEPS:
        y = ops.pitch_shift(wavs.to(gpu), SR, n_steps).cpu().double()
        assert y.shape == wavs.shape
        ref64 = R.pitch_shift(wavs, SR, n_steps, dtype=torch.float64)
        ref32 = R.pitch_shift(wavs, SR, n_steps, dtype=torch.float32).double()
        e_gpu = (y - ref64).norm(dim=1) / ref64.norm(dim=1)
        e_ref = (ref32 - ref64).norm(dim=1) / ref64.norm(dim=1)
        for i, name in enumerate(names):
            lines.append("n_steps %+3d %-6s e_gpu %.4e  e_ref32 %.4e" % (n_steps, name, float(e_gpu[i]), float(e_ref[i])))
        _record("pitch shift: relative RMS error", lines)
        assert bool((e_gpu <= 2 * e_ref).all()), (n_steps, e_gpu.tolist(), e_ref.tolist())


def test_pitch_shift_never_holds_the_dense_bank(gpu):
    """64 x 10 s at n_steps = +1 (16951 -> 16000, coprime): the peak stays below the live input, both spectrograms and the
    output plus the 4 * n * (W + 1) bytes of the table plus 16 MB (the dense bank alone would be 2 GB)."""
    from vcvits_amd import ops
    B, T, n_fft, hop = 64, 10 * SR, 512, 128
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(B, T, generator=g)).to(gpu)
    c = ops.resample_consts(ops.pitch_shift_consts(T, SR, 1)["orig_freq"], SR)
    assert (c["o"], c["n"]) == (16951, 16000)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = ops.pitch_shift(x, SR, 1)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    frames = T // hop + 1
    specs = 8 * B * (n_fft // 2 + 1) * (frames + ops.phase_vocoder_frames(frames, _rate(1)))
    budget = specs + 4 * B * T + 4 * c["n"] * (c["W"] + 1) + (16 << 20)  # the input is live before the measurement starts
    print("pitch_shift 64 x 10 s, +1: peak %.1f MB over the input, budget %.1f MB" % (peak / 2 ** 20, budget / 2 ** 20))
    assert y.shape == x.shape and peak <= budget, (peak, budget)


@pytest.mark.parametrize("n_steps", [-12, -7, 4, 12])
def test_it_shifts_pitch(gpu, n_steps):
    """A steady 220 Hz harmonic tone: the median voiced f0 (ops.pyin) of the interior frames of the shifted tone is within
    one pYIN bin (10 cents; 1e-3 cents for the float32 bin frequencies) of 220 * 2 ** (n_steps / 12)."""
    from vcvits_amd import ops
    x = torch.from_numpy(R.tone(SR, 220.0, seconds=1.0)).to(gpu)
    y = ops.pitch_shift(x, SR, n_steps)
    assert y.shape == x.shape
    f0, voiced, _, _, _ = ops.pyin(y.unsqueeze(0))
    f0, voiced = f0[0, 3:-3].cpu().numpy(), voiced[0, 3:-3].cpu().numpy()
    assert voiced.mean() > 0.9
    cents = 1200 * np.log2(np.median(f0[voiced]) / (220.0 * 2 ** (n_steps / 12)))
    print("pitch shift %+d: median f0 off by %.2f cents" % (n_steps, cents))
    assert abs(cents) <= 10.0 + 1e-3


def test_batch_invariance_and_determinism(gpu, utterances):
    from vcvits_amd import ops
    for orig, new in ((48000, 16000), (16000, 44100), (16951, 16000)):
        x, lens = _ragged(orig, seed=7)
        xd = x.to(gpu)
        y = ops.resample(xd, orig, new, lengths=lens)
        assert torch.equal(y, ops.resample(xd, orig, new, lengths=lens))
        for i, ln in enumerate(lens):
            alone = ops.resample(xd[i, :ln].clone(), orig, new)
            assert torch.equal(y[i, :alone.shape[0]], alone) and not bool(y[i, alone.shape[0]:].any())
    _, wavs = utterances
    wd = wavs.to(gpu)
    for n_steps in (1, -5):
        y = ops.pitch_shift(wd, SR, n_steps)
        assert torch.equal(y, ops.pitch_shift(wd, SR, n_steps))
        for i in range(wd.shape[0]):
            assert torch.equal(y[i], ops.pitch_shift(wd[i].clone(), SR, n_steps))


def _stereo_wav(path, rate=48000, seconds=1.0):
    left, right = R.tone(rate, 220.0, seconds, seed=1), R.tone(rate, 220.0, seconds, seed=2)
    data = np.stack([left, right], axis=1)
    pcm = np.clip(np.rint(data * 32767), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    return torch.mean(torch.from_numpy((pcm.astype(np.float32) / np.float32(32768)).T.copy()), dim=0)


def test_public_surface(gpu, tmp_path):
    from vcvits_amd import ops
    from vits.data.audio import coarse_f0, estimate_pitch, get_pitch, infer_inputs, load_audio, shift_audio
    from vits.data.dataset.vc_ms import VoiceConversionMultiSpeakerDataset, cache_paths
    from vits.hparams import HParams
    path = str(tmp_path / "utt.wav")
    decoded = _stereo_wav(path)
    for sr in (None, 48000):
        got = load_audio(path, sr=sr)
        assert got.device.type == "cpu" and torch.equal(got, decoded)
    at16 = load_audio(path, sr=16000)
    assert at16.device.type == "cpu" and torch.equal(at16, ops.resample(decoded.to(gpu), 48000, 16000).cpu())
    assert at16.shape[0] == 16000
    want = coarse_f0(estimate_pitch(at16, 16000, 2048, 2048, 320), f0_bin=512)
    pitch = get_pitch(path, 2048, 2048, 512, sr=16000)
    assert pitch.device.type == "cpu" and torch.equal(pitch, want) and pitch.shape[0] == 1
    # device in, device out; host in, host out
    shifted = shift_audio(at16, 16000, 3)
    assert shifted.device.type == "cpu" and shifted.shape == at16.shape
    on_dev = shift_audio(at16.to(gpu), 16000, 3)
    assert on_dev.is_cuda and torch.equal(on_dev.cpu(), shifted)
    hp = HParams(source_sampling_rate=16000, target_sampling_rate=48000, filter_length=2048, win_length=2048, num_pitch=512,
                 hop_length=320)
    audio_norm, classes = infer_inputs(hp, path, sr=16000, pitch_shift=3)
    assert torch.equal(audio_norm, at16.unsqueeze(0))
    assert torch.equal(classes, coarse_f0(estimate_pitch(shifted, 16000, 2048, 2048, 320)))
    assert not torch.equal(classes, coarse_f0(estimate_pitch(at16, 16000, 2048, 2048, 320)))
    # the dataset fills its cache through the package's own functions and reads it back without them
    cache = tmp_path / "cache"
    cache.mkdir()
    item = VoiceConversionMultiSpeakerDataset([[path, "3"]], hp, str(cache), load_audio=load_audio, get_pitch=get_pitch)[0]
    assert item["sid"] == 3 and torch.equal(item["x_wav"], at16.unsqueeze(0)) and torch.equal(item["x_pitch"], want)
    assert torch.equal(item["y_wav"], decoded.unsqueeze(0))
    assert all(os.path.exists(p) for p in cache_paths(str(cache), path, hp))
    again = VoiceConversionMultiSpeakerDataset([[path, "3"]], hp, str(cache))[0]
    assert all(torch.equal(again[k], item[k]) for k in ("x_wav", "x_pitch", "y_wav"))

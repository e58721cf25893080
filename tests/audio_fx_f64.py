"""Restatement of torchaudio's resampling, phase vocoder and pitch shift as the reference calls them (test oracle only).

The reference resamples with `torchaudio.transforms.Resample(orig, new)` and shifts pitch with
`torchaudio.functional.pitch_shift` (torchaudio 2.0.1; vits/data/audio.py:95-107,158-180, infer.py:39-46).  torchaudio is not
a dependency of this project, so this file restates `_get_sinc_resample_kernel`, `_apply_sinc_resample_kernel`,
`phase_vocoder` and `pitch_shift` step by step over torch-CPU; parity with torchaudio itself is UNPINNED (DESIGN 3.1,
unpinned #6).  It shares no code with vcvits_amd/ops/audio_fx.py.  Every function takes the dtype it computes in, so the same
text runs in float64 (the yardstick) and in float32 (what the reference computes).

Points decided here (the kernels follow this file):
 1. `transforms.Resample` forms its bank with dtype=None: float64 throughout, rounded once to float32, and `-p / n` is the
    true division of an int64 tensor (float32) before it meets the float64 tap positions.  That is `sinc_taps(dtype=None)` and
    what the product's table holds.  `functional.resample` (the call inside pitch_shift) forms the bank in the waveform's
    dtype instead, without the float64 detour: `sinc_taps(dtype=torch.float32 / torch.float64)`, used by `pitch_shift` below.
    The product uses the once-rounded float64 bank there too, which is the closer of the two to exact arithmetic.
 2. width = ceil(6 * o / base), left pad width, right pad width + o, output length ceil(n * L / o).
 3. The vocoder's time steps are float32(s * rate) with the product formed in double (torch.arange on the CPU) whatever the
    dtype of the run: the float64 yardstick differs from the reference in rounding only, not in its time grid.  alpha, floor(ts)
    and (ts + 1).long() (the float32 sum, truncated) come from that float32 value.
 4. int(sample_rate / rate) truncates; round(T / rate) is Python's round; torch.istft(length=) keeps the overlap-add's tail
    past hop * (F' - 1) (up to n_fft / 2 more samples) and zero-fills only past that.
 5. Taps with |t| >= 6 before clamping are exactly zero once rounded to float32 from float64 (test_audio_fx_cpu.py asserts
    it); formed in float32 they are below 1e-20.  A bank too large to hold ([16000, 1, 33916] for one semitone at 16 kHz) is
    therefore evaluated on the band of each output sample only (`resample(..., dense=False)`).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LOWPASS_WIDTH = 6
ROLLOFF = 0.99
DENSE_LIMIT = 1 << 24  # bank elements up to which the dense conv1d is run


def ratio(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_WIDTH * o / base)
    return o, n, base, width


def band_bound(orig_freq, new_freq):
    """Upper bound on the taps of one phase with |t| < 6: an open interval of length 12 * o / base, plus one for rounding."""
    o, n, base, width = ratio(orig_freq, new_freq)
    return min(2 * width + o, int(math.floor(2 * LOWPASS_WIDTH * o / base)) + 2)


def sinc_taps(orig_freq, new_freq, p, k, dtype=None):
    """_get_sinc_resample_kernel's arithmetic for phases p and tap indices k (int64 tensors, broadcast against each other;
    torchaudio takes p = arange(n)[:, None] and k = arange(2 * width + o)).  Returns (taps, t before clamping)."""
    o, n, base, width = ratio(orig_freq, new_freq)
    idx_dtype = dtype if dtype is not None else torch.float64
    idx = (k - width).to(idx_dtype) / o
    neg_p = -p if dtype is None else (-p).to(dtype)
    t = neg_p / n + idx  # dtype None: int64 / int -> float32, promoted to float64 by the sum
    t = t * base
    raw = t.clone()
    t = t.clamp(-LOWPASS_WIDTH, LOWPASS_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_WIDTH / 2) ** 2
    t = t * math.pi
    scale = base / o
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels = kernels * (window * scale)
    if dtype is None:
        kernels = kernels.to(torch.float32)
    return kernels, raw


def sinc_kernel(orig_freq, new_freq, dtype=None, phases=None):
    """The dense bank [n (or len(phases)), 1, 2 * width + o], its width, and t before clamping."""
    o, n, base, width = ratio(orig_freq, new_freq)
    p = torch.arange(n) if phases is None else torch.as_tensor(phases, dtype=torch.int64)
    k = torch.arange(2 * width + o)
    kern, raw = sinc_taps(orig_freq, new_freq, p[:, None], k[None, :], dtype)
    return kern[:, None, :], width, raw


def band_of(raw):
    """(first tap with |t| < 6, number of such taps) per row of t [rows, taps]."""
    inside = raw.abs() < LOWPASS_WIDTH
    first = torch.argmax(inside.to(torch.int8), dim=1)
    return first, inside.sum(dim=1)


def _band_windows(orig_freq, new_freq, j, length):
    """For output samples j: (phase p, tap indices k [len(j), Wb], valid mask, index of each tap's input sample)."""
    o, n, base, width = ratio(orig_freq, new_freq)
    i, p = j // n, j % n
    k0 = torch.floor(width + o * p.to(torch.float64) / n - LOWPASS_WIDTH * o / base).to(torch.int64) - 3
    k = k0[:, None] + torch.arange(band_bound(orig_freq, new_freq) + 6)[None, :]
    src = i[:, None] * o + k - width
    ok = (k >= 0) & (k < 2 * width + o) & (src >= 0) & (src < length)
    return p, k, ok, src


def resample(wave, orig_freq, new_freq, dtype=torch.float64, kernel_dtype=None, dense=None, terms=False):
    """_apply_sinc_resample_kernel over the bank sinc_taps(dtype=kernel_dtype): wave [L] -> [ceil(n * L / o)], computed in
    `dtype`.  dense: run F.conv1d over the full bank (default when it holds at most DENSE_LIMIT elements); otherwise each
    output sample sums the taps of its band.  terms=True also returns sum_k |tap_k| |x_k| per output sample."""
    o, n, base, width = ratio(orig_freq, new_freq)
    x = torch.as_tensor(wave).to(dtype)
    length = x.shape[0]
    target = int(math.ceil(n * length / o))
    if int(orig_freq) == int(new_freq):
        return (x, x.abs()) if terms else x
    if dense is None:
        dense = n * (2 * width + o) <= DENSE_LIMIT
    if dense:
        kern = sinc_kernel(orig_freq, new_freq, kernel_dtype)[0].to(dtype)
        xp = F.pad(x[None], (width, width + o))
        y = F.conv1d(xp[:, None], kern, stride=o).transpose(1, 2).reshape(1, -1)[0, :target]
        if terms:
            a = F.conv1d(xp[:, None].abs(), kern.abs(), stride=o).transpose(1, 2).reshape(1, -1)[0, :target]
            return y, a
        return y
    y = torch.empty(target, dtype=dtype)
    a = torch.empty(target, dtype=dtype)
    for lo in range(0, target, 1 << 16):
        j = torch.arange(lo, min(target, lo + (1 << 16)))
        p, k, ok, src = _band_windows(orig_freq, new_freq, j, length)
        taps = sinc_taps(orig_freq, new_freq, p[:, None], k, kernel_dtype)[0].to(dtype)
        xs = torch.where(ok, x[src.clamp(0, length - 1)], torch.zeros((), dtype=dtype))
        taps = torch.where(ok, taps, torch.zeros((), dtype=dtype))
        y[lo:lo + len(j)] = (taps * xs).sum(dim=1)
        a[lo:lo + len(j)] = (taps.abs() * xs.abs()).sum(dim=1)
    return (y, a) if terms else y


def time_steps(n_frames, rate):
    """torch.arange(0, n_frames, rate, dtype=float32) on the CPU: ceil(n_frames / rate) values float32(s * rate)."""
    count = int(math.ceil(n_frames / rate))
    return torch.from_numpy((np.arange(count, dtype=np.float64) * float(rate)).astype(np.float32))


def phase_vocoder(spec, rate, phase_advance, dtype=torch.float64, parts=False):
    """torchaudio.functional.phase_vocoder: spec complex [..., n_freq, F], phase_advance [n_freq, 1] -> [..., n_freq, F'].
    parts=True returns (magnitude, accumulated phase) instead of polar(magnitude, phase)."""
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    spec = torch.as_tensor(spec).to(cdtype)
    phase_advance = torch.as_tensor(phase_advance).to(dtype)
    if rate == 1.0:
        return spec
    ts = time_steps(spec.shape[-1], rate)  # float32, whatever dtype
    alphas = (ts % 1.0).to(dtype)
    phase_0 = spec[..., :1].angle()
    spec = F.pad(spec, [0, 2])
    spec_0 = spec.index_select(-1, ts.long())
    spec_1 = spec.index_select(-1, (ts + 1).long())
    angle_0, angle_1 = spec_0.angle(), spec_1.angle()
    norm_0, norm_1 = spec_0.abs(), spec_1.abs()
    phase = angle_1 - angle_0 - phase_advance
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = phase + phase_advance
    phase = torch.cat([phase_0, phase[..., :-1]], dim=-1)
    phase_acc = torch.cumsum(phase, -1)
    mag = alphas * norm_1 + (1 - alphas) * norm_0
    if parts:
        return mag, phase_acc
    return torch.polar(mag, phase_acc)


def stft(wave, n_fft=512, dtype=torch.float64):
    """pitch_shift's forward transform: hop n_fft // 4, Hann window of n_fft, center=True, reflect padding."""
    x = torch.as_tensor(wave).to(dtype)
    return torch.stft(x, n_fft, n_fft // 4, n_fft, window=torch.hann_window(n_fft, dtype=dtype), center=True,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)


def pitch_shift(wave, sample_rate, n_steps, bins_per_octave=12, n_fft=512, dtype=torch.float64, stages=False):
    """torchaudio.functional.pitch_shift(wave [..., T], sample_rate, n_steps) computed in `dtype`."""
    x = torch.as_tensor(wave).to(dtype)
    shape = x.shape
    x = x.reshape(-1, shape[-1])
    hop = n_fft // 4
    ori_len = shape[-1]
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    spec = stft(x, n_fft, dtype)
    phase_advance = torch.linspace(0, math.pi * hop, spec.shape[-2], dtype=dtype)[..., None]
    stretched = phase_vocoder(spec, rate, phase_advance, dtype)
    len_stretch = int(round(ori_len / rate))
    y = torch.istft(stretched, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, dtype=dtype),
                    length=len_stretch)
    orig = int(sample_rate / rate)
    rows = [resample(r, orig, sample_rate, dtype=dtype, kernel_dtype=dtype) for r in y]
    out = torch.zeros((len(rows), ori_len), dtype=dtype)
    for i, r in enumerate(rows):
        keep = min(ori_len, r.shape[0])
        out[i, :keep] = r[:keep]
    out = out.reshape(shape)
    if stages:
        return out, {"rate": rate, "spec": spec, "stretched": stretched, "len_stretch": len_stretch, "orig_freq": orig,
                     "istft": y}
    return out


# ---- seeded test signals (shared by the CPU and GPU tests) ----------------------------------------------------------
def _harmonic(f_inst, sr, amp, rng, n_harm=5):
    phase = 2 * np.pi * np.cumsum(f_inst) / sr
    return amp * sum((0.6 ** h) * np.sin((h + 1) * phase + rng.uniform(0, 2 * np.pi)) for h in range(n_harm))


def signals(sr, seconds=1.0, seed=0, floor=1e-3):
    """{name: float32 [T]}: a vowel with vibrato, a glide, tones with silence gaps, white noise; each over a noise floor of
    `floor` of full scale, so that no STFT bin is exactly zero."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    tt = np.arange(n) / sr
    out = {}
    f = 160 * (1 + 0.02 * np.sin(2 * np.pi * 5.5 * tt)) * (1 + 0.004 * rng.standard_normal(n))
    out["vowel"] = _harmonic(f, sr, 0.25, rng)
    out["glide"] = _harmonic(90 * (700 / 90) ** (tt / tt[-1]), sr, 0.3, rng)
    gaps = _harmonic(np.where(tt < 0.5 * seconds, 220.0, 330.0), sr, 0.3, rng)
    gaps[(tt > 0.3 * seconds) & (tt < 0.45 * seconds)] = 0.0
    gaps[tt > 0.85 * seconds] = 0.0
    out["gaps"] = gaps
    out["noise"] = 0.1 * rng.standard_normal(n)
    return {k: np.asarray(v + floor * rng.standard_normal(n), dtype=np.float32) for k, v in out.items()}


def tone(sr, f0, seconds=1.0, seed=0, floor=1e-3):
    """A steady harmonic tone at f0 over the noise floor."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    return np.asarray(_harmonic(np.full(n, float(f0)), sr, 0.3, rng) + floor * rng.standard_normal(n), dtype=np.float32)

"""Resampling, phase vocoder and pitch shift (csrc/audio_fx.hip): torchaudio.transforms.Resample with its defaults and
torchaudio.functional.pitch_shift as the reference's load_audio / shift_audio / infer.py call them (vits/data/audio.py:158-180,
infer.py:36-48), batched.

Part of `vcvits_amd.ops` (the package re-exports every name: `from vcvits_amd import ops; ops.resample(...)`).  The band of
the sinc filter bank is built on the device once per rate pair (n * W taps, never the dense [n, 2 * width + o] bank); every
launch goes to libvcvits_hip.so on the current stream.  There is no CPU fallback: CPU tensors raise."""
import math

import torch

from .._lib import check, lib, ptr, stream
from .stft import _stft_consts, stft_complex

RESAMPLE_LOWPASS_WIDTH = 6
RESAMPLE_ROLLOFF = 0.99
_resample_dev = {}
_pv_advance = {}


def resample_consts(orig_freq, new_freq):
    """torchaudio's derived constants of a rate pair, plus the band width W of the device table: o, n (rates over their gcd),
    base = min(o, n) * 0.99, width = ceil(6 * o / base), n_taps = 2 * width + o (the dense bank's row), and
    W = floor(12 * o / base) + 2 >= the taps k of any phase with |t| < 6 (an open interval of length 12 * o / base holds at most
    floor(.) + 1 integers; one more for the rounding of its ends)."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("resample: positive integer rates expected, got %r -> %r" % (orig_freq, new_freq))
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * RESAMPLE_ROLLOFF
    width = math.ceil(RESAMPLE_LOWPASS_WIDTH * o / base)
    n_taps = 2 * width + o
    W = min(n_taps, int(math.floor(2 * RESAMPLE_LOWPASS_WIDTH * o / base)) + 2)
    return {"o": o, "n": n, "base": base, "width": width, "n_taps": n_taps, "W": W}


def resample_out_len(n_samples, orig_freq, new_freq):
    """ceil(new * n_samples / orig): samples torchaudio keeps of a row of n_samples."""
    c = resample_consts(orig_freq, new_freq)
    return -((-c["n"] * int(n_samples)) // c["o"])


def resample_table(device, orig_freq, new_freq):
    """(consts, first int32 [n], taps float32 [W, n]) on `device`, built by the table kernel once per rate pair and device."""
    c = resample_consts(orig_freq, new_freq)
    key = (str(device), c["o"], c["n"])
    if key not in _resample_dev:
        if torch.device(device).type != "cuda":
            raise RuntimeError("vcvits_amd: the resampling table is not on the GPU; the HIP path has no CPU fallback")
        first = torch.empty((c["n"],), dtype=torch.int32, device=device)
        taps = torch.empty((c["W"], c["n"]), dtype=torch.float32, device=device)
        with torch.cuda.device(first.device):
            check(lib().vcv_resample_table(c["o"], c["n"], c["width"], c["W"], c["base"], ptr(first), ptr(taps), stream()),
                  "vcv_resample_table")
        _resample_dev[key] = (c, first, taps)
    return _resample_dev[key]


def _fx_gpu(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("vcvits_amd: %s is not on the GPU; the HIP path has no CPU fallback" % what)
    return t.detach().contiguous()


def _fx_rows(wav, what):
    """float32 [B, T] view of a [T] or [B, T] device waveform, and whether it was 1-D."""
    wav = _fx_gpu(wav, what)
    flat = wav.dim() == 1
    if flat:
        wav = wav.unsqueeze(0)
    if wav.dim() != 2 or wav.dtype != torch.float32 or wav.shape[1] < 1:
        raise ValueError("%s must be a non-empty float32 [B, T] or [T] tensor" % what)
    return wav, flat


def _resample_rows(x, lens, orig_freq, new_freq, out_len):
    """x [B, T] -> [B, out_len]: the resampled rows, zero from ceil(n * len / o) on (cut or padded to out_len)."""
    c, first, taps = resample_table(x.device, orig_freq, new_freq)
    B, T = x.shape
    if max(T, out_len) >= 2 ** 31 - 1024:  # sample indices are 32-bit in the kernel (their products with o and n 64-bit)
        raise NotImplementedError("resample: rows of %d -> %d samples overflow the kernel's indices" % (T, out_len))
    y = torch.empty((B, out_len), dtype=torch.float32, device=x.device)
    status = lib().vcv_resample_apply(ptr(x), ptr(lens), ptr(y), B, T, out_len, c["o"], c["n"], c["width"], c["W"],
                                      ptr(first), ptr(taps), stream())
    if status == -1 and c["o"] > 32 * c["n"]:  # VCV_EINVAL from the launcher's LDS check
        raise NotImplementedError("resample: %d -> %d decimates by more than the kernel's LDS tile holds" % (orig_freq, new_freq))
    check(status, "vcv_resample_apply")
    return y


def resample(wav, orig_freq, new_freq, lengths=None):
    """torchaudio.transforms.Resample(orig_freq, new_freq)(wav) (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) of each
    row of wav [B, T] (or [T]) float32 on the GPU at its own length (`lengths`, default T, as ops.pyin takes them):
    [B, ceil(new * T / orig)], zeros past a row's own ceil(new * length / orig).  Equal rates return `wav` itself."""
    if int(orig_freq) == int(new_freq):
        resample_consts(orig_freq, new_freq)
        _fx_gpu(wav, "wav")
        return wav
    x, flat = _fx_rows(wav, "wav")
    B, T = x.shape
    lens = None
    if lengths is not None:
        ns = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(ns) != B or any(v < 0 or v > T for v in ns):
            raise ValueError("resample: %d lengths for %d rows of %d samples, or one outside [0, T]" % (len(ns), B, T))
        lens = torch.tensor(ns, dtype=torch.int32).to(x.device, non_blocking=True)
    y = _resample_rows(x, lens, orig_freq, new_freq, resample_out_len(T, orig_freq, new_freq))
    return y[0] if flat else y


def phase_vocoder_frames(n_frames, rate):
    """len(torch.arange(0, n_frames, rate)): ceil(n_frames / rate) in double."""
    return int(math.ceil(n_frames / rate))


def phase_vocoder(spec, rate, hop_length):
    """torchaudio.functional.phase_vocoder(spec, rate, linspace(0, pi * hop_length, n_freq)[:, None]): complex64
    [B, n_freq, F] (or [n_freq, F]) on the GPU -> [B, n_freq, ceil(F / rate)].  The phase is accumulated in float64
    (torchaudio's float32 cumsum is the noisier of the two).  rate 1 returns `spec` itself, as torchaudio does."""
    spec = _fx_gpu(spec, "spec")
    rate = float(rate)
    if not rate > 0.0:
        raise ValueError("phase_vocoder: rate must be positive, got %r" % (rate,))
    if rate == 1.0:
        return spec
    flat = spec.dim() == 2
    if flat:
        spec = spec.unsqueeze(0)
    if spec.dim() != 3 or spec.dtype != torch.complex64:
        raise ValueError("phase_vocoder: complex64 [B, n_freq, F] or [n_freq, F] expected")
    B, NF, F_ = spec.shape
    key = (str(spec.device), NF, int(hop_length))
    if key not in _pv_advance:
        _pv_advance[key] = torch.linspace(0, math.pi * int(hop_length), NF).to(spec.device)
    Fo = phase_vocoder_frames(F_, rate)
    s = torch.view_as_real(spec).contiguous()
    out = torch.empty((B, NF, Fo, 2), dtype=torch.float32, device=spec.device)
    check(lib().vcv_phase_vocoder(ptr(s), ptr(out), ptr(_pv_advance[key]), B, NF, F_, Fo, rate, stream()), "vcv_phase_vocoder")
    out = torch.view_as_complex(out)
    return out[0] if flat else out


def istft_ordered(spec, n_fft, length):
    """torch.istft(spec, n_fft, hop_length=n_fft // 4, window=hann(n_fft), center=True, length=length) of complex64
    [B, n_fft / 2 + 1, F] -> [B, length] (zeros past the overlap-add's end), bit-reproducible: frames are summed in order, where
    ops.istft adds them with atomics."""
    s = torch.view_as_real(_fx_gpu(spec, "spec")).contiguous()
    if s.dim() != 4 or s.dtype != torch.float32 or s.shape[1] != n_fft // 2 + 1:
        raise ValueError("istft_ordered: complex64 [B, n_fft / 2 + 1, F] expected")
    if n_fft < 64 or n_fft > 1024 or n_fft & (n_fft - 1):
        raise NotImplementedError("istft_ordered: n_fft a power of two in [64, 1024] (pitch_shift's default: 512)")
    B, _, F_, _ = s.shape
    win, tw = _stft_consts(s.device, n_fft)
    out = torch.empty((B, int(length)), dtype=torch.float32, device=s.device)
    check(lib().vcv_istft_ordered(ptr(s), ptr(win), ptr(tw), ptr(out), B, F_, n_fft, int(length), stream()), "vcv_istft_ordered")
    return out


def pitch_shift_consts(T, sample_rate, n_steps, bins_per_octave=12):
    """torchaudio.functional.pitch_shift's derived numbers: rate = 2 ** (-n_steps / bins_per_octave), the stretched length
    round(T / rate) (Python's round) and the rate int(sample_rate / rate) (truncated) it is resampled from."""
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    return {"rate": rate, "len_stretch": int(round(T / rate)), "orig_freq": int(sample_rate / rate)}


def pitch_shift(wav, sample_rate, n_steps, bins_per_octave=12, n_fft=512):
    """torchaudio.functional.pitch_shift(wav, sample_rate, n_steps, bins_per_octave, n_fft) with its default window and hop
    (n_fft // 4): wav [B, T] (or [T]) float32 on the GPU -> the same shape.  STFT, phase vocoder, inverse STFT to round(T / rate)
    samples, resampling from int(sample_rate / rate) to sample_rate over the band table, cut or zero-padded to T.  Rows share
    T and n_steps."""
    x, flat = _fx_rows(wav, "wav")
    B, T = x.shape
    if T <= n_fft // 2:
        raise ValueError("pitch_shift: %d samples cannot be reflect-padded by n_fft / 2 = %d" % (T, n_fft // 2))
    hop = n_fft // 4
    c = pitch_shift_consts(T, sample_rate, n_steps, bins_per_octave)
    if c["len_stretch"] < 1 or c["orig_freq"] < 1:
        raise ValueError("pitch_shift: n_steps=%r leaves no samples" % (n_steps,))
    spec = stft_complex(x, n_fft=n_fft, hop=hop, pad=n_fft // 2, reflect=True)
    stretched = phase_vocoder(spec, c["rate"], hop)
    del spec
    y = istft_ordered(stretched, n_fft, c["len_stretch"])
    del stretched
    if c["orig_freq"] == int(sample_rate):  # nothing to resample: cut or pad (n_steps = 0, or a step too small to matter)
        out = torch.zeros((B, T), dtype=torch.float32, device=x.device)
        keep = min(T, y.shape[1])
        out[:, :keep] = y[:, :keep]
    else:
        out = _resample_rows(y, None, c["orig_freq"], int(sample_rate), T)
    return out[0] if flat else out

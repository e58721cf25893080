"""Audio loading, resampling, pitch shift, pitch estimation, pitch binning and inference plumbing of the data path
(reference: vits/data/audio.py:17-76,158-239, infer.py:36-62,81).

`estimate_pitch(method='pyin')` runs librosa.pyin's algorithm as HIP kernels (vcvits_amd/ops/pitch.py, csrc/pyin.hip); the
pitch classes the model is conditioned on are `coarse_f0` of its result.  `load_audio` / `get_pitch` decode WAV files on the
host (`vcvits_amd.utils.load_wav_to_torch`) and resample on the GPU; `shift_audio` is torchaudio's pitch_shift on the GPU
(vcvits_amd/ops/audio_fx.py, csrc/audio_fx.hip).  torchaudio is not a dependency."""
import math

import numpy as np
import torch

from ..utils import load_wav_to_torch


def coarse_f0(f0, f0_min=50.0, f0_max=1100.0, f0_bin=512):
    """Hz -> integer pitch class in [1, f0_bin-1] on a mel scale (vits/data/audio.py:65-76): voiced frames map
    linearly in mel between f0_min and f0_max onto [1, f0_bin-1]; unvoiced (f0 = 0 -> mel 0) and anything that
    lands at or below 1 become class 1; values past the top class saturate; half-to-even rounding (torch.round).
    Returns a float tensor of whole numbers, as the reference does (callers cast with .long())."""
    f0 = torch.as_tensor(f0, dtype=torch.float32)
    mel_min = 1127.0 * math.log(1.0 + f0_min / 700.0)
    mel_max = 1127.0 * math.log(1.0 + f0_max / 700.0)
    mel = 1127.0 * torch.log(1.0 + f0 / 700.0)
    scaled = (mel - mel_min) * (f0_bin - 2) / (mel_max - mel_min) + 1.0
    mel = torch.where(mel > 0, scaled, mel)
    mel = torch.clamp(mel, min=1.0, max=float(f0_bin - 1))
    out = torch.round(mel)
    if out.numel() and not (float(out.max()) < f0_bin and float(out.min()) >= 1):
        raise AssertionError((float(out.max()), float(out.min())))
    return out


def infer_length_scale(data_hparams):
    """Frames of the target rate per source sample (infer.py:81): the `length_scale` handed to
    SynthesizerSVC.infer so the content features (source rate / 320) are resampled to target frames."""
    return (data_hparams.target_sampling_rate / data_hparams.hop_length) / data_hparams.source_sampling_rate


def normalize_pitch(pitch, mean, std):
    """In place, zeros kept (vits/data/audio.py:17-22)."""
    zeros = (pitch == 0.0)
    pitch -= mean[:, None]
    pitch /= std[:, None]
    pitch[zeros] = 0.0
    return pitch


def _pitch_args(sr, n_fft, win_length, hop_length, method, n_formants):
    if method != "pyin":
        raise ValueError("estimate_pitch: method=%r (only 'pyin', as the reference)" % (method,))
    if n_formants > 1:
        raise NotImplementedError("estimate_pitch: n_formants > 1 (the reference raises too)")
    from ..ops.pitch import pyin_consts, _pyin_check_consts
    _pyin_check_consts(pyin_consts(int(sr), int(win_length), int(hop_length)), int(win_length))
    return int((n_fft - hop_length) / 2)


def _as_wave(audio):
    """1-D float32 tensor; host arrays are checked for finite samples here (device ones by the kernel's flag)."""
    on_device = isinstance(audio, torch.Tensor) and audio.is_cuda
    if isinstance(audio, torch.Tensor):
        x = audio.detach()
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(audio, dtype=np.float32)))
    if x.dim() != 1:
        raise ValueError("estimate_pitch: a 1-D waveform expected, got shape %s" % (tuple(x.shape),))
    x = x.to(torch.float32)
    if not on_device and not bool(torch.isfinite(x).all()):
        raise ValueError("estimate_pitch: audio buffer is not finite everywhere")
    return x, on_device


def estimate_pitch(audio, sr, n_fft, win_length, hop_length, method="pyin", normalize_mean=None, normalize_std=None,
                   n_formants=1):
    """librosa.pyin(frame_length=win_length, hop_length, fmin=C2, fmax=C7, center=False) of `audio` reflect-padded by
    int((n_fft - hop_length) / 2), unvoiced frames 0 (vits/data/audio.py:24-63).  1-D numpy array or tensor in; float32
    [1, F] out, on the CPU for host input and on the input's device for device input.  The pitch tracking runs on the
    GPU either way (there is no CPU path)."""
    if type(normalize_mean) is float or type(normalize_mean) is list:
        normalize_mean = torch.tensor(normalize_mean)
    if type(normalize_std) is float or type(normalize_std) is list:
        normalize_std = torch.tensor(normalize_std)
    pad = _pitch_args(sr, n_fft, win_length, hop_length, method, n_formants)
    x, on_device = _as_wave(audio)
    from ..ops.pitch import pyin, pyin_lengths
    pyin_lengths(None, 1, x.shape[0], int(win_length), int(hop_length), pad)  # too short: ValueError before any device work
    dev = x.device if on_device else torch.device("cuda", torch.cuda.current_device())
    f0, _, _, _, _ = pyin(x.to(dev).unsqueeze(0), sr=int(sr), frame_length=int(win_length), hop_length=int(hop_length),
                          pad=pad)
    pitch = f0 if on_device else f0.cpu()
    if normalize_mean is not None:
        assert normalize_std is not None
        pitch = normalize_pitch(pitch, normalize_mean.to(pitch.device), normalize_std.to(pitch.device))
    return pitch


def pitch_classes(wav, lengths, sr, n_fft, win_length, hop_length=320, f0_bin=512):
    """Batched `coarse_f0(estimate_pitch(wav[b, :lengths[b]], ...), f0_bin)`: wav [B, T] (or [B, 1, T]) on the GPU, each row
    framed at its own length.  Returns (classes float32 [B, Fmax] on wav's device, whole numbers, 0 past a row's frames;
    frames per row, CPU int64 [B])."""
    pad = _pitch_args(sr, n_fft, win_length, hop_length, "pyin", 1)
    if wav.dim() == 3 and wav.shape[1] == 1:
        wav = wav[:, 0]
    from ..ops.pitch import pyin
    _, _, _, cls, n_frames = pyin(wav, lengths, sr=int(sr), frame_length=int(win_length), hop_length=int(hop_length),
                                  pad=pad, f0_bin=int(f0_bin))
    return cls, n_frames


def _current_gpu():
    return torch.device("cuda", torch.cuda.current_device())


def _load_at(filename, sr):
    """(samples on the CPU, or on the GPU when they were resampled there; their rate)."""
    audio, sampling_rate = load_wav_to_torch(filename)
    if sr is not None and sampling_rate != sr:
        from ..ops.audio_fx import resample
        return resample(audio.to(_current_gpu()), sampling_rate, int(sr)), int(sr)
    return audio, sampling_rate


def load_audio(filename, sr=None):
    """Decoded samples of a WAV file (channels averaged), resampled to `sr` when it is given and differs from the file's rate
    (vits/data/audio.py:158-172).  1-D float32 on the CPU, as the reference returns it; the resampling runs on the GPU."""
    return _load_at(filename, sr)[0].cpu()


def shift_audio(audio, sr=None, pitch_shift=0):
    """torchaudio.functional.pitch_shift(audio, sr, pitch_shift), or `audio` itself for pitch_shift = 0
    (vits/data/audio.py:174-180).  [T] or [B, T] float32; a CPU tensor comes back on the CPU, a device tensor stays on its
    device.  The shift runs on the GPU either way (there is no CPU path)."""
    if pitch_shift == 0:
        return audio
    if sr is None:
        raise ValueError("shift_audio: a sampling rate is needed to shift the pitch")
    from ..ops.audio_fx import pitch_shift as _shift
    x = torch.as_tensor(audio)
    if x.is_cuda:
        return _shift(x.to(torch.float32), int(sr), pitch_shift)
    return _shift(x.to(torch.float32).to(_current_gpu()), int(sr), pitch_shift).cpu()


def get_pitch(filename, filter_length, win_length, num_pitch, sr=None):
    """Pitch classes [1, F] of a WAV file at rate `sr` (the file's when None): coarse_f0(estimate_pitch(load_audio(filename,
    sr), hop 320), f0_bin=num_pitch), on the CPU (vits/data/audio.py:213-239)."""
    audio, sampling_rate = _load_at(filename, sr)
    pitch = estimate_pitch(audio, sr=sampling_rate, n_fft=filter_length, win_length=win_length, hop_length=320)
    return coarse_f0(pitch.cpu(), f0_bin=num_pitch)


def infer_inputs(data_hparams, filename, sr=16000, pitch_shift=0):
    """infer.py:36-62 (`get_audio`): (audio_norm [1, T], pitch classes [1, F]) of a WAV file resampled to `sr`; the classes
    come from the audio shifted by `pitch_shift` semitones, the returned audio is the unshifted one.  Both on the CPU."""
    audio, sampling_rate = _load_at(filename, sr)
    audio = audio.cpu()
    shifted = shift_audio(audio, sampling_rate, pitch_shift)
    pitch = estimate_pitch(shifted, sr=sampling_rate, n_fft=data_hparams.filter_length, win_length=data_hparams.win_length,
                           hop_length=320)
    return audio.unsqueeze(0), coarse_f0(pitch)

"""Observability helpers of the trainer (reference: vits/utils.py:61-102), SURVEY section 8f rank 4, and the WAV reader
behind the data path (vits/utils.py:134-140)."""
import struct

import numpy as np


def summarize(writer, global_step, scalars={}, histograms={}, images={}, audios={}, audio_sampling_rate=22050):
    """Write one validation / training summary through a TensorBoard-style writer (any object with add_scalar /
    add_histogram / add_image / add_audio), same call pattern as vits/utils.py:61-69."""
    for k, v in scalars.items():
        writer.add_scalar(k, v, global_step)
    for k, v in histograms.items():
        writer.add_histogram(k, v, global_step)
    for k, v in images.items():
        writer.add_image(k, v, global_step, dataformats="HWC")
    for k, v in audios.items():
        writer.add_audio(k, v, global_step, audio_sampling_rate)


# five anchors of a viridis-like map (dark violet -> blue -> green -> yellow), linearly interpolated
_ANCHORS = np.array([[68, 1, 84], [59, 82, 139], [33, 145, 140], [94, 201, 98], [253, 231, 37]], dtype=np.float32)


def plot_spectrogram_to_numpy(spectrogram, height=200, width=1000):
    """[channels, frames] -> uint8 HWC image, origin at the bottom (low channels at the bottom rows), values
    mapped linearly from (min, max) through a perceptual colour map and nearest-neighbour resized to
    height x width.  The reference renders the same picture with matplotlib (utils.py:79-102: imshow,
    origin='lower', aspect='auto', a colour bar and axis labels); matplotlib is not a dependency here, so the
    frame decorations are omitted -- the pixel content is for eyeballing, not a parity item."""
    s = np.asarray(spectrogram, dtype=np.float32)
    if s.ndim != 2 or s.size == 0:
        raise ValueError("plot_spectrogram_to_numpy: expected a non-empty [channels, frames] array")
    lo, hi = float(np.nanmin(s)), float(np.nanmax(s))
    t = (np.nan_to_num(s, nan=lo) - lo) / (hi - lo) if hi > lo else np.zeros_like(s)
    rows = (np.arange(height) * s.shape[0] // height)[::-1]  # origin='lower'
    cols = np.arange(width) * s.shape[1] // width
    t = t[rows][:, cols] * (len(_ANCHORS) - 1)
    i0 = np.clip(np.floor(t).astype(np.int64), 0, len(_ANCHORS) - 2)
    f = (t - i0)[..., None]
    img = _ANCHORS[i0] * (1 - f) + _ANCHORS[i0 + 1] * f
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


_WAV_PCM, _WAV_FLOAT, _WAV_EXTENSIBLE = 1, 3, 0xFFFE


def _wav_chunks(raw, path):
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise ValueError("load_wav_to_torch: %s is not a RIFF/WAVE file (only WAV PCM 16 / 24 / 32-bit and 32-bit float "
                         "are decoded here; convert other containers first)" % path)
    pos, chunks = 12, {}
    while pos + 8 <= len(raw):
        tag, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
        chunks.setdefault(tag, raw[pos + 8:pos + 8 + size])
        pos += 8 + size + (size & 1)  # chunks are word-aligned
    if b"fmt " not in chunks or b"data" not in chunks or len(chunks[b"fmt "]) < 16:
        raise ValueError("load_wav_to_torch: %s has no fmt / data chunk" % path)
    return chunks[b"fmt "], chunks[b"data"]


def load_wav_to_torch(full_path):
    """(float32 [T], sampling rate) of a RIFF/WAVE file: the samples scaled to [-1, 1) as torchaudio.load scales them
    (int16 / 2**15, int24 / 2**23, int32 / 2**31, float32 as stored) and the channels averaged (vits/utils.py:134-140).
    Host code; any other container or sample format raises ValueError."""
    import torch
    with open(full_path, "rb") as f:
        raw = f.read()
    fmt, data = _wav_chunks(raw, full_path)
    tag, channels, rate, _, align, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == _WAV_EXTENSIBLE and len(fmt) >= 26:
        tag = struct.unpack("<H", fmt[24:26])[0]  # the sub-format GUID starts with the plain format tag
    if channels < 1 or align != channels * (bits // 8) or (tag, bits) not in ((_WAV_PCM, 16), (_WAV_PCM, 24), (_WAV_PCM, 32),
                                                                               (_WAV_FLOAT, 32)):
        raise ValueError("load_wav_to_torch: %s holds format tag %d with %d bits in %d channels; only WAV PCM 16 / 24 / 32-bit "
                         "and 32-bit float are decoded here" % (full_path, tag, bits, channels))
    n = len(data) // align * channels
    if tag == _WAV_FLOAT:
        x = np.frombuffer(data, dtype="<f4", count=n).astype(np.float32)
    elif bits == 16:
        x = np.frombuffer(data, dtype="<i2", count=n).astype(np.float32) / np.float32(2 ** 15)
    elif bits == 32:
        x = (np.frombuffer(data, dtype="<i4", count=n).astype(np.float64) / 2.0 ** 31).astype(np.float32)
    else:
        b = np.frombuffer(data, dtype=np.uint8, count=3 * n).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / np.float32(2 ** 23)
    wav = torch.from_numpy(np.ascontiguousarray(x.reshape(-1, channels).T))  # [channels, T], as torchaudio.load returns it
    return torch.mean(wav, dim=0), int(rate)

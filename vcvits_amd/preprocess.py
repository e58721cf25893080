"""Feature-cache entry points of the reference's preprocess.py (vits/preprocess.py:18-22, 64-73) without fairseq.

`load_hubert(path, device)` is the reference's function over vcvits_amd.model.hubert.HubertFeatureExtractor, and
`hubert_features(model, audio_norm)` is the block that writes `*.feature.pt`: pad 40 + 40 samples, extract_features,
transpose, squeeze, move to the CPU.  `hubert_features_batch(model, audios)` gives the same result for a list of files of
any lengths from padded batches (extract_features(lengths=): a row of a padded batch is the row computed alone), which is
how to fill the feature cache at the batched throughput.  `model.set_feature_extractor(load_hubert(path, "cuda"))` plugs the same object into
the content encoder."""
import torch
from torch.nn import functional as F

from .model.hubert import HubertFeatureExtractor

HUBERT_WINDOW, HUBERT_DOWNSAMPLE = 400, 320


def load_hubert(path, device):
    """preprocess.py:18-22: the frozen HuBERT of a fairseq checkpoint file, in eval mode on `device`."""
    hubert = HubertFeatureExtractor.from_checkpoint(path).to(device)
    hubert.eval()
    return hubert


def hubert_features(model, audio_norm):
    """preprocess.py:64-73: audio_norm [1, T] in [-1, 1] -> HuBERT features [E, T'] on the CPU (what `*.feature.pt` holds)."""
    pad = (HUBERT_WINDOW - HUBERT_DOWNSAMPLE) // 2
    wav = F.pad(audio_norm, (pad, pad))
    device = next(model.parameters()).device
    feats, _ = model.extract_features(wav.squeeze(1).to(device))
    return feats.transpose(1, -1).squeeze(0).to("cpu")


def hubert_features_batch(model, audios, max_batch_samples=2_560_000):
    """hubert_features for a list of audio_norm tensors [1, T_i] of any lengths, computed in padded batches: a list of CPU
    [E, T'_i] tensors in input order, each what hubert_features(model, audios[i]) returns.  Every row is padded 40 + 40
    samples as there, and that padded length is the row's length.  The files are sorted by length and cut into batches of
    B rows with B * T_max <= max_batch_samples (the default is 16 rows of 10 s); a longer file goes alone."""
    pad = (HUBERT_WINDOW - HUBERT_DOWNSAMPLE) // 2
    device = next(model.parameters()).device
    n = [int(a.shape[-1]) + 2 * pad for a in audios]
    order = sorted(range(len(audios)), key=lambda i: n[i])
    out = [None] * len(audios)
    i = 0
    while i < len(order):
        j = i + 1
        while j < len(order) and (j + 1 - i) * n[order[j]] <= max_batch_samples:
            j += 1
        rows = order[i:j]
        lengths = [n[r] for r in rows]
        wav = torch.zeros((len(rows), lengths[-1]), dtype=torch.float32)
        for b, r in enumerate(rows):
            wav[b, pad:lengths[b] - pad] = audios[r].reshape(-1)
        feats, _ = model.extract_features(wav.to(device), lengths=lengths)
        feats = feats.to("cpu")
        for b, (r, f) in enumerate(zip(rows, model.frame_lengths(lengths).tolist())):
            out[r] = feats[b, :f].transpose(0, 1)
        i = j
    return out

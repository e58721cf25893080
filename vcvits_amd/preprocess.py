"""Feature-cache entry points of the reference's preprocess.py (vits/preprocess.py:18-22, 64-73) without fairseq.

`load_hubert(path, device)` is the reference's function over vcvits_amd.model.hubert.HubertFeatureExtractor, and
`hubert_features(model, audio_norm)` is the block that writes `*.feature.pt`: pad 40 + 40 samples, extract_features,
transpose, squeeze, move to the CPU.  `model.set_feature_extractor(load_hubert(path, "cuda"))` plugs the same object into
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

"""Host-side data path of the voice-conversion trainer: batch schema + collate,
cache-key layout of the pre-processed tensors, pitch estimation and binning, and the inference length-scale plumbing,
as in the reference (vits/data/*).  Host logic except `estimate_pitch` / `pitch_classes` (pYIN) and the resampling / pitch shift behind `load_audio` / `shift_audio`
/ `get_pitch` / `infer_inputs`, which run as HIP kernels."""
from .audio import (coarse_f0, estimate_pitch, get_pitch, infer_inputs, infer_length_scale, load_audio,  # noqa: F401
                    normalize_pitch, pitch_classes, shift_audio)
from .collate import VoiceConversionMultiSpeakerCollate  # noqa: F401
from .sampler import DistributedUtteranceSampler, rank_indices  # noqa: F401

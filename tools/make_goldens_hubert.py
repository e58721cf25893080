"""Write tests/golden/hubert_small.npz: two toy transformers.HubertModel instances (random init, fixed seed, nothing
downloaded) with their weights renamed to fairseq's state_dict keys, one input, and the outputs that pin the restatement
in tests/hubert_f64.py: `last_hidden_state` (extract_features(output_layer=None)) and `hidden_states[1]` (output_layer=1).

  a  feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False   (hubert_base_ls960's architecture)
  b  feat_extract_norm="layer", conv_bias=True,  do_stable_layer_norm=True    (hubert_large / xtralarge's)

Both keep the real conv kernels and strides, the 128-tap position conv in 16 groups, exact GELU and eps 1e-5; widths are
toy so the file stays small.  Needs `transformers` on the authoring machine only; the tests read the .npz.

    HF_HUB_OFFLINE=1 python tools/make_goldens_hubert.py
"""
import os
import re
import sys

os.environ.setdefault("HF_HUB_OFFLINE", "1")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "hubert_small.npz")

CONV_DIM, EMBED, FFN, HEADS, LAYERS, SAMPLES = 24, 48, 64, 2, 2, 400 + 320 * 8

RENAMES = [
    (r"^feature_extractor\.conv_layers\.(\d+)\.conv\.", r"feature_extractor.conv_layers.\1.0."),
    (r"^feature_projection\.layer_norm\.", "layer_norm."),
    (r"^feature_projection\.projection\.", "post_extract_proj."),
    (r"^encoder\.pos_conv_embed\.conv\.parametrizations\.weight\.original0$", "encoder.pos_conv.0.weight_g"),
    (r"^encoder\.pos_conv_embed\.conv\.parametrizations\.weight\.original1$", "encoder.pos_conv.0.weight_v"),
    (r"^encoder\.pos_conv_embed\.conv\.weight_g$", "encoder.pos_conv.0.weight_g"),
    (r"^encoder\.pos_conv_embed\.conv\.weight_v$", "encoder.pos_conv.0.weight_v"),
    (r"^encoder\.pos_conv_embed\.conv\.bias$", "encoder.pos_conv.0.bias"),
    (r"^encoder\.layers\.(\d+)\.attention\.", r"encoder.layers.\1.self_attn."),
    (r"^encoder\.layers\.(\d+)\.layer_norm\.", r"encoder.layers.\1.self_attn_layer_norm."),
    (r"^encoder\.layers\.(\d+)\.feed_forward\.intermediate_dense\.", r"encoder.layers.\1.fc1."),
    (r"^encoder\.layers\.(\d+)\.feed_forward\.output_dense\.", r"encoder.layers.\1.fc2."),
]


def fairseq_name(key, layer_mode):
    m = re.match(r"^feature_extractor\.conv_layers\.(\d+)\.layer_norm\.(weight|bias)$", key)
    if m:  # GroupNorm sits at index 2 of the block; the layer-norm mode wraps its LayerNorm in a Sequential (index 2.1)
        return "feature_extractor.conv_layers.%s.2.%s%s" % (m.group(1), "1." if layer_mode else "", m.group(2))
    for pat, rep in RENAMES:
        new, n = re.subn(pat, rep, key)
        if n:
            return new
    return key


def build(layer_mode, seed):
    from transformers import HubertConfig, HubertModel
    cfg = HubertConfig(
        hidden_size=EMBED, num_hidden_layers=LAYERS, num_attention_heads=HEADS, intermediate_size=FFN, hidden_act="gelu",
        hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0,
        layerdrop=0.0, layer_norm_eps=1e-5, feat_extract_norm="layer" if layer_mode else "group",
        feat_extract_activation="gelu", feat_proj_layer_norm=True, conv_dim=(CONV_DIM,) * 7, conv_stride=(5, 2, 2, 2, 2, 2, 2),
        conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_bias=bool(layer_mode), num_conv_pos_embeddings=128,
        num_conv_pos_embedding_groups=16, do_stable_layer_norm=bool(layer_mode), apply_spec_augment=False,
        mask_time_prob=0.0, mask_feature_prob=0.0)
    torch.manual_seed(seed)
    model = HubertModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # move every parameter off its init value (norm gains of 1, biases of 0 would hide a swapped pair)
        for name, p in model.named_parameters():
            if name == "masked_spec_embed":
                continue
            if p.dim() == 1 or name.endswith("original0") or name.endswith("weight_g"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif "feature_extractor" in name:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[1] * p.shape[2])) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p[0].numel()) ** 0.5)
    return model


def main():
    arrays = {}
    g = torch.Generator().manual_seed(11)
    t = torch.arange(SAMPLES, dtype=torch.float32) / 16000.0
    source = torch.stack([0.3 * torch.sin(2 * torch.pi * 220.0 * (b + 1) * t) + 0.1 * torch.randn(SAMPLES, generator=g)
                          for b in range(2)])
    arrays["source"] = source.numpy()
    for tag, layer_mode in (("a", False), ("b", True)):
        model = build(layer_mode, 20 + layer_mode)
        with torch.no_grad():
            out = model(source, output_hidden_states=True)
        arrays[tag + "/last_hidden_state"] = out.last_hidden_state.numpy()
        arrays[tag + "/hidden_states_1"] = out.hidden_states[1].numpy()
        for k, v in model.state_dict().items():
            if k == "masked_spec_embed":
                continue
            arrays[tag + "/sd/" + fairseq_name(k, layer_mode)] = v.numpy()
    np.savez_compressed(OUT, **arrays)
    print("%s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())

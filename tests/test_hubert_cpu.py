"""CPU: the HuBERT restatement (tests/hubert_f64.py) against transformers.HubertModel's recorded outputs
(tests/golden/hubert_small.npz, tools/make_goldens_hubert.py), and the host side of vcvits_amd/model/hubert.py: architecture
inference from a fairseq state_dict, the checkpoint round trip, and the argument checks that come before any device work."""
import os

import numpy as np
import pytest
import torch

import hubert_f64 as R
from vcvits_amd.model.hubert import HubertFeatureExtractor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hubert_small.npz")
ARCH = {"a": dict(extractor_mode="default", layer_norm_first=False, num_heads=2),
        "b": dict(extractor_mode="layer_norm", layer_norm_first=True, num_heads=2)}


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    out = {"source": torch.from_numpy(z["source"])}
    for tag in ARCH:
        out[tag] = {"sd": {k[len(tag) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + "/sd/")},
                    None: torch.from_numpy(z[tag + "/last_hidden_state"]), 1: torch.from_numpy(z[tag + "/hidden_states_1"])}
    return out


@pytest.mark.parametrize("output_layer", [None, 1])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_equals_transformers(golden, tag, output_layer):
    """two float32 implementations of one model differ in summation order only: relative L2 <= 1e-5 (the float32 run of a
    model of this size sits below 1e-6 of its float64 run)"""
    want = golden[tag][output_layer]
    got = R.run(golden[tag]["sd"], golden["source"], "f32", output_layer=output_layer, **ARCH[tag])
    assert tuple(got.shape) == tuple(want.shape) == (2, R.out_frames(golden["source"].shape[1]), 48)
    d = R.rel_l2(got, want)
    print("%s output_layer=%s: float32 restatement vs transformers %.3e (max abs %.3e)" % (tag, output_layer, d, R.max_abs(got, want)))
    assert d <= 1e-5
    assert R.rel_l2(R.run(golden[tag]["sd"], golden["source"], "f64", output_layer=output_layer, **ARCH[tag]), want) <= 1e-5


def test_golden_is_small():
    assert os.path.getsize(GOLDEN) < 822 * 1024


def _toy(mode, **kw):
    return R.random_state_dict(5, extractor_mode=mode, conv_dim=16, embed_dim=32, ffn_dim=48, layers=3,
                               conv_bias=mode == "layer_norm", **kw)


def test_from_state_dict_infers_both_architectures(golden):
    a = HubertFeatureExtractor.from_state_dict(golden["a"]["sd"], heads=2)
    assert (a.extractor_mode, a.layer_norm_first, a.conv_bias) == ("default", False, False)
    assert (a.conv_dim, a.embed_dim, a.ffn_dim, a.n_layers, a.heads) == (24, 48, 64, 2, 2)
    assert a.conv_kernels == (10, 3, 3, 3, 3, 2, 2) and a.conv_strides == (5, 2, 2, 2, 2, 2, 2)
    assert (a.conv_pos, a.conv_pos_groups) == (128, 16)
    b = HubertFeatureExtractor.from_state_dict(golden["b"]["sd"], heads=2)
    assert (b.extractor_mode, b.layer_norm_first, b.conv_bias) == ("layer_norm", True, True)
    for m, tag in ((a, "a"), (b, "b")):
        sd = m.state_dict()
        assert set(sd) == set(golden[tag]["sd"])
        assert all(torch.equal(sd[k], golden[tag]["sd"][k]) for k in sd)
        assert not m.training and not any(p.requires_grad for p in m.parameters())
        assert m.out_frames(400) == 1 and m.out_frames(399) == 0 and m.out_frames(16000) == 49
    # every inferred value can be overridden; widths without a default head count ask for one
    c = HubertFeatureExtractor.from_state_dict(golden["a"]["sd"], heads=3, layer_norm_first=True)
    assert c.heads == 3 and c.layer_norm_first and c.extractor_mode == "default"
    with pytest.raises(ValueError, match="heads"):
        HubertFeatureExtractor.from_state_dict(golden["a"]["sd"])


def test_default_head_counts():
    for embed, heads in ((768, 12), (1024, 16), (1280, 16)):
        sd = {"feature_extractor.conv_layers.%d.0.weight" % i: torch.zeros(8, 1 if i == 0 else 8, k)
              for i, k in enumerate((10, 3, 3, 3, 3, 2, 2))}
        sd.update({"feature_extractor.conv_layers.0.2.weight": torch.zeros(8), "post_extract_proj.weight": torch.zeros(embed, 8),
                   "encoder.layers.0.fc1.weight": torch.zeros(16, embed), "encoder.pos_conv.0.weight_v": torch.zeros(embed, embed // 16, 128)})
        cfg = HubertFeatureExtractor.config_from_state_dict(sd)
        assert cfg["heads"] == heads and cfg["layers"] == 1 and cfg["conv_pos_groups"] == 16


@pytest.mark.parametrize("mode", ["default", "layer_norm"])
def test_from_checkpoint_round_trip(tmp_path, mode):
    sd = _toy(mode)
    extra = dict(sd)
    extra.update({"mask_emb": torch.zeros(32), "label_embs_concat": torch.zeros(10, 8), "final_proj.weight": torch.zeros(8, 32),
                  "final_proj.bias": torch.zeros(8)})
    path = str(tmp_path / "hubert.pt")
    torch.save({"cfg": {"model": {"extractor_mode": mode, "layer_norm_first": mode == "layer_norm", "encoder_attention_heads": 4,
                                  "conv_bias": mode == "layer_norm", "conv_pos": 128, "conv_pos_groups": 16}},
                "model": extra}, path)
    m = HubertFeatureExtractor.from_checkpoint(path)
    assert (m.extractor_mode, m.layer_norm_first, m.heads, m.n_layers) == (mode, mode == "layer_norm", 4, 3)
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert HubertFeatureExtractor.from_checkpoint(path, heads=2).heads == 2
    # a checkpoint without a cfg mapping still loads from its shapes
    torch.save({"cfg": None, "model": extra}, path)
    assert HubertFeatureExtractor.from_checkpoint(path, heads=4).extractor_mode == mode


class _TaskDictionary:
    """stands for fairseq.data.Dictionary, which published checkpoints pickle in task_state"""
    loaded = 0

    def __init__(self):
        self.symbols = ["<s>", "a"]

    def __setstate__(self, state):
        _TaskDictionary.loaded += 1
        self.__dict__.update(state)


def test_from_checkpoint_skips_foreign_objects(tmp_path):
    """a file that pickles objects of other classes beside the tensors loads without importing or running those classes"""
    sd = _toy("layer_norm")
    path = str(tmp_path / "with_task_state.pt")
    torch.save({"cfg": {"model": {"extractor_mode": "layer_norm", "layer_norm_first": True, "encoder_attention_heads": 4}},
                "model": sd, "task_state": {"dictionaries": [_TaskDictionary()]}}, path)
    with pytest.raises(Exception):
        torch.load(path, map_location="cpu")  # (the weights-only loader refuses the file: the case under test)
    m = HubertFeatureExtractor.from_checkpoint(path)
    assert _TaskDictionary.loaded == 0
    got = m.state_dict()
    assert m.heads == 4 and set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_missing_encoder_key_is_reported(tmp_path):
    sd = _toy("default")
    del sd["encoder.layers.1.self_attn.k_proj.bias"]
    with pytest.raises(KeyError, match="encoder.layers.1.self_attn.k_proj.bias"):
        HubertFeatureExtractor.from_state_dict(sd, heads=4)
    path = str(tmp_path / "broken.pt")
    torch.save({"cfg": {"model": {"encoder_attention_heads": 4}}, "model": sd}, path)
    with pytest.raises(KeyError, match="k_proj.bias"):
        HubertFeatureExtractor.from_checkpoint(path)
    torch.save({"weights": sd}, path)
    with pytest.raises(KeyError, match="model"):
        HubertFeatureExtractor.from_checkpoint(path)


def test_argument_checks_come_before_device_work():
    m = HubertFeatureExtractor.from_state_dict(_toy("default"), heads=4)
    with pytest.raises(ValueError, match="399 samples"):
        m.extract_features(torch.zeros(2, 399))
    with pytest.raises(NotImplementedError, match="mask"):
        m.extract_features(torch.zeros(2, 800), mask=True)
    with pytest.raises(NotImplementedError, match="padding"):
        m.extract_features(torch.zeros(2, 800), padding_mask=torch.zeros(2, 800, dtype=torch.bool))
    with pytest.raises(ValueError, match="output_layer"):
        m.extract_features(torch.zeros(2, 800), output_layer=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a CPU tensor is an error, never a slow path
        m.extract_features(torch.zeros(2, 800))


def test_reachable_through_the_reference_paths():
    import vits.model.hubert
    import vits.preprocess
    import vcvits_amd.preprocess
    assert vits.model.hubert.HubertFeatureExtractor is HubertFeatureExtractor
    assert vits.preprocess.load_hubert is vcvits_amd.preprocess.load_hubert

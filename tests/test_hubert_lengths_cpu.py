"""CPU: the host side of extract_features(lengths=) (vcvits_amd/model/hubert.py): the frame arithmetic, the argument checks
that come before any device work, and the declaration of the new entry points in the C header."""
import os
import re

import pytest
import torch

import hubert_f64 as R
from vcvits_amd.model.hubert import HubertFeatureExtractor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    sd = R.random_state_dict(5, extractor_mode="default", conv_dim=16, embed_dim=32, ffn_dim=48, layers=1)
    return HubertFeatureExtractor.from_state_dict(sd, heads=4)


def test_frame_lengths_is_out_frames(model):
    n = list(range(400, 4001))
    want = [R.out_frames(v) for v in n]
    got = model.frame_lengths(n)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.tolist() == want
    assert model.frame_lengths(torch.tensor(n, dtype=torch.int32)).tolist() == want
    assert want[0] == 1 and want[319] == 1 and want[320] == 2 and want[-1] == 12
    assert model.receptive_field() == 400


@pytest.mark.parametrize("lengths", [
    [800],                                          # one entry for two rows
    [[800, 800]],                                   # [1, B]
    torch.tensor([[800], [800]]),                   # [B, 1]
    torch.tensor(800),                              # a scalar
], ids=["short", "1xB", "Bx1", "scalar"])
def test_lengths_of_the_wrong_shape_raise(model, lengths):
    with pytest.raises(ValueError, match="row"):
        model.extract_features(torch.zeros(2, 800), lengths=lengths)


@pytest.mark.parametrize("lengths", [[800.0, 800.0], torch.tensor([800, 800], dtype=torch.float32),
                                     torch.tensor([True, True])], ids=["list", "tensor", "bool"])
def test_lengths_that_are_not_integers_raise(model, lengths):
    with pytest.raises(ValueError, match="row"):
        model.extract_features(torch.zeros(2, 800), lengths=lengths)


def test_an_entry_outside_the_row_raises_and_names_the_row(model):
    with pytest.raises(ValueError, match=r"lengths\[1\] = 801: row 1 "):
        model.extract_features(torch.zeros(3, 800), lengths=[800, 801, 800])
    with pytest.raises(ValueError, match=r"lengths\[2\] = 399: row 2 .*receptive field \(400\)"):
        model.extract_features(torch.zeros(3, 800), lengths=torch.tensor([800, 400, 399]))
    with pytest.raises(ValueError, match="row 0"):
        model.extract_features(torch.zeros(3, 800), lengths=[-1, 800, 800])
    with pytest.raises(ValueError, match="row 0"):
        model.forward(torch.zeros(1, 800), lengths=[0])


def test_valid_lengths_reach_the_device_check(model):
    """accepted lengths (list, int32 and int64 tensors) pass the host checks: the next error is the missing GPU"""
    for lengths in ([800, 400], torch.tensor([400, 800], dtype=torch.int32), torch.tensor([799, 401])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.extract_features(torch.zeros(2, 800), lengths=lengths)


def test_padding_mask_still_raises(model):
    with pytest.raises(NotImplementedError, match="padding"):
        model.extract_features(torch.zeros(2, 800), padding_mask=torch.zeros(2, 800, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="padding"):
        model.extract_features(torch.zeros(2, 800), padding_mask=torch.zeros(2, 800, dtype=torch.bool), lengths=[800, 800])


def test_new_entry_points_are_declared_and_bound():
    """the header declares them (so test_library_exports_every_declared_symbol covers them) with the argument lists the
    Python bindings use"""
    from vcvits_amd import _lib
    text = open(os.path.join(ROOT, "include", "vcvits_hip.h")).read()
    for name, n_args in (("vcv_hubert_attn_fwd_len", 12), ("vcv_hubert_groupnorm_gelu_len", 10), ("vcv_hubert_mask_frames", 7)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, text, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib._ARGTYPES[name])
        assert "const int*" in m.group(1)
        assert name in _lib.EXPORTS


def test_ops_and_preprocess_carry_the_new_names():
    import inspect
    import vits.preprocess
    from vcvits_amd import ops, preprocess
    assert ops.mask_frames is ops.hubert.mask_frames
    for fn in (ops.hubert_attention, ops.hubert_attention_qkv, ops.groupnorm_gelu):
        assert inspect.signature(fn).parameters["lengths"].default is None
    assert vits.preprocess.hubert_features_batch is preprocess.hubert_features_batch
    assert inspect.signature(preprocess.hubert_features_batch).parameters["max_batch_samples"].default == 2_560_000

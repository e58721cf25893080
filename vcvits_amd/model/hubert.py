"""HuBERT feature extractor on the HIP kernels: fairseq's HubertModel.extract_features in inference, without fairseq.

The reference keeps a frozen fairseq HuBERT behind HubertContentEncoder (content_encoder.py:32-35, 53-58) and behind its
feature cache (preprocess.py:18-22, 60-74).  This module is that model for the two published architectures:

  base   (hubert_base_ls960)            extractor_mode "default"    (GroupNorm on conv layer 0), post-LN encoder, 12 x 64
  large  (hubert_large / xtralarge)     extractor_mode "layer_norm" (conv bias, LayerNorm per conv layer), pre-LN encoder,
                                        16 x 64 / 16 x 80

Parameters carry fairseq's state_dict names, so `ckpt["model"]` loads as it is; the pre-training heads (mask_emb,
label_embs_concat, final_proj) are not part of the model.  Inference only: no masking, no dropout, no gradients.

Rows of unequal length.  Without `lengths=` the rows of a batch are computed as fairseq computes them without a padding
mask: the zeros behind a shorter row take part in the layer-0 GroupNorm, the position conv and every attention softmax.
With `extract_features(source, lengths=)` the features of a row in a padded batch are the features of that row computed
alone: the GroupNorm statistics are counted per row, the frames behind a row's end are zeroed before the position conv
(the padding a row alone sees there), the attention keys are bounded per row, and the features behind a row's end come
back as exact zeros with a frame padding mask.  Everything between those steps is per frame, and nothing valid reads a
frame behind a row's end.  This is NOT fairseq's `padding_mask`: fairseq keeps the padded zeros in the GroupNorm and
derives the frame mask by a chunking rule, so `padding_mask=` stays unbuilt and raises.

The tensor layout is [B, C, T] throughout.  Every linear layer and convolution is ops.conv_forward (so they follow
set_compute_dtype: split-operand fp32 or bf16 operands), residual + LayerNorm is ops.layernorm_c, and attention, GroupNorm +
GELU, LayerNorm + GELU and bias + GELU are the kernels of ops/hubert.py.  The conv-ready weights (weight norm of the position
conv folded, linear weights as 1-tap convs) are laid into one flat device buffer once per load and registered as a parameter
region, so the packed copies the conv kernels read are made once."""
import pickle
import types

import torch
from torch import nn

from .. import ops

CONV_KERNELS = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDES = (5, 2, 2, 2, 2, 2, 2)
DEFAULT_HEADS = {768: 12, 1024: 16, 1280: 16}
EPS = 1e-5


class _Foreign:
    """Stands in for any object of a checkpoint whose class is not a tensor, a storage or a plain container (a fairseq
    Dictionary in `task_state`, an argparse / omegaconf object in old `args`): built without importing or running its class."""

    def __init__(self, *a, **kw):
        pass

    def __call__(self, *a, **kw):
        return _Foreign()

    def __setstate__(self, state):
        pass

    def __reduce_ex__(self, protocol):
        return (_Foreign, ())

    def get(self, key, default=None):
        return default


_PLAIN_BUILTINS = ("set", "frozenset", "list", "dict", "tuple", "int", "float", "bool", "str", "bytes", "bytearray", "complex",
                   "slice", "range", "object")


_TENSOR_GLOBALS = {("collections", "OrderedDict"), ("torch", "Size"), ("torch", "device"),
                   ("torch._utils", "_rebuild_tensor"), ("torch._utils", "_rebuild_tensor_v2"),
                   ("torch._utils", "_rebuild_parameter"), ("torch.storage", "UntypedStorage"),
                   ("torch.storage", "TypedStorage")}


def _tensor_global(module, name):
    """The globals a pickled tensor needs, after torch's own weights-only list: the rebuild functions, the storage classes,
    dtypes, torch.Size and torch.device.  Nothing else of torch (no callable a crafted REDUCE could aim at) and no numpy."""
    if (module, name) in _TENSOR_GLOBALS:
        return True
    if module != "torch":
        return False
    obj = getattr(torch, name, None)
    return isinstance(obj, torch.dtype) or (name.endswith("Storage") and isinstance(obj, type))


class _StubUnpickler(pickle.Unpickler):
    """Tensors, storages and plain containers load as they are; every other global becomes _Foreign (numpy scalars and
    arrays included: nothing of "model" or "cfg" is one)."""

    def find_class(self, module, name):
        if _tensor_global(module, name) or (module == "builtins" and name in _PLAIN_BUILTINS):
            return super().find_class(module, name)
        return _Foreign


_stub_pickle = types.SimpleNamespace(Unpickler=_StubUnpickler, load=lambda f, **kw: _StubUnpickler(f, **kw).load(),
                                     __name__="vcvits_amd.model.hubert._stub_pickle")


def _load_checkpoint(path):
    """torch.load(path, map_location="cpu"); a file that torch's weights-only loader refuses because it pickles foreign
    objects beside the tensors is read again with those objects stubbed (no foreign code is imported or run)."""
    try:
        return torch.load(path, map_location="cpu")
    except pickle.UnpicklingError:
        return torch.load(path, map_location="cpu", weights_only=False, pickle_module=_stub_pickle)


class _P(nn.Module):
    """A bag of frozen parameters under one state_dict prefix (`weight` / `bias` / `weight_g` / `weight_v`)."""

    def __init__(self, **shapes):
        super().__init__()
        for name, shape in shapes.items():
            if shape is not None:
                init = torch.ones(shape) if name in ("weight_g",) else torch.zeros(shape)
                self.register_parameter(name, nn.Parameter(init, requires_grad=False))


def _norm(c):
    m = _P(weight=(c,), bias=(c,))
    nn.init.ones_(m.weight)
    return m


def _linear(o, i):
    m = _P(weight=(o, i), bias=(o,))
    nn.init.normal_(m.weight, 0.0, i ** -0.5)
    return m


class _Bag(nn.Module):
    pass


class HubertFeatureExtractor(nn.Module):
    """extract_features(source [B, T]) -> (features [B, T', embed_dim], None), T' = the conv stack's output length
    ((T - 400) // 320 + 1 with the published kernels and strides); with lengths= (valid samples per row) the second element
    is the frame padding mask [B, T'] and every row equals that row computed alone."""

    def __init__(self, conv_dim=512, embed_dim=768, ffn_dim=3072, layers=12, heads=12, extractor_mode="default",
                 layer_norm_first=False, conv_bias=False, conv_kernels=CONV_KERNELS, conv_strides=CONV_STRIDES,
                 conv_pos=128, conv_pos_groups=16):
        super().__init__()
        extractor_mode = str(getattr(extractor_mode, "name", extractor_mode))
        if extractor_mode not in ("default", "layer_norm"):
            raise ValueError("extractor_mode must be 'default' or 'layer_norm', got %r" % (extractor_mode,))
        if len(conv_kernels) != len(conv_strides) or not conv_kernels:
            raise ValueError("conv_kernels and conv_strides must have one entry per conv layer")
        if embed_dim % heads or embed_dim % conv_pos_groups:
            raise ValueError("embed_dim %d is not a multiple of heads %d and position-conv groups %d"
                             % (embed_dim, heads, conv_pos_groups))
        self.conv_dim, self.embed_dim, self.ffn_dim, self.n_layers, self.heads = conv_dim, embed_dim, ffn_dim, layers, heads
        self.extractor_mode, self.layer_norm_first, self.conv_bias = extractor_mode, bool(layer_norm_first), bool(conv_bias)
        self.conv_kernels, self.conv_strides = tuple(int(k) for k in conv_kernels), tuple(int(s) for s in conv_strides)
        self.conv_pos, self.conv_pos_groups = int(conv_pos), int(conv_pos_groups)

        self.feature_extractor = _Bag()
        blocks, cin = [], 1
        for i, k in enumerate(self.conv_kernels):
            conv = _P(weight=(conv_dim, cin, k), bias=(conv_dim,) if conv_bias else None)
            nn.init.normal_(conv.weight, 0.0, (2.0 / (cin * k)) ** 0.5)
            d = {"0": conv}
            if extractor_mode == "layer_norm":
                d["2"] = nn.ModuleDict({"1": _norm(conv_dim)})
            elif i == 0:
                d["2"] = _norm(conv_dim)
            blocks.append(nn.ModuleDict(d))
            cin = conv_dim
        self.feature_extractor.conv_layers = nn.ModuleList(blocks)
        self.layer_norm = _norm(conv_dim)
        self.post_extract_proj = _linear(embed_dim, conv_dim)
        self.encoder = _Bag()
        pos = _P(weight_g=(1, 1, conv_pos), weight_v=(embed_dim, embed_dim // conv_pos_groups, conv_pos), bias=(embed_dim,))
        nn.init.normal_(pos.weight_v, 0.0, 1.0)
        self.encoder.pos_conv = nn.ModuleDict({"0": pos})
        enc_layers = []
        for _ in range(layers):
            lay = _Bag()
            lay.self_attn = _Bag()
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                setattr(lay.self_attn, n, _linear(embed_dim, embed_dim))
            lay.self_attn_layer_norm = _norm(embed_dim)
            lay.fc1 = _linear(ffn_dim, embed_dim)
            lay.fc2 = _linear(embed_dim, ffn_dim)
            lay.final_layer_norm = _norm(embed_dim)
            enc_layers.append(lay)
        self.encoder.layers = nn.ModuleList(enc_layers)
        self.encoder.layer_norm = _norm(embed_dim)
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        object.__setattr__(self, "_ready", None)  # (key, flat buffer, {name: view}) of the conv-ready weights

    # ------------------------------------------------------------------------------------------------------ loading
    @classmethod
    def config_from_state_dict(cls, sd, **overrides):
        """Constructor arguments read off the shapes and key names of a fairseq `["model"]` dict."""
        def need(k):
            if k not in sd:
                raise KeyError("HuBERT state_dict has no %r" % k)
            return sd[k]

        n = 0
        while "feature_extractor.conv_layers.%d.0.weight" % n in sd:
            n += 1
        if n == 0:
            need("feature_extractor.conv_layers.0.0.weight")
        cfg = {"conv_dim": int(need("feature_extractor.conv_layers.0.0.weight").shape[0]),
               "conv_kernels": tuple(int(sd["feature_extractor.conv_layers.%d.0.weight" % i].shape[2]) for i in range(n)),
               "extractor_mode": "layer_norm" if "feature_extractor.conv_layers.0.2.1.weight" in sd else "default",
               "conv_bias": "feature_extractor.conv_layers.0.0.bias" in sd}
        cfg["conv_strides"] = CONV_STRIDES if n == len(CONV_STRIDES) else None
        proj, fc1 = need("post_extract_proj.weight"), need("encoder.layers.0.fc1.weight")
        cfg["embed_dim"], cfg["ffn_dim"] = int(proj.shape[0]), int(fc1.shape[0])
        layers = 0
        while "encoder.layers.%d.fc1.weight" % layers in sd:
            layers += 1
        cfg["layers"] = layers
        wv = need("encoder.pos_conv.0.weight_v")
        cfg["conv_pos"], cfg["conv_pos_groups"] = int(wv.shape[2]), cfg["embed_dim"] // int(wv.shape[1])
        cfg["layer_norm_first"] = cfg["extractor_mode"] == "layer_norm"  # the published models pair them
        cfg["heads"] = DEFAULT_HEADS.get(cfg["embed_dim"])
        cfg.update({k: v for k, v in overrides.items() if v is not None})
        if cfg["heads"] is None:
            raise ValueError("embed_dim %d has no default head count (known: %s); pass heads=" % (cfg["embed_dim"], DEFAULT_HEADS))
        if cfg["conv_strides"] is None:
            raise ValueError("%d conv layers: pass conv_strides= (the default covers the published 7-layer stack)" % n)
        return cfg

    @classmethod
    def from_state_dict(cls, sd, **overrides):
        """The model of a fairseq `["model"]` dict: widths, layer counts and the norm mode come from the shapes and keys,
        `layer_norm_first` follows the norm mode, heads default to {768: 12, 1024: 16, 1280: 16}; every constructor argument
        can be overridden.  Pre-training heads and other extra keys are ignored; a missing key of the model is an error."""
        model = cls(**cls.config_from_state_dict(sd, **overrides))
        res = model.load_state_dict({k: v for k, v in sd.items() if torch.is_tensor(v)}, strict=False)
        if res.missing_keys:
            raise KeyError("HuBERT state_dict misses %s" % ", ".join(sorted(res.missing_keys)))
        return model

    @classmethod
    def from_checkpoint(cls, path, **overrides):
        """A fairseq checkpoint file ({"cfg": {"model": {...}}, "model": state_dict}); needs no fairseq import: objects of
        fairseq's own classes elsewhere in the file (`task_state`, old `args`) are skipped, only "model" and "cfg" are read."""
        ckpt = _load_checkpoint(path)
        if not isinstance(ckpt, dict) or "model" not in ckpt:
            raise KeyError("%s is not a fairseq checkpoint: no 'model' entry" % (path,))
        cfg = ckpt.get("cfg")
        mcfg = cfg.get("model") if hasattr(cfg, "get") else None
        kw = {}
        if hasattr(mcfg, "get"):
            for theirs, ours in (("extractor_mode", "extractor_mode"), ("layer_norm_first", "layer_norm_first"),
                                 ("encoder_attention_heads", "heads"), ("conv_bias", "conv_bias"), ("conv_pos", "conv_pos"),
                                 ("conv_pos_groups", "conv_pos_groups")):
                if mcfg.get(theirs) is not None:
                    kw[ours] = mcfg.get(theirs)
        kw.update(overrides)
        return cls.from_state_dict(ckpt["model"], **kw)

    # ------------------------------------------------------------------------------------------------------ weights
    def out_frames(self, n_samples):
        t = int(n_samples)
        for k, s in zip(self.conv_kernels, self.conv_strides):
            t = (t - k) // s + 1 if t >= k else 0
        return t

    def receptive_field(self):
        """Samples that give one output frame (400 with the published kernels and strides)."""
        need = 1
        for k, s in zip(reversed(self.conv_kernels), reversed(self.conv_strides)):
            need = (need - 1) * s + k
        return need

    def frame_lengths(self, lengths):
        """Output frames of rows with `lengths` valid samples (a list or an integer tensor): out_frames per entry, as an
        int64 CPU tensor of the same shape."""
        t = torch.as_tensor(lengths).detach().to("cpu")
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("lengths must be integers, got %s" % t.dtype)
        return torch.tensor([self.out_frames(v) for v in t.reshape(-1).tolist()], dtype=torch.int64).reshape(t.shape)

    def _check_lengths(self, lengths, B, T):
        """The host copy (int64 CPU [B]) of `lengths`, checked; every failure is a ValueError that names the row."""
        t = torch.as_tensor(lengths).detach()
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("lengths must hold one integer sample count per row of source, got dtype %s" % t.dtype)
        if tuple(t.shape) != (B,):
            raise ValueError("lengths must hold one sample count per row of source: shape [%d] expected, got %s"
                             % (B, list(t.shape)))
        host = t.to("cpu", torch.int64)  # the one copy to the host when lengths lives on the GPU
        need = self.receptive_field()
        for b, v in enumerate(host.tolist()):
            if v > T:
                raise ValueError("lengths[%d] = %d: row %d cannot be longer than source (%d samples)" % (b, v, b, T))
            if v < need:
                raise ValueError("lengths[%d] = %d: row %d is shorter than the conv stack's receptive field (%d)"
                                 % (b, v, b, need))
        return host

    def _weights(self, device):
        """{name: float32 view} of the conv-ready weights on `device`, all inside one flat buffer that is registered as a
        parameter region (ops.register_param_region: the conv kernels' packed copies are cached per region).  Rebuilt when a
        parameter was replaced, moved or written."""
        params = list(self.named_parameters())
        key = (str(device), tuple(p.data_ptr() for _, p in params), sum(p._version for _, p in params))
        ready = self._ready
        if ready is not None and ready[0] == key:
            return ready[2]
        if ready is not None:
            ops.unregister_param_region(ready[1])
        items = []
        for name, p in params:
            t = p.detach().to(torch.float32)
            if name.endswith("weight_g"):
                continue
            if name.endswith("weight_v"):  # weight_norm(dim=2): one norm per tap, over the other two axes
                g = dict(params)[name[:-1] + "g"].detach().to(torch.float32)
                t = t * (g / torch.sqrt((t * t).sum(dim=(0, 1), keepdim=True)))
                name = name[:-2]
            if t.dim() == 2:
                t = t.unsqueeze(-1)
            items.append((name, t))
        got = dict(items)
        for i in range(self.n_layers):  # q, k and v as one projection: x is read once, one launch instead of three
            p = "encoder.layers.%d.self_attn." % i
            for kind in ("weight", "bias"):
                items.append((p + "qkv." + kind, torch.cat([got[p + n + "_proj." + kind] for n in "qkv"], dim=0)))
        items = [(n, t) for n, t in items if ".self_attn.q_proj." not in n and ".self_attn.k_proj." not in n
                 and ".self_attn.v_proj." not in n]
        total = sum((t.numel() + 63) // 64 * 64 for _, t in items)
        flat = torch.empty((total,), dtype=torch.float32, device=device)
        views, off = {}, 0
        for name, t in items:
            v = flat[off:off + t.numel()].view(t.shape)
            v.copy_(t)
            views[name] = v
            off += (t.numel() + 63) // 64 * 64
        ops.register_param_region(flat)
        object.__setattr__(self, "_ready", (key, flat, views))
        return views

    def __del__(self):
        ready = getattr(self, "_ready", None)
        if ready is not None:
            try:
                ops.unregister_param_region(ready[1])
            except Exception:
                pass

    # ------------------------------------------------------------------------------------------------------ forward
    def _attn_block(self, w, p, x, fr=None):
        return ops.hubert_attention_qkv(ops.conv_forward(x, w[p + ".qkv.weight"], w[p + ".qkv.bias"]), self.heads, lengths=fr)

    def extract_features(self, source, padding_mask=None, mask=False, output_layer=None, lengths=None):
        """fairseq's HubertModel.extract_features for inference: source [B, T] float32 on the GPU ->
        (features [B, T', embed_dim], None).  output_layer None: the encoder output; n (1-based): the output of layer n (a
        pre-LN model then skips the final encoder.layer_norm, as fairseq does).

        lengths (a list, a CPU tensor or a GPU tensor of B integers): the valid samples of each row of a padded batch, each
        between the receptive field of the conv stack and T.  The result is then (features, frame_padding_mask [B, T'] bool,
        True where a frame is padding), the valid frames of row b (frame_lengths(lengths)[b] of them) are what
        extract_features(source[b:b + 1, :lengths[b]]) gives, and the features under the mask are exact zeros, whatever the
        samples behind a row's end hold.  The per-layer counts are computed on the host, so lengths on the GPU costs one
        copy to the host (and a wait for the queue); a list or a CPU tensor costs none."""
        if padding_mask is not None:
            raise NotImplementedError("HubertFeatureExtractor: fairseq's padding masks are not built (the reference passes "
                                      "none); for rows of unequal length pass lengths=")
        if mask:
            raise NotImplementedError("HubertFeatureExtractor: masking is a pre-training feature; inference only")
        if not isinstance(source, torch.Tensor) or source.dim() != 2:
            raise ValueError("source must be a [B, T] waveform tensor")
        if output_layer is not None and not 1 <= int(output_layer) <= self.n_layers:
            raise ValueError("output_layer must be None or in [1, %d]" % self.n_layers)
        B, T = source.shape
        frames = self.out_frames(T)
        if frames < 1:
            raise ValueError("source of %d samples is shorter than the conv stack's receptive field (%d)"
                             % (T, self.receptive_field()))
        host = None if lengths is None else self._check_lengths(lengths, B, T)
        if not source.is_cuda:
            raise RuntimeError("vcvits_amd: source is not on the GPU; the HIP path has no CPU fallback")
        with torch.no_grad():
            w = self._weights(source.device)
            n0 = fr = pad_mask = None
            if host is not None:
                # what the kernels need of the lengths: layer 0's output samples per row (the GroupNorm counts) and the
                # output frames per row, both >= 1 after _check_lengths; one upload
                k0, s0 = self.conv_kernels[0], self.conv_strides[0]
                fr_host = self.frame_lengths(host)
                # (from pinned memory and without waiting: a pageable copy would hold the host until the queue has drained)
                dev = torch.stack([(host - k0) // s0 + 1, fr_host]).to(torch.int32).pin_memory().to(source.device, non_blocking=True)
                n0, fr = dev[0], dev[1]
                pad_mask = (torch.arange(frames)[None, :] >= fr_host[:, None]).pin_memory().to(source.device, non_blocking=True)
            x = source.detach().to(torch.float32).contiguous().unsqueeze(1)
            for i, s in enumerate(self.conv_strides):
                p = "feature_extractor.conv_layers.%d" % i
                x = ops.conv_forward(x, w[p + ".0.weight"], w.get(p + ".0.bias"), stride=s)
                if self.extractor_mode == "layer_norm":
                    x = ops.layernorm_c_gelu(x, w[p + ".2.1.weight"], w[p + ".2.1.bias"], EPS, inplace=True)
                elif i == 0:
                    x = ops.groupnorm_gelu(x, w[p + ".2.weight"], w[p + ".2.bias"], EPS, inplace=True, lengths=n0)
                else:
                    x = ops.bias_gelu(x, inplace=True)
            x = ops.layernorm_c(x, None, w["layer_norm.weight"], w["layer_norm.bias"], EPS)
            x = ops.conv_forward(x, w["post_extract_proj.weight"], w["post_extract_proj.bias"])
            if fr is not None:  # the position conv of a row alone sees zeros behind the row's end
                x = ops.mask_frames(x, fr, inplace=True)
            pos = ops.conv_forward(x, w["encoder.pos_conv.0.weight"], w["encoder.pos_conv.0.bias"], pad=self.conv_pos // 2,
                                   groups=self.conv_pos_groups)  # an even kernel yields one frame too many: dropped below
            if self.layer_norm_first:
                x = ops.bias_gelu(pos, res=x, frames=frames)
            else:
                x = ops.layernorm_c(x, ops.bias_gelu(pos, frames=frames), w["encoder.layer_norm.weight"],
                                    w["encoder.layer_norm.bias"], EPS)
            n_run = self.n_layers if output_layer is None else int(output_layer)
            for i in range(n_run):
                p = "encoder.layers.%d" % i
                ln1 = (w[p + ".self_attn_layer_norm.weight"], w[p + ".self_attn_layer_norm.bias"])
                ln2 = (w[p + ".final_layer_norm.weight"], w[p + ".final_layer_norm.bias"])
                ow, ob = w[p + ".self_attn.out_proj.weight"], w[p + ".self_attn.out_proj.bias"]
                if self.layer_norm_first:
                    a = self._attn_block(w, p + ".self_attn", ops.layernorm_c(x, None, ln1[0], ln1[1], EPS), fr)
                    x = ops.conv_forward(a, ow, ob, res=x)
                    h = ops.conv_forward(ops.layernorm_c(x, None, ln2[0], ln2[1], EPS), w[p + ".fc1.weight"], w[p + ".fc1.bias"])
                    x = ops.conv_forward(ops.bias_gelu(h, inplace=True), w[p + ".fc2.weight"], w[p + ".fc2.bias"], res=x)
                else:
                    a = ops.conv_forward(self._attn_block(w, p + ".self_attn", x, fr), ow, ob)
                    x = ops.layernorm_c(x, a, ln1[0], ln1[1], EPS)
                    h = ops.conv_forward(x, w[p + ".fc1.weight"], w[p + ".fc1.bias"])
                    h = ops.conv_forward(ops.bias_gelu(h, inplace=True), w[p + ".fc2.weight"], w[p + ".fc2.bias"])
                    x = ops.layernorm_c(x, h, ln2[0], ln2[1], EPS)
            if self.layer_norm_first and output_layer is None:
                x = ops.layernorm_c(x, None, w["encoder.layer_norm.weight"], w["encoder.layer_norm.bias"], EPS)
            if fr is not None:
                x = ops.mask_frames(x, fr, inplace=True)
            return x.transpose(1, 2).contiguous(), pad_mask

    def forward(self, source, padding_mask=None, mask=False, output_layer=None, lengths=None):
        return self.extract_features(source, padding_mask=padding_mask, mask=mask, output_layer=output_layer, lengths=lengths)

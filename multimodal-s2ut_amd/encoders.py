"""What the forward-only HF / timm encoders share: asr.py (wav2vec2 CTC), units.py (HuBERT units) and
vision.py (ViT features).  Checkpoint reading, the checked getter with its device copies, the transformer
layer dictionary and the one layer loop (pre-LN or post-LN) on the GEMM, LayerNorm and flash-attention
kernels of the training path, and SpeechEncoder: the feature extractor's conv stack, the feature
projection, the grouped positional convolution and the packing of utterances as [B, Tmax, d] that the two
speech models have in common.  Weights are repacked into the kernels' layouts once, at load."""
import json
import os
import struct
import wave as _wave

import numpy as np
import torch

from . import kernels as K
from .vocoder import pack_conv_weight

SAMPLE_RATE = 16000
NORM_EPS = 1e-7            # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm
CONV_LN_EPS = 1e-5         # nn.LayerNorm's default, in the feature extractor's conv layers
CONFIG_DEFAULTS = {
    "feat_extract_norm": "group", "feat_extract_activation": "gelu", "hidden_act": "gelu", "conv_bias": False,
    "do_stable_layer_norm": False, "conv_dim": [512] * 7, "conv_kernel": [10, 3, 3, 3, 3, 2, 2],
    "conv_stride": [5, 2, 2, 2, 2, 2, 2], "hidden_size": 768, "num_attention_heads": 12, "intermediate_size": 3072,
    "num_hidden_layers": 12, "num_conv_pos_embeddings": 128, "num_conv_pos_embedding_groups": 16,
    "layer_norm_eps": 1e-5, "vocab_size": 32, "pad_token_id": 0, "add_adapter": False,
}
_ST_DTYPES = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16, "I64": torch.int64}
# module names of one transformer layer: first norm, q|k|v (concatenated in this order), attention output,
# second norm, MLP in, MLP out
HF_LAYER = ("layer_norm", ("attention.q_proj", "attention.k_proj", "attention.v_proj"), "attention.out_proj",
            "final_layer_norm", "feed_forward.intermediate_dense", "feed_forward.output_dense")
TIMM_LAYER = ("norm1", ("attn.qkv",), "attn.proj", "norm2", "mlp.fc1", "mlp.fc2")


# ------------------------------------------------------------------------------------------ files

def read_safetensors(path):
    """{name: tensor} of a .safetensors file: 8-byte little-endian header length, JSON header
    ({name: {dtype, shape, data_offsets}}), then the raw little-endian tensors."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 8:
        raise ValueError(f"{path}: not a safetensors file")
    (hlen,) = struct.unpack("<Q", raw[:8])
    if hlen > len(raw) - 8:
        raise ValueError(f"{path}: header length {hlen} exceeds the file")
    header = json.loads(raw[8:8 + hlen].decode("utf-8"))
    data = memoryview(raw)[8 + hlen:]
    out = {}
    for name, meta in header.items():
        if name == "__metadata__":
            continue
        if meta["dtype"] not in _ST_DTYPES:
            raise NotImplementedError(f"{path}: tensor '{name}' has dtype {meta['dtype']}")
        dt = _ST_DTYPES[meta["dtype"]]
        b0, b1 = meta["data_offsets"]
        shape = tuple(meta["shape"])
        numel = int(np.prod(shape)) if shape else 1
        if not (0 <= b0 <= b1 <= len(data)) or b1 - b0 != numel * torch.empty(0, dtype=dt).element_size():
            raise ValueError(f"{path}: tensor '{name}' has offsets {b0}..{b1} for shape {shape}")
        out[name] = torch.frombuffer(bytearray(data[b0:b1]), dtype=dt).reshape(shape) if numel else torch.empty(shape, dtype=dt)
    return out


def load_state_dict(model_dir):
    """Weights of an HF model directory: model.safetensors (in-tree reader) or pytorch_model.bin."""
    st = os.path.join(model_dir, "model.safetensors")
    if os.path.exists(st):
        return read_safetensors(st)
    pt = os.path.join(model_dir, "pytorch_model.bin")
    if os.path.exists(pt):
        return torch.load(pt, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"{model_dir}: neither model.safetensors nor pytorch_model.bin")


def read_json(model_dir, name, required=False):
    """The parsed JSON file of an HF model directory; None where an optional one is absent."""
    path = os.path.join(model_dir, name)
    if not os.path.exists(path):
        if required:
            raise FileNotFoundError(f"{model_dir}: {name} is missing")
        return None
    with open(path) as f:
        return json.load(f)


def read_wav(path):
    """(fp32 numpy [n] = the first channel's int16 / 32768, sample rate) of a 16-bit PCM WAV file."""
    with _wave.open(path, "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise ValueError(f"{path}: 16-bit PCM expected (sample width {w.getsampwidth()}, {w.getcomptype()})")
        sr, ch = w.getframerate(), w.getnchannels()
        x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, ch)[:, 0]
    return x.astype(np.float32) / 32768.0, sr


def wave_batches(root, files, batch_size, sampling_rate, min_samples=0):
    """(names, waveforms) of batch_size of the WAV files under root at a time, in order; every file at the
    model's sample rate and of at least min_samples samples."""
    for i in range(0, len(files), batch_size):
        names, waves = files[i:i + batch_size], []
        for f in names:
            x, sr = read_wav(os.path.join(root, f))
            if sr != sampling_rate:
                raise ValueError(f"{f}: sample rate {sr}, the model expects {sampling_rate}")
            if len(x) < min_samples:
                raise ValueError(f"{f}: {len(x)} samples are fewer than the feature extractor's receptive field of "
                                 f"{min_samples}")
            waves.append(x)
        yield names, waves


# ------------------------------------------------------------------------------------------ weights

class Weights:
    """The checked getter of a state dict and the device copies of what it returns.  what starts the
    message for a missing key ("ViT checkpoint"); hints: {name: text added to that name's shape error}."""

    def __init__(self, sd, what, device, hints=None):
        self.sd, self.what, self.device, self.hints = sd, what, torch.device(device), hints or {}

    def get(self, name, shape):
        # the kernels trust these shapes: the packed images and the GEMMs are sized by them
        if name not in self.sd:
            raise KeyError(f"{self.what}: '{name}' is missing")
        t = self.sd[name]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, the config implies {tuple(shape)}" +
                             self.hints.get(name, ""))
        return t.float()

    def f32(self, t):
        return t.contiguous().to(self.device)

    def f16(self, t):
        return t.half().contiguous().to(self.device)


def layer_dict(w, p, d, Fd, names):
    """One transformer layer's fp16 weights under the key prefix p: ln1_g ln1_b wqkv bqkv wo bo ln2_g ln2_b
    w1 b1 w2 b2.  w: Weights; names: HF_LAYER or TIMM_LAYER."""
    ln1, qkv, wo, ln2, fc1, fc2 = names
    r = 3 * d // len(qkv)

    def t(n, kind, *shape):
        return w.f16(w.get(f"{p}{n}.{kind}", shape))

    return {"ln1_g": t(ln1, "weight", d), "ln1_b": t(ln1, "bias", d),
            "wqkv": w.f16(torch.cat([w.get(f"{p}{n}.weight", (r, d)) for n in qkv])),
            "bqkv": w.f16(torch.cat([w.get(f"{p}{n}.bias", (r,)) for n in qkv])),
            "wo": t(wo, "weight", d, d), "bo": t(wo, "bias", d),
            "ln2_g": t(ln2, "weight", d), "ln2_b": t(ln2, "bias", d),
            "w1": t(fc1, "weight", Fd, d), "b1": t(fc1, "bias", Fd), "w2": t(fc2, "weight", d, Fd), "b2": t(fc2, "bias", d)}


def transformer_layers(Hb, layers, H, eps, lens32=None, *, post_ln=False, on_qkv=None):
    """Transformer layers (packed q|k|v with bias, erf-GELU MLP, both residuals in the GEMM epilogue) over
    fp16 [B, Tmax, d] -> fp16 [B * Tmax, d]; layers: layer_dict()s.  Pre-LN (wav2vec2 with stable layer
    norm, ViT): each LayerNorm feeds its sublayer.  post_ln (HuBERT-base): it follows the residual sum.
    on_qkv(layer index, qkv fp16 [B * Tmax, 3 d]) is called right after a layer's qkv GEMM, on the same stream."""
    B, Tm, d = Hb.shape
    R, hd = B * Tm, d // H
    X = Hb.reshape(R, d)
    for l, L in enumerate(layers):
        y = X if post_ln else K.layernorm(X, L["ln1_g"], L["ln1_b"], eps)[0]
        qkv = K.linear(y, L["wqkv"], L["bqkv"])
        if on_qkv is not None:
            on_qkv(l, qkv)
        o = torch.empty(R, d, dtype=K.F16, device=X.device)
        K.mha_fwd(qkv, qkv[:, d:], qkv[:, 2 * d:], o, 3 * d, 3 * d, 3 * d, d, B, H, Tm, Tm, hd, hd ** -0.5,
                  key_len=lens32)
        X = K.linear(o, L["wo"], L["bo"], epi=K.EPI_DROP_RESID, aux=X)
        if post_ln:
            X = K.layernorm(X, L["ln1_g"], L["ln1_b"], eps)[0]
        y = X if post_ln else K.layernorm(X, L["ln2_g"], L["ln2_b"], eps)[0]
        z = torch.empty(R, L["w1"].shape[0], dtype=K.F16, device=X.device)
        f = K.linear(y, L["w1"], L["b1"], epi=K.EPI_GELU_DROP, out2=z)
        X = K.linear(f, L["w2"], L["b2"], epi=K.EPI_DROP_RESID, aux=X)
        if post_ln:
            X = K.layernorm(X, L["ln2_g"], L["ln2_b"], eps)[0]
    return X


# ------------------------------------------------------------------------------------------ speech

def validate_config(cfg, family, defaults, norm, stable_ln, bias_optional):
    """Validated copy of a wav2vec2-style config.json dict (the keys the forward reads) over defaults.
    family names the model in the messages; norm and stable_ln are the feat_extract_norm and the
    do_stable_layer_norm the family's forward implements; bias_optional: conv_bias false is allowed."""
    c = dict(defaults)
    c.update(cfg)
    if c["feat_extract_norm"] != norm:
        raise NotImplementedError(f"{family} feat_extract_norm '{c['feat_extract_norm']}' is not supported (only "
                                  f"\"{norm}\")")
    if bool(c["do_stable_layer_norm"]) != stable_ln:
        raise NotImplementedError(f"{family} with do_stable_layer_norm {str(not stable_ln).lower()} "
                                  f"({'post' if stable_ln else 'pre'}-LN encoder) is not supported")
    if c.get("add_adapter"):
        raise NotImplementedError(f"{family} adapters (add_adapter) are not supported")
    for key in ("feat_extract_activation", "hidden_act"):
        if c[key] != "gelu":
            raise NotImplementedError(f"{family} {key} '{c[key]}' is not supported (only \"gelu\")")
    if not c["conv_bias"] and not bias_optional:
        raise NotImplementedError(f"{family} with conv_bias false is not supported")
    n = len(c["conv_dim"])
    if n < 1 or len(c["conv_kernel"]) != n or len(c["conv_stride"]) != n:
        raise ValueError(f"{family} config: conv_dim, conv_kernel and conv_stride differ in length")
    d, H = c["hidden_size"], c["num_attention_heads"]
    if d % H or d // H not in K.FLASH_HD:
        raise NotImplementedError(f"{family} head dim {d}/{H} (hidden_size / num_attention_heads) is not supported "
                                  f"(the attention kernel has {K.FLASH_HD})")
    if d % c["num_conv_pos_embedding_groups"]:
        raise ValueError(f"{family} config: num_conv_pos_embedding_groups does not divide hidden_size")
    return c


def frame_counts(n, kernels, strides):
    """Frames after each feature-extractor layer for n samples: (T - k) // s + 1, layer by layer."""
    out = []
    for k, s in zip(kernels, strides):
        n = (n - k) // s + 1 if n >= k else 0
        out.append(n)
    return out


def receptive_field(kernels, strides):
    """Samples one output frame of the feature extractor spans (400 for the released models)."""
    r = 1
    for k, s in zip(reversed(kernels), reversed(strides)):
        r = (r - 1) * s + k
    return r


def fold_pos_conv_weight_norm(sd, prefix="wav2vec2."):
    """State dict with the positional convolution's weight norm folded (weight_norm(dim=2): w = g v / |v|,
    the norm over dims (0, 1) of each tap).  Accepts ``weight_g / weight_v`` and
    ``parametrizations.weight.original0 / original1``; a plain ``weight`` passes through.  prefix: what
    the checkpoint puts in front of ``encoder.`` ("wav2vec2.", "hubert." or "")."""
    base = prefix + "encoder.pos_conv_embed.conv."
    out = dict(sd)
    for gk, vk in (("weight_g", "weight_v"), ("parametrizations.weight.original0", "parametrizations.weight.original1")):
        if base + vk in sd:
            v, g = sd[base + vk].float(), sd[base + gk].float()
            norm = v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
            out[base + "weight"] = v * (g.reshape(1, 1, -1) / norm)
            del out[base + gk], out[base + vk]
    return out


class _ConvLayer:
    __slots__ = ("w", "b", "g", "be", "cout", "k", "stride")

    def __init__(self, w, b, g, be, cout, k, stride):
        self.w, self.b, self.g, self.be, self.cout, self.k, self.stride = w, b, g, be, cout, k, stride


class SpeechEncoder:
    """What HF's Wav2Vec2Model and HubertModel share in eval mode: the loading of the conv stack, the feature
    projection, the positional convolution, encoder.layer_norm and the first n_layers transformer layers from
    under the key prefix p, and the forward up to the layers.  A subclass supplies extract()."""

    def __init__(self, w, c, p, n_layers, sampling_rate):
        self.cfg, self.device, self.sampling_rate = c, w.device, int(sampling_rate)
        get, f32, f16 = w.get, w.f32, w.f16
        d, Hh = c["hidden_size"], c["num_attention_heads"]
        self.d, self.H, self.hd, self.eps = d, Hh, d // Hh, float(c["layer_norm_eps"])
        self.post_ln = not c["do_stable_layer_norm"]
        self.kernels, self.strides = list(c["conv_kernel"]), list(c["conv_stride"])
        self.min_samples = receptive_field(self.kernels, self.strides)
        self.conv, cin = [], 1
        for i, (co, k, s) in enumerate(zip(c["conv_dim"], self.kernels, self.strides)):
            q = f"{p}feature_extractor.conv_layers.{i}."
            W = get(q + "conv.weight", (co, cin, k))
            wt = f32(W[:, 0, :].t()) if i == 0 else pack_conv_weight(W).to(w.device)
            b = f32(get(q + "conv.bias", (co,))) if c["conv_bias"] else None
            normed = i == 0 or c["feat_extract_norm"] == "layer"      # "group": a GroupNorm after layer 0 only
            g = f32(get(q + "layer_norm.weight", (co,))) if normed else None
            be = f32(get(q + "layer_norm.bias", (co,))) if normed else None
            self.conv.append(_ConvLayer(wt, b, g, be, co, k, s))
            cin = co
        q = p + "feature_projection."
        self.fp_ln = bool(c.get("feat_proj_layer_norm", True))
        if self.fp_ln:
            self.fp_g, self.fp_b = f16(get(q + "layer_norm.weight", (cin,))), f16(get(q + "layer_norm.bias", (cin,)))
        self.fp_w, self.fp_bias = f16(get(q + "projection.weight", (d, cin))), f16(get(q + "projection.bias", (d,)))
        self.pos_k, self.pos_groups = int(c["num_conv_pos_embeddings"]), int(c["num_conv_pos_embedding_groups"])
        q = p + "encoder.pos_conv_embed.conv."
        cg = d // self.pos_groups
        Wp = get(q + "weight", (d, cg, self.pos_k))
        self.pos_w = torch.cat([pack_conv_weight(Wp[g * cg:(g + 1) * cg]) for g in range(self.pos_groups)]).to(w.device)
        self.pos_b = f32(get(q + "bias", (d,)))
        q = p + "encoder.layer_norm."
        self.enc_g, self.enc_b = f16(get(q + "weight", (d,))), f16(get(q + "bias", (d,)))
        Fd = c["intermediate_size"]
        self.layers = [layer_dict(w, f"{p}encoder.layers.{l}.", d, Fd, HF_LAYER) for l in range(n_layers)]

    def _wave(self, wave, sr=None):
        if sr is not None and int(sr) != self.sampling_rate:
            raise ValueError(f"the model was trained on {self.sampling_rate} Hz audio, got {sr} Hz")
        x = torch.as_tensor(wave, dtype=torch.float32).reshape(-1)
        if x.numel() < self.min_samples:
            raise ValueError(f"utterance of {x.numel()} samples is shorter than the feature extractor's receptive "
                             f"field of {self.min_samples}")
        return x.to(self.device).contiguous()

    def positional(self, h, out=None):
        """h + GELU(pos_conv(h)) over the extractor's fp16 [T, d] of one utterance.  The convolution yields
        T + 1 frames for an even kernel and HF drops the last: T outputs either way."""
        return K.asr_conv(h, self.pos_w, self.pos_b, self.d, self.pos_k, 1, self.pos_k // 2, self.pos_groups,
                          T_out=h.shape[0], res=h, out=out)

    def utterance(self, x, out=None):
        """fp32 waveform on the device -> fp16 [T, d] (into out, if given): extract(), then positional()."""
        return self.positional(self.extract(x), out)

    def pack(self, waves, sr=None):
        """Waveforms -> (fp16 [B, Tmax, d] of utterance() rows, zero past an utterance's length; lens (list);
        lens32 on the device, None for a single utterance: nothing to mask).  One utterance at a time: no
        padding enters a convolution."""
        xs = [self._wave(w, sr) for w in waves]
        lens = [frame_counts(x.numel(), self.kernels, self.strides)[-1] for x in xs]
        if len(xs) == 1:
            return self.utterance(xs[0]).unsqueeze(0), lens, None
        Hb = torch.zeros(len(xs), max(lens), self.d, dtype=K.F16, device=self.device)
        for b, x in enumerate(xs):
            self.utterance(x, out=Hb[b, :lens[b]])
        return Hb, lens, torch.tensor(lens, dtype=torch.int32, device=self.device)

    def layers_forward(self, Hb, lens32=None):
        """The loaded transformer layers over fp16 [B, Tmax, d] -> fp16 [B * Tmax, d]."""
        return transformer_layers(Hb, self.layers, self.H, self.eps, lens32, post_ln=self.post_ln)

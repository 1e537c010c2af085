"""CPU restatement of HF Wav2Vec2ForCTC's forward (feat_extract_norm "layer", do_stable_layer_norm, eval
mode) with Wav2Vec2Processor's normalisation and greedy CTC decoding, in torch fp32, for the ASR tests.
Nothing here imports the product package.  ``transformers`` is not installed: this file restates the
library's arithmetic from its documented architecture, it is not checked against the library.

Two modes, the convention of tests/vocoder_ref.py.  The fp32 restatement (emulate=False) is the reference
every GPU result is compared with.  The fp16-storage emulation (emulate=True) does the same arithmetic in
fp32 but rounds the weights the product keeps in fp16, and every tensor the product stores in fp16,
through .half().float() at the places where multimodal-s2ut_amd/asr.py stores one; its distance from the
fp32 restatement is the error floor a test's allowance is a multiple of (TOL_FACTOR).  The product keeps
in fp32: the waveform and its normalisation, layer 0's weights, every convolution's bias and the
extractor's LayerNorm parameters, the head's bias and the logits.

Tensors are time-major [T, C] at this module's interfaces, as in the product."""
import json
import math
import os
import struct
import wave as _wave

import numpy as np
import torch
import torch.nn.functional as F

TOL_FACTOR = 3.0            # allowance = TOL_FACTOR x the emulation's own max-abs distance
NORM_EPS, CONV_LN_EPS = 1e-7, 1e-5
KERNELS, STRIDES = [10, 3, 3, 3, 3, 2, 2], [5, 2, 2, 2, 2, 2, 2]

BASE = dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, feat_extract_activation="gelu",
            hidden_act="gelu", conv_kernel=KERNELS, conv_stride=STRIDES, num_conv_pos_embeddings=128,
            layer_norm_eps=1e-5, vocab_size=32, pad_token_id=0)
SMALL = dict(BASE, conv_dim=[64] * 7, hidden_size=128, num_attention_heads=2, intermediate_size=256,
             num_hidden_layers=2, num_conv_pos_embedding_groups=2)
# the released large models' widths, two layers deep
WIDE = dict(BASE, conv_dim=[512] * 7, hidden_size=1024, num_attention_heads=16, intermediate_size=4096,
            num_hidden_layers=2, num_conv_pos_embedding_groups=16)
VOCAB = {t: i for i, t in enumerate(["<pad>", "<s>", "</s>", "<unk>", "|"] + list("ETAONIHSRDLUMWCFGYPBVKJXQZ") + ["'"])}


def _q(emulate):
    return (lambda t: t.half().float()) if emulate else (lambda t: t)


# ------------------------------------------------------------------------------------------ fixtures

def make_state_dict(cfg, seed=0, style="g_v", blank_bias=0.0):
    """Seeded state dict under HF's key names.  style "g_v": pos_conv_embed.conv.weight_g / weight_v;
    "param": ...conv.parametrizations.weight.original0 / original1.  Scales keep a unit-variance input
    at roughly unit variance.  blank_bias is added to the head's bias at the pad id: with +2, greedy
    decoding sees blank frames and repeats."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    sd = {}

    def ln(name, n):
        sd[name + ".weight"], sd[name + ".bias"] = 1.0 + 0.1 * rn(n), 0.1 * rn(n)

    def lin(name, nout, nin, gain=1.0):
        sd[name + ".weight"], sd[name + ".bias"] = gain * rn(nout, nin) / nin ** 0.5, 0.1 * rn(nout)

    cin = 1
    for i, (co, k) in enumerate(zip(cfg["conv_dim"], cfg["conv_kernel"])):
        p = f"wav2vec2.feature_extractor.conv_layers.{i}"
        sd[p + ".conv.weight"], sd[p + ".conv.bias"] = rn(co, cin, k) / (cin * k) ** 0.5, 0.1 * rn(co)
        ln(p + ".layer_norm", co)
        cin = co
    d, Fd, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    ln("wav2vec2.feature_projection.layer_norm", cin)
    lin("wav2vec2.feature_projection.projection", d, cin)
    k, cg = cfg["num_conv_pos_embeddings"], d // cfg["num_conv_pos_embedding_groups"]
    gk, vk = ("weight_g", "weight_v") if style == "g_v" else \
        ("parametrizations.weight.original0", "parametrizations.weight.original1")
    p = "wav2vec2.encoder.pos_conv_embed.conv."
    sd[p + vk] = rn(d, cg, k)
    sd[p + gk] = ((d / k) ** 0.5 * (1.0 + 0.1 * rn(k))).abs().view(1, 1, k)   # folded taps of std 1 / sqrt(cg k)
    sd[p + "bias"] = 0.1 * rn(d)
    for l in range(cfg["num_hidden_layers"]):
        p = f"wav2vec2.encoder.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + "attention." + n, d, d)
        ln(p + "layer_norm", d)
        lin(p + "feed_forward.intermediate_dense", Fd, d)
        lin(p + "feed_forward.output_dense", d, Fd)
        ln(p + "final_layer_norm", d)
    ln("wav2vec2.encoder.layer_norm", d)
    lin("lm_head", V, d)
    sd["lm_head.bias"][cfg["pad_token_id"]] += blank_bias
    sd["wav2vec2.masked_spec_embed"] = rn(d)           # present in released checkpoints, unused in eval mode
    return sd


def make_wave(n, seed=0, dc=0.0):
    """Seeded chirp plus noise (plus a DC offset), quantised: int16 numpy [n]."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = 0.3 * np.sin(2 * np.pi * (200.0 + 900.0 * t) * t) + 0.05 * g.standard_normal(n) + dc
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def to_float(pcm):
    return torch.from_numpy(pcm.astype(np.float32) / 32768.0)


def write_wav(path, pcm, sr=16000, channels=1):
    with _wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.repeat(pcm.astype("<i2")[:, None], channels, 1).tobytes())


def write_safetensors(path, sd):
    """The format's documented layout: u64 LE header length, JSON header, raw LE tensors."""
    codes = {torch.float32: "F32", torch.float16: "F16", torch.int64: "I64"}
    header, blobs, off = {"__metadata__": {"format": "pt"}}, [], 0
    for name, t in sd.items():
        b = t.contiguous().numpy().tobytes()
        header[name] = {"dtype": codes[t.dtype], "shape": list(t.shape), "data_offsets": [off, off + len(b)]}
        blobs.append(b)
        off += len(b)
    h = json.dumps(header).encode("utf-8")
    h += b" " * (-len(h) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)) + h + b"".join(blobs))


def write_model_dir(path, sd, cfg, fmt="bin", vocab=VOCAB, tokenizer_cfg=None):
    """An HF model directory: config.json, vocab.json, the weights, optionally tokenizer_config.json."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    with open(os.path.join(path, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    if tokenizer_cfg is not None:
        with open(os.path.join(path, "tokenizer_config.json"), "w") as f:
            json.dump(tokenizer_cfg, f)
    if fmt == "bin":
        torch.save(sd, os.path.join(path, "pytorch_model.bin"))
    else:
        write_safetensors(os.path.join(path, "model.safetensors"), sd)


# ------------------------------------------------------------------------------------------ pieces

def frame_count(n, kernels=KERNELS, strides=STRIDES):
    for k, s in zip(kernels, strides):
        n = (n - k) // s + 1
    return n


def normalise(x):
    """Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm: (x - mean) / sqrt(var + 1e-7), population variance."""
    return (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + NORM_EPS)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def conv0(x, W, b, g, be, stride, *, normalize=True, emulate=False):
    """kernels.asr_conv0: waveform [n] -> [T0, C]; W [C, 1, k], nothing but the output is rounded."""
    xn = normalise(x) if normalize else x
    v = F.conv1d(xn[None, None], W, b, stride=stride)[0].t()
    return _q(emulate)(gelu(F.layer_norm(v, (v.shape[1],), g, be, CONV_LN_EPS)))


def conv_strided(x, W, b, stride, *, emulate=False):
    """kernels.asr_conv without a residual: x [T, Cin], W [Cout, Cin, k] -> [(T - k) // stride + 1, Cout]."""
    q = _q(emulate)
    return q(F.conv1d(q(x).t()[None], q(W), b, stride=stride)[0].t())


def ln_gelu(x, g, be, eps=CONV_LN_EPS, *, emulate=False):
    """kernels.asr_ln_gelu: GELU(LayerNorm(x)) over fp16-stored rows, fp32 parameters."""
    q = _q(emulate)
    return q(gelu(F.layer_norm(q(x), (x.shape[1],), g, be, eps)))


def fold_pos(g, v):
    """weight_norm(dim=2): w = g v / |v|, the norm over dims (0, 1) of each tap."""
    return v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())


def pos_conv(h, W, b, groups, *, emulate=False):
    """h + GELU(Conv1d(h; k, padding k // 2, groups)) with the last frame dropped for an even k."""
    q = _q(emulate)
    k = W.shape[2]
    v = F.conv1d(q(h).t()[None], q(W), b, padding=k // 2, groups=groups)[0].t()
    if k % 2 == 0:
        v = v[:-1]
    return q(q(h) + gelu(v))


def attention(qkv, H, *, emulate=False):
    """Self-attention over [T, 3 d] = q | k | v rows (no mask) -> [T, d]; the scores are scaled by hd^-0.5."""
    qq = _q(emulate)
    T, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    q_, k_, v_ = (qkv[:, i * d:(i + 1) * d].reshape(T, H, hd).transpose(0, 1) for i in range(3))
    P = torch.softmax(q_ @ k_.transpose(1, 2) * hd ** -0.5, dim=-1)
    return qq((qq(P) @ v_).transpose(0, 1).reshape(T, d))


def _w(sd, emulate):
    q = _q(emulate)
    return (lambda n: q(sd[n + ".weight"].float())), (lambda n: q(sd[n + ".bias"].float()))


def pos_weight(sd):
    p = "wav2vec2.encoder.pos_conv_embed.conv."
    for gk, vk in (("weight_g", "weight_v"), ("parametrizations.weight.original0", "parametrizations.weight.original1")):
        if p + vk in sd:
            return fold_pos(sd[p + gk].float(), sd[p + vk].float())
    return sd[p + "weight"].float()


def forward(sd, cfg, x, emulate=False):
    """Waveform fp32 [n] -> fp32 logits [T, V]."""
    q = _q(emulate)
    W, B = _w(sd, emulate)
    raw = lambda n: sd[n].float()
    eps = cfg["layer_norm_eps"]
    p = "wav2vec2.feature_extractor.conv_layers."
    h = conv0(x, raw(p + "0.conv.weight"), raw(p + "0.conv.bias"), raw(p + "0.layer_norm.weight"),
              raw(p + "0.layer_norm.bias"), cfg["conv_stride"][0], emulate=emulate)
    for i in range(1, len(cfg["conv_dim"])):
        h = conv_strided(h, raw(f"{p}{i}.conv.weight"), raw(f"{p}{i}.conv.bias"), cfg["conv_stride"][i], emulate=emulate)
        h = ln_gelu(h, raw(f"{p}{i}.layer_norm.weight"), raw(f"{p}{i}.layer_norm.bias"), emulate=emulate)
    ln = lambda t, n: q(F.layer_norm(t, (t.shape[1],), W(n), B(n), eps))
    lin = lambda t, n: t @ W(n).t() + B(n)
    h = q(lin(ln(h, "wav2vec2.feature_projection.layer_norm"), "wav2vec2.feature_projection.projection"))
    h = pos_conv(h, pos_weight(sd), raw("wav2vec2.encoder.pos_conv_embed.conv.bias"), cfg["num_conv_pos_embedding_groups"],
                 emulate=emulate)
    for l in range(cfg["num_hidden_layers"]):
        p = f"wav2vec2.encoder.layers.{l}."
        y = ln(h, p + "layer_norm")
        qkv = q(torch.cat([lin(y, p + f"attention.{n}_proj") for n in "qkv"], 1))
        o = attention(qkv, cfg["num_attention_heads"], emulate=emulate)
        h = q(h + lin(o, p + "attention.out_proj"))
        y = ln(h, p + "final_layer_norm")
        z = q(lin(y, p + "feed_forward.intermediate_dense"))
        h = q(h + lin(q(gelu(z)), p + "feed_forward.output_dense"))
    y = ln(h, "wav2vec2.encoder.layer_norm")
    return y @ W("lm_head").t() + raw("lm_head.bias")


_CACHE = {}


def reference(cfg_name, seed, n, wave_seed, blank_bias=0.0, dc=0.0):
    """(sd, pcm, fp32 logits, emulated logits) of a fixture, computed once per process and shared."""
    key = (cfg_name, seed, n, wave_seed, blank_bias, dc)
    if key not in _CACHE:
        cfg = {"small": SMALL, "wide": WIDE}[cfg_name]
        sd = make_state_dict(cfg, seed, blank_bias=blank_bias)
        pcm = make_wave(n, wave_seed, dc)
        x = to_float(pcm)
        with torch.no_grad():
            _CACHE[key] = (sd, pcm, forward(sd, cfg, x), forward(sd, cfg, x, emulate=True))
    return _CACHE[key]


# the end-to-end fixtures of tests/test_gpu_asr.py: (config, weight seed, samples, wave seed, blank bias)
E2E_FIXTURES = [("small", 0, 8000, 1, 0.0), ("small", 0, 12345, 2, 0.0), ("small", 0, 48000, 3, 0.0),
                ("small", 0, 8000, 1, 2.0), ("small", 0, 12345, 2, 2.0), ("small", 0, 48000, 3, 2.0)]
MARGIN_CAP = 0.25           # at most this share of frames may have a top-2 margin below 2 x allowance


def margins(logits):
    top = logits.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


# ------------------------------------------------------------------------------------------ decoding

CLEANUP = ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"),
           (" 's", "'s"), (" 've", "'ve"), (" 're", "'re"))


def decode(ids, vocab=VOCAB, blank=0, delimiter="|", cleanup=True):
    """Wav2Vec2CTCTokenizer.decode of per-frame ids: collapse runs, drop the blank, '|' -> ' ', strip."""
    inv = {i: t for t, i in vocab.items()}
    toks, prev = [], None
    for i in ids:
        i = int(i)
        if i != prev and i != blank:
            toks.append(" " if inv[i] == delimiter else inv[i])
        prev = i
    s = "".join(toks).strip()
    if cleanup:
        for a, b in CLEANUP:
            s = s.replace(a, b)
    return s

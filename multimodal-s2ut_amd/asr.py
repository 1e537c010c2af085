"""ASR transcription of synthesized speech: HF ``Wav2Vec2ForCTC`` (the wav2vec2-large family with
feat_extract_norm "layer" and do_stable_layer_norm) forward on HIP kernels, then greedy CTC decoding --
the step of the reference pipeline between the vocoder and BLEU (mm_s2ut/scripts/transcript.py).

Forward only.  The feature extractor and the positional convolution run one utterance at a time on the
kernels of csrc/asr.hip (no padding ever enters a convolution); the transformer layers run on the GEMM,
LayerNorm and flash-attention kernels of the training path, on up to ``batch_size`` utterances packed
as [B, Tmax, d] with key-length masking.  Activations are time-major fp16 [T, C]; the logits are fp32.
Weight norm is folded and the weights are repacked into the kernels' layouts once, at load.

``transformers`` is not a dependency: the semantics are restated here (and in tests/asr_ref.py), the
checkpoint's key names and tensor layouts pin the loader."""
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
CLEANUP = ((" .", "."), (" ?", "?"), (" !", "!"), (" ,", ","), (" ' ", "'"), (" n't", "n't"), (" 'm", "'m"),
           (" 's", "'s"), (" 've", "'ve"), (" 're", "'re"))
_ST_DTYPES = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16, "I64": torch.int64}


class NonFiniteLogits(RuntimeError):
    """An utterance's logits hold inf or NaN (fp16 activations overflowed): no transcript is written."""


def parse_config(cfg):
    """Validated copy of a Wav2Vec2 config.json dict (the keys the forward reads)."""
    c = dict(CONFIG_DEFAULTS)
    c.update(cfg)
    if c["feat_extract_norm"] != "layer":
        raise NotImplementedError(f"wav2vec2 feat_extract_norm '{c['feat_extract_norm']}' is not supported (only "
                                  "\"layer\": the wav2vec2-large family)")
    if not c["do_stable_layer_norm"]:
        raise NotImplementedError("wav2vec2 with do_stable_layer_norm false (post-LN encoder) is not supported")
    if c.get("add_adapter"):
        raise NotImplementedError("wav2vec2 adapters (add_adapter) are not supported")
    for key in ("feat_extract_activation", "hidden_act"):
        if c[key] != "gelu":
            raise NotImplementedError(f"wav2vec2 {key} '{c[key]}' is not supported (only \"gelu\")")
    if not c["conv_bias"]:
        raise NotImplementedError("wav2vec2 with conv_bias false is not supported")
    n = len(c["conv_dim"])
    if n < 1 or len(c["conv_kernel"]) != n or len(c["conv_stride"]) != n:
        raise ValueError("wav2vec2 config: conv_dim, conv_kernel and conv_stride differ in length")
    d, H = c["hidden_size"], c["num_attention_heads"]
    if d % H or d // H not in K.FLASH_HD:
        raise NotImplementedError(f"wav2vec2 head dim {d}/{H} is not supported (the attention kernel has "
                                  f"{K.FLASH_HD})")
    if d % c["num_conv_pos_embedding_groups"]:
        raise ValueError("wav2vec2 config: num_conv_pos_embedding_groups does not divide hidden_size")
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


def read_wav(path):
    """(fp32 numpy [n] = the first channel's int16 / 32768, sample rate) of a 16-bit PCM WAV file."""
    with _wave.open(path, "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise ValueError(f"{path}: 16-bit PCM expected (sample width {w.getsampwidth()}, {w.getcomptype()})")
        sr, ch = w.getframerate(), w.getnchannels()
        x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, ch)[:, 0]
    return x.astype(np.float32) / 32768.0, sr


def collapse(ids, blank):
    """Frame ids -> CTC token ids: runs of equal ids collapse to one, then the blank drops."""
    out, prev = [], None
    for i in ids:
        i = int(i)
        if i != prev and i != blank:
            out.append(i)
        prev = i
    return out


def tokens_to_text(tokens, id_to_token, delimiter="|", cleanup=True, lower=False):
    """Collapsed token ids -> text as Wav2Vec2CTCTokenizer decodes them: the word delimiter becomes a
    space, the string is stripped (and lower-cased with do_lower_case), and with cleanup HF's fixed list
    of replacements applies."""
    s = "".join(" " if id_to_token[t] == delimiter else id_to_token[t] for t in tokens).strip()
    if lower:
        s = s.lower()
    if cleanup:
        for a, b in CLEANUP:
            s = s.replace(a, b)
    return s


def greedy_decode(ids, id_to_token, blank, delimiter="|", cleanup=True, lower=False):
    """Per-frame argmax ids -> text (host restatement of the device path: collapse + tokens_to_text)."""
    return tokens_to_text(collapse(ids, blank), id_to_token, delimiter, cleanup, lower)


def prenorm_layers(Hb, layers, H, eps, lens32=None):
    """Pre-LN transformer layers (packed q|k|v with bias, erf-GELU MLP, both residuals in the GEMM
    epilogue) over fp16 [B, Tmax, d] -> fp16 [B * Tmax, d].  layers: dicts of ln1_g ln1_b wqkv bqkv wo bo
    ln2_g ln2_b w1 b1 w2 b2.  Shared by the wav2vec2 encoder here and the ViT blocks of vision.py."""
    B, Tm, d = Hb.shape
    R, hd = B * Tm, d // H
    X = Hb.reshape(R, d)
    for L in layers:
        y = K.layernorm(X, L["ln1_g"], L["ln1_b"], eps)[0]
        qkv = K.linear(y, L["wqkv"], L["bqkv"])
        o = torch.empty(R, d, dtype=K.F16, device=X.device)
        K.mha_fwd(qkv, qkv[:, d:], qkv[:, 2 * d:], o, 3 * d, 3 * d, 3 * d, d, B, H, Tm, Tm, hd, hd ** -0.5,
                  key_len=lens32)
        X = K.linear(o, L["wo"], L["bo"], epi=K.EPI_DROP_RESID, aux=X)
        y = K.layernorm(X, L["ln2_g"], L["ln2_b"], eps)[0]
        z = torch.empty(R, L["w1"].shape[0], dtype=K.F16, device=X.device)
        f = K.linear(y, L["w1"], L["b1"], epi=K.EPI_GELU_DROP, out2=z)
        X = K.linear(f, L["w2"], L["b2"], epi=K.EPI_DROP_RESID, aux=X)
    return X


class _ConvLayer:
    __slots__ = ("w", "b", "g", "be", "cout", "k", "stride")

    def __init__(self, w, b, g, be, cout, k, stride):
        self.w, self.b, self.g, self.be, self.cout, self.k, self.stride = w, b, g, be, cout, k, stride


class Wav2Vec2CTC:
    """HF Wav2Vec2ForCTC in eval mode plus Wav2Vec2Processor's normalisation and greedy decoding."""

    def __init__(self, state_dict, config, vocab, tokenizer_cfg=None, preprocessor_cfg=None, device="cuda"):
        self.cfg = c = parse_config(config)
        self.device = dev = torch.device(device)
        tok, pre = dict(tokenizer_cfg or {}), dict(preprocessor_cfg or {})
        self.delimiter = tok.get("word_delimiter_token", "|")
        self.cleanup = bool(tok.get("clean_up_tokenization_spaces", True))
        self.lower = bool(tok.get("do_lower_case", False))
        if not pre.get("do_normalize", True):
            raise NotImplementedError("preprocessor_config.json with do_normalize false is not supported (the "
                                      "layer-norm wav2vec2 models normalise each utterance)")
        self.sampling_rate = int(pre.get("sampling_rate", SAMPLE_RATE))
        self.blank = int(c["pad_token_id"])
        self.V = V = int(c["vocab_size"])
        self.id_to_token = {int(i): t for t, i in vocab.items()}
        if sorted(self.id_to_token) != list(range(V)):
            raise ValueError(f"vocab.json (with added_tokens.json, where the directory has one) does not map onto "
                             f"the ids 0..{V - 1} of the head (vocab_size {V})")
        if not 0 <= self.blank < V:
            raise ValueError(f"pad_token_id {self.blank} outside the vocabulary of {V}")
        sd = fold_pos_conv_weight_norm(state_dict)
        d, Hh, Fd = c["hidden_size"], c["num_attention_heads"], c["intermediate_size"]
        self.d, self.H, self.hd, self.eps = d, Hh, d // Hh, float(c["layer_norm_eps"])

        def get(name, shape):
            # the kernels trust these shapes: the packed images are sized by them
            if name not in sd:
                raise KeyError(f"wav2vec2 checkpoint: '{name}' is missing")
            t = sd[name]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} has shape {tuple(t.shape)}, the config implies {tuple(shape)}")
            return t.float()

        f32 = lambda t: t.contiguous().to(dev)
        f16 = lambda t: t.half().contiguous().to(dev)
        self.kernels, self.strides = list(c["conv_kernel"]), list(c["conv_stride"])
        self.min_samples = receptive_field(self.kernels, self.strides)
        self.conv, cin = [], 1
        for i, (co, k, s) in enumerate(zip(c["conv_dim"], self.kernels, self.strides)):
            p = f"wav2vec2.feature_extractor.conv_layers.{i}."
            W = get(p + "conv.weight", (co, cin, k))
            w = f32(W[:, 0, :].t()) if i == 0 else pack_conv_weight(W).to(dev)
            self.conv.append(_ConvLayer(w, f32(get(p + "conv.bias", (co,))), f32(get(p + "layer_norm.weight", (co,))),
                                        f32(get(p + "layer_norm.bias", (co,))), co, k, s))
            cin = co
        p = "wav2vec2.feature_projection."
        self.fp_g, self.fp_b = f16(get(p + "layer_norm.weight", (cin,))), f16(get(p + "layer_norm.bias", (cin,)))
        self.fp_w, self.fp_bias = f16(get(p + "projection.weight", (d, cin))), f16(get(p + "projection.bias", (d,)))
        self.pos_k, self.pos_groups = int(c["num_conv_pos_embeddings"]), int(c["num_conv_pos_embedding_groups"])
        p = "wav2vec2.encoder.pos_conv_embed.conv."
        cg = d // self.pos_groups
        Wp = get(p + "weight", (d, cg, self.pos_k))
        self.pos_w = torch.cat([pack_conv_weight(Wp[g * cg:(g + 1) * cg]) for g in range(self.pos_groups)]).to(dev)
        self.pos_b = f32(get(p + "bias", (d,)))
        self.layers = []
        for l in range(c["num_hidden_layers"]):
            p = f"wav2vec2.encoder.layers.{l}."
            a = p + "attention."
            self.layers.append({
                "ln1_g": f16(get(p + "layer_norm.weight", (d,))), "ln1_b": f16(get(p + "layer_norm.bias", (d,))),
                "wqkv": f16(torch.cat([get(a + f"{n}_proj.weight", (d, d)) for n in "qkv"])),
                "bqkv": f16(torch.cat([get(a + f"{n}_proj.bias", (d,)) for n in "qkv"])),
                "wo": f16(get(a + "out_proj.weight", (d, d))), "bo": f16(get(a + "out_proj.bias", (d,))),
                "ln2_g": f16(get(p + "final_layer_norm.weight", (d,))), "ln2_b": f16(get(p + "final_layer_norm.bias", (d,))),
                "w1": f16(get(p + "feed_forward.intermediate_dense.weight", (Fd, d))),
                "b1": f16(get(p + "feed_forward.intermediate_dense.bias", (Fd,))),
                "w2": f16(get(p + "feed_forward.output_dense.weight", (d, Fd))),
                "b2": f16(get(p + "feed_forward.output_dense.bias", (d,))),
            })
        self.enc_g, self.enc_b = f16(get("wav2vec2.encoder.layer_norm.weight", (d,))), \
            f16(get("wav2vec2.encoder.layer_norm.bias", (d,)))
        self.Vp = K.round_up(V, 8)
        hw = torch.zeros(self.Vp, d)
        hw[:V] = get("lm_head.weight", (V, d))
        self.head_w, self.head_b = f16(hw), f32(get("lm_head.bias", (V,)))

    @classmethod
    def from_pretrained(cls, model_dir, device="cuda"):
        def js(name, required=False):
            path = os.path.join(model_dir, name)
            if not os.path.exists(path):
                if required:
                    raise FileNotFoundError(f"{model_dir}: {name} is missing")
                return None
            with open(path) as f:
                return json.load(f)

        vocab = dict(js("vocab.json", True))
        vocab.update(js("added_tokens.json") or {})          # tokens the tokenizer keeps outside vocab.json
        return cls(load_state_dict(model_dir), js("config.json", True), vocab, js("tokenizer_config.json"),
                   js("preprocessor_config.json"), device)

    # ---------------------------------------------------------------------------------- forward

    def _wave(self, wave, sr=None):
        if sr is not None and int(sr) != self.sampling_rate:
            raise ValueError(f"the model was trained on {self.sampling_rate} Hz audio, got {sr} Hz")
        x = torch.as_tensor(wave, dtype=torch.float32).reshape(-1)
        if x.numel() < self.min_samples:
            raise ValueError(f"utterance of {x.numel()} samples is shorter than the feature extractor's receptive "
                             f"field of {self.min_samples}")
        return x.to(self.device).contiguous()

    def extract(self, x):
        """fp32 waveform on the device -> fp16 [T, d]: the feature extractor and the feature projection."""
        stats = K.wave_stats(x, NORM_EPS)
        c0 = self.conv[0]
        h = K.asr_conv0(x, stats, c0.w, c0.b, c0.g, c0.be, c0.stride, CONV_LN_EPS)
        for c in self.conv[1:]:
            h = K.asr_conv(h, c.w, c.b, c.cout, c.k, c.stride)
            K.asr_ln_gelu(h, c.g, c.be, CONV_LN_EPS)
        y = K.layernorm(h, self.fp_g, self.fp_b, self.eps)[0]
        return K.linear(y, self.fp_w, self.fp_bias)

    def positional(self, h, out=None):
        """h + GELU(pos_conv(h)) over fp16 [T, d].  The convolution yields T + 1 frames for an even kernel and
        HF drops the last: T outputs either way."""
        return K.asr_conv(h, self.pos_w, self.pos_b, self.d, self.pos_k, 1, self.pos_k // 2, self.pos_groups,
                          T_out=h.shape[0], res=h, out=out)

    def features(self, x, out=None):
        return self.positional(self.extract(x), out)

    def encode(self, Hb, lens32=None):
        """fp16 [B, Tmax, d] (rows past an utterance's length: anything finite) -> fp32 [B, Tmax, Vp]: the
        stable-LN layers, encoder.layer_norm and the head without its bias (ctc_greedy adds it)."""
        return self.head(self.layers_forward(Hb, lens32), Hb.shape[0], Hb.shape[1])

    def layers_forward(self, Hb, lens32=None):
        """The stable-LN transformer layers over fp16 [B, Tmax, d] -> fp16 [B * Tmax, d]."""
        return prenorm_layers(Hb, self.layers, self.H, self.eps, lens32)

    def head(self, X, B, Tm):
        """encoder.layer_norm and lm_head (bias left to ctc_greedy): fp16 [B * Tmax, d] -> fp32 [B, Tmax, Vp]."""
        y = K.layernorm(X, self.enc_g, self.enc_b, self.eps)[0]
        logits = torch.empty(B, Tm, self.Vp, dtype=torch.float32, device=X.device)
        K.gemm(y, self.head_w, logits, B * Tm, self.Vp, self.d, lda=self.d, ldb=self.d, ldc=self.Vp, epi=K.EPI_F32)
        return logits

    def forward_batch(self, waves, sr=None):
        """Waveforms -> (logits fp32 [B, Tmax, Vp] with the head's bias, lens (list), ids, out, count, bad:
        kernels.ctc_greedy's results), all on the device."""
        xs = [self._wave(w, sr) for w in waves]
        lens = [frame_counts(x.numel(), self.kernels, self.strides)[-1] for x in xs]
        B, Tm = len(xs), max(lens)
        if B == 1:
            Hb, lens32 = self.features(xs[0]).unsqueeze(0), None
        else:
            Hb = torch.zeros(B, Tm, self.d, dtype=K.F16, device=self.device)
            for b, x in enumerate(xs):
                self.features(x, out=Hb[b, :lens[b]])
            lens32 = torch.tensor(lens, dtype=torch.int32, device=self.device)
        logits = self.encode(Hb, lens32)
        return (logits, lens) + K.ctc_greedy(logits, self.V, self.blank, lens32, self.head_b)

    def _texts(self, lens, out, count, bad, cleanup):
        cleanup = self.cleanup if cleanup is None else cleanup
        count, bad, out = count.tolist(), bad.tolist(), out.cpu()
        for b, flag in enumerate(bad):
            if flag:
                raise NonFiniteLogits(f"utterance {b} of the batch ({lens[b]} frames): non-finite logits (the fp16 "
                                      "activations overflowed); no transcript written")
        return [tokens_to_text(out[b, :count[b]].tolist(), self.id_to_token, self.delimiter, cleanup, self.lower)
                for b in range(len(lens))]

    def logits(self, wave, sr=None):
        """fp32 [T, V] logits of one utterance (on the device)."""
        logits, lens, _, _, _, bad = self.forward_batch([wave], sr)
        if int(bad[0]):
            raise NonFiniteLogits(f"non-finite logits ({lens[0]} frames): the fp16 activations overflowed")
        return logits[0, :lens[0], :self.V]

    def transcribe(self, wave, sr=None, cleanup=None):
        return self.transcribe_many([wave], 1, sr, cleanup)[0]

    def transcribe_many(self, waves, batch_size=8, sr=None, cleanup=None):
        """Transcripts of the waveforms, in order; the encoder runs on batch_size utterances at a time."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        waves, texts = list(waves), []
        for i in range(0, len(waves), batch_size):
            _, lens, _, out, count, bad = self.forward_batch(waves[i:i + batch_size], sr)
            texts += self._texts(lens, out, count, bad, cleanup)
        return texts


def wav_sort_key(name):
    """The reference's order of {i}_pred.wav files: by the integer before the first '_'."""
    try:
        return int(name.split("_")[0])
    except ValueError:
        raise ValueError(f"'{name}': file names must start with an integer and '_' ({{i}}_pred.wav); the "
                         "directory must hold nothing but the synthesized WAV files") from None


def transcribe_dir(model, wav_dir, transcript_txt, batch_size=8):
    """Transcribe every file of wav_dir in the reference's order; transcripts joined by newlines with
    no trailing newline, as the reference writes them.  -> the number of files."""
    files = sorted(os.listdir(wav_dir), key=wav_sort_key)
    texts = []
    for i in range(0, len(files), batch_size):
        waves = []
        for f in files[i:i + batch_size]:
            x, sr = read_wav(os.path.join(wav_dir, f))
            if sr != model.sampling_rate:
                raise ValueError(f"{f}: sample rate {sr}, the model expects {model.sampling_rate}")
            waves.append(x)
        texts += model.transcribe_many(waves, batch_size)
    with open(transcript_txt, "w") as f:
        f.write("\n".join(texts))
    return len(files)

"""Speech-to-unit quantisation: HF ``HubertModel`` (the HuBERT-base family: feat_extract_norm "group",
post-LN encoder) features at layer ``km_layer`` on HIP kernels, then their nearest k-means centroid -- the
reference pipeline's scripts/preprocess/3_cluster.sh (fairseq's quantize_with_kmeans.py) and its
scripts/speech_to_speech_translation/mhubert.py.  The units are the model's training targets and the
vocoder's input.

Forward only.  As in asr.py, the feature extractor and the positional convolution run one utterance at a
time (no padding enters a convolution or the GroupNorm statistics) on csrc/units.hip's hubert_conv0 and
csrc/asr.hip's asr_conv; the post-LN layers run on the GEMM, LayerNorm and flash-attention kernels of the
training path over utterances packed as [B, Tmax, d] with key-length masking; kmeans_assign quantises
the packed rows without writing the [rows, centroids] distances.  Only ``km_layer`` layers are loaded
and run.  The loaders are asr.py's."""
import json
import os

import numpy as np
import torch

from . import kernels as K
from .asr import (CONFIG_DEFAULTS, CONV_LN_EPS, NORM_EPS, SAMPLE_RATE, _ConvLayer, fold_pos_conv_weight_norm,
                  frame_counts, load_state_dict, read_safetensors, read_wav, receptive_field)  # noqa: F401
from .vocoder import pack_conv_weight

PREFIXES = ("", "hubert.", "wav2vec2.")
HUBERT_DEFAULTS = dict(CONFIG_DEFAULTS, feat_proj_layer_norm=True)


class NonFiniteFeatures(RuntimeError):
    """An utterance's features hold inf or NaN (fp16 activations overflowed): no units are written."""


def parse_config(cfg):
    """Validated copy of a Hubert config.json dict (the keys the forward reads)."""
    c = dict(HUBERT_DEFAULTS)
    c.update(cfg)
    if c["feat_extract_norm"] != "group":
        raise NotImplementedError(f"hubert feat_extract_norm '{c['feat_extract_norm']}' is not supported (only "
                                  "\"group\": the HuBERT-base family)")
    if c["do_stable_layer_norm"]:
        raise NotImplementedError("hubert with do_stable_layer_norm true (pre-LN encoder) is not supported")
    if c.get("add_adapter"):
        raise NotImplementedError("hubert adapters (add_adapter) are not supported")
    for key in ("feat_extract_activation", "hidden_act"):
        if c[key] != "gelu":
            raise NotImplementedError(f"hubert {key} '{c[key]}' is not supported (only \"gelu\")")
    n = len(c["conv_dim"])
    if n < 1 or len(c["conv_kernel"]) != n or len(c["conv_stride"]) != n:
        raise ValueError("hubert config: conv_dim, conv_kernel and conv_stride differ in length")
    d, H = c["hidden_size"], c["num_attention_heads"]
    if d % H or d // H not in K.FLASH_HD:
        raise NotImplementedError(f"hubert head dim {d}/{H} (hidden_size / num_attention_heads) is not supported "
                                  f"(the attention kernel has {K.FLASH_HD})")
    if d % c["num_conv_pos_embedding_groups"]:
        raise ValueError("hubert config: num_conv_pos_embedding_groups does not divide hidden_size")
    return c


def check_km_layer(km_layer, cfg):
    km, L = int(km_layer), int(cfg["num_hidden_layers"])
    if not 0 <= km <= L:
        raise ValueError(f"km_layer {km_layer} outside [0, {L}] (num_hidden_layers)")
    return km


def strip_prefix(sd):
    """The state dict with its model prefix ("", "hubert." or "wav2vec2.") removed from every key."""
    probe = "feature_extractor.conv_layers.0.conv.weight"
    for p in PREFIXES:
        if p + probe in sd:
            return {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    raise KeyError(f"hubert checkpoint: '{probe}' is missing under every prefix of {PREFIXES}")


def load_centroids(path):
    """fp32 numpy [Kc, d] from a .npy file or a joblib-pickled scikit-learn k-means (``cluster_centers_``)."""
    if path.endswith(".npy"):
        Cm = np.load(path)
    else:
        try:
            import joblib
        except ImportError:
            raise ImportError(f"{path}: a joblib-pickled k-means model needs the 'joblib' package (and "
                              "scikit-learn); or save its cluster_centers_ with numpy.save as a .npy file") from None
        km = joblib.load(path)
        if not hasattr(km, "cluster_centers_"):
            raise ValueError(f"{path}: the unpickled {type(km).__name__} has no cluster_centers_")
        Cm = km.cluster_centers_
    Cm = np.ascontiguousarray(Cm, dtype=np.float32)
    if Cm.ndim != 2 or Cm.shape[0] < 1:
        raise ValueError(f"{path}: centroids [Kc, d] expected, got {Cm.shape}")
    return Cm


def merge(code):
    """Runs of equal units collapsed (host restatement of the device path)."""
    out = []
    for c in code:
        c = int(c)
        if not out or out[-1] != c:
            out.append(c)
    return out


class HubertUnits:
    """HF HubertModel in eval mode up to hidden_states[km_layer], then nearest-centroid units."""

    def __init__(self, state_dict, config, centroids, km_layer=11, preprocessor_cfg=None, device="cuda"):
        self.cfg = c = parse_config(config)
        self.km_layer = check_km_layer(km_layer, c)
        self.device = dev = torch.device(device)
        pre = dict(preprocessor_cfg or {})
        self.normalize = bool(pre.get("do_normalize", False))   # no preprocessor config: the samples as they are
        self.sampling_rate = int(pre.get("sampling_rate", SAMPLE_RATE))
        sd = fold_pos_conv_weight_norm(strip_prefix(state_dict), "")
        d, Hh, Fd = c["hidden_size"], c["num_attention_heads"], c["intermediate_size"]
        self.d, self.H, self.hd, self.eps = d, Hh, d // Hh, float(c["layer_norm_eps"])
        Cm = torch.as_tensor(np.asarray(centroids), dtype=torch.float32)
        if Cm.dim() != 2 or Cm.shape[1] != d:
            raise ValueError(f"centroids of shape {tuple(Cm.shape)} do not match the model's feature width {d}")
        self.n_units = Cm.shape[0]
        self.c_hi, self.c_lo, self.c_norm = K.kmeans_pack(Cm.to(dev))

        def get(name, shape):
            # the kernels trust these shapes: the packed images are sized by them
            if name not in sd:
                raise KeyError(f"hubert checkpoint: '{name}' is missing")
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
            p = f"feature_extractor.conv_layers.{i}."
            W = get(p + "conv.weight", (co, cin, k))
            w = f32(W[:, 0, :].t()) if i == 0 else pack_conv_weight(W).to(dev)
            b = f32(get(p + "conv.bias", (co,))) if c["conv_bias"] else None
            g = f32(get(p + "layer_norm.weight", (co,))) if i == 0 else None
            be = f32(get(p + "layer_norm.bias", (co,))) if i == 0 else None
            self.conv.append(_ConvLayer(w, b, g, be, co, k, s))
            cin = co
        p = "feature_projection."
        self.fp_ln = bool(c["feat_proj_layer_norm"])
        if self.fp_ln:
            self.fp_g, self.fp_b = f16(get(p + "layer_norm.weight", (cin,))), f16(get(p + "layer_norm.bias", (cin,)))
        self.fp_w, self.fp_bias = f16(get(p + "projection.weight", (d, cin))), f16(get(p + "projection.bias", (d,)))
        self.pos_k, self.pos_groups = int(c["num_conv_pos_embeddings"]), int(c["num_conv_pos_embedding_groups"])
        p = "encoder.pos_conv_embed.conv."
        cg = d // self.pos_groups
        Wp = get(p + "weight", (d, cg, self.pos_k))
        self.pos_w = torch.cat([pack_conv_weight(Wp[g * cg:(g + 1) * cg]) for g in range(self.pos_groups)]).to(dev)
        self.pos_b = f32(get(p + "bias", (d,)))
        self.enc_g, self.enc_b = f16(get("encoder.layer_norm.weight", (d,))), f16(get("encoder.layer_norm.bias", (d,)))
        self.layers = []
        for l in range(self.km_layer):                 # the layers past km_layer are neither loaded nor run
            p = f"encoder.layers.{l}."
            a = p + "attention."
            self.layers.append({
                "wqkv": f16(torch.cat([get(a + f"{n}_proj.weight", (d, d)) for n in "qkv"])),
                "bqkv": f16(torch.cat([get(a + f"{n}_proj.bias", (d,)) for n in "qkv"])),
                "wo": f16(get(a + "out_proj.weight", (d, d))), "bo": f16(get(a + "out_proj.bias", (d,))),
                "ln1_g": f16(get(p + "layer_norm.weight", (d,))), "ln1_b": f16(get(p + "layer_norm.bias", (d,))),
                "w1": f16(get(p + "feed_forward.intermediate_dense.weight", (Fd, d))),
                "b1": f16(get(p + "feed_forward.intermediate_dense.bias", (Fd,))),
                "w2": f16(get(p + "feed_forward.output_dense.weight", (d, Fd))),
                "b2": f16(get(p + "feed_forward.output_dense.bias", (d,))),
                "ln2_g": f16(get(p + "final_layer_norm.weight", (d,))), "ln2_b": f16(get(p + "final_layer_norm.bias", (d,))),
            })

    @classmethod
    def from_pretrained(cls, model_dir, km_path, km_layer=11, device="cuda"):
        def js(name, required=False):
            path = os.path.join(model_dir, name)
            if not os.path.exists(path):
                if required:
                    raise FileNotFoundError(f"{model_dir}: {name} is missing")
                return None
            with open(path) as f:
                return json.load(f)

        return cls(load_state_dict(model_dir), js("config.json", True), load_centroids(km_path), km_layer,
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
        c0 = self.conv[0]
        stats = K.wave_stats(x, NORM_EPS) if self.normalize else None
        h = K.hubert_conv0(x, stats, c0.w, c0.b, c0.g, c0.be, c0.stride, CONV_LN_EPS)
        for c in self.conv[1:]:
            h = K.asr_conv(h, c.w, c.b, c.cout, c.k, c.stride, gelu=True)
        if self.fp_ln:
            h = K.layernorm(h, self.fp_g, self.fp_b, self.eps)[0]
        return K.linear(h, self.fp_w, self.fp_bias)

    def positional(self, x, out=None):
        """h + GELU(pos_conv(h)) over the extractor's fp16 [T, d] of one utterance (T outputs: HF drops the
        last frame of an even kernel)."""
        h = self.extract(x)
        return K.asr_conv(h, self.pos_w, self.pos_b, self.d, self.pos_k, 1, self.pos_k // 2, self.pos_groups,
                          T_out=h.shape[0], res=h, out=out)

    def hidden0(self, Hb):
        """hidden_states[0] = encoder.layer_norm over packed fp16 [B, Tmax, d] rows of positional()."""
        B, Tm, d = Hb.shape
        return K.layernorm(Hb.reshape(B * Tm, d), self.enc_g, self.enc_b, self.eps)[0].reshape(B, Tm, d)

    def layers_forward(self, Hb, lens32=None):
        """The first km_layer post-LN layers over fp16 [B, Tmax, d] -> fp16 [B, Tmax, d]."""
        B, Tm, d = Hb.shape
        R, eps = B * Tm, self.eps
        X = Hb.reshape(R, d)
        for L in self.layers:
            qkv = K.linear(X, L["wqkv"], L["bqkv"])
            o = torch.empty(R, d, dtype=K.F16, device=X.device)
            K.mha_fwd(qkv, qkv[:, d:], qkv[:, 2 * d:], o, 3 * d, 3 * d, 3 * d, d, B, self.H, Tm, Tm, self.hd,
                      self.hd ** -0.5, key_len=lens32)
            X = K.layernorm(K.linear(o, L["wo"], L["bo"], epi=K.EPI_DROP_RESID, aux=X), L["ln1_g"], L["ln1_b"], eps)[0]
            z = torch.empty(R, L["w1"].shape[0], dtype=K.F16, device=X.device)
            f = K.linear(X, L["w1"], L["b1"], epi=K.EPI_GELU_DROP, out2=z)
            X = K.layernorm(K.linear(f, L["w2"], L["b2"], epi=K.EPI_DROP_RESID, aux=X), L["ln2_g"], L["ln2_b"], eps)[0]
        return X.reshape(B, Tm, d)

    def features_batch(self, waves, sr=None):
        """Waveforms -> (fp16 [B, Tmax, d] features at km_layer, lens (list), lens32 or None), on the device;
        the rows past an utterance's length hold finite values that mean nothing."""
        xs = [self._wave(w, sr) for w in waves]
        lens = [frame_counts(x.numel(), self.kernels, self.strides)[-1] for x in xs]
        B, Tm = len(xs), max(lens)
        if B == 1:
            Hb, lens32 = self.positional(xs[0]).unsqueeze(0), None
        else:
            Hb = torch.zeros(B, Tm, self.d, dtype=K.F16, device=self.device)
            for b, x in enumerate(xs):
                self.positional(x, out=Hb[b, :lens[b]])
            lens32 = torch.tensor(lens, dtype=torch.int32, device=self.device)
        return self.layers_forward(self.hidden0(Hb), lens32).contiguous(), lens, lens32

    def forward_batch(self, waves, sr=None):
        """Waveforms -> (features, lens, code, merged, count, bad: kernels.kmeans_assign's results)."""
        Fb, lens, lens32 = self.features_batch(waves, sr)
        return (Fb, lens) + K.kmeans_assign(Fb, self.c_hi, self.c_lo, self.c_norm, lens32)

    def features(self, wave, sr=None):
        """fp16 [T, d] features of one utterance at km_layer (on the device)."""
        Fb, lens, _ = self.features_batch([wave], sr)
        return Fb[0, :lens[0]]

    def units(self, wave, sr=None):
        """(code, merged_code) of one utterance, as Python lists."""
        return self.units_many([wave], 1, sr)[0]

    def units_many(self, waves, batch_size=8, sr=None):
        """[(code, merged_code)] of the waveforms, in order; the layers run on batch_size utterances at a time."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        waves, res = list(waves), []
        for i in range(0, len(waves), batch_size):
            _, lens, code, merged, count, bad = self.forward_batch(waves[i:i + batch_size], sr)
            code, merged, count, bad = code.cpu(), merged.cpu(), count.tolist(), bad.tolist()
            for b, flag in enumerate(bad):
                if flag:
                    raise NonFiniteFeatures(f"utterance {i + b} ({lens[b]} frames): non-finite features (the fp16 "
                                            "activations overflowed); no units written")
            res += [(code[b, :lens[b]].tolist(), merged[b, :count[b]].tolist()) for b in range(len(lens))]
        return res


def read_manifest(path):
    """fairseq's manifest: the root directory on the first line, then ``relative/path<TAB>n_samples``.
    -> (root, [relative paths])."""
    with open(path) as f:
        lines = [ln.rstrip("\n") for ln in f]
    if not lines or not lines[0].strip():
        raise ValueError(f"{path}: the first line must name the root directory")
    files = []
    for i, ln in enumerate(lines[1:], 2):
        if not ln.strip():
            continue
        parts = ln.split("\t")
        if len(parts) != 2 or not parts[1].strip().isdigit():
            raise ValueError(f"{path}:{i}: 'relative/path<TAB>n_samples' expected, got {ln!r}")
        files.append(parts[0])
    return lines[0].strip(), files


def quantize_manifest(model, manifest_path, out_path, extension=".wav", batch_size=8, reduce=False):
    """Units of every file of the manifest, in its order, one line each:
    ``{basename without extension}|{units joined by spaces}``.  -> the number of files."""
    root, files = read_manifest(manifest_path)
    lines = []
    for i in range(0, len(files), batch_size):
        waves = []
        for f in files[i:i + batch_size]:
            x, sr = read_wav(os.path.join(root, f))
            if sr != model.sampling_rate:
                raise ValueError(f"{f}: sample rate {sr}, the model expects {model.sampling_rate}")
            if len(x) < model.min_samples:
                raise ValueError(f"{f}: {len(x)} samples are fewer than the feature extractor's receptive field of "
                                 f"{model.min_samples}")
            waves.append(x)
        for f, (code, merged) in zip(files[i:i + batch_size], model.units_many(waves, batch_size)):
            base = os.path.basename(f)
            if extension and base.endswith(extension):
                base = base[:-len(extension)]
            lines.append(base + "|" + " ".join(str(u) for u in (merged if reduce else code)))
    with open(out_path, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    return len(files)

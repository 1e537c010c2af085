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
and run.  The loaders, the layer loop and the packing are encoders.py's (SpeechEncoder, shared with
asr.py); what is here is the group-norm feature extractor, the centroids and the units.

decode / decode_many are mhubert.py's HubertCode.decode at its defaults (beamsearch=True, top_k=10,
beamsize=200): kmeans_topk keeps each frame's top_k nearest centroids and their Euclidean distances,
units_beam (csrc/units_beam.hip) runs the reference's length-penalised beam search over them in its float32
arithmetic, one block per utterance; beam_decode_host is the NumPy restatement the kernel equals bit for bit."""
import os

import numpy as np
import torch

from . import kernels as K
from .encoders import (CONFIG_DEFAULTS, CONV_LN_EPS, NORM_EPS, SAMPLE_RATE, SpeechEncoder, Weights,
                       fold_pos_conv_weight_norm, load_state_dict, read_json, validate_config, wave_batches)
from .encoders import frame_counts as frame_counts      # re-exported: part of this module's surface

PREFIXES = ("", "hubert.", "wav2vec2.")
HUBERT_DEFAULTS = dict(CONFIG_DEFAULTS, feat_proj_layer_norm=True)


class NonFiniteFeatures(RuntimeError):
    """An utterance's features hold inf or NaN (fp16 activations overflowed): no units are written."""


def parse_config(cfg):
    """Validated copy of a Hubert config.json dict (the keys the forward reads)."""
    return validate_config(cfg, "hubert", HUBERT_DEFAULTS, "group", False, True)


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


def pairwise_sum(a):
    """numpy.sum of up to 32 contiguous float32 values, in the order numpy adds them (its pairwise_sum below
    the 128-element block), one float32 rounding per addition: sequential below 8 values; from 8 on, eight
    accumulators over the whole groups of eight, ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), then the tail one at a
    time.  csrc/units_beam.hip adds in this order."""
    a = np.asarray(a, dtype=np.float32)
    k = a.shape[0]
    if not 1 <= k <= K.KMEANS_TOPK_MAX:
        raise NotImplementedError(f"pairwise_sum: 1 to {K.KMEANS_TOPK_MAX} values, got {k}")
    if k < 8:
        res = a[0]
        for i in range(1, k):
            res = np.float32(res + a[i])
        return np.float32(res)
    n8 = k - k % 8
    r = a[:8].copy()
    for i in range(8, n8, 8):
        r = (r + a[i:i + 8]).astype(np.float32)
    res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))
                     + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
    for i in range(n8, k):
        res = np.float32(res + a[i])
    return res


def beam_steps(idx, val, beamsize):
    """The beam search of the reference's mhubert.py HubertCode.decode(beamsearch=True) as it evaluates
    under NumPy >= 2 (all of it float32), frame by frame: yields (parent, token, score) arrays of the kept
    sequences, in the reference's order.  A sequence is carried as (score, run count, last token); the
    reference's stable sort over (sequence, j) order is a stable argsort of the flattened scores."""
    idx, val = np.asarray(idx), np.asarray(val, dtype=np.float32)
    if idx.ndim != 2 or idx.shape != val.shape or idx.shape[1] < 1:
        raise ValueError(f"beam_decode_host: idx, val [T, top_k] expected, got {idx.shape}, {val.shape}")
    T, k = idx.shape
    K.check_beam_limits(k, beamsize)
    score, runs, last = np.ones(1, dtype=np.float32), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    for t in range(T):
        s = pairwise_sum(val[t])
        if not (np.isfinite(s) and s > 0):
            raise NonFiniteFeatures(f"frame {t}: the {k} nearest distances sum to {s}")
        r = (val[t] / s).astype(np.float32)
        new = np.ones((len(score), k), dtype=bool) if t == 0 else idx[t][None, :] != last[:, None]
        m = runs[:, None] + new
        rate = (m.astype(np.float64) / np.float64(T)).astype(np.float32)
        cand = (score[:, None] + (rate * r[None, :]).astype(np.float32)).astype(np.float32).reshape(-1)
        keep = np.argsort(cand, kind="stable")[:beamsize]
        parent, j = keep // k, keep % k
        score, runs, last = cand[keep], m.reshape(-1)[keep], idx[t][j].astype(np.int64)
        yield parent, last, score


def beam_decode_host(idx, val, beamsize=200):
    """beam_code of the reference's decode from the frames' top_k indices and distances [T, top_k] (host
    restatement of kernels.units_beam, which equals it bit for bit) -> a list of T units."""
    steps = [(p, tok) for p, tok, _ in beam_steps(idx, val, beamsize)]
    out, p = [], 0
    for parent, tok in reversed(steps):
        out.append(int(tok[p]))
        p = int(parent[p])
    return out[::-1]


class HubertUnits(SpeechEncoder):
    """HF HubertModel in eval mode up to hidden_states[km_layer], then nearest-centroid units (centroids None:
    the features only)."""

    def __init__(self, state_dict, config, centroids, km_layer=11, preprocessor_cfg=None, device="cuda"):
        c = parse_config(config)
        self.km_layer = check_km_layer(km_layer, c)
        pre = dict(preprocessor_cfg or {})
        self.normalize = bool(pre.get("do_normalize", False))   # no preprocessor config: the samples as they are
        w = Weights(fold_pos_conv_weight_norm(strip_prefix(state_dict), ""), "hubert checkpoint", device)
        if centroids is None:                                   # features only (kmeans.py trains the codebook from them)
            self.n_units, self.c_hi, self.c_lo, self.c_norm = 0, None, None, None
        else:
            Cm = torch.as_tensor(np.asarray(centroids), dtype=torch.float32)
            if Cm.dim() != 2 or Cm.shape[1] != c["hidden_size"]:
                raise ValueError(f"centroids of shape {tuple(Cm.shape)} do not match the model's feature width "
                                 f"{c['hidden_size']}")
            self.n_units = Cm.shape[0]
            self.c_hi, self.c_lo, self.c_norm = K.kmeans_pack(Cm.to(w.device))
        # the layers past km_layer are neither loaded nor run
        super().__init__(w, c, "", self.km_layer, pre.get("sampling_rate", SAMPLE_RATE))

    @classmethod
    def from_pretrained(cls, model_dir, km_path, km_layer=11, device="cuda"):
        """km_path None: no centroids, features only (features, features_batch)."""
        return cls(load_state_dict(model_dir), read_json(model_dir, "config.json", True),
                   None if km_path is None else load_centroids(km_path), km_layer,
                   read_json(model_dir, "preprocessor_config.json"), device)

    # ---------------------------------------------------------------------------------- forward

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

    def hidden0(self, Hb):
        """hidden_states[0] = encoder.layer_norm over packed fp16 [B, Tmax, d] rows of positional()."""
        B, Tm, d = Hb.shape
        return K.layernorm(Hb.reshape(B * Tm, d), self.enc_g, self.enc_b, self.eps)[0].reshape(B, Tm, d)

    def layers_forward(self, Hb, lens32=None):
        """The first km_layer post-LN layers over fp16 [B, Tmax, d] -> fp16 [B, Tmax, d]."""
        return super().layers_forward(Hb, lens32).reshape(Hb.shape)

    def features_batch(self, waves, sr=None):
        """Waveforms -> (fp16 [B, Tmax, d] features at km_layer, lens (list), lens32 or None), on the device;
        the rows past an utterance's length hold finite values that mean nothing."""
        Hb, lens, lens32 = self.pack(waves, sr)
        return self.layers_forward(self.hidden0(Hb), lens32).contiguous(), lens, lens32

    def forward_batch(self, waves, sr=None):
        """Waveforms -> (features, lens, code, merged, count, bad: kernels.kmeans_assign's results)."""
        if self.c_hi is None:
            raise RuntimeError("this HubertUnits was loaded without centroids: it extracts features only")
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

    def decode(self, wave, beamsearch=True, top_k=10, beamsize=200, sr=None):
        """The reference's mhubert.py HubertCode.decode of one utterance (decode_many's dict)."""
        return self.decode_many([wave], 1, beamsearch, top_k, beamsize, sr)[0]

    def decode_many(self, waves, batch_size=8, beamsearch=True, top_k=10, beamsize=200, sr=None):
        """The reference's HubertCode.decode of every waveform, in order -> a list of dicts: ``code`` [T] and
        ``merged_code`` (lists), ``topk_code`` int32 [T, top_k] and ``topk_distance`` fp32 [T, top_k] (numpy: the
        top_k nearest centroids of each frame and their Euclidean distances, ascending; ties to the lower
        index) and, with beamsearch, ``beam_code`` [T] and ``beam_merged_code`` (lists): the length-penalised
        beam search over them, kernels.kmeans_topk and kernels.units_beam.  The reference's ``distance``
        ([T, centroids], the matrix kmeans_topk exists not to write) and ``center_diff`` are not returned.
        One host read per batch of batch_size utterances."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if self.c_hi is None:
            raise RuntimeError("this HubertUnits was loaded without centroids: it extracts features only")
        top_k, beamsize = K.check_beam_limits(top_k, beamsize if beamsearch else 1)
        waves, res = list(waves), []
        for i in range(0, len(waves), batch_size):
            Fb, lens, lens32 = self.features_batch(waves[i:i + batch_size], sr)
            B, Tm = Fb.shape[:2]
            idx, dist, bad = K.kmeans_topk(Fb, self.c_hi, self.c_lo, self.c_norm, lens32, top_k=top_k)
            parts = [idx.reshape(B, -1), dist.view(torch.int32).reshape(B, -1), bad[:, None]]
            if beamsearch:
                beam, bmerged, bcount, bbad = K.units_beam(idx, dist, lens32, beamsize=beamsize)
                parts += [beam, bmerged, bcount[:, None], bbad[:, None]]
            host = torch.cat(parts, 1).cpu().numpy()            # the batch's one host read
            n = Tm * top_k
            for b, T in enumerate(lens):
                row = host[b]
                if row[2 * n] or (beamsearch and row[-1]):
                    raise NonFiniteFeatures(f"utterance {i + b} ({T} frames): non-finite features (the fp16 "
                                            "activations overflowed) or a frame at zero distance from its "
                                            f"{top_k} nearest centroids; no units written")
                tk = row[:n].reshape(Tm, top_k)[:T].copy()
                code = tk[:, 0].tolist()
                out = {"code": code, "merged_code": merge(code), "topk_code": tk,
                       "topk_distance": row[n:2 * n].view(np.float32).reshape(Tm, top_k)[:T].copy()}
                if beamsearch:
                    o = 2 * n + 1
                    out["beam_code"] = row[o:o + T].tolist()
                    out["beam_merged_code"] = row[o + Tm:o + Tm + int(row[o + 2 * Tm])].tolist()
                res.append(out)
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


def quantize_manifest(model, manifest_path, out_path, extension=".wav", batch_size=8, reduce=False, beamsearch=False,
                      top_k=10, beamsize=200):
    """Units of every file of the manifest, in its order, one line each:
    ``{basename without extension}|{units joined by spaces}``.  beamsearch: the beam decode's units
    (decode_many's beam_code, or beam_merged_code with reduce) instead of the nearest centroids.
    -> the number of files."""
    root, files = read_manifest(manifest_path)
    lines = []
    for names, waves in wave_batches(root, files, batch_size, model.sampling_rate, model.min_samples):
        if beamsearch:
            pairs = [(r["beam_code"], r["beam_merged_code"])
                     for r in model.decode_many(waves, batch_size, True, top_k, beamsize)]
        else:
            pairs = model.units_many(waves, batch_size)
        for f, (code, merged) in zip(names, pairs):
            base = os.path.basename(f)
            if extension and base.endswith(extension):
                base = base[:-len(extension)]
            lines.append(base + "|" + " ".join(str(u) for u in (merged if reduce else code)))
    with open(out_path, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    return len(files)

"""CPU restatement of HF HubertModel's forward (feat_extract_norm "group", post-LN encoder, eval mode) up
to hidden_states[km_layer], and of the k-means quantisation of those features into units, in torch fp32,
for the speech-to-unit tests.  Nothing here imports the product package or ``transformers``; the
restatement is pinned against the library by the goldens of scripts/gen_hf_golden.py
(tests/golden/hubert_hf_small_*.npz, read by tests/test_units.py).

Two modes, the convention of tests/asr_ref.py (whose pieces this file reuses).  emulate=False is the fp32
reference.  emulate=True does the same arithmetic in fp32 but rounds the weights the product keeps in fp16
and every tensor the product stores in fp16 through .half().float() where multimodal-s2ut_amd/units.py
stores one; its distance from the fp32 restatement is the floor a GPU allowance is TOL_FACTOR times.  The
product keeps in fp32: the waveform, layer 0's weights, every convolution's bias, the GroupNorm
parameters, the centroids' norms (the centroids themselves enter as fp16 hi + lo images of 22 bits)."""
import numpy as np
import torch
import torch.nn.functional as F

import asr_ref as AR
from asr_ref import MARGIN_CAP, TOL_FACTOR, _q, gelu, make_wave, to_float   # noqa: F401  (re-exported)

GN_EPS = 1e-5
BASE = dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False, feat_proj_layer_norm=True,
            feat_extract_activation="gelu", hidden_act="gelu", conv_kernel=AR.KERNELS, conv_stride=AR.STRIDES,
            num_conv_pos_embeddings=128, layer_norm_eps=1e-5)
SMALL = dict(BASE, conv_dim=[64] * 7, hidden_size=128, num_attention_heads=2, intermediate_size=256,
             num_hidden_layers=3, num_conv_pos_embedding_groups=2)
# HuBERT-base's widths, two layers deep
WIDE = dict(BASE, conv_dim=[512] * 7, hidden_size=768, num_attention_heads=12, intermediate_size=3072,
            num_hidden_layers=2, num_conv_pos_embedding_groups=16)
KM_LAYER = {"small": 2, "wide": 2}
KC = {"small": 100, "wide": 1000}
CFGS = {"small": SMALL, "wide": WIDE}
WAVES = [(8000, 1), (12345, 2), (48000, 3)]          # (samples, asr_ref.make_wave seed): 24, 38, 149 frames


# ------------------------------------------------------------------------------------------ fixtures

def make_state_dict(cfg, seed=0, prefix="", style="param"):
    """Seeded HubertModel state dict under HF's key names (prefix "" as HubertModel saves them, "hubert."
    as HubertForCTC does).  style "param": pos_conv_embed.conv.parametrizations.weight.original0 / 1;
    "g_v": weight_g / weight_v.  Scales keep a unit-variance input at roughly unit variance."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    sd = {}

    def ln(name, n):
        sd[name + ".weight"], sd[name + ".bias"] = 1.0 + 0.1 * rn(n), 0.1 * rn(n)

    def lin(name, nout, nin):
        sd[name + ".weight"], sd[name + ".bias"] = rn(nout, nin) / nin ** 0.5, 0.1 * rn(nout)

    cin = 1
    for i, (co, k) in enumerate(zip(cfg["conv_dim"], cfg["conv_kernel"])):
        p = f"feature_extractor.conv_layers.{i}"
        # no norm behind layers 1..: a gain of 1.6 keeps GELU's output near unit variance
        sd[p + ".conv.weight"] = (1.0 if i == 0 else 1.6) * rn(co, cin, k) / (cin * k) ** 0.5
        if cfg["conv_bias"]:
            sd[p + ".conv.bias"] = 0.1 * rn(co)
        if i == 0:
            ln(p + ".layer_norm", co)
        cin = co
    d, Fd = cfg["hidden_size"], cfg["intermediate_size"]
    if cfg.get("feat_proj_layer_norm", True):
        ln("feature_projection.layer_norm", cin)
    lin("feature_projection.projection", d, cin)
    k, cg = cfg["num_conv_pos_embeddings"], d // cfg["num_conv_pos_embedding_groups"]
    gk, vk = ("weight_g", "weight_v") if style == "g_v" else \
        ("parametrizations.weight.original0", "parametrizations.weight.original1")
    p = "encoder.pos_conv_embed.conv."
    sd[p + vk] = rn(d, cg, k)
    sd[p + gk] = ((d / k) ** 0.5 * (1.0 + 0.1 * rn(k))).abs().view(1, 1, k)
    sd[p + "bias"] = 0.1 * rn(d)
    ln("encoder.layer_norm", d)
    for l in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + "attention." + n, d, d)
        ln(p + "layer_norm", d)
        lin(p + "feed_forward.intermediate_dense", Fd, d)
        lin(p + "feed_forward.output_dense", d, Fd)
        ln(p + "final_layer_norm", d)
    sd["masked_spec_embed"] = rn(d)                    # present in released checkpoints, unused in eval mode
    return {prefix + k_: v for k_, v in sd.items()}


def checksums(sd):
    """{key: float64 [sum, sum of squares]} of a state dict: what the goldens record of the weights."""
    return {k: np.array([float(v.double().sum()), float(v.double().pow(2).sum())]) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------ pieces

def conv0(x, W, b, g, be, stride, *, normalize=False, emulate=False):
    """kernels.hubert_conv0: waveform [n] -> [T0, C]; GroupNorm(C groups) = per-channel mean and biased
    variance over the T0 frames.  Nothing but the output is rounded."""
    xn = AR.normalise(x) if normalize else x
    v = F.conv1d(xn[None, None], W, b, stride=stride)
    return _q(emulate)(gelu(F.group_norm(v, W.shape[0], g, be, GN_EPS))[0].t())


def conv_gelu(x, W, b, stride, *, emulate=False):
    """kernels.asr_conv(gelu=True): x [T, Cin] -> GELU(conv + bias), rounded once after the GELU."""
    q = _q(emulate)
    return q(gelu(F.conv1d(q(x).t()[None], q(W), b, stride=stride)[0].t()))


def pos_weight(sd, p="encoder.pos_conv_embed.conv."):
    for gk, vk in (("weight_g", "weight_v"), ("parametrizations.weight.original0", "parametrizations.weight.original1")):
        if p + vk in sd:
            return AR.fold_pos(sd[p + gk].float(), sd[p + vk].float())
    return sd[p + "weight"].float()


def forward(sd, cfg, x, km_layer, *, normalize=False, emulate=False, want=None):
    """Waveform fp32 [n] -> fp32 [T, d] = hidden_states[km_layer] of HubertModel (sd under the prefix "").
    want: a dict that receives "layer0" ([T0, C]) and "h0" (hidden_states[0])."""
    q = _q(emulate)
    W, B = AR._w(sd, emulate)
    raw = lambda n: sd[n].float() if n in sd else None
    eps = cfg["layer_norm_eps"]
    p = "feature_extractor.conv_layers."
    h = conv0(x, raw(p + "0.conv.weight"), raw(p + "0.conv.bias"), raw(p + "0.layer_norm.weight"),
              raw(p + "0.layer_norm.bias"), cfg["conv_stride"][0], normalize=normalize, emulate=emulate)
    if want is not None:
        want["layer0"] = h
    for i in range(1, len(cfg["conv_dim"])):
        h = conv_gelu(h, raw(f"{p}{i}.conv.weight"), raw(f"{p}{i}.conv.bias"), cfg["conv_stride"][i], emulate=emulate)
    ln = lambda t, n: q(F.layer_norm(t, (t.shape[1],), W(n), B(n), eps))
    lin = lambda t, n: t @ W(n).t() + B(n)
    if cfg.get("feat_proj_layer_norm", True):
        h = ln(h, "feature_projection.layer_norm")
    h = q(lin(h, "feature_projection.projection"))
    h = AR.pos_conv(h, pos_weight(sd), raw("encoder.pos_conv_embed.conv.bias"), cfg["num_conv_pos_embedding_groups"],
                    emulate=emulate)
    h = ln(h, "encoder.layer_norm")
    if want is not None:
        want["h0"] = h
    for l in range(km_layer):
        p = f"encoder.layers.{l}."
        qkv = q(torch.cat([lin(h, p + f"attention.{n}_proj") for n in "qkv"], 1))
        o = AR.attention(qkv, cfg["num_attention_heads"], emulate=emulate)
        h = ln(q(h + lin(o, p + "attention.out_proj")), p + "layer_norm")
        z = q(lin(h, p + "feed_forward.intermediate_dense"))
        h = ln(q(h + lin(q(gelu(z)), p + "feed_forward.output_dense")), p + "final_layer_norm")
    return h


def scores(feats, centroids):
    """float64 [T, Kc]: |C_c|^2 - 2 f . C_c (the squared distance less the row's own |f|^2)."""
    f, c = feats.double(), centroids.double()
    return c.pow(2).sum(1)[None] - 2.0 * f @ c.t()


def assign(feats, centroids):
    return scores(feats, centroids).argmin(1)


def merge(code):
    """Runs of equal units collapsed (itertools.groupby's keys)."""
    out = []
    for c in code:
        c = int(c)
        if not out or out[-1] != c:
            out.append(c)
    return out


def kmeans_emulation(X16, centroids):
    """fp32 scores rounded where kmeans_assign rounds: fp16 hi / lo centroid images (lo scaled by 2^11), the
    two dot products accumulated in fp32, joined, then cnorm - 2 dot in fp32.  X16: the fp16 rows."""
    Cm = centroids.float()
    hi = Cm.half()
    lo = ((Cm - hi.float()) * 2048.0).half()
    x = X16.float()
    dot = x @ hi.float().t() + (x @ lo.float().t()) * (1.0 / 2048.0)
    return Cm.double().pow(2).sum(1).float()[None] - 2.0 * dot


_CACHE = {}


TRAIN = {"small": [(n, 100 + 7 * i + j) for j, (n, _) in enumerate(WAVES) for i in range(8)],
         "wide": [(16000, 100 + i) for i in range(4)]}


def make_centroids(cfg_name, Kc=None, seed=0, sd_seed=0):
    """fp32 [Kc, d] centroids that sit among the model's own features, from the fp32 features of seeded
    training waves (TRAIN: other noise seeds than the fixtures'; for "small" at the fixtures' lengths, since
    GroupNorm and attention make a frame's features depend on the utterance's length).  With at least 4
    rows per centroid: ten Lloyd steps from rows drawn at random, a cluster that runs empty keeping its row,
    so every centroid is some frame's nearest.  With fewer: rows (cycled) plus noise of std 0.5."""
    Kc = Kc or KC[cfg_name]
    key = ("centroids", cfg_name, Kc, seed, sd_seed)
    if key not in _CACHE:
        cfg, sd = CFGS[cfg_name], make_state_dict(CFGS[cfg_name], sd_seed)
        with torch.no_grad():
            Fm = torch.cat([forward(sd, cfg, to_float(make_wave(n, ws)), KM_LAYER[cfg_name]) for n, ws in TRAIN[cfg_name]])
        g = torch.Generator().manual_seed(seed)
        if Fm.shape[0] >= 4 * Kc:
            Cm = Fm[torch.randperm(Fm.shape[0], generator=g)[:Kc]].clone()
            for _ in range(10):
                a = assign(Fm, Cm)
                for c in a.unique().tolist():
                    Cm[c] = Fm[a == c].mean(0)
        else:
            Cm = Fm[torch.arange(Kc) % Fm.shape[0]] + 0.5 * torch.randn(Kc, Fm.shape[1], generator=g)
        _CACHE[key] = Cm.contiguous()
    return _CACHE[key]


def reference(cfg_name, n, wave_seed, seed=0, normalize=False):
    """(sd, pcm, fp32 features, emulated features) at km_layer of a fixture, computed once per process."""
    key = (cfg_name, seed, n, wave_seed, normalize)
    if key not in _CACHE:
        cfg = CFGS[cfg_name]
        sd = make_state_dict(cfg, seed)
        pcm = make_wave(n, wave_seed)
        x = to_float(pcm)
        with torch.no_grad():
            _CACHE[key] = (sd, pcm, forward(sd, cfg, x, KM_LAYER[cfg_name], normalize=normalize),
                           forward(sd, cfg, x, KM_LAYER[cfg_name], normalize=normalize, emulate=True))
    return _CACHE[key]


def safe_frames(ref, centroids, a):
    """bool [T]: frames whose winner c1 no feature perturbation of at most a per element on either side can
    change: s_c - s_c1 >= 2 * (2 a |C_c - C_c1|_1) for every other centroid c."""
    S = scores(ref, centroids)
    win = S.argmin(1)
    gap = S - S.gather(1, win[:, None])
    l1 = torch.cdist(centroids.double(), centroids.double(), p=1)[win]
    ok = gap >= 4.0 * a * l1
    ok[torch.arange(len(win)), win] = True
    return ok.all(1)

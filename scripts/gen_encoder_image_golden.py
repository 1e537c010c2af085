"""Golden digests of the weight images the three encoders (asr.py, units.py, vision.py) pack at load: for
every tensor a model holds, its dtype, shape and the sha256 of its contiguous bytes, built on the CPU from
the tests' seeded fixtures.  The loaders decide what bytes land on the device; this pins them.

  tests/golden/encoder_images.json   {model: {tensor name: {dtype, shape, sha256} or null (a tensor the
      variant does not have, e.g. a conv bias with conv_bias false)}} for
        wav2vec2                 Wav2Vec2CTC on asr_ref.SMALL, seed 0
        hubert, hubert_bias, hubert_no_fp_ln
                                 HubertUnits on hubert_ref.SMALL, seed 0, km_layer 2, 20 x 128 centroids from
                                 default_rng(0); with conv_bias true; with feat_proj_layer_norm false
        vit                      ViTFeatures on vit_ref.SMALL, seed 0
      The speech fixtures' weight-normed positional convolution goes in as a plain weight (plain_pos_conv).

tests/test_encoders.py rebuilds the same models through images() and compares everything exactly.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_encoder_image_golden.py
"""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "encoder_images.json")


def tensors(m):
    """{name: tensor or None} of a model: its tensor attributes, its conv layers and its layer dicts."""
    out = {k: v for k, v in vars(m).items() if isinstance(v, torch.Tensor)}
    for i, c in enumerate(getattr(m, "conv", [])):
        out.update({f"conv{i}.{k}": getattr(c, k) for k in ("w", "b", "g", "be")})
    for l, L in enumerate(m.layers):
        out.update({f"layers{l}.{k}": v for k, v in L.items()})
    return out


def digest(t):
    if t is None:
        return None
    raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
    return {"dtype": str(t.dtype), "shape": list(t.shape), "sha256": hashlib.sha256(raw).hexdigest()}


def plain_pos_conv(sd):
    """The state dict with the positional convolution's weight-norm pair replaced by a plain ``weight`` (the
    pair's direction v), which the loaders pass through unfolded: the fold takes a square root whose last bit
    differs between CPUs (seen: Intel and AMD hosts, same torch), so pos_w's bytes are pinned behind it --
    the grouped packing -- and the fold keeps its tolerance tests (tests/test_asr.py, tests/test_units.py)."""
    base = next(k for k in sd if k.endswith("pos_conv_embed.conv.bias"))[:-len("bias")]
    g, v = next(p for p in (("weight_g", "weight_v"), ("parametrizations.weight.original0",
                                                       "parametrizations.weight.original1")) if base + p[1] in sd)
    out = {k: t for k, t in sd.items() if k not in (base + g, base + v)}
    out[base + "weight"] = sd[base + v]
    return out


def images():
    """{model: {tensor name: digest}} of the five fixture models, built on the CPU."""
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import asr_ref as AR
    import hubert_ref as HR
    import vit_ref as VR
    A, U, V = (importlib.import_module("multimodal-s2ut_amd." + n) for n in ("asr", "units", "vision"))
    cents = np.random.default_rng(0).standard_normal((20, 128)).astype(np.float32)

    def hubert(**over):
        cfg = dict(HR.SMALL, **over)
        return U.HubertUnits(plain_pos_conv(HR.make_state_dict(cfg, 0)), cfg, cents, 2, device="cpu")

    models = {"wav2vec2": A.Wav2Vec2CTC(plain_pos_conv(AR.make_state_dict(AR.SMALL, 0)), AR.SMALL, AR.VOCAB, device="cpu"),
              "hubert": hubert(conv_bias=False), "hubert_bias": hubert(conv_bias=True),
              "hubert_no_fp_ln": hubert(feat_proj_layer_norm=False),
              "vit": V.ViTFeatures(VR.make_state_dict(VR.SMALL, 0), VR.SMALL, device="cpu")}
    return {name: {k: digest(t) for k, t in sorted(tensors(m).items())} for name, m in models.items()}


def main():
    with open(OUT, "w") as f:
        json.dump(images(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

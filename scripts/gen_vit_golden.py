"""Golden fixtures for the ViT image feature extractor, from the ``transformers`` library's own ViTModel
and from Pillow, on CPU.

Run by hand where ``transformers`` and ``PIL`` are installed; never by a test and never on a GPU machine
(the tests read the committed .npz files and import nothing of ``transformers``).

  tests/golden/vit_hf_small.npz     ViTModel(add_pooling_layer=False, layer_norm_eps=1e-6, hidden_act="gelu",
      attn_implementation="eager") at vit_ref.SMALL, loaded with vit_ref.make_state_dict(SMALL, 0) mapped from
      timm's key names onto HF's (nothing missing, nothing unexpected), on the pixels of vit_ref.GOLDEN_IMAGES:
      out32 = last_hidden_state in fp32, out64 = the same model run in double, noise = max|out32 - out64|
      (what a test's allowance is a multiple of), pix_sum = float64 [sum, sum of squares] of the input,
      sum_<key> = the same of every weight (the weights themselves are not stored).
  tests/golden/vit_pillow_s48.npz   u8_<w>x<h> = uint8 [48, 48, 3]: Pillow's Image.resize(BICUBIC) to
      torchvision's Resize(48) size and the CenterCrop(48) of vit_ref.make_image(w, h, 0), for vit_ref.SIZES_48;
      pillow = the library's version.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_vit_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")


def to_hf(sd, cfg, keys):
    """timm's VisionTransformer keys -> transformers' ViTModel keys (qkv split into three).  keys: the HF
    model's own state-dict keys; the library renamed the encoder's modules in its 5.x releases (layers.N.attention.
    q_proj ... mlp.fc2, before: encoder.layer.N.attention.attention.query ... output.dense), both are mapped."""
    d = cfg["d"]
    out = {"embeddings.cls_token": sd["cls_token"], "embeddings.position_embeddings": sd["pos_embed"],
           "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
           "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
           "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    new = "layers.0.attention.q_proj.weight" in keys
    qkv = ("attention.q_proj", "attention.k_proj", "attention.v_proj") if new else \
        ("attention.attention.query", "attention.attention.key", "attention.attention.value")
    proj, fc1, fc2 = ("attention.o_proj", "mlp.fc1", "mlp.fc2") if new else \
        ("attention.output.dense", "intermediate.dense", "output.dense")
    for l in range(cfg["layers"]):
        s, t = f"blocks.{l}.", (f"layers.{l}." if new else f"encoder.layer.{l}.")
        for wb in ("weight", "bias"):
            for i, n in enumerate(qkv):
                out[f"{t}{n}.{wb}"] = sd[f"{s}attn.qkv.{wb}"][i * d:(i + 1) * d]
            out[f"{t}{proj}.{wb}"] = sd[f"{s}attn.proj.{wb}"]
            out[f"{t}layernorm_before.{wb}"] = sd[f"{s}norm1.{wb}"]
            out[f"{t}layernorm_after.{wb}"] = sd[f"{s}norm2.{wb}"]
            out[f"{t}{fc1}.{wb}"] = sd[f"{s}mlp.fc1.{wb}"]
            out[f"{t}{fc2}.{wb}"] = sd[f"{s}mlp.fc2.{wb}"]
    return out


def main():
    try:
        import PIL
        import transformers
        from transformers import ViTConfig, ViTModel
    except ImportError as e:
        print(f"{e}: nothing written", file=sys.stderr)
        return 1
    import vit_ref as VR

    torch.manual_seed(0)
    os.makedirs(OUT, exist_ok=True)
    cfg = VR.SMALL
    sd = VR.make_state_dict(cfg, 0)
    hf_cfg = ViTConfig(hidden_size=cfg["d"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                       intermediate_size=cfg["mlp"], hidden_act="gelu", layer_norm_eps=1e-6, image_size=cfg["image_size"],
                       patch_size=cfg["patch"], qkv_bias=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                       attn_implementation="eager")
    model = ViTModel(hf_cfg, add_pooling_layer=False)
    missing, unexpected = model.load_state_dict(to_hf(sd, cfg, set(model.state_dict())), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.eval()
    x = VR.pixels([VR.make_image(w, h, s) for w, h, s in VR.GOLDEN_IMAGES], cfg["image_size"])
    with torch.no_grad():
        out32 = model(pixel_values=x).last_hidden_state
        out64 = model.double()(pixel_values=x.double()).last_hidden_state
    noise = float((out32.double() - out64).abs().max())
    out = {"out32": out32.numpy(), "out64": out64.numpy(), "noise": np.float64(noise),
           "pix_sum": np.array([float(x.double().sum()), float(x.double().pow(2).sum())])}
    out.update({"sum_" + k: v for k, v in VR.checksums(sd).items()})
    path = os.path.join(OUT, "vit_hf_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes (transformers {transformers.__version__}); outputs up to "
          f"{float(out64.abs().max()):.2f}, max|fp32 - double| {noise:.2e}")

    out = {"pillow": np.array(PIL.__version__)}
    for w, h in VR.SIZES_48:
        out[f"u8_{w}x{h}"] = VR.pillow_transform_u8(VR.make_image(w, h, 0), 48)
    path = os.path.join(OUT, "vit_pillow_s48.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes (Pillow {PIL.__version__})")
    return 0


if __name__ == "__main__":
    sys.exit(main())

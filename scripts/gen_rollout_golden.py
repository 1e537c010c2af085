"""Golden fixtures for the ViT attention rollout, on CPU.

Run by hand on a machine that has the reference project and ``transformers``; never by a test and never on a
GPU machine (the tests read the committed .npz files).  Only recorded numbers are written.

  tests/golden/rollout_reference.npz   the reference's own ``rollout(attentions, discard_ratio, head_fusion)``
      (scripts/extract_feature/vit_rollout.py, loaded with ``cv2`` and ``torchvision`` stubbed out of
      sys.modules: the function is pure torch) on rollout_ref.attention_stack(T, H, L, seed) with a batch axis of
      one, for rollout_ref.STACKS x FUSIONS x RATIOS: mask_<T>_<fusion>_<ratio> = its fp32 result, sum_<T> =
      float64 [sum, sum of squares] of the input stack (the inputs themselves are seeded, not stored).  An input
      with a tie at the k-th smallest entry is refused: torch.topk leaves ties unspecified.
  tests/golden/rollout_clip_small.npz  CLIPVisionModel(hidden_act="gelu", layer_norm_eps=1e-6,
      attn_implementation="eager", output_attentions) at rollout_ref.CLIP_SMALL, loaded with
      rollout_ref.make_state_dict(CLIP_SMALL, 0) mapped from timm's key names onto HF's (nothing missing, nothing
      unexpected), on the pixels of rollout_ref.CLIP_IMAGES: out32 / out64 = post_layernorm of every token in
      fp32 / double, att64 = the per-layer probabilities [L, B, H, T, T] in double, att32 the same in fp32,
      noise / att_noise = max|fp32 - double| of each, pix_sum and sum_<key> as in vit_hf_small.npz.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_rollout_golden.py --reference /path/to/reference
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")


def load_reference_rollout(ref_root):
    """The reference's rollout function; its module imports cv2 and torchvision, which it does not need."""
    path = os.path.join(ref_root, "mm_s2ut", "scripts", "extract_feature", "vit_rollout.py")
    names = ("cv2", "torchvision", "torchvision.transforms")
    saved = {n: sys.modules.get(n) for n in names}
    for name in names:
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    try:
        spec = importlib.util.spec_from_file_location("reference_vit_rollout", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:                                             # the stubs must not outlive the import
        for name, old in saved.items():
            if old is None:
                del sys.modules[name]
            else:
                sys.modules[name] = old
    return mod.rollout


def reference_golden(ref_root):
    import rollout_ref as RR
    fn = load_reference_rollout(ref_root)
    out = {}
    for seed, (T, H, L) in enumerate(RR.STACKS):
        A = RR.attention_stack(T, H, L, seed)
        out[f"sum_{T}"] = np.array([float(A.double().sum()), float(A.double().pow(2).sum())])
        for fusion in RR.FUSIONS:
            for ratio in RR.RATIOS:
                k = RR.discard_count(T, ratio)
                gaps = [RR.tie_gap(RR.fuse(A[l], fusion), k) for l in range(L)]
                if min(gaps) <= 0:
                    raise SystemExit(f"T {T} {fusion} ratio {ratio}: a tie at the k-th smallest entry; refused")
                mask = fn([A[l][None].clone() for l in range(L)], ratio, fusion)
                out[f"mask_{T}_{fusion}_{ratio}"] = np.asarray(mask, dtype=np.float32)
                print(f"T {T} H {H} L {L} {fusion} ratio {ratio}: smallest gap at k {min(gaps):.1e}")
    path = os.path.join(OUT, "rollout_reference.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


def to_clip(sd, cfg, keys):
    """timm's pre-norm VisionTransformer keys -> transformers' CLIPVisionModel keys (qkv split into three).
    keys: the HF model's own state-dict keys; its 5.x releases dropped the ``vision_model.`` prefix, both are mapped."""
    d = cfg["d"]
    v = "vision_model." if any(k.startswith("vision_model.") for k in keys) else ""
    out = {v + "embeddings.class_embedding": sd["cls_token"][0, 0], v + "embeddings.position_embedding.weight": sd["pos_embed"][0],
           v + "embeddings.patch_embedding.weight": sd["patch_embed.proj.weight"],
           v + "pre_layrnorm.weight": sd["norm_pre.weight"], v + "pre_layrnorm.bias": sd["norm_pre.bias"],
           v + "post_layernorm.weight": sd["norm.weight"], v + "post_layernorm.bias": sd["norm.bias"]}
    for l in range(cfg["layers"]):
        s, t = f"blocks.{l}.", f"{v}encoder.layers.{l}."
        for wb in ("weight", "bias"):
            for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
                out[f"{t}self_attn.{n}.{wb}"] = sd[f"{s}attn.qkv.{wb}"][i * d:(i + 1) * d]
            out[f"{t}self_attn.out_proj.{wb}"] = sd[f"{s}attn.proj.{wb}"]
            out[f"{t}layer_norm1.{wb}"] = sd[f"{s}norm1.{wb}"]
            out[f"{t}layer_norm2.{wb}"] = sd[f"{s}norm2.{wb}"]
            out[f"{t}mlp.fc1.{wb}"] = sd[f"{s}mlp.fc1.{wb}"]
            out[f"{t}mlp.fc2.{wb}"] = sd[f"{s}mlp.fc2.{wb}"]
    return out


def clip_golden():
    import transformers
    from transformers import CLIPVisionConfig, CLIPVisionModel
    import rollout_ref as RR
    import vit_ref as VR

    cfg = RR.CLIP_SMALL
    sd = RR.make_state_dict(cfg, 0)
    hf_cfg = CLIPVisionConfig(hidden_size=cfg["d"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                              intermediate_size=cfg["mlp"], hidden_act="gelu", layer_norm_eps=1e-6,
                              image_size=cfg["image_size"], patch_size=cfg["patch"], attention_dropout=0.0,
                              attn_implementation="eager")
    model = CLIPVisionModel(hf_cfg)
    mapped = to_clip(sd, cfg, set(model.state_dict()))
    missing, unexpected = model.load_state_dict(mapped, strict=False)
    missing = [k for k in missing if not k.endswith("position_ids")]        # a buffer of arange, not a weight
    assert not missing and not unexpected, (missing, unexpected)
    model.eval()
    x = RR.pixels([VR.make_image(w, h, s) for w, h, s in RR.CLIP_IMAGES], cfg["image_size"])

    def run(m, xx):
        with torch.no_grad():
            o = m(pixel_values=xx, output_attentions=True)
            post = getattr(m, "vision_model", m).post_layernorm
            return post(o.last_hidden_state), torch.stack(list(o.attentions))

    out32, att32 = run(model, x)
    out64, att64 = run(model.double(), x.double())
    assert att64.shape == (cfg["layers"], x.shape[0], cfg["heads"], 10, 10), att64.shape
    noise = float((out32.double() - out64).abs().max())
    att_noise = float((att32.double() - att64).abs().max())
    out = {"out32": out32.numpy(), "out64": out64.numpy(), "att32": att32.numpy(), "att64": att64.numpy(),
           "noise": np.float64(noise), "att_noise": np.float64(att_noise),
           "pix_sum": np.array([float(x.double().sum()), float(x.double().pow(2).sum())])}
    out.update({"sum_" + k: v for k, v in VR.checksums(sd).items()})
    path = os.path.join(OUT, "rollout_clip_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes (transformers {transformers.__version__}); tokens up to "
          f"{float(out64.abs().max()):.2f}, max|fp32 - double| tokens {noise:.2e}, probabilities {att_noise:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project")
    args = ap.parse_args()
    torch.manual_seed(0)
    os.makedirs(OUT, exist_ok=True)
    reference_golden(args.reference)
    try:
        clip_golden()
    except ImportError as e:
        print(f"{e}: rollout_clip_small.npz not written", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

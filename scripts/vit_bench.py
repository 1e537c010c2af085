"""Timing of the ViT image feature extractor (multimodal-s2ut_amd/vision.py) at vit_base_patch16_384 with
seeded random weights on synthetic 500 x 375 images, B = 1, 8, 32.

    python scripts/vit_bench.py [--batches 1,8,32] [--warmup 3] [--repeats 10] [--out FILE]

HIP events on the stream the kernels run on, warm-up first, median [min .. max] of the repeats.  Every time
is event time around one call, host launch gaps included, so the rates are event-time rates, not kernel
shares of peak.  FLOPs are the algorithm's, counted from the shapes below (2 per multiply-add): the layer
GEMMs, the attention's QK^T and PV, the patch embedding.  The front end's bytes are the source images read
once plus the patch rows written once.  On the same machine and the same images: one-thread Pillow
resize + crop with torch's ToTensor / Normalize arithmetic, the host work the kernel replaces, and Pillow's
JPEG decode of the same pictures."""
import argparse
import importlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PEAK_TF, HBM_TBS = 2500.0, 8.0        # MI355X: dense fp16 MFMA and HBM3E, spec


def flops_per_image(cfg):
    d, Fd, L, T = cfg["d"], cfg["mlp"], cfg["layers"], (cfg["image_size"] // cfg["patch"]) ** 2 + 1
    layers = L * 2 * T * (3 * d * d + d * d + 2 * d * Fd)
    attn = L * 2 * 2 * T * T * d
    patch = 2 * (T - 1) * 3 * cfg["patch"] ** 2 * d
    return layers, attn, patch


def host_time(fn, repeats):
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="vit_base_patch16_384")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("vit_bench needs a GPU: a CPU run gives no timing")
    import vit_ref as VR
    from asr_bench import timed
    V = importlib.import_module("multimodal-s2ut_amd.vision")
    K = importlib.import_module("multimodal-s2ut_amd.kernels")

    cfg = V.model_config(args.model)
    m = V.ViTFeatures(VR.make_state_dict(cfg, 0), cfg, device="cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    images = [VR.make_image(args.width, args.height, i) for i in range(max(batches))]
    fl = flops_per_image(cfg)
    lines = [f"vit_bench: {args.model} (d {m.d}, {cfg['layers']} layers, {m.T} tokens), {args.width}x{args.height} images; "
             f"{torch.cuda.get_device_name(0)}",
             f"  FLOP per image: layers {fl[0] / 1e9:.1f} G, attention {fl[1] / 1e9:.1f} G, patch embed {fl[2] / 1e9:.2f} G, "
             f"total {sum(fl) / 1e9:.1f} G"]
    print("\n".join(lines), flush=True)

    def row(name, t, note=""):
        lines.append(f"  {name:<44s} {t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]{note}")
        print(lines[-1], flush=True)

    w, r = args.warmup, args.repeats
    for B in batches:
        ims = images[:B]
        lines.append(f" B = {B}")
        print(lines[-1], flush=True)
        desc, tab, rows = m.plan([(im.shape[1], im.shape[0]) for im in ims])
        buf = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(m.device)
        out = torch.empty(B, m.npatch, 3 * m.P ** 2, dtype=K.F16, device=m.device)
        nbytes = buf.numel() + out.numel() * 2
        t = timed(lambda: K.vision_patches(buf, desc, tab, m.norm_tab, m.S, m.P, rows, out=out), w, r)
        row("front end (kernel + descriptor upload)", t, f", {nbytes / t[0] / 1e9:.3f} TB/s of {HBM_TBS} ({nbytes / 1e6:.1f} MB)")
        row("front end with image upload (patches())", timed(lambda: m.patches(ims), w, r))
        P = m.patches(ims)
        row("patch embed + assembly", t := timed(lambda: m.embed(P), w, r), f", {B * fl[2] / t[0] / 1e9:.1f} TF/s")
        X = m.embed(P)
        row("layers", t := timed(lambda: V.transformer_layers(X, m.layers, m.H, V.LN_EPS), w, r),
            f", {B * (fl[0] + fl[1]) / t[0] / 1e9:.1f} TF/s = {B * (fl[0] + fl[1]) / t[0] / 1e9 / PEAK_TF:.3f} of peak")
        Y = V.transformer_layers(X, m.layers, m.H, V.LN_EPS)
        host = torch.empty(B, m.T, m.d, dtype=K.F16, pin_memory=True)

        def tail():
            y = K.layernorm(Y, m.norm_g, m.norm_b, V.LN_EPS)[0]
            K.nonfinite_rows(y.view(B, -1))
            host.copy_(y.view(B, m.T, m.d), non_blocking=True)
        row("final LN + non-finite check + copy-out (fp16)", timed(tail, w, r))
        t = timed(lambda: m.forward_device(ims), w, r)
        row("device forward, images -> tokens", t, f", {B / t[0] * 1e3:.0f} images/s, {B * sum(fl) / t[0] / 1e9:.1f} TF/s = "
            f"{B * sum(fl) / t[0] / 1e9 / PEAK_TF:.3f} of peak (the training step's GEMM family: 0.29)")
        dst = torch.empty(B, m.T, m.d)
        m.features(ims, out=dst)
        t = host_time(lambda: m.features(ims, out=dst), r)
        row("features(): with copy-out and fp32 widening", t, f", {B / t[0] * 1e3:.0f} images/s (host clock)")

    try:
        from PIL import Image
    except ImportError:
        lines.append("  PIL is not installed: no host baseline")
    else:
        torch.set_num_threads(1)
        im = images[0]
        S = m.S

        def host_transform():
            u8 = VR.pillow_transform_u8(im, S)
            return (torch.from_numpy(u8.copy()).permute(2, 0, 1).float() / 255 - 0.5) / 0.5
        lines.append(" host, one thread, per image")
        print(lines[-1], flush=True)
        row("Pillow resize + crop + torch normalise", host_time(host_transform, 20))
        for q in (75, 95):
            bio = io.BytesIO()
            Image.fromarray(im).save(bio, format="JPEG", quality=q)
            data = bio.getvalue()
            row(f"Pillow JPEG decode, quality {q} ({len(data) // 1024} KiB, noise image)",
                host_time(lambda: np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), 20))
        y, x = np.mgrid[0:args.height, 0:args.width]
        smooth = np.stack([128 + 100 * np.sin(x / 40.0 + c) * np.cos(y / 30.0) for c in range(3)], -1).astype(np.uint8)
        bio = io.BytesIO()
        Image.fromarray(smooth).save(bio, format="JPEG", quality=90)
        data = bio.getvalue()
        row(f"Pillow JPEG decode, smooth image ({len(data) // 1024} KiB)",
            host_time(lambda: np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), 20))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

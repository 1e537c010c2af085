"""Timing of the ViT attention rollout (multimodal-s2ut_amd/vision.py ViTFeatures.rollout_device) at vit_base
shapes (577 tokens, 12 heads, 12 layers) with seeded random weights on synthetic 500 x 375 images, B = 8.

    python scripts/rollout_bench.py [--batch 8] [--warmup 3] [--repeats 10] [--out FILE]

After a warm-up the three contenders alternate in one process, round by round, so that clocks and caches
drift for all alike: the plain forward (forward_device), the rollout (the same forward with the fused
probabilities formed per layer, then the discard and the chain), and a torch-on-device baseline that runs the
same forward but materialises each layer's [B, H, T, T] probabilities with torch ops (matmul, softmax, mean)
and finishes with torch.topk, index assignment and matmul, the reference's own steps moved to the device.  HIP
events on the stream the kernels run on; median [min .. max] of the repeats; every time is event time around
one call, host launch gaps included.  The three rollout kernels are also timed alone on the buffers of one
pass."""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def torch_rollout(m, images, ratio):
    """The reference's steps with torch ops on the device: the probabilities of every layer materialised."""
    B, T, H = len(images), m.T, m.H
    d = m.d
    fused = []

    def on_qkv(l, qkv):
        q, k = (qkv[:, i * d:(i + 1) * d].float().view(B, T, H, d // H).transpose(1, 2) for i in range(2))
        fused.append(torch.softmax(q @ k.transpose(2, 3) * (d // H) ** -0.5, dim=-1).mean(dim=1))
    m.tokens(m.embed(m.patches(images)), on_qkv=on_qkv)
    eye = torch.eye(T, device=m.device)
    kk = int(T * T * ratio)
    masks = []
    for b in range(B):
        result = eye
        for F in fused:
            flat = F[b].reshape(-1)
            _, idx = flat.topk(kk, -1, False)
            flat[idx[idx != 0]] = 0
            a = (flat.view(T, T) + eye) / 2
            a = a / a.sum(dim=-1)
            result = a @ result
        mask = result[0, 1:]
        masks.append(mask / mask.max())
    return torch.stack(masks)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default="vit_base_patch16_384")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--discard-ratio", type=float, default=0.9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench needs a GPU: a CPU run gives no timing")
    import vit_ref as VR
    from asr_bench import timed
    V = importlib.import_module("multimodal-s2ut_amd.vision")
    K = importlib.import_module("multimodal-s2ut_amd.kernels")

    cfg = V.model_config(args.model)
    m = V.ViTFeatures(VR.make_state_dict(cfg, 0), cfg, device="cuda:0")
    B, T, L, ratio = args.batch, m.T, len(m.layers), args.discard_ratio
    images = [VR.make_image(500, 375, i) for i in range(B)]
    ws_bytes = 4 * B * L * T * T
    lines = [f"rollout_bench: {args.model} (d {m.d}, {m.H} heads, {L} layers, {T} tokens), B = {B}, discard ratio {ratio}; "
             f"{torch.cuda.get_device_name(0)}",
             f"  workspace [B, L, T, T] fp32: {ws_bytes / 2 ** 20:.1f} MiB (bound {V.ROLLOUT_WS_BYTES >> 20} MiB, "
             f"{m.rollout_chunk()} images per pass)"]
    print("\n".join(lines), flush=True)

    contenders = [("forward_device alone", lambda: m.forward_device(images)),
                  ("rollout (forward + probabilities + discard + chain)", lambda: m.rollout_device(images, "mean", ratio)),
                  ("torch on device (probabilities materialised, topk, matmul)", lambda: torch_rollout(m, images, ratio))]
    got = m.rollout_device(images, "mean", ratio)[0]
    ref = torch_rollout(m, images, ratio)
    lines.append(f"  max |rollout - torch baseline| over the masks: {float((got - ref).abs().max()):.2e} (topk ties and fp32 "
                 f"summation order differ)")
    print(lines[-1], flush=True)
    for _ in range(args.warmup):
        for _, fn in contenders:
            fn()
    times = [[] for _ in contenders]
    for _ in range(args.repeats):
        for ts, (_, fn) in zip(times, contenders):
            ts.append(timed(fn, 0, 1)[0])
    med = []
    for (name, _), ts in zip(contenders, times):
        med.append(statistics.median(ts))
        lines.append(f"  {name:<62s} {med[-1]:9.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]")
        print(lines[-1], flush=True)
    lines.append(f"  rollout over the plain forward: +{med[1] - med[0]:.3f} ms ({med[1] / med[0]:.2f} x); the torch baseline is "
                 f"{med[2] / med[1]:.2f} x the rollout")
    print(lines[-1], flush=True)

    # the kernels alone, on the buffers of one pass
    qkv = (torch.randn(B * T, 3 * m.d, generator=torch.Generator().manual_seed(0))).half().to(m.device)
    ws = torch.empty(B, L, T, T, dtype=torch.float32, device=m.device)
    for l in range(L):
        K.rollout_probs(qkv, B, m.H, T, "mean", out=ws[:, l])
    keep = ws.clone()
    w, r = args.warmup, args.repeats
    t = timed(lambda: K.rollout_probs(qkv, B, m.H, T, "mean", out=ws[:, 0]), w, r)
    lines.append(f"  rollout_probs, one layer                                       {t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]")
    k = K.rollout_discard_count(T, ratio)

    def discard():
        ws.copy_(keep)
        K.rollout_discard(ws, k)
    tc = timed(lambda: ws.copy_(keep), w, r)
    t = timed(discard, w, r)
    lines.append(f"  rollout_discard, {B * L} matrices (with a {tc[0]:.3f} ms restore copy)      {t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]")
    t = timed(lambda: K.rollout_chain(ws, "reference"), w, r)
    lines.append(f"  rollout_chain, {B} images x {L} layers                            {t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]")
    print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Timing of the speech-to-unit step (multimodal-s2ut_amd/units.py) at the HuBERT-base configuration with
seeded random weights and 1000 random centroids: one 5 s utterance alone and 16 of them in one batch.

    python scripts/units_bench.py [--seconds 5] [--batch 16] [--layers 11] [--repeats 20] [--out FILE]

HIP events on the stream the kernels run on, warm-up first, median (min .. max) of the repeats.  Every time
is event time around one call, host launch gaps included.  kmeans_assign's FLOPs are the algorithm's, 2 R Kc
d (the kernel issues twice that: a hi and a lo product per term); its two chunk widths are timed on the same
rows, since the narrow one exists for the single-utterance case."""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--layers", type=int, default=11, help="km_layer of a 12-layer model")
    ap.add_argument("--centroids", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("units_bench needs a GPU: a CPU run gives no timing")
    import asr_ref as AR
    import hubert_ref as HR
    from asr_bench import timed
    U = importlib.import_module("multimodal-s2ut_amd.units")
    K = importlib.import_module("multimodal-s2ut_amd.kernels")

    cfg = dict(HR.WIDE, num_hidden_layers=12)
    cents = torch.randn(args.centroids, cfg["hidden_size"], generator=torch.Generator().manual_seed(1))
    m = U.HubertUnits(HR.make_state_dict(cfg, 0), cfg, cents.numpy(), args.layers, device="cuda:0")
    n = int(args.seconds * 16000)
    waves = [AR.to_float(AR.make_wave(n, 10 + i)) for i in range(args.batch)]
    x = m._wave(waves[0])
    T = U.frame_counts(n, m.kernels, m.strides)[-1]
    lines = [f"units_bench: {args.seconds} s utterances ({n} samples, {T} frames), batch {args.batch}, km_layer "
             f"{args.layers}, {args.centroids} centroids, d {m.d}; {torch.cuda.get_device_name(0)}"]

    def row(name, fn, flops=None):
        med, lo, hi = timed(fn, args.warmup, args.repeats)
        tf = f", {flops / med / 1e9:.2f} TF/s" if flops else ""
        lines.append(f"  {name:<46s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f}){tf}")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    c0 = m.conv[0]
    row("hubert_conv0 (layer 0, GroupNorm over time)", lambda: K.hubert_conv0(x, None, c0.w, c0.b, c0.g, c0.be, c0.stride))
    row("extractor + projection, 1 utterance", lambda: m.extract(x))
    row("features at km_layer, 1 utterance", lambda: m.features_batch(waves[:1]))
    row(f"features at km_layer, {args.batch} utterances", lambda: m.features_batch(waves))
    for B in (1, args.batch):
        Fb = m.features_batch(waves[:B])[0]
        R = Fb.shape[0] * Fb.shape[1]
        fl = 2.0 * R * args.centroids * m.d
        for chunk in (64, 256):
            row(f"kmeans_assign + fold, {R} rows, chunk {chunk}",
                lambda: K.kmeans_assign(Fb, m.c_hi, m.c_lo, m.c_norm, chunk=chunk), fl)
        try:      # what the kernel replaces: the [R, Kc] scores written out (fp16 centroids), then an argmin
            row(f"torch fp16 matmul + argmin, {R} rows (baseline)",
                lambda: (m.c_norm[None] - 2.0 * (Fb.reshape(R, -1) @ m.c_hi[:args.centroids].t()).float()).argmin(1), fl)
        except RuntimeError as e:
            lines.append(f"  torch baseline unavailable: {str(e).splitlines()[0]}")
    row("units, 1 utterance (end to end, with the copy back)", lambda: m.units(waves[0]))
    row(f"units_many, {args.batch} utterances", lambda: m.units_many(waves, args.batch))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Timing of the top-k beam decode of speech units (kernels.kmeans_topk, kernels.units_beam) on random
features that sit among 1000 random centroids of width 768, at the reference's defaults top_k 10, beamsize 200.

    python scripts/units_beam_bench.py [--batch 8] [--frames 500] [--repeats 20] [--out FILE]

HIP events on the stream the kernels run on, warm-up first, median (min .. max) of the repeats (the scheme
of scripts/units_bench.py): every time is event time around one call, host launch gaps and the allocation
of the outputs included.  kmeans_topk is timed next to kmeans_assign on the same rows (both with their fold),
units_beam at the full and at half the frame count, and the host restatement units.beam_decode_host on one
utterance of half the frame count with time.perf_counter on this machine's CPU."""
import argparse
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--centroids", type=int, default=1000)
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--beamsize", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("units_beam_bench needs a GPU: a CPU run gives no timing")
    from asr_bench import timed
    U = importlib.import_module("multimodal-s2ut_amd.units")
    K = importlib.import_module("multimodal-s2ut_amd.kernels")

    g = torch.Generator().manual_seed(1)
    B, T, d, Kc = args.batch, args.frames, args.width, args.centroids
    cents = torch.randn(Kc, d, generator=g)
    which = torch.randint(0, Kc, (B, T), generator=g)
    stay = torch.rand(B, T, generator=g) < 0.6                  # runs, as speech has them
    for t in range(1, T):
        which[:, t] = torch.where(stay[:, t], which[:, t - 1], which[:, t])
    X = (cents[which] + 0.5 * torch.randn(B, T, d, generator=g)).half().cuda()
    packed = tuple(t.cuda() for t in K.kmeans_pack(cents))
    lines = [f"units_beam_bench: batch {B} x {T} frames, d {d}, {Kc} centroids, top_k {args.top_k}, beamsize "
             f"{args.beamsize}; {torch.cuda.get_device_name(0)}"]

    def row(name, fn):
        med, lo, hi = timed(fn, args.warmup, args.repeats)
        lines.append(f"  {name:<52s} {med:9.3f} ms ({lo:.3f} .. {hi:.3f})")
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    row(f"kmeans_assign + fold, {B * T} rows", lambda: K.kmeans_assign(X, *packed))
    row(f"kmeans_topk + fold, {B * T} rows, top_k {args.top_k}", lambda: K.kmeans_topk(X, *packed, top_k=args.top_k))
    idx, dist, bad = K.kmeans_topk(X, *packed, top_k=args.top_k)
    assert bad.tolist() == [0] * B
    for Tb in (T // 2, T):
        i2, d2 = idx[:, :Tb].contiguous(), dist[:, :Tb].contiguous()
        row(f"units_beam, batch {B}, {Tb} frames", lambda: K.units_beam(i2, d2, beamsize=args.beamsize))
    beam = K.units_beam(idx[:, :T // 2].contiguous(), dist[:, :T // 2].contiguous(), beamsize=args.beamsize)[0]
    ih, dh = idx[0, :T // 2].cpu().numpy(), dist[0, :T // 2].cpu().numpy()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        host = U.beam_decode_host(ih, dh, args.beamsize)
        ts.append((time.perf_counter() - t0) * 1e3)
    assert host == beam[0].tolist()
    lines.append(f"  {'beam_decode_host (NumPy, CPU), 1 utterance, ' + str(T // 2) + ' frames':<52s} {sorted(ts)[1]:9.3f} ms "
                 f"({min(ts):.3f} .. {max(ts):.3f}); equal to the device's: True")
    print(lines[-1], flush=True)
    greedy = sum(len(U.merge(idx[b, :, 0].tolist())) for b in range(B))
    merged = K.units_beam(idx, dist, beamsize=args.beamsize)[2].sum().item()
    lines.append(f"  merged units over the batch: greedy {greedy}, beam {merged}")
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

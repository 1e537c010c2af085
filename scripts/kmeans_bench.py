"""Wall time of UnitKMeans.fit on synthetic features, and scikit-learn's time per mini-batch step on the CPU.

    python scripts/kmeans_bench.py [--rows 1000000] [--dim 768] [--clusters 1000] [--repeats 3]      (GPU)
    python scripts/kmeans_bench.py --sklearn-steps 5                                                 (CPU)

GPU: fp16 rows around `clusters` seeded centres; one short warm-up fit (loads the code objects), then `repeats`
fits each of fairseq's defaults (n_init 20, max_iter 150, batch 10000, max_no_improvement 100: the rule may stop
the fit early, the steps run are printed) and of the same with max_no_improvement None (all max_iter * rows /
batch steps).  A host clock around fit, the device queue drained before and after.
CPU (--sklearn-steps N): scikit-learn's _mini_batch_step on fp32 rows of the same shapes with BLAS limited to one
thread, as MiniBatchKMeans.fit runs it: seconds per step over N steps after one warm-up step.  A per-step figure;
a whole fit's time is that times the steps, plus 20 k-means++ seedings, and is not measured."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sklearn_steps(args):
    from sklearn.cluster import _kmeans as SK
    rs = np.random.RandomState(0)
    K, d, bs = args.clusters, args.dim, args.batch
    C = rs.standard_normal((K, d)).astype(np.float32)
    Cn = np.empty_like(C)
    w, counts = np.ones(bs, np.float32), np.zeros(K, np.float32)
    times = []
    with SK._get_threadpool_controller().limit(limits=1, user_api="blas"):
        for i in range(args.sklearn_steps + 1):
            Xb = (C[rs.randint(0, K, bs)] + 0.5 * rs.standard_normal((bs, d))).astype(np.float32)
            t0 = time.perf_counter()
            SK._mini_batch_step(Xb, w, C, Cn, counts, rs, random_reassign=False, reassignment_ratio=0.0, n_threads=1)
            times.append(time.perf_counter() - t0)
            C, Cn = Cn, C
    t = np.array(times[1:])
    print(f"scikit-learn _mini_batch_step, batch {bs} x {d}, {K} clusters, one BLAS thread: median {np.median(t):.3f} s "
          f"[{t.min():.3f} .. {t.max():.3f}] per step over {len(t)} steps")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sklearn-steps", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.sklearn_steps:
        return sklearn_steps(args)
    import torch
    KM = importlib.import_module("multimodal-s2ut_amd.kmeans")
    assert torch.cuda.is_available(), "the fit is timed on the GPU only"
    g = torch.Generator(device=args.device).manual_seed(0)
    cen = torch.randn(args.clusters, args.dim, generator=g, device=args.device)
    X = torch.empty(args.rows, args.dim, dtype=torch.float16, device=args.device)
    for r0 in range(0, args.rows, 100000):                       # in slices: no fp32 copy of the whole set
        r1 = min(args.rows, r0 + 100000)
        pick = torch.randint(0, args.clusters, (r1 - r0,), generator=g, device=args.device)
        X[r0:r1] = (cen[pick] + 0.5 * torch.randn(r1 - r0, args.dim, generator=g, device=args.device)).half()
    KM.learn_kmeans(X[:20000].contiguous(), 16, max_iter=2, batch_size=1000, n_init=2)        # warm-up
    for label, mni in (("fairseq's defaults", 100), ("max_no_improvement None", None)):
        secs, steps = [], []
        for _ in range(args.repeats):
            km, s = KM.learn_kmeans(X, args.clusters, batch_size=args.batch, max_no_improvement=mni, seed=1337)
            secs.append(s)
            steps.append(km.n_steps_)
        print(f"UnitKMeans.fit [{args.rows}, {args.dim}] fp16, K {args.clusters}, {label}: median {np.median(secs):.2f} s "
              f"[{min(secs):.2f} .. {max(secs):.2f}] over {args.repeats} fits, steps {steps}, EWA inertia "
              f"{km.ewa_inertia_:.4f}", flush=True)


if __name__ == "__main__":
    sys.exit(main())

"""Timing of R-Drop (--rdrop-alpha), one MI355X, HIP events.  Recorded, not gated.

(a) The pair kernels ``ls_xent_rdrop_fwd`` + ``ls_xent_rdrop_bwd`` at 2R = 40000 rows, V = 1004,
    ld = 1024 (every 7th target pad) against the plain ``ls_xent_fwd`` + ``ls_xent_bwd`` on the same
    2R rows and against the torch composition of the definition (fp32 log_softmax, two F.kl_div,
    label-smoothed CE, autograd backward).  5 warm-up calls, then 9 repeats of 20 calls; median
    [min .. max] of the repeats.  The backward runs in place, so every call works on the gradient
    the previous call left: the traffic is the same, the values are not logits.
(b) ms per training step of the base configuration (bench.py's model, batches and GPU front end,
    eager mode) with rdrop_alpha = 0.3 at half of bench.py's max-tokens against the plain step at
    the full max-tokens: the same number of rows passes through the model in both; the difference
    is the duplication copies and the criterion.  The two trainers alternate windows of ``--steps``
    steps; median [min .. max] over ``--reps`` windows each.

    python scripts/rdrop_bench.py [--max-tokens 40000] [--steps 8] [--reps 7] [--skip-step]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
mm = importlib.import_module("multimodal-s2ut_amd")
K = mm.kernels


def timed(fn, warm=5, reps=9, calls=20):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / calls * 1e3)
    us = np.sort(us)
    return float(np.median(us)), float(us[0]), float(us[-1])


def kernels():
    rows, V, ld, eps, pad, A = 40000, 1004, 1024, 0.2, 1, 0.3
    R = rows // 2
    g = torch.Generator(device="cuda").manual_seed(0)
    src = torch.randn(rows, ld, device="cuda", generator=g).half()
    t1 = torch.randint(2, V, (R,), device="cuda", generator=g)
    t1[6::7] = pad
    t2 = torch.cat((t1, t1))
    one = torch.ones(1, device="cuda")
    out2, out3 = torch.empty(2, device="cuda"), torch.empty(3, device="cuda")
    buf = src.clone()

    def pair():
        lse = K.ls_xent_rdrop_fwd(buf, ld, t1, rows, V, eps, pad, A, call_out=out3)
        K.ls_xent_rdrop_bwd(buf, ld, t1, rows, V, eps, pad, A, lse, one, buf)

    def plain():
        lse = K.ls_xent_fwd(buf, ld, t2, rows, V, eps, pad, None, call_out=out2)
        K.ls_xent_bwd(buf, ld, t2, rows, V, eps, pad, lse, one, buf)

    def pair_fwd():
        K.ls_xent_rdrop_fwd(src, ld, t1, rows, V, eps, pad, A, call_out=out3)

    def plain_fwd():
        K.ls_xent_fwd(src, ld, t2, rows, V, eps, pad, None, call_out=out2)

    keep = t1.ne(pad).unsqueeze(-1)

    def composed():
        z = src[:, :V].float().requires_grad_(True)
        lp = F.log_softmax(z, -1)
        p = lp.exp()
        kl = (F.kl_div(lp[:R], p[R:], reduction="none") * keep).sum() + \
             (F.kl_div(lp[R:], p[:R], reduction="none") * keep).sum()
        k2 = torch.cat((keep, keep))
        nll = -(lp.gather(1, t2.unsqueeze(1)) * k2).sum()
        smooth = -(lp * k2).sum()
        ei = eps / (V - 1)
        ((1 - eps - ei) * nll + ei * smooth + A * kl / 2).backward()
        return z.grad.half()

    floor = rows * ld * 2
    print(f"(a) 2R = {rows} rows, V = {V}, ld = {ld}: logits {floor / 1e6:.1f} MB; floor traffic fwd {floor / 1e6:.1f} MB, "
          f"fwd + bwd {3 * floor / 1e6:.1f} MB", flush=True)
    for name, fn, by in (("ls_xent_rdrop fwd + bwd", pair, 3 * floor), ("ls_xent fwd + bwd (plain)", plain, 3 * floor),
                         ("ls_xent_rdrop fwd", pair_fwd, floor), ("ls_xent fwd (plain)", plain_fwd, floor),
                         ("torch composition fwd + bwd", composed, None)):
        buf.copy_(src)
        t = timed(fn, calls=20 if by else 3)
        rate = f"  {by / t[0] / 1e6:.2f} TB/s of the floor traffic" if by else ""
        print(f"{name:<30s} {t[0]:9.1f} us  [{t[1]:.1f} .. {t[2]:.1f}]{rate}", flush=True)


def steps(args):
    sys.argv = sys.argv[:1]
    import bench
    cfg = mm.default_cfg()
    fe = bench.frontend_mod.FbankFrontend(torch.device("cuda"))
    runs = []
    for name, alpha, mt in (("plain, max-tokens %d" % args.max_tokens, 0.0, args.max_tokens),
                            ("rdrop 0.3, max-tokens %d" % (args.max_tokens // 2), 0.3, args.max_tokens // 2)):
        c = dict(cfg, rdrop_alpha=alpha) if alpha > 0 else dict(cfg)
        np.random.seed(1)
        model = mm.MMS2UTModel(c, device="cuda").init_params(seed=1)
        tr = bench.trainer_mod.Trainer(model, lr=5e-4, world_size=1)
        batches = bench.make_batches(c, 0, args.nbatches, mt, torch.device("cuda"), fe)

        def step(i, tr=tr, batches=batches):
            wb, batch = batches[i % len(batches)][:2]

            def frontend():
                batch.src = fe(wb)
            return tr.train_step(batch, prologue=frontend)

        for i in range(16):          # loss-scale settling, as bench.py
            step(i)
            if not tr.opt.stats()["overflow"]:
                break
        for i in range(len(batches)):
            step(i)
        rows = [(int(b[1].prev.numel()) * (2 if alpha > 0 else 1), int(b[1].prev.shape[0])) for b in batches]
        runs.append((name, step, rows, []))
    for rep in range(args.reps):
        for name, step, rows, ms in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(args.steps):
                step(i)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
    print(f"(b) base configuration, eager steps, {args.nbatches} resident batches, windows of {args.steps} steps, "
          f"{args.reps} alternating windows each", flush=True)
    for name, step, rows, ms in runs:
        ms = np.sort(ms)
        print(f"{name:<32s} {np.median(ms):8.2f} ms/step  [{ms[0]:.2f} .. {ms[-1]:.2f}]  target rows through the "
              f"model per batch {[r for r, _ in rows]}, sentences {[b for _, b in rows]}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-tokens", type=int, default=40000)
    ap.add_argument("--nbatches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rdrop_bench: needs a GPU")
    if not a.skip_kernels:
        kernels()
    if not a.skip_step:
        steps(a)

"""Timing of the validation path.

1. The forward-only scoring kernel ``ls_xent_eval`` against the training forward ``ls_xent_fwd_log``
   at the base shape: 12,080 rows x 1004 columns, ld 1024, every 7th target pad.  HIP events, the
   scheme of scripts/noise_bench.py: 5 warm-up calls, then 9 repeats of 20 calls; median
   [min .. max] of the repeats.
2. One validation pass (``Trainer.validate``: no host read per batch) over the test corpus
   (tests/manifest_corpus.py: 8 utterances, batches of --max-tokens 300, base model) against the
   same resident batches through ``Trainer.valid_step`` with an ``.item()`` of loss and nll per
   batch.  Wall time around a device synchronise: 2 warm-up passes, median [min .. max] of 9."""
import importlib
import os
import sys
import tempfile
import time

import numpy as np
import torch

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


def wall(fn, warm=2, reps=9):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.sort(ms)
    return float(np.median(ms)), float(ms[0]), float(ms[-1])


def kernels():
    rows, V, ld, eps, pad = 12080, 1004, 1024, 0.2, 1
    logits = torch.randn(rows, ld, device="cuda").half()
    target = torch.randint(0, V, (rows,), device="cuda")
    target[::7] = pad
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    log = torch.zeros(2, device="cuda")
    out = torch.empty(2, device="cuda")
    by = rows * V * 2
    for name, fn in (("ls_xent_eval", lambda: K.ls_xent_eval(logits, ld, target, rows, V, eps, pad, stats)),
                     ("ls_xent_fwd_log", lambda: K.ls_xent_fwd(logits, ld, target, rows, V, eps, pad, log, call_out=out))):
        t = timed(fn)
        print(f"{name:<18s} {t[0]:7.1f} us  [{t[1]:.1f} .. {t[2]:.1f}]  {by / 1e6:.1f} MB of logits", flush=True)


def passes():
    from manifest_corpus import write_corpus
    M = mm.manifest
    cfg = mm.default_cfg()
    model = mm.MMS2UTModel(cfg, device="cuda").init_params(seed=1)
    tr = mm.trainer.Trainer(model)
    with tempfile.TemporaryDirectory() as d:
        c = write_corpus(d, frames=(150, 97, 200, 61, 88, 131, 45, 170), di=cfg["image_feat_dim"], ti=12, split="valid")
        ds = M.MultiModalS2SManifest(d, "valid", M.UnitDictionary.for_codes(cfg["vocab_size"] - 4),
                                     data_cfg=M.load_data_config(os.path.join(d, "config.yaml")),
                                     image_feat_path=[c["feat_dir"]], is_train=False)
        batches = [b for b, _ in M.DeviceLoader(ds, ds.batches(300), dict(cfg, multitask=None), "cuda")]
    torch.cuda.synchronize()

    def per_batch():
        tot = [0.0, 0.0]
        for b in batches:
            loss, nll = tr.valid_step(b)
            tot[0] += loss.item()
            tot[1] += nll.item()
        return tot

    ntok = sum(b.ntokens for b in batches)
    print(f"{len(batches)} batches, {ntok} target tokens", flush=True)
    for name, fn in (("Trainer.validate (one host read)", lambda: tr.validate(batches)),
                     ("valid_step + .item() per batch", per_batch)):
        t = wall(fn)
        print(f"{name:<34s} {t[0]:7.2f} ms  [{t[1]:.2f} .. {t[2]:.2f}]", flush=True)


if __name__ == "__main__":
    kernels()
    passes()

"""Isolated timing of the unit vocoder (multimodal-s2ut_amd/vocoder.py) at the released model's shape
(unit_hifigan_*_km1000_lj_dur: rates 5,4,4,2,2, 512 initial channels, 320 samples per unit) with random
weights, on utterances of 50 / 250 / 500 units without duration prediction (320 samples per unit, so
the lengths are fixed) and 250 units with it.

Per length: HIP events around 20 back-to-back synthesize() calls, 3 warm-up rounds, then the
median [min .. max] of 7 repeats; samples/s and the real-time factor (audio seconds per second of
wall time) follow from the median.  Also printed: kernel launches per utterance, the time of the
tests' CPU restatement (torch fp32, 16 threads, one run after one warm-up), and the same forward
issued with one library call per kernel from Python (synthesize_stepwise) next to the one-call
path.  Not part of bench.py."""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vocoder_ref as VR  # noqa: E402

V = importlib.import_module("multimodal-s2ut_amd.vocoder")
SR = 16000


def timed(fn, warm=3, reps=7, calls=20):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    ms = np.sort(ms)
    return float(np.median(ms)), float(ms[0]), float(ms[-1])


def gen_flops(cfg, T):
    """Algorithmic FLOPs (2 per multiply-add) of the generator's convolutions for T frames."""
    ch, fl = cfg["upsample_initial_channel"], 2 * T * cfg["model_in_dim"] * cfg["upsample_initial_channel"] * 7
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        fl += 2 * T * ch * (ch // 2) * k                  # ConvTranspose1d: every input row meets all k taps
        T, ch = T * u, ch // 2
        for rk, dils in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            fl += 2 * len(dils) * 2 * T * ch * ch * rk
    return fl + 2 * T * ch * 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, nargs="+", default=[50, 250, 500])
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement's timing")
    args = ap.parse_args()
    torch.set_num_threads(16)
    sd = VR.make_state_dict(VR.RELEASED, seed=1)
    voc = V.CodeHiFiGAN(sd, VR.RELEASED, device="cuda")
    print(f"device: {torch.cuda.get_device_name(0)}; released shape, random weights (seed 1)", flush=True)
    for T in args.units:
        codes = torch.randint(0, 1000, (T,), generator=torch.Generator().manual_seed(T)).cuda()
        n = voc.synthesize(codes).numel()
        med, lo, hi = timed(lambda: voc.synthesize(codes))
        line = (f"T={T:4d} units  {n:7d} samples  {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]  "
                f"{n / med * 1e3 / 1e6:7.2f} Msamples/s  RTF {n / SR / (med * 1e-3):7.1f}x  launches {voc.launches}  "
                f"{gen_flops(VR.RELEASED, T) / 1e9:6.1f} GFLOP = {gen_flops(VR.RELEASED, T) / med / 1e9:5.1f} TFLOP/s")
        if not args.no_cpu:
            VR.forward(sd, VR.RELEASED, codes.cpu())
            t0 = time.perf_counter()
            VR.forward(sd, VR.RELEASED, codes.cpu())
            cpu = (time.perf_counter() - t0) * 1e3
            line += f"  CPU restatement {cpu:8.1f} ms ({cpu / med:.1f}x)"
        print(line, flush=True)
    T = 250
    codes = torch.randint(0, 1000, (T,), generator=torch.Generator().manual_seed(T)).cuda()
    med, lo, hi = timed(lambda: voc.synthesize_stepwise(codes))
    print(f"T={T:4d} units, one library call per kernel (synthesize_stepwise): {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]", flush=True)
    n = voc.synthesize(codes, dur_prediction=True).numel()
    med, lo, hi = timed(lambda: voc.synthesize(codes, dur_prediction=True))
    print(f"T={T:4d} units + duration prediction  {n:7d} samples  {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]  "
          f"RTF {n / SR / (med * 1e-3):7.1f}x  launches {voc.launches}", flush=True)
    med, lo, hi = timed(lambda: voc.durations(codes), calls=20)
    print(f"duration predictor alone (2 launches, T=250): {med * 1e3:.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]", flush=True)


if __name__ == "__main__":
    main()

"""Isolated time of the operand-reading fused epilogues (residual-dropout, ReLU-dropout backward,
accumulate, gate) and of the plain / ReLU-dropout ones on the step's NT shapes, with the default
epilogue path and with the fp32-staged one (mms2ut_gemm_set_epilogue(1)).  MMS2UT_LIB selects the
library, so two builds can be compared in one GPU session.
usage: python scripts/epi_aux_bench.py [reps]"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K = importlib.import_module("multimodal-s2ut_amd").kernels
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def t(fn, reps=REPS):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def operands(M, N, Kd):
    g = torch.Generator(device="cuda").manual_seed(M + N + Kd)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return ((r(M, Kd) * 0.5).half(), (r(N, Kd) * 0.05).half(), (r(N) * 0.1).half(), r(M, N).half(),
            torch.empty(M, N, dtype=torch.float16, device="cuda"))


rows = []
for M, N, Kd, forms in ((10000, 768, 768, ("plain", "resid")), (10000, 768, 3072, ("resid",)),
                        (12000, 3072, 768, ("relu", "relu_bwd")), (10000, 3072, 768, ("plain", "relu")),
                        (12000, 768, 768, ("resid", "acc"))):
    x, W, b, aux, out = operands(M, N, Kd)
    cases = {
        "plain": lambda: K.linear(x, W, b, out=out),
        "relu": lambda: K.linear(x, W, b, out=out, epi=K.EPI_RELU_DROP, p=0.1, drop=(1, 4096)),
        "resid": lambda: K.linear(x, W, b, out=out, epi=K.EPI_DROP_RESID, aux=aux, p=0.1, drop=(1, 4096)),
        "relu_bwd": lambda: K.linear(x, W, out=out, epi=K.EPI_RELU_DROP_BWD, aux=aux, p=0.1, drop=(1, 4096)),
        "acc": lambda: K.linear(x, W, out=out, epi=K.EPI_F16_ACC),
    }
    for name in forms:
        us = []
        try:
            for staged in (0, 1):
                K.call("mms2ut_gemm_set_epilogue", staged)
                us.append(t(cases[name]))
        finally:
            K.call("mms2ut_gemm_set_epilogue", 0)
        fl = 2.0 * M * N * Kd
        print(f"{M:6d} x {N:4d} x {Kd:4d} {name:9s} default {us[0]:7.1f} us ({fl / us[0] / 1e6:5.0f} TF)   "
              f"fp32-staged {us[1]:7.1f} us", flush=True)

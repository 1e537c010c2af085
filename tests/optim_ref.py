"""fairseq's fp16 optimizer step, restated in float64 on the CPU (test infrastructure).

What the device-resident optimizer (optim.py, csrc/loss_optim.hip) has to compute, written out from
fairseq's published sources and sharing no code with the package or with oracle/ref_model.py (so the
two restatements check each other, tests/test_optim_ref.py):

  FP16Optimizer            g = fp16 grad * 1/(loss_scale * max(sample_size, 1)); norm = |g|_2;
                           a non-finite norm is an overflow: nothing is updated
  clip_grad_norm           g *= clip / norm when clip > 0 and norm > clip
  InverseSquareRootSchedule  lr at the count of *completed* (non-skipped) updates
  Adam.step                p -= wd lr p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
                           p -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)
  DynamicLossScaler        halve on overflow (FloatingPointError at the minimum scale), double when
                           the iterations since the last overflow are a multiple of the window
  Trainer._check_grad_norms  the norms of all ranks are finite and differ by >= 1e-6 relative

fairseq is not importable here, so none of this is pinned against the library itself.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U32 = 2.0 ** -24     # unit roundoff of fp32


def f32r(x):
    """x rounded to fp32, as a Python float: what a C ``float`` argument receives."""
    return float(np.float32(x))


def multiply_factor(loss_scale, sample_size):
    ss = 1.0 if sample_size is None else max(float(sample_size), 1.0)
    return 1.0 / (float(loss_scale) * ss)


def inverse_sqrt_lr(updates, hp):
    wu, peak, init = hp["warmup_updates"], hp["lr"], hp["warmup_init_lr"]
    if wu > 0 and updates < wu:
        return init + updates * ((peak - init) / wu)
    return peak * math.sqrt(max(wu, 1)) / math.sqrt(max(updates, 1))


def adam_update(p, m, v, g, lr, step_size, b1, b2, eps, wd):
    """One Adam element update in the dtype of ``p`` (every scalar is rounded to that dtype first, every
    operation rounds once: no fused multiply-add).  -> new (p, m, v); the inputs are left alone."""
    dt = p.dtype
    c = lambda x: torch.tensor(float(x), dtype=dt)
    one = c(1.0)
    if wd != 0:
        p = p - c(wd) * c(lr) * p
    m = c(b1) * m + (one - c(b1)) * g
    v = c(b2) * v + (one - c(b2)) * g * g
    p = p - c(step_size) * m / (v.sqrt() + c(eps))
    return p, m, v


def ref_step(state, grad16, sample_size, hp):
    """One FP16Optimizer + Adam step in fp64.

    state: {"master", "exp_avg", "exp_avg_sq": fp64 tensors, "updates": completed updates,
            "loss_scale": the scale the gradient was computed under}
    hp:    {"lr", "warmup_updates", "warmup_init_lr", "betas", "eps", "weight_decay", "clip_norm"}
    -> (new state, info); info holds mult, gnorm, overflow and, when the step is applied, clip_coef, lr,
    step_size and the unscaled, clipped gradient g.  On overflow the new state is the old one (the loss
    scale is the scaler's business: LossScaler below)."""
    mult = multiply_factor(state["loss_scale"], sample_size)
    g = grad16.to(F64) * mult
    gnorm = float(torch.sqrt((g * g).sum()))
    info = {"mult": mult, "gnorm": gnorm, "overflow": not math.isfinite(gnorm)}
    if info["overflow"]:
        return dict(state), info
    clip = hp["clip_norm"]
    coef = clip / gnorm if (clip > 0 and gnorm > clip) else 1.0
    g = g * coef
    lr = inverse_sqrt_lr(state["updates"], hp)
    t = state["updates"] + 1
    b1, b2 = hp["betas"]
    step_size = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    p, m, v = adam_update(state["master"].to(F64), state["exp_avg"].to(F64), state["exp_avg_sq"].to(F64), g,
                          lr, step_size, b1, b2, hp["eps"], hp["weight_decay"])
    info.update(clip_coef=coef, lr=lr, step_size=step_size, g=g)
    return {"master": p, "exp_avg": m, "exp_avg_sq": v, "updates": t, "loss_scale": state["loss_scale"]}, info


class LossScaler:
    """DynamicLossScaler (tolerance 0, no threshold).  step(overflow) is one iteration; at the minimum
    scale it keeps the scale, turns ``fatal`` and raises FloatingPointError."""

    def __init__(self, init_scale, scale_window, min_loss_scale=1e-4):
        self.scale, self.window, self.min_scale = float(init_scale), int(scale_window), float(min_loss_scale)
        self.it, self.last_overflow, self.fatal = 0, -1, False

    def step(self, overflow):
        it = self.it
        self.it += 1
        if not overflow:
            if (it - self.last_overflow) % self.window == 0:
                self.scale *= 2.0
            return
        self.last_overflow = it
        if self.scale / 2.0 <= self.min_scale:
            self.fatal = True
            raise FloatingPointError(f"Minimum loss scale reached ({self.min_scale})")
        self.scale /= 2.0


# a 60-iteration script of overflowing iterations: isolated (3, 20), back to back (10-12, 40-41), and, for
# each of the windows 1, 2, 3 and 5, one right after a growth (1: every clean iteration grows; 2: 26 after
# 25; 3: 30 after 29; 5: 48 after 47)
OVERFLOW_ITS = frozenset({3, 10, 11, 12, 20, 26, 30, 40, 41, 48})


def ref_grad_norm_check(norms):
    """True when the ranks' norms are inconsistent: all finite and max|n_r - n_0| / (n_0 + 1e-6) >= 1e-6,
    every operation in fp32 (one rounding each), as on the device."""
    n = np.asarray(norms, dtype=np.float32)
    if not np.all(np.isfinite(n)):
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        dmax = np.float32(0.0)
        for x in n:
            dmax = np.maximum(dmax, np.abs(np.float32(x - n[0])))
        return bool(np.float32(dmax / np.float32(n[0] + np.float32(1e-6))) >= np.float32(1e-6))


def gnorm_bound(n, nparts):
    """Relative error bound of the device grad norm: each of the nparts * 256 threads keeps a running fp32
    sum of k = ceil(n / (nparts * 256)) + 8 non-negative terms (a 16-B load is 8 of them), the squares and
    the 8 levels of the wave / block reduction add 8 more roundings, the square root halves the relative
    error of the sum, and the fp32 cast, the square root and the multiply add one rounding each."""
    k = -(-n // (nparts * 256)) + 8
    return (k + 8) / 2 * U32 + 3 * U32


# ------------------------------------------------------------------------------------------------
# the inputs of the element-math tests and of the fp32 yardstick (one definition for both)
# ------------------------------------------------------------------------------------------------

CASE_N = 1_000_003            # elements of the base case; a test of n elements takes the first n
CASE_BETAS = (f32r(0.9), f32r(0.98))
CASE_EPS = f32r(1e-8)
CASE_WDS = (0.0, f32r(0.01))
CASE_STEPS = (1, 3)
_cases = {}


def adam_case(step):
    """The element-math case of Adam step ``step`` (1: m = v = 0; 3: a state two updates in): fp32 master,
    m, v, fp16 grad of CASE_N elements, and the fp32 scalars of the device state vector (every one
    exactly representable in fp32, so the fp32 and the fp64 run start from the same numbers)."""
    if step in _cases:
        return _cases[step]
    gen = torch.Generator().manual_seed(100 + step)
    n = CASE_N
    loss_scale, sample_size = 128.0, 1000.0
    c = {"step": step, "p": torch.randn(n, generator=gen) * 0.05,
         "g16": (torch.randn(n, generator=gen) * 3e-3 * loss_scale * sample_size).half()}
    if step == 1:
        c["m"], c["v"] = torch.zeros(n), torch.zeros(n)
    else:
        c["m"] = torch.randn(n, generator=gen) * 2e-3
        c["v"] = (torch.randn(n, generator=gen) * 3e-3) ** 2 * 0.04 + 1e-9
    b1, b2 = CASE_BETAS
    lr = f32r(1e-7 + (step - 1) * (1e-3 - 1e-7) / 3)
    c["mult"] = f32r(1.0 / np.float32(loss_scale * sample_size))
    c["clip_coef"] = f32r(0.8)
    c["lr"] = lr
    c["step_size"] = f32r(lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step))
    _cases[step] = c
    return c


def adam_case_run(case, wd, dtype):
    """The case's update in ``dtype`` (fp32: what a correct fp32 implementation gives; fp64: the
    reference), the gradient scaled as on the device: fp16 -> dtype, times (mult * clip_coef).
    -> (p, m, v, p before the update)."""
    b1, b2 = CASE_BETAS
    c = lambda x: torch.tensor(x, dtype=dtype)
    g = case["g16"].to(dtype) * (c(case["mult"]) * c(case["clip_coef"]))
    p0 = case["p"].to(dtype)
    p, m, v = adam_update(p0, case["m"].to(dtype), case["v"].to(dtype), g, case["lr"], case["step_size"],
                          b1, b2, CASE_EPS, wd)
    return p, m, v, p0


def max_rel(x, ref, denom):
    """max over elements of |x - ref| / denom in fp64; 0 / 0 counts as 0."""
    err = (x.to(F64) - ref.to(F64)).abs()
    d = denom.to(F64)
    r = torch.where(err == 0, torch.zeros_like(err), err / d)
    return float(r.max()) if r.numel() else 0.0


def rel_errors(p, m, v, ref):
    """Elementwise errors against ref = (p64, m64, v64, p0): p relative to |p64| + |p64 - p0|, m and v
    relative to their own magnitude."""
    p64, m64, v64, p0 = ref
    return {"p": max_rel(p, p64, p64.abs() + (p64 - p0).abs()), "m": max_rel(m, m64, m64.abs()),
            "v": max_rel(v, v64, v64.abs())}


_e32 = {}


def measure_e32():
    """The fp32 yardstick: {"p", "m", "v"} -> the largest elementwise error of the fp32 CPU run of every
    element-math case (CASE_STEPS x CASE_WDS, CASE_N elements each) against its fp64 run."""
    if not _e32:
        worst = {"p": 0.0, "m": 0.0, "v": 0.0}
        for step in CASE_STEPS:
            for wd in CASE_WDS:
                case = adam_case(step)
                p, m, v, _ = adam_case_run(case, wd, torch.float32)
                e = rel_errors(p, m, v, adam_case_run(case, wd, F64))
                worst = {k: max(worst[k], e[k]) for k in worst}
        _e32.update(worst)
    return dict(_e32)


# norms for the cross-rank check, chosen in fp32 so that the relative difference is far from the 1e-6
# threshold (tests/test_optim_ref.py verifies that): name -> (norms, expected flag)
_N0 = np.float32(3.0)
NORM_CHECK_CASES = {
    "equal": ([_N0, _N0, _N0], False),
    "below": ([_N0, np.float32(_N0 * np.float32(1 + 0.5e-6))], False),
    "above": ([_N0, np.float32(_N0 * np.float32(1 + 2e-6))], True),
    "above_last_of_4": ([_N0, _N0, _N0, np.float32(_N0 * np.float32(1 - 2e-6))], True),
    "inf": ([_N0, np.float32("inf")], False),
    "nan_first": ([np.float32("nan"), _N0], False),
    "neg_inf_and_far": ([_N0, np.float32(7.0), np.float32("-inf")], False),
}

"""GPU: device-resident FP16Optimizer/Adam/DynamicLossScaler/inverse_sqrt (optim.py + loss_optim.hip)
against the oracle restatement of fairseq's (oracle/ref_model.py: fp16_optimizer_step,
DynamicLossScaler, inverse_sqrt_lr) over several updates, and every kernel path and state transition of
the optimizer step against the fp64 restatement of tests/optim_ref.py.

All comparisons of parameters and moments are elementwise (a maximum over elements, never a norm ratio).

The element-math tolerance is defined from the fp32 yardstick E32 (tests/test_optim_ref.py measures it: the
Adam update of the element-math cases done in fp32 on the CPU against fp64, master relative to |p| + |dp|,
the moments relative to their own magnitude), not from the kernels:

    E32[master]     = 4.57e-07
    E32[exp_avg]    = 1.53e-03
    E32[exp_avg_sq] = 2.29e-07

The kernels must stay within 4 x E32 (FMA contraction, the device's division and square root).  exp_avg =
b1 m + (1 - b1) g cancels where its terms have opposite signs, which is why its figure is large; it is
also held to 6 roundings of its two terms, which does not depend on the cancellation.  The grad norm is
held to the derived bound optim_ref.gnorm_bound.  fp16 parameters are exactly master.half()."""
import math

import numpy as np
import pytest
import torch

import optim_ref as O
from conftest import pkg
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

GUARD = 64
S16, S32 = 123.0, -7.5      # sentinels of the guard elements (fp16 / fp32 buffers)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mm = pkg()
    return mm, mm.kernels, torch.device("cuda")


class _Params:
    def __init__(self, n, dev):
        g = torch.Generator().manual_seed(0)
        self.flat = (torch.randn(n, generator=g) * 0.05).half().to(dev)
        self.grad = torch.zeros(n, dtype=torch.float16, device=dev)


def _guarded(n, dtype, dev, fill, a=GUARD):
    """(buffer, view [a:a+n]) with the elements on both sides of the view set to ``fill``."""
    buf = torch.full((a + n + GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[a:a + n]


def _guards_intact(buf, n, fill, a=GUARD):
    f = torch.tensor(fill, dtype=buf.dtype, device=buf.device)
    return bool((buf[:a] == f).all()) and bool((buf[a + n:] == f).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _ost(K, dev, **kw):
    o = torch.zeros(K.OST_SIZE, dtype=torch.float32)
    o[K.OST_LOSS_SCALE], o[K.OST_LAST_OVERFLOW], o[K.OST_CLIP_COEF] = 128.0, -1.0, 1.0
    for k, v in kw.items():
        o[getattr(K, "OST_" + k)] = v
    return o.to(dev)


def _f32(x):
    return np.float32(x)


# ------------------------------------------------------------------------------------------------
# the 7-step run against the oracle, and the cross-rank FATAL case
# ------------------------------------------------------------------------------------------------

def _state(opt):
    return {"master": opt.master.cpu(), "exp_avg": opt.exp_avg.cpu(), "exp_avg_sq": opt.exp_avg_sq.cpu()}


def _check_one_step(before, after, g16, sample_size, loss_scale, updates, hp, tag):
    """One device step against optim_ref.ref_step started from the device's own state before it, element
    by element.  ``hp`` holds the fp32 values the kernels received.  The bounds are a priori (u = 2^-24):

      g     the device's unscaled gradient carries dg = 4u (the multiply factor: a product and a division;
            two more products), a clipped one gnorm_bound + 6u (the norm's error and a division on top)
      m     4 roundings of its two terms, plus dg on the gradient term
      v     4 roundings of itself, plus 2.5 dg on the gradient term
      p     4 roundings of |p| + |dp|; dp (decay + Adam) to rel = 2e-6 + 2 dg (lr to 1e-6, asserted by the
            caller; step size, sqrt(v), the division and the products below 1e-6 + 2 dg); m's bound
            carried through step_size / (sqrt(v) + eps)

    -> (reference state, info)."""
    u = O.U32
    n = g16.numel()
    st = {k: v.double() for k, v in before.items()}
    st.update(updates=updates, loss_scale=loss_scale)
    new, info = O.ref_step(st, g16, sample_size, hp)
    if info["overflow"]:
        for k in before:
            assert _same_bits(before[k], after[k]), (tag, k, "changed by a skipped step")
        return new, info
    b1, b2 = hp["betas"]
    dg = 4 * u if info["clip_coef"] == 1.0 else O.gnorm_bound(n, 1024) + 6 * u
    g = info["g"].abs()
    p0, m0 = st["master"].abs(), st["exp_avg"].abs()
    tol_m = 4 * u * (b1 * m0 + (1 - b1) * g) + dg * (1 - b1) * g
    tol_v = 4 * u * new["exp_avg_sq"] + 2.5 * dg * (1 - b2) * g * g
    denom = new["exp_avg_sq"].sqrt() + hp["eps"]
    dp = hp["weight_decay"] * info["lr"] * p0 + info["step_size"] * new["exp_avg"].abs() / denom
    tol_p = 4 * u * (p0 + dp) + (2e-6 + 2 * dg) * dp + info["step_size"] * tol_m / denom
    for k, tol in (("master", tol_p), ("exp_avg", tol_m), ("exp_avg_sq", tol_v)):
        err = (after[k].double() - new[k]).abs()
        worst = O.max_rel(after[k], new[k], tol)
        assert bool((err <= tol).all()), (tag, k, f"error / bound = {worst:.3g}")
    return new, info


def _hp32(lr, warmup_updates, warmup_init_lr, betas, eps, wd, clip):
    return dict(lr=O.f32r(lr), warmup_updates=warmup_updates, warmup_init_lr=O.f32r(warmup_init_lr),
                betas=(O.f32r(betas[0]), O.f32r(betas[1])), eps=O.f32r(eps), weight_decay=O.f32r(wd),
                clip_norm=O.f32r(clip))


@pytest.mark.parametrize("clip", [10.0, 0.05])
def test_fp16_adam_matches_fairseq_restatement(clip):
    """7 updates at n = 1_000_003 against the oracle's fp32 chain (norm-wise, as before) and, step by
    step and element by element, against the fp64 reference: master, exp_avg and exp_avg_sq; the fp16
    parameters are master.half() bit for bit."""
    mm, K, dev = _gpu()
    n = 1_000_003
    P = _Params(n, dev)
    kw = dict(lr=1e-3, betas=(0.9, 0.98), clip_norm=clip, init_scale=128.0, scale_window=2,
              warmup_updates=3, warmup_init_lr=1e-7)
    opt = mm.optim.FP16Adam(P, **kw)
    hp = _hp32(1e-3, 3, 1e-7, (0.9, 0.98), 1e-8, 0.0, clip)
    master = P.flat.float().cpu()
    ea, eas = torch.zeros(n), torch.zeros(n)
    scaler = R.DynamicLossScaler(128.0, scale_window=2)
    done = 0
    gen = torch.Generator().manual_seed(1)
    for it in range(7):
        ss = 1000.0 + 17 * it
        g = (torch.randn(n, generator=gen) * 3e-3 * scaler.loss_scale * ss / 1000).half()
        if it == 2:
            g[12345] = float("inf")  # fp16 overflow in backward
        P.grad.copy_(g.to(dev))
        before, ls = _state(opt), scaler.loss_scale
        opt.step(torch.tensor([ss], device=dev))
        st = opt.stats()
        lr = R.inverse_sqrt_lr(done, 1e-3, 3, 1e-7)
        norm, overflow = R.fp16_optimizer_step([master], [g], [(ea, eas)], done + 1, lr,
                                               1.0 / (scaler.loss_scale * ss), clip_norm=clip)
        assert st["overflow"] == overflow, it
        if not overflow:
            assert abs(st["lr"] - lr) <= 1e-6 * lr
        _, info = _check_one_step(before, _state(opt), g, ss, ls, done, hp, it)
        assert info["overflow"] == overflow
        if overflow:
            scaler.overflow()
        else:
            done += 1
            scaler.update()
            assert abs(st["gnorm"] - norm) <= 1e-4 * norm, (it, st["gnorm"], norm)
            assert abs(st["gnorm"] - info["gnorm"]) <= O.gnorm_bound(n, 1024) * info["gnorm"], it
        assert st["loss_scale"] == scaler.loss_scale, (it, st["loss_scale"], scaler.loss_scale)
        assert st["step"] == done
        m = opt.master.cpu()
        err = ((m - master).norm() / master.norm()).item()
        assert err < 1e-5, (it, err)
        assert _same_bits(P.flat, m.half()), it
        assert torch.allclose(P.flat.cpu().float(), master.half().float(), rtol=1e-3, atol=1e-7), it


def test_fatal_state_is_sticky():
    """an inconsistent grad norm across ranks (Trainer._check_grad_norms) in a step the
    host does not read makes the device state FATAL for good: that step and every later one apply
    no update, and the next host check raises FloatingPointError (on every rank: the state vector
    is identical on all of them)."""
    mm, K, dev = _gpu()
    P = _Params(4096, dev)
    opt = mm.optim.FP16Adam(P, lr=1e-3, warmup_updates=0, init_scale=1.0)
    ss = torch.tensor([100.0], device=dev)
    P.grad.fill_(0.01)
    opt.step(ss)
    st = opt.check_fatal()
    assert st["step"] == 1
    assert abs(st["lr"] - 1e-3) <= 1e-6 * 1e-3      # no warmup: lr_peak at 0 completed updates
    m0 = opt.master.clone()
    buf = torch.tensor([1.0, 2.0], device=dev)      # two ranks' norms that disagree
    opt.step(ss, check=lambda ost: K.grad_norm_check(buf, 2, 0, ost, 1))
    opt.step(ss)                                    # a clean step later: still no update
    torch.cuda.synchronize()
    assert torch.equal(opt.master, m0)
    st = opt.stats()
    assert st["inconsistent"] and st["fatal"] and st["step"] == 1
    with pytest.raises(FloatingPointError, match="inconsistent"):
        opt.check_fatal()


# ------------------------------------------------------------------------------------------------
# K.adam: element math, guards, alignment, grid stride, skip paths
# ------------------------------------------------------------------------------------------------

_refs = {}


def _case_ref(step, wd):
    """fp64 reference (p, m, v, p0) of the whole element-math case, computed once."""
    if (step, wd) not in _refs:
        _refs[step, wd] = O.adam_case_run(O.adam_case(step), wd, O.F64)
    return _refs[step, wd]


def _case_ost(K, dev, case):
    return _ost(K, dev, MULT=case["mult"], CLIP_COEF=case["clip_coef"], LR=case["lr"], STEP_SIZE=case["step_size"],
                STEP=case["step"])


def _m_terms_bound(case, sl):
    """6 roundings of the two terms of exp_avg (see the module docstring)."""
    b1 = O.CASE_BETAS[0]
    g = case["g16"][sl].double().abs() * (case["mult"] * case["clip_coef"])
    return 6 * O.U32 * (b1 * case["m"][sl].double().abs() + (1 - b1) * g)


ADAM_SIZES = [1, 7, 8, 9, 2047, 2048, 8 * 256 * 3 + 5]


@pytest.mark.parametrize("step", O.CASE_STEPS)
@pytest.mark.parametrize("wd", O.CASE_WDS, ids=["wd0", "wd0.01"])
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_element_math(n, wd, step):
    """K.adam on a hand-filled state vector: master, exp_avg and exp_avg_sq within 4 x E32 of fp64 element
    by element, param == master.half() exactly, grad untouched, and nothing written outside [a, a + n)."""
    mm, K, dev = _gpu()
    e32 = O.measure_e32()
    case, ref = O.adam_case(step), _case_ref(step, wd)
    sl = slice(0, n)
    pb, p = _guarded(n, torch.float16, dev, S16)
    gb, g = _guarded(n, torch.float16, dev, S16)
    mb, master = _guarded(n, torch.float32, dev, S32)
    eb, ea = _guarded(n, torch.float32, dev, S32)
    sb, eas = _guarded(n, torch.float32, dev, S32)
    p.copy_(case["p"][sl].half())
    g.copy_(case["g16"][sl])
    master.copy_(case["p"][sl])
    ea.copy_(case["m"][sl])
    eas.copy_(case["v"][sl])
    g_before = gb.clone()
    b1, b2 = O.CASE_BETAS
    K.adam(p, g, master, ea, eas, _case_ost(K, dev, case), b1, b2, O.CASE_EPS, wd)
    torch.cuda.synchronize()
    out_p, out_m, out_v = master.cpu(), ea.cpu(), eas.cpu()
    e = O.rel_errors(out_p, out_m, out_v, tuple(t[sl] for t in ref))
    print(f"adam n={n} wd={wd:g} step={step}: " + "  ".join(f"{k} {e[k]:.2e} (4 x E32 = {4 * e32[k]:.2e})" for k in e))
    for k in e:
        assert e[k] <= 4 * e32[k], (k, e[k], 4 * e32[k])
    assert bool(((out_m.double() - ref[1][sl]).abs() <= _m_terms_bound(case, sl)).all())
    assert _same_bits(p, out_p.half())
    assert _same_bits(gb, g_before)
    assert _guards_intact(pb, n, S16) and _guards_intact(mb, n, S32)
    assert _guards_intact(eb, n, S32) and _guards_intact(sb, n, S32)


def test_adam_rejects_a_misaligned_view():
    """A view starting at element 4 is 8-byte but not 16-byte aligned in the fp16 buffers: refused by the
    library before any launch, nothing written."""
    mm, K, dev = _gpu()
    n, a = 16, 4
    case = O.adam_case(3)
    bufs = [_guarded(n, dt, dev, f, a=a) for dt, f in ((torch.float16, S16), (torch.float16, S16),
                                                        (torch.float32, S32), (torch.float32, S32), (torch.float32, S32))]
    for (_, view), src in zip(bufs, (case["p"], case["g16"], case["p"], case["m"], case["v"])):
        view.copy_(src[:n])
    assert bufs[0][1].data_ptr() % 16 == 8 and bufs[0][1].data_ptr() % 8 == 0
    before = [b.clone() for b, _ in bufs]
    with pytest.raises(mm._lib.HipError, match="16-B aligned"):
        K.adam(*(v for _, v in bufs), _case_ost(K, dev, case), *O.CASE_BETAS, O.CASE_EPS, 0.0)
    torch.cuda.synchronize()
    for (b, _), b0 in zip(bufs, before):
        assert _same_bits(b, b0)


def test_adam_grid_stride():
    """n = 16_777_216 + 8 * 1000 + 5: more than the 8192-block cap covers in one pass, so threads stride,
    and a scalar tail.  The inputs repeat the element-math case with its period of 1_000_003 elements (odd:
    no power-of-two stride maps an element onto a copy of itself), so every element is one E32 was measured
    on and the fp64 reference is that case's.  The result is also bit-identical to the same update issued as
    three 8-aligned slices (the deferred-chunk shape)."""
    mm, K, dev = _gpu()
    e32 = O.measure_e32()
    n, step, wd = 16_777_216 + 8 * 1000 + 5, 3, O.CASE_WDS[1]
    case = O.adam_case(step)
    idx = torch.arange(n, device=dev) % O.CASE_N
    master0, m0, v0, g = (case[k].to(dev)[idx] for k in ("p", "m", "v", "g16"))
    p0 = master0.half()
    ost = _case_ost(K, dev, case)
    b1, b2 = O.CASE_BETAS
    one = [p0.clone(), g, master0.clone(), m0.clone(), v0.clone()]
    K.adam(*one, ost, b1, b2, O.CASE_EPS, wd)
    cuts = [0, 8 * 700_001, 8 * 1_500_000, n]
    three = [p0.clone(), g, master0.clone(), m0.clone(), v0.clone()]
    for a, b in zip(cuts, cuts[1:]):
        K.adam(*(t[a:b] for t in three), ost, b1, b2, O.CASE_EPS, wd)
    torch.cuda.synchronize()
    assert torch.equal(g, case["g16"].to(dev)[idx])
    ref = tuple(t.to(dev)[idx] for t in _case_ref(step, wd))
    e = O.rel_errors(one[2], one[3], one[4], ref)
    print("adam grid stride: " + "  ".join(f"{k} {e[k]:.2e} (4 x E32 = {4 * e32[k]:.2e})" for k in e))
    for k in e:
        assert e[k] <= 4 * e32[k], (k, e[k], 4 * e32[k])
    assert torch.equal(_bits(one[0]), _bits(one[2].half()))
    for x, y, name in zip(one, three, ("param", "grad", "master", "exp_avg", "exp_avg_sq")):
        assert torch.equal(_bits(x), _bits(y)), name


@pytest.mark.parametrize("flag", ["OVERFLOW", "INCONSISTENT", "FATAL"])
def test_adam_skips_on_flag(flag):
    mm, K, dev = _gpu()
    n = 2053
    case = O.adam_case(3)
    bufs = [case["p"][:n].half().to(dev), case["g16"][:n].to(dev), case["p"][:n].to(dev), case["m"][:n].to(dev),
            case["v"][:n].to(dev)]
    before = [b.clone() for b in bufs]
    ost = _case_ost(K, dev, case)
    ost[getattr(K, "OST_" + flag)] = 1.0
    K.adam(*bufs, ost, *O.CASE_BETAS, O.CASE_EPS, O.CASE_WDS[1])
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert _same_bits(b, b0)


# ------------------------------------------------------------------------------------------------
# K.grad_norm: the unrolled loop, the strided remainder, the scalar tail; overflow in every region
# ------------------------------------------------------------------------------------------------

GNORM_SIZES = [1, 7, 8, 9, 6143, 6144 * 8 // 8 + 8, 8 * 256 * 13 + 3]
GNORM_PARTS = [1, 3, 1024]


def _regions(n, nparts):
    """name -> an element index inside each region of grad_sqnorm_kernel that (n, nparts) has: the 4x-unrolled
    loop (a vector of a thread's third load, where there is one), the strided remainder, the scalar tail."""
    n8, S = n // 8, nparts * 256
    unrolled, rest = [], []
    for j in range(n8):
        first = j % S + (j // S // 4) * 4 * S          # the vector that thread's unrolled iteration starts at
        (unrolled if first + 3 * S < n8 else rest).append(j)
    r = {"first": 0, "last": n - 1}
    if unrolled:
        third = [j for j in unrolled if (j // S) % 4 == 2]
        r["unrolled"] = third[len(third) // 2] * 8 + 5
        r["unrolled_4th"] = [j for j in unrolled if (j // S) % 4 == 3][-1] * 8 + 7
    if rest:
        r["remainder"] = rest[len(rest) // 2] * 8 + 3
    if n % 8:
        r["tail"] = n8 * 8 + (n % 8) // 2
    return r


def test_grad_norm_regions_are_covered():
    """The sizes reach every loop of the kernel, alone and together (nparts = 1 and 3 put them on both sides
    of n/8 > 3 * nparts * 256)."""
    has = lambda n, parts: set(_regions(n, parts)) - {"first", "last"}
    assert has(7, 1) == {"tail"} and has(8, 1) == {"remainder"} and has(9, 3) == {"remainder", "tail"}
    assert has(6143, 1) == {"remainder", "tail"}                      # n/8 = 767 < 768: no unrolled iteration
    assert has(6152, 1) == {"unrolled", "unrolled_4th", "remainder"}    # n/8 = 769: thread 0 unrolls once
    assert has(26627, 1) == has(26627, 3) == {"unrolled", "unrolled_4th", "remainder", "tail"}
    assert has(6152, 3) == {"remainder"} and has(26627, 1024) == {"remainder", "tail"}


def _run_grad_norm(K, g, ss, nparts, dev):
    ost = _ost(K, dev, LOSS_SCALE=64.0, GNORM=-1.0, OVERFLOW=-1.0)
    K.grad_norm(g, ost, None if ss is None else torch.tensor([ss], device=dev), nparts)
    return ost


def _expected_mult(ss):
    ss = 1.0 if ss is None else max(ss, 1.0)
    return _f32(1.0) / (_f32(64.0) * _f32(ss))


def _assert_gnorm(o, K, g64, ss, n, nparts, tag):
    mult = _expected_mult(ss)
    assert float(o[K.OST_MULT]) == float(mult), (tag, float(o[K.OST_MULT]), float(mult))
    want = math.sqrt(float((g64 * g64).sum())) * float(mult)
    rel = abs(float(o[K.OST_GNORM]) - want) / want
    assert rel <= O.gnorm_bound(n, nparts), (tag, rel, O.gnorm_bound(n, nparts))
    assert float(o[K.OST_OVERFLOW]) == 0.0, tag
    return rel


@pytest.mark.parametrize("nparts", GNORM_PARTS)
@pytest.mark.parametrize("n", GNORM_SIZES)
def test_grad_norm_value(n, nparts):
    """ost[GNORM] = fp64 norm x multiplier within the derived bound, ost[MULT] exact, for sample_size given,
    below 1, None and 0.  The elements around the view hold inf: reading one would show as an overflow."""
    mm, K, dev = _gpu()
    gen = torch.Generator().manual_seed(n * 7 + nparts)
    g16 = (torch.randn(n, generator=gen) * 100).half()
    g16[g16 == 0] = 1.0
    buf, g = _guarded(n, torch.float16, dev, float("inf"))
    g.copy_(g16)
    variants = [1017.0, None, 0.0, 0.5]
    osts = torch.stack([_run_grad_norm(K, g, ss, nparts, dev) for ss in variants]).cpu()
    worst = max(_assert_gnorm(o, K, g16.double(), ss, n, nparts, ss) for o, ss in zip(osts, variants))
    print(f"grad_norm n={n} nparts={nparts}: rel {worst:.2e} (bound {O.gnorm_bound(n, nparts):.2e})")
    assert _expected_mult(None) == _expected_mult(0.0) == _expected_mult(0.5) == _f32(1 / 64.0)


@pytest.mark.parametrize("nparts", GNORM_PARTS)
@pytest.mark.parametrize("n", GNORM_SIZES)
def test_grad_norm_overflow_in_every_region(n, nparts):
    """inf, -inf and nan planted at element 0, inside the unrolled region, inside the remainder, in the
    scalar tail and at the last element each set OVERFLOW; a buffer of 65504 everywhere does not."""
    mm, K, dev = _gpu()
    g = torch.empty(n, dtype=torch.float16, device=dev)
    runs = []
    for name, pos in _regions(n, nparts).items():
        for val in (float("inf"), float("-inf"), float("nan")):
            g.fill_(0.25)
            g[pos] = val
            runs.append(((name, pos, val), _run_grad_norm(K, g, 1017.0, nparts, dev)))
    g.fill_(65504.0)
    top = _run_grad_norm(K, g, 1017.0, nparts, dev).cpu()
    for tag, ost in runs:
        assert float(ost[K.OST_OVERFLOW]) == 1.0, tag
    _assert_gnorm(top, K, torch.full((n,), 65504.0, dtype=O.F64), 1017.0, n, nparts, "fp16 max")


# ------------------------------------------------------------------------------------------------
# FP16Adam.step: the loss-scale state machine, clipping and the schedule over 60 iterations
# ------------------------------------------------------------------------------------------------

SCHEDULES = [  # scale_window, warmup_updates, clip_norm, weight_decay
    (1, 0, 0.0, 0.0), (2, 1, 0.05, 0.01), (3, 3, 10.0, 0.0), (5, 0, 0.05, 0.01),
    (2, 3, 0.0, 0.01), (1, 1, 10.0, 0.0), (3, 0, 10.0, 0.01), (5, 1, 0.0, 0.0)]


@pytest.mark.parametrize("window,warmup,clip,wd", SCHEDULES)
def test_step_state_machine(window, warmup, clip, wd):
    """60 iterations of FP16Adam.step at n = 64 under optim_ref.OVERFLOW_ITS (isolated and back-to-back
    overflows, one right after a growth), compared with optim_ref after every step: overflow, loss scale and
    step count exact, lr to 1e-6, gnorm to its bound, master / exp_avg / exp_avg_sq element by element
    (bit-unchanged when the step is skipped), the clip coefficient (exactly 1 with clip = 0)."""
    mm, K, dev = _gpu()
    n = 64
    P = _Params(n, dev)
    hp = _hp32(1e-3, warmup, 1e-7, (0.9, 0.98), 1e-8, wd, clip)
    opt = mm.optim.FP16Adam(P, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"],
                            clip_norm=hp["clip_norm"], init_scale=128.0, scale_window=window,
                            warmup_updates=warmup, warmup_init_lr=hp["warmup_init_lr"])
    scaler = O.LossScaler(128.0, window)
    gen = torch.Generator().manual_seed(window * 100 + warmup)
    amps = (1e-4, 3e-3, 0.5, 3.0)           # true gradient norms of about 8e-4, 0.024, 4 and 24
    sizes = (4.0, None, 7.0, 0.0, 5.0)      # sample sizes; None and 0 leave the factor at 1 / loss_scale
    done, clipped, unclipped, top_norm = 0, 0, 0, 0.0
    for it in range(60):
        ls, ss = scaler.scale, sizes[it % len(sizes)]
        # what backward leaves under this loss scale (summed over ss samples), saturating short of fp16's
        # maximum so that only the scripted iterations overflow
        g16 = (torch.randn(n, generator=gen) * amps[(it + it // 4) % 4] * ls * max(ss or 1.0, 1.0)).clamp(-6e4, 6e4).half()
        if it in O.OVERFLOW_ITS:
            g16[(0, n - 1, 17)[it % 3]] = (float("inf"), float("nan"))[it % 2]
        P.grad.copy_(g16.to(dev))
        before = _state(opt)
        opt.step(None if ss is None else torch.tensor([ss], device=dev))
        st, o = opt.stats(), opt.ost.cpu()
        _, info = _check_one_step(before, _state(opt), g16, ss, ls, done, hp, it)
        assert info["overflow"] == (it in O.OVERFLOW_ITS)
        assert st["overflow"] == info["overflow"], it
        scaler.step(info["overflow"])
        assert float(o[K.OST_MULT]) == float(_f32(1.0) / (_f32(ls) * _f32(max(ss or 1.0, 1.0)))), it
        if not info["overflow"]:
            done += 1
            assert abs(st["lr"] - info["lr"]) <= 1e-6 * info["lr"], (it, st["lr"], info["lr"])
            gb = O.gnorm_bound(n, 1024)
            assert abs(st["gnorm"] - info["gnorm"]) <= gb * info["gnorm"], (it, st["gnorm"], info["gnorm"])
            coef = float(o[K.OST_CLIP_COEF])
            top_norm = max(top_norm, st["gnorm"])
            if info["clip_coef"] == 1.0:
                assert coef == 1.0, (it, coef)
                unclipped += 1
            else:
                assert abs(coef - info["clip_coef"]) <= (gb + 2 * O.U32) * info["clip_coef"], (it, coef)
                clipped += 1
        assert st["loss_scale"] == scaler.scale, (it, st["loss_scale"], scaler.scale)
        assert st["step"] == done and not st["fatal"] and not st["inconsistent"], it
        assert _same_bits(P.flat, opt.master.cpu().half()), it
    assert done == 60 - len(O.OVERFLOW_ITS) and unclipped > 0
    assert top_norm > 10.0, "no step with a norm above 10"
    assert (clipped == 0) if clip == 0 else (clipped > 0)


def test_minimum_loss_scale_is_fatal():
    """init 1.0, minimum 0.25: an overflow halves to 0.5; the next one would reach 0.25 <= 0.25, so the
    scale stays 0.5 and the state turns FATAL for good: a clean step updates nothing and does not count."""
    mm, K, dev = _gpu()
    n = 64
    P = _Params(n, dev)
    opt = mm.optim.FP16Adam(P, lr=1e-3, warmup_updates=0, init_scale=1.0, min_loss_scale=0.25, scale_window=2)
    ss = torch.tensor([10.0], device=dev)
    clean = torch.full((n,), 0.01, dtype=torch.float16, device=dev)
    bad = clean.clone()
    bad[n - 1] = float("inf")
    P.grad.copy_(clean)
    opt.step(ss)
    st = opt.check_fatal()
    assert st["step"] == 1 and st["loss_scale"] == 1.0 and not st["overflow"]
    state0, p0 = _state(opt), P.flat.clone()
    P.grad.copy_(bad)
    opt.step(ss)
    st = opt.check_fatal()
    assert st["overflow"] and st["loss_scale"] == 0.5 and not st["fatal"] and st["step"] == 1
    opt.step(ss)
    st = opt.stats()
    assert st["overflow"] and st["loss_scale"] == 0.5 and st["fatal"] and st["step"] == 1
    with pytest.raises(FloatingPointError, match="Minimum loss scale"):
        opt.check_fatal()
    for grad in (clean, bad, clean):
        P.grad.copy_(grad)
        opt.step(ss)
        st = opt.stats()
        assert st["fatal"] and st["loss_scale"] == 0.5 and st["step"] == 1 and not st["inconsistent"]
        with pytest.raises(FloatingPointError, match="Minimum loss scale"):
            opt.check_fatal()
    for k, v in _state(opt).items():
        assert _same_bits(v, state0[k]), k
    assert _same_bits(P.flat, p0)


# ------------------------------------------------------------------------------------------------
# K.grad_norm_check
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [1, 2, 8, 70])
def test_grad_norm_check_stage0(world):
    """Stage 0 writes ost[GNORM] into slot ``rank`` and 0 into the other world - 1 slots, nothing else
    (world = 70 strides over the 64 threads)."""
    mm, K, dev = _gpu()
    ost = _ost(K, dev, GNORM=2.5)
    ost0 = ost.clone()
    for rank in sorted({0, world // 2, world - 1, min(65, world - 1)}):
        b, view = _guarded(world, torch.float32, dev, S32)
        K.grad_norm_check(view, world, rank, ost, 0)
        want = torch.zeros(world)
        want[rank] = 2.5
        assert torch.equal(view.cpu(), want), (world, rank)
        assert _guards_intact(b, world, S32)
    assert torch.equal(ost, ost0)


def _flag(K, dev, norms, ost=None):
    ost = _ost(K, dev, GNORM=3.0) if ost is None else ost
    buf = torch.tensor(np.asarray(norms, dtype=np.float32), device=dev)
    before = buf.clone()
    K.grad_norm_check(buf, buf.numel(), 0, ost, 1)
    assert _same_bits(buf, before)
    return float(ost[K.OST_INCONSISTENT]), ost


@pytest.mark.parametrize("name", sorted(O.NORM_CHECK_CASES))
def test_grad_norm_check_stage1(name):
    """Equal norms, a relative difference of 0.5e-6 and any non-finite entry do not flag; 2e-6 does.  The
    expected flag is optim_ref.ref_grad_norm_check's (fp32 arithmetic, unambiguous at these inputs)."""
    mm, K, dev = _gpu()
    norms, expected = O.NORM_CHECK_CASES[name]
    assert O.ref_grad_norm_check(norms) == expected
    flag, ost = _flag(K, dev, norms)
    assert flag == float(expected), (name, flag)
    o = ost.cpu()
    assert float(o[K.OST_FATAL]) == 0.0 and float(o[K.OST_GNORM]) == 3.0


def test_grad_norm_check_is_sticky_and_reads_every_rank():
    mm, K, dev = _gpu()
    same = [np.float32(3.0)] * 70
    off = list(same)
    off[69] = O.NORM_CHECK_CASES["above"][0][1]
    assert not O.ref_grad_norm_check(same) and O.ref_grad_norm_check(off)
    flag, ost = _flag(K, dev, same)
    assert flag == 0.0
    flag, ost = _flag(K, dev, off, ost)
    assert flag == 1.0
    flag, ost = _flag(K, dev, same, ost)          # a consistent step later: the flag stays
    assert flag == 1.0


def test_grad_norm_check_rejects_bad_arguments():
    mm, K, dev = _gpu()
    ost = _ost(K, dev, GNORM=3.0)
    buf = torch.tensor([1.0, 2.0], device=dev)
    for world, rank, stage in ((2, 2, 0), (2, 5, 1), (2, -1, 0), (0, 0, 0), (2, 0, 2), (2, 1, -1)):
        with pytest.raises(mm._lib.HipError, match="grad_norm_check"):
            K.grad_norm_check(buf, world, rank, ost, stage)
    torch.cuda.synchronize()
    assert buf.tolist() == [1.0, 2.0] and float(ost[K.OST_INCONSISTENT]) == 0.0


# ------------------------------------------------------------------------------------------------
# K.scale_f16, K.accum_f16_f32, K.set_f32
# ------------------------------------------------------------------------------------------------

VEC_SIZES = [8, 2048, 8 * 256 * 5 + 8, 8_388_608 + 8 * 77]    # the last one is above the 4096-block cap


def _fp16_inputs(n):
    """n fp16 values: subnormals, the smallest normal, +-65504 and +-inf first, then a walk through every
    non-NaN fp16 bit pattern (31 is coprime to their number, so the large size visits all of them)."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    pat = bits.view(torch.float16)
    pat = pat[~torch.isnan(pat)]
    x = pat[(torch.arange(n) * 31) % pat.numel()].clone()
    x[:8] = torch.tensor([2.0 ** -24, -3 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0,
                          float("inf"), float("-inf")]).half()
    return x


@pytest.mark.parametrize("n", VEC_SIZES)
@pytest.mark.parametrize("alpha", [0.5, 1 / 3, 0.125])
def test_scale_f16_bit_exact(n, alpha):
    """x *= alpha is (x.float() * alpha).half() bit for bit (alpha in fp32, one rounding to fp16, results
    that land in the subnormal range included); nothing outside the view is written."""
    mm, K, dev = _gpu()
    x = _fp16_inputs(n)
    want = (x.float() * torch.tensor(alpha, dtype=torch.float32)).half()
    buf, view = _guarded(n, torch.float16, dev, S16)
    view.copy_(x)
    K.scale_f16(view, alpha)
    assert _same_bits(view, want)
    assert _guards_intact(buf, n, S16)
    if n == 8:
        sub = want[:4].float().abs()
        assert bool((sub < 2.0 ** -14).all()), "the first four results are meant to be subnormal"


@pytest.mark.parametrize("n", VEC_SIZES)
def test_accum_f16_f32_bit_exact(n):
    mm, K, dev = _gpu()
    x = _fp16_inputs(n)
    acc0 = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 10
    want = acc0 + x.float()
    buf, acc = _guarded(n, torch.float32, dev, S32)
    acc.copy_(acc0)
    xd = x.to(dev)
    K.accum_f16_f32(acc, xd)
    assert _same_bits(acc, want)
    assert _same_bits(xd, x)
    assert _guards_intact(buf, n, S32)


def test_scale_and_accum_empty_and_rejections():
    """n = 0 is a no-op; n % 8 != 0 and a view that is not 16-byte aligned are refused before any launch."""
    mm, K, dev = _gpu()
    hb, h = _guarded(32, torch.float16, dev, S16)
    fb, f = _guarded(32, torch.float32, dev, S32)
    h.fill_(1.0)
    f.fill_(2.0)
    h0, f0 = hb.clone(), fb.clone()
    K.scale_f16(h[:0], 0.5)
    K.accum_f16_f32(f[:0], h[:0])
    with pytest.raises(mm._lib.HipError, match="scale_f16"):
        K.scale_f16(h[:12], 0.5)
    with pytest.raises(mm._lib.HipError, match="scale_f16"):
        K.scale_f16(h[4:12], 0.5)
    with pytest.raises(mm._lib.HipError, match="accum_f16_f32"):
        K.accum_f16_f32(f[:12], h[:12])
    with pytest.raises(mm._lib.HipError, match="accum_f16_f32"):
        K.accum_f16_f32(f[:8], h[4:12])
    with pytest.raises(mm._lib.HipError, match="accum_f16_f32"):
        K.accum_f16_f32(f[2:10], h[:8])
    assert h[4:12].data_ptr() % 16 == 8 and f[2:10].data_ptr() % 16 == 8
    torch.cuda.synchronize()
    assert _same_bits(hb, h0) and _same_bits(fb, f0)


def test_set_f32_lengths():
    """Lengths 0..8 write exactly that many values; 9 is refused."""
    mm, K, dev = _gpu()
    vals = [1.5, -2.25, 3.0, 0.0, -0.5, 1e-3, 65504.0, -1.0, 9.0]
    for L in range(9):
        buf, view = _guarded(8, torch.float32, dev, S32)
        view.fill_(S32)
        K.set_f32(view, vals[:L])
        out = buf.cpu()
        want = torch.full_like(out, S32)
        want[GUARD:GUARD + L] = torch.tensor(vals[:L], dtype=torch.float32)
        assert _same_bits(out, want), L
    buf, view = _guarded(16, torch.float32, dev, S32)
    with pytest.raises(mm._lib.HipError, match="set_f32"):
        K.set_f32(view, vals)
    torch.cuda.synchronize()
    assert bool((buf == S32).all())

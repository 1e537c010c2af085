"""CPU: the fp64 optimizer restatement (tests/optim_ref.py) against the oracle's independent fp32
restatement (oracle/ref_model.py), a hand-computed answer, and the fp32 yardstick E32 that the GPU
element-math tolerance of tests/test_gpu_optim.py is defined from."""
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as O
from oracle import ref_model as R

ULP32 = 2.0 ** -23


def _hp(**kw):
    hp = dict(lr=1e-3, warmup_updates=3, warmup_init_lr=1e-7, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.0,
              clip_norm=10.0)
    hp.update(kw)
    return hp


@pytest.mark.parametrize("clip", [10.0, 0.05, 0.0])
def test_ref_step_agrees_with_oracle(clip):
    """wd = 0: one fp64 step from the oracle's fp32 state lands within 4 fp32 ulps of |p| + |dp| of the
    oracle's next state, element by element (the oracle rounds p once and dp a few times); norm, overflow
    and lr agree; an overflowing step changes nothing in either."""
    n = 4099
    gen = torch.Generator().manual_seed(5)
    master = (torch.randn(n, generator=gen) * 0.05).half().float()
    ea, eas = torch.zeros(n), torch.zeros(n)
    hp = _hp(clip_norm=clip)
    done, loss_scale = 0, 128.0
    for it in range(6):
        ss = 1000.0 + 17 * it
        g = (torch.randn(n, generator=gen) * 3e-3 * loss_scale * ss / 1000 * (100.0 if it == 4 else 1.0)).half()
        if it == 2:
            g[n - 1] = float("nan")
        state = {"master": master.double(), "exp_avg": ea.double(), "exp_avg_sq": eas.double(), "updates": done,
                 "loss_scale": loss_scale}
        new, info = O.ref_step(state, g, ss, hp)
        lr = R.inverse_sqrt_lr(done, hp["lr"], hp["warmup_updates"], hp["warmup_init_lr"])
        p0 = master.clone()
        norm, overflow = R.fp16_optimizer_step([master], [g], [(ea, eas)], done + 1, lr, 1.0 / (loss_scale * ss),
                                               clip_norm=clip)
        assert info["overflow"] == overflow == (it == 2)
        if overflow:
            assert new["updates"] == done and torch.equal(new["master"], p0.double())
            assert torch.equal(master, p0)
            continue
        done += 1
        assert new["updates"] == done
        assert abs(info["lr"] - lr) <= 1e-15 * lr
        assert abs(info["gnorm"] - norm) <= 1e-5 * norm, (info["gnorm"], norm)
        assert (info["clip_coef"] < 1.0) == (clip > 0 and norm > clip)
        p64 = new["master"]
        bound = 4 * ULP32 * (p64.abs() + (p64 - p0.double()).abs())
        err = (master.double() - p64).abs()
        assert bool((err <= bound).all()), (it, float((err / bound).max()))
        assert O.max_rel(eas, new["exp_avg_sq"], new["exp_avg_sq"].abs()) <= 4 * ULP32
        m_bound = 4 * ULP32 * (0.9 * state["exp_avg"].abs() + 0.1 * info["g"].abs())
        assert bool(((ea.double() - new["exp_avg"]).abs() <= m_bound).all())


def test_ref_step_known_answer():
    """Three elements, two steps, wd = 0.01, lr = 0.1 (no warmup: lr_peak at 0 and at 1 completed updates),
    b1 = 0.5, b2 = 0.75, eps = 1, loss scale 2, sample size 4 (factor 1/8), clip 5.

    step 1: g = (2, -4, 0), norm sqrt(20) < 5.  p *= 0.999 -> (0.999, -1.998, 0.4995); m = g/2 = (1, -2, 0);
            v = g^2/4 = (1, 4, 0); step size 0.1 sqrt(0.25)/0.5 = 0.1; p -= 0.1 m/(sqrt(v) + 1)
            = (0.999 - 0.05, -1.998 + 0.2/3, 0.4995).
    step 2: raw g = (6, 0, -8), norm 10 > 5: coefficient 0.5, g = (3, 0, -4).  p *= 0.999;
            m = (0.5 + 1.5, -1, -2) = (2, -1, -2); v = (0.75 + 2.25, 3, 4) = (3, 3, 4);
            step size 0.1 sqrt(1 - 0.5625)/0.75 = 0.0881917...; p -= that * m/(sqrt(v) + 1)."""
    hp = dict(lr=0.1, warmup_updates=0, warmup_init_lr=0.0, betas=(0.5, 0.75), eps=1.0, weight_decay=0.01,
              clip_norm=5.0)
    st = {"master": torch.tensor([1.0, -2.0, 0.5], dtype=O.F64), "exp_avg": torch.zeros(3, dtype=O.F64),
          "exp_avg_sq": torch.zeros(3, dtype=O.F64), "updates": 0, "loss_scale": 2.0}
    st, info = O.ref_step(st, torch.tensor([16.0, -32.0, 0.0]).half(), 4.0, hp)
    assert not info["overflow"] and info["clip_coef"] == 1.0 and info["lr"] == 0.1 and info["mult"] == 0.125
    assert abs(info["gnorm"] - 20 ** 0.5) < 1e-14
    assert np.allclose(st["master"].numpy(), [0.949, -1.998 + 0.2 / 3, 0.4995], rtol=0, atol=1e-15)
    assert st["exp_avg"].tolist() == [1.0, -2.0, 0.0] and st["exp_avg_sq"].tolist() == [1.0, 4.0, 0.0]
    st, info = O.ref_step(st, torch.tensor([48.0, 0.0, -64.0]).half(), 4.0, hp)
    assert info["gnorm"] == 10.0 and info["clip_coef"] == 0.5 and info["lr"] == 0.1 and st["updates"] == 2
    assert abs(info["step_size"] - 0.08819171036881969) < 1e-16
    assert st["exp_avg"].tolist() == [2.0, -1.0, -2.0] and st["exp_avg_sq"].tolist() == [3.0, 3.0, 4.0]
    assert np.allclose(st["master"].numpy(), [0.8834901872036249, -1.8971215936018127, 0.5577949735792131],
                       rtol=0, atol=1e-15)


def test_ref_step_multiplier_and_lr_edges():
    assert O.multiply_factor(128.0, None) == O.multiply_factor(128.0, 0.0) == 1 / 128.0
    assert O.multiply_factor(4.0, 0.5) == 0.25 and O.multiply_factor(4.0, 8.0) == 1 / 32.0
    hp = _hp(warmup_updates=0)
    assert [O.inverse_sqrt_lr(k, hp) for k in (0, 1, 4)] == [1e-3, 1e-3, 5e-4]
    hp = _hp(warmup_updates=4)
    assert O.inverse_sqrt_lr(0, hp) == 1e-7 and abs(O.inverse_sqrt_lr(4, hp) - 1e-3) < 1e-18
    assert abs(O.inverse_sqrt_lr(16, hp) - 5e-4) < 1e-18
    for k in range(12):
        for wu in (0, 1, 3):
            assert abs(O.inverse_sqrt_lr(k, _hp(warmup_updates=wu)) - R.inverse_sqrt_lr(k, 1e-3, wu, 1e-7)) < 1e-18


@pytest.mark.parametrize("window", [1, 2, 3, 5])
def test_scaler_agrees_with_oracle(window):
    """The 60-iteration script of optim_ref.OVERFLOW_ITS, which for every window holds an overflow right
    after a growth."""
    a, b = O.LossScaler(128.0, window), R.DynamicLossScaler(128.0, scale_window=window)
    after_growth = 0
    for it in range(60):
        before = a.scale
        if it in O.OVERFLOW_ITS:
            a.step(True)
            b.overflow()
            assert a.scale == before / 2
            after_growth += it > 0 and grew
        else:
            a.step(False)
            b.update()
        grew = a.scale > before
        assert a.scale == b.loss_scale, (it, a.scale, b.loss_scale)
        assert (a.it, a.last_overflow) == (b._iter, b._last_overflow_iter)
    assert after_growth >= 1, "the pattern has no overflow right after a growth for this window"


def test_scaler_raises_at_minimum_scale():
    """init 1.0, minimum 0.25: 1 -> 0.5, then 0.25 <= 0.25: the scale stays 0.5 and both raise."""
    a, b = O.LossScaler(1.0, 2, 0.25), R.DynamicLossScaler(1.0, scale_window=2, min_loss_scale=0.25)
    a.step(True)
    b.overflow()
    assert a.scale == b.loss_scale == 0.5 and not a.fatal
    with pytest.raises(FloatingPointError, match="Minimum loss scale"):
        a.step(True)
    with pytest.raises(FloatingPointError):
        b.overflow()
    assert a.scale == b.loss_scale == 0.5 and a.fatal and a.it == b._iter == 2


def test_grad_norm_check_cases_are_unambiguous():
    """The shared inputs sit far from the threshold (in exact arithmetic the ratio is below 0.9e-6 or
    above 1.1e-6, fp32 rounding moves it by ~1e-13), so the fp32 reference's answer is the true one."""
    for name, (norms, expected) in O.NORM_CHECK_CASES.items():
        n = np.asarray(norms, dtype=np.float64)
        assert all(float(np.float32(x)) == float(x) or np.isnan(x) for x in n), name
        assert O.ref_grad_norm_check(norms) == expected, name
        if np.all(np.isfinite(n)):
            ratio = np.max(np.abs(n - n[0])) / (n[0] + 1e-6)
            assert ratio < 0.9e-6 or ratio > 1.1e-6, (name, ratio)
            assert expected == (ratio >= 1e-6), name
    assert O.ref_grad_norm_check([1.0]) is False and O.ref_grad_norm_check([0.0, 0.0]) is False
    assert O.ref_grad_norm_check([0.0, 1e-13]) is False and O.ref_grad_norm_check([0.0, 1e-3]) is True


def test_fp32_yardstick_is_recorded(capsys):
    """E32: the elementwise error of the Adam update done in fp32 on the CPU against fp64, on the inputs
    of the GPU element-math tests.  It is of the size fp32 rounding explains, and the values stand in the
    docstring of tests/test_gpu_optim.py, whose tolerance is 4 x E32."""
    e = O.measure_e32()
    with capsys.disabled():
        print(f"\nE32 (fp32 CPU vs fp64): p {e['p']:.2e}  exp_avg {e['m']:.2e}  exp_avg_sq {e['v']:.2e}")
    assert 0 < e["p"] < 16 * O.U32 and 0 < e["v"] < 8 * O.U32
    # exp_avg = b1 m + (1 - b1) g cancels where the two terms have opposite signs: relative to the result
    # the error is unbounded in principle; relative to the terms it is a few roundings
    assert 0 < e["m"] < 1e-2
    doc = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_optim.py")).read().split('"""')[1]
    for k, name in (("p", "master"), ("m", "exp_avg"), ("v", "exp_avg_sq")):
        assert re.search(rf"E32\[{name}\]\s*=\s*{re.escape(f'{e[k]:.2e}')}", doc), (name, f"{e[k]:.2e}")

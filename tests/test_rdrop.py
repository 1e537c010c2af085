"""CPU: the R-Drop definition (tests/rdrop_ref.py, fairseq's compute_kl_loss restated literally)
against the closed forms the HIP kernels implement, and the host plumbing of --rdrop-alpha: the
train parser, the criterion built from the args, the model config switch and the log record."""
import math

import pytest
import torch

import rdrop_ref as RR
from conftest import pkg

PAD = 1


def _case(R, V, seed, pad_every=7, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(2 * R, V, generator=g, dtype=torch.float64) * scale
    t = torch.randint(2, V, (R,), generator=g)
    if pad_every:
        t[::pad_every] = PAD
    return z, t


@pytest.mark.parametrize("R,V", [(1, 37), (5, 37), (9, 257), (16, 1004)])
@pytest.mark.parametrize("eps,alpha", [(0.0, 0.5), (0.2, 5.0)])
def test_restatement_equals_closed_forms(R, V, eps, alpha):
    z, t = _case(R, V, seed=R * 1000 + V)
    loss, nll, kl, grad = RR.rdrop_loss_and_grad(z, t, eps, PAD, alpha, gloss=3.0)
    closs, cnll, ckl, cgrad = RR.closed_form(z, t, eps, PAD, alpha, gloss=3.0)
    assert abs(loss - closs) <= 1e-12 * abs(loss)
    assert abs(nll - cnll) <= 1e-12 * max(abs(nll), 1.0)
    assert abs(kl - ckl) <= 1e-12 * max(abs(kl), 1e-3)
    assert (grad - cgrad).abs().max() <= 1e-12 * grad.abs().max()
    # and kl is the two masked KL divergences written out
    lp = torch.log_softmax(z, -1)
    p, q = lp[:R].exp(), lp[R:].exp()
    keep = t.ne(PAD)
    direct = 0.5 * ((p * (lp[:R] - lp[R:])).sum(-1) + (q * (lp[R:] - lp[:R])).sum(-1))[keep].sum()
    assert abs(kl - direct) <= 1e-12 * max(abs(kl), 1e-3)


def test_identical_halves_give_zero_kl_and_twice_the_ce():
    z, t = _case(6, 37, seed=3)
    z[6:] = z[:6]
    loss, nll, kl, grad = RR.rdrop_loss_and_grad(z, t, 0.2, PAD, 0.7)
    # F.kl_div takes log(exp(lq)), which is lq only to rounding; the closed form is exactly zero
    assert abs(kl) <= 1e-15
    assert RR.closed_form(z, t, 0.2, PAD, 0.7)[2] == 0.0
    from fairseq_stub import _label_smoothed_nll_loss
    ce1, nll1 = _label_smoothed_nll_loss(torch.log_softmax(z[:6], -1), t, 0.2, ignore_index=PAD)
    assert abs(loss - 2 * ce1) <= 1e-12 * abs(loss) and abs(nll - 2 * nll1) <= 1e-12 * abs(nll)
    assert (grad[:6] - grad[6:]).abs().max() <= 1e-15


def test_pad_pairs_contribute_nothing():
    z, t = _case(8, 37, seed=5, pad_every=3)
    loss, nll, kl, grad = RR.rdrop_loss_and_grad(z, t, 0.2, PAD, 2.0)
    pad = t.eq(PAD)
    assert pad.any() and not pad.all()
    assert (grad[:8][pad] == 0).all() and (grad[8:][pad] == 0).all()
    keep = torch.cat((~pad, ~pad))
    l2, n2, k2, _ = RR.rdrop_loss_and_grad(z[keep], t[~pad], 0.2, PAD, 2.0)
    assert abs(loss - l2) <= 1e-12 * abs(loss) and abs(kl - k2) <= 1e-12 * abs(kl) and abs(nll - n2) <= 1e-12 * abs(nll)
    # changing a pad pair's logits changes nothing
    z2 = z.clone()
    z2[:8][pad] += 3.0
    l3, _, k3, _ = RR.rdrop_loss_and_grad(z2, t, 0.2, PAD, 2.0)
    assert l3 == loss and k3 == kl


# ------------------------------------------------------------------------------------ plumbing
BASE = ["--synthetic", "--fp16", "--share-decoder-input-output-embed"]


def test_train_parser_rdrop_alpha():
    P = pkg("plugins")
    p = P.build_parser()
    assert p.parse_args(BASE).rdrop_alpha == 0.0
    a = p.parse_args(BASE + ["--rdrop-alpha", "0.5"])
    assert a.rdrop_alpha == 0.5 and isinstance(a.rdrop_alpha, float)
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ["--rdrop-alpha", "-0.1"])
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ["--rdrop-alpha", "nan"])


def test_criterion_and_cfg_carry_the_flag():
    P = pkg("plugins")
    p = P.build_parser()
    for argv, want in ((BASE, 0.0), (BASE + ["--rdrop-alpha", "0.3"], 0.3)):
        args = p.parse_args(argv)
        task = P.MultiModalSpeechToSpeechTask.setup_task(args)
        crit = task.build_criterion(args)
        assert crit.rdrop_alpha == want and crit.eps == 0.2
        cfg = P.cfg_from_args(args, None, task.vocab_size)
        assert cfg.get("rdrop_alpha", 0.0) == want
        assert ("rdrop_alpha" in cfg) == (want > 0)       # absent at 0: the plain step's config, unchanged
    assert P.SpeechToUnitCriterion(task, 0.2, False, rdrop_alpha=1.5).rdrop_alpha == 1.5
    assert P.SpeechToUnitCriterion(task, 0.2).rdrop_alpha == 0.0
    with pytest.raises(ValueError):
        P.SpeechToUnitCriterion(task, 0.2, False, rdrop_alpha=-1.0)
    with pytest.raises(ValueError):
        P.cfg_from_args(type(args)(**dict(vars(args), rdrop_alpha=-0.5)), None, task.vocab_size)
    # saved with the checkpoint's args (cli._save keeps every scalar flag), ignored by generation
    assert isinstance(vars(args)["rdrop_alpha"], float)
    merged = P.merge_generate_args(type(args)(data="d", path="x.pt"), args)
    assert merged.rdrop_alpha == 0.0


def test_log_record_prints_rdrop_kl_loss():
    cli = pkg("cli")
    st = {"lr": 1e-3, "gnorm": 2.0, "loss_scale": 128.0, "overflow": 0}
    ln2 = math.log(2.0)
    plain = cli.log_record(10, [400.0, 300.0, 50.0, 4.0, 50.0], st, 500.0, 2.0)
    assert "rdrop_kl_loss" not in plain
    assert plain["loss"] == 400.0 / 50.0 / ln2 and plain["nll_loss"] == 300.0 / 50.0 / ln2
    rec = cli.log_record(10, [800.0, 600.0, 50.0, 4.0, 50.0, 7.5], st, 500.0, 2.0)
    assert rec["rdrop_kl_loss"] == 7.5 / 50.0 / ln2
    assert rec["loss"] == 800.0 / 50.0 / ln2 and rec["num_updates"] == 10
    assert {k: v for k, v in rec.items() if k not in ("rdrop_kl_loss", "loss", "nll_loss", "ppl")} == \
        {k: v for k, v in plain.items() if k not in ("loss", "nll_loss", "ppl")}

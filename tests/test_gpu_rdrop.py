"""GPU: R-Drop (--rdrop-alpha).  The pair-KL loss kernels (kernels.ls_xent_rdrop_fwd / _bwd) against
the fp64 restatement of fairseq's criterion (tests/rdrop_ref.py) on the same fp16 logits, their CE
half pinned bit for bit to ls_xent_fwd / ls_xent_bwd, and the plumbing: duplicate_batch, the
trainer's eager and graph steps, the log, and the fairseq drop-in criterion.

Tolerances: loss / nll / kl sums 1e-4 relative and the gradient 2e-3 relative (test_ls_xent's, for
the same fp32 row arithmetic and fp16 gradient); pad rows and pad columns exactly zero."""
import warnings

import numpy as np
import pytest
import torch

import rdrop_ref as RR
from conftest import pkg
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

PAD = 1
PARTS = 512     # include/mms2ut.h MMS_LS_XENT_PARTS


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    k = pkg().kernels
    assert k.LS_XENT_PARTS == PARTS
    return k


def _inputs(R_, V, ld, seed, pad_first=0):
    """fp16 logits [2R, ld] with 60000 in the pad columns, first-half targets [R] with every 7th
    pad (rows 6, 13, ...) and, with pad_first, the first ``pad_first`` pairs pad as well."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(2 * R_, ld, generator=g) * 2).half()
    logits[:, V:] = 60000.0
    target = torch.randint(2, V, (R_,), generator=g)
    target[6::7] = PAD
    target[:pad_first] = PAD
    return logits.cuda(), target.cuda()


def _relerr(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def _fwd(K, logits, target, V, eps, alpha, acc=None, acc_kl=None):
    rows, ld = logits.shape
    out = torch.full((3,), float("nan"), device="cuda")
    lse = K.ls_xent_rdrop_fwd(logits, ld, target, rows, V, eps, PAD, alpha, acc, acc_kl, call_out=out)
    return out, lse


def _check_against_reference(K, logits, target, V):
    rows, ld = logits.shape
    R_ = rows // 2
    pad_rows = torch.cat((target.eq(PAD), target.eq(PAD)))
    z64 = logits[:, :V].double()
    for eps, alpha in ((0.0, 0.5), (0.0, 5.0), (0.2, 0.5), (0.2, 5.0)):
        ref_loss, ref_nll, ref_kl, ref_grad = RR.rdrop_loss_and_grad(z64, target, eps, PAD, alpha, gloss=3.0)
        out, lse = _fwd(K, logits, target, V, eps, alpha)
        got = out.tolist()
        print(f"R {R_} V {V} ld {ld} eps {eps} A {alpha}: got {got} ref {[float(ref_loss), float(ref_nll), float(ref_kl)]}")
        assert _relerr(got[0], float(ref_loss)) <= 1e-4
        assert _relerr(got[1], float(ref_nll)) <= 1e-4
        assert _relerr(got[2], float(ref_kl)) <= 1e-4
        dz = logits.clone()
        g = torch.tensor([3.0], device="cuda")
        K.ls_xent_rdrop_bwd(dz, ld, target, rows, V, eps, PAD, alpha, lse, g, dz)      # in place
        torch.cuda.synchronize()
        err = _rel(dz[:, :V], ref_grad)
        print(f"   gradient rel {err:.3e}")
        assert err <= 2e-3
        assert torch.equal(dz[:, V:], torch.zeros_like(dz[:, V:]))                    # pad columns
        assert torch.equal(dz[pad_rows], torch.zeros_like(dz[pad_rows]))              # pad rows


@pytest.mark.parametrize("V,ld", [(1004, 1024), (1004, 1008), (37, 40), (257, 260), (4096, 4096)])
@pytest.mark.parametrize("R_", [1, 3, 5, 130, 4 * PARTS + 3])   # odd pair counts, < one block, grid-stride
def test_kernels_match_fp64_restatement(K, R_, V, ld):
    logits, target = _inputs(R_, V, ld, seed=R_ * 13 + V)
    assert R_ < 7 or bool(target.eq(PAD).any())
    _check_against_reference(K, logits, target, V)


@pytest.mark.parametrize("V,ld", [(1004, 1024), (37, 40)])
def test_first_block_of_pairs_all_pad(K, V, ld):
    logits, target = _inputs(130, V, ld, seed=77 + V, pad_first=4)
    assert bool(target[:4].eq(PAD).all())
    _check_against_reference(K, logits, target, V)


def test_all_pairs_pad_gives_zeros(K):
    logits, _ = _inputs(9, 1004, 1008, seed=4)
    target = torch.full((9,), PAD, dtype=torch.int64, device="cuda")
    out, lse = _fwd(K, logits, target, 1004, 0.2, 0.5)
    assert out.tolist() == [0.0, 0.0, 0.0]
    dz = logits.clone()
    K.ls_xent_rdrop_bwd(dz, 1008, target, 18, 1004, 0.2, PAD, 0.5, lse, torch.ones(1, device="cuda"), dz)
    assert torch.equal(dz, torch.zeros_like(dz))


def test_target_out_of_range_poisons_the_sums(K):
    logits, target = _inputs(5, 37, 40, seed=8)
    for bad in (37, -3, 10 ** 7):
        t = target.clone()
        t[2] = bad
        out, _ = _fwd(K, logits, t, 37, 0.2, 0.5)
        got = out.tolist()
        assert np.isnan(got[0]) and np.isnan(got[1]), (bad, got)


def _one_ulp(x):
    """every fifth element of an fp16 tensor moved by one ulp (one step of its bit pattern)"""
    y = x.clone().view(torch.int16).view(-1)
    y[::5] += 1
    return y.view(torch.float16).view(x.shape)


@pytest.mark.parametrize("R_,V,ld", [(5, 37, 40), (130, 1004, 1024), (3, 257, 260), (5, 4096, 4096)])
def test_near_identical_halves(K, R_, V, ld):
    """Copy 2 is copy 1 with every fifth logit moved by one fp16 ulp, so kl is tiny (5e-7 .. 1e-4)
    and any cancellation in the kernel would show.  The yardstick is the literal formula
    (log_softmax, two F.kl_div) evaluated by torch in fp32 on the same input: the kernel may be off
    from the fp64 value by at most 4 x that evaluation's own error (the factor covers a different
    summation order).  The kernel forms d = lp - lq as (z_p - z_q) - (lse_p - lse_q): the logit
    difference is exact and the rounding of the lse difference is one constant per pair, which
    multiplies sum_v (p_v - q_v) ~ 0, so it is far more accurate than the fp32 literal form.
    Measured on an MI355X, |kernel - fp64| vs |fp32 literal - fp64| (ratio): 6.1e-11 vs 4.8e-7
    (1e-4) at 5 x 37, 9.5e-11 vs 2.4e-5 (4e-6) at 130 x 1004, 5.5e-11 vs 4.1e-7 (1e-4) at 3 x 257,
    2.2e-11 vs 1.2e-6 (2e-5) at 5 x 4096; also in DESIGN.md section 8, R-Drop."""
    g = torch.Generator().manual_seed(R_ + V)
    a = (torch.randn(R_, ld, generator=g) * 2).half()
    a[:, V:] = 60000.0
    b = _one_ulp(a)
    b[:, V:] = 60000.0
    logits = torch.cat((a, b)).cuda()
    target = torch.randint(2, V, (R_,), generator=g).cuda()
    z = logits[:, :V]
    ref = float(RR.rdrop_loss(z.double(), target, 0.2, PAD, 0.5)[2])
    f32 = float(RR.rdrop_loss(z.float(), target, 0.2, PAD, 0.5)[2])
    out, _ = _fwd(K, logits, target, V, 0.2, 0.5)
    got = out[2].item()
    e_k, e_32 = abs(got - ref), abs(f32 - ref)
    print(f"R {R_} V {V}: kl fp64 {ref:.9e} kernel {got:.9e} (err {e_k:.3e}) fp32 torch {f32:.9e} (err {e_32:.3e}) "
          f"ratio {e_k / max(e_32, 1e-300):.4f}")
    assert ref > 0 and e_32 > 0
    assert e_k <= 4 * e_32


@pytest.mark.parametrize("with_pad", [False, True])
@pytest.mark.parametrize("R_,V,ld,eps", [(130, 1004, 1024, 0.2), (5, 37, 40, 0.0), (4 * PARTS + 3, 1004, 1008, 0.2),
                                         (3, 4096, 4096, 0.2)])
def test_identical_halves_pin_the_ce_half(K, R_, V, ld, eps, with_pad):
    """kl == 0.0 exactly, lse and the in-place gradient bit-equal to ls_xent_fwd / ls_xent_bwd on
    the 2R rows, loss and nll equal to their sums to 1e-6.  A pad pair's logits are never read, so
    its two lse entries are 0 instead of ls_xent_fwd's values (nothing reads either): they are
    compared on the non-pad rows, and on every row in the cases without pad targets."""
    half, target = _inputs(R_, V, ld, seed=5 * R_ + V)
    half = half[:R_]
    if with_pad:
        target[R_ // 2] = PAD
    else:
        target[target.eq(PAD)] = 3
    logits = torch.cat((half, half)).contiguous()
    rows = 2 * R_
    t2 = torch.cat((target, target))
    out, lse = _fwd(K, logits, target, V, eps, 5.0)
    plain = torch.zeros(2, device="cuda")
    lse_plain = K.ls_xent_fwd(logits, ld, t2, rows, V, eps, PAD, plain)
    torch.cuda.synchronize()
    assert out[2].item() == 0.0
    keep = t2.ne(PAD)
    assert torch.equal(lse[keep], lse_plain[keep])
    assert torch.equal(lse[~keep], torch.zeros_like(lse[~keep]))
    assert _relerr(out[0].item(), plain[0].item()) <= 1e-6 and _relerr(out[1].item(), plain[1].item()) <= 1e-6
    g = torch.tensor([3.0], device="cuda")
    dz_plain = torch.full_like(logits, float("nan"))
    K.ls_xent_bwd(logits, ld, t2, rows, V, eps, PAD, lse_plain, g, dz_plain)
    dz = logits.clone()
    K.ls_xent_rdrop_bwd(dz, ld, target, rows, V, eps, PAD, 5.0, lse, g, dz)
    torch.cuda.synchronize()
    ne = dz[keep].view(torch.int16) != dz_plain[keep].view(torch.int16)
    n_ne = int(ne.sum())
    print(f"R {R_} V {V} ld {ld} pad {with_pad}: {n_ne} of {ne.numel()} gradient elements differ in bits")
    if n_ne:
        a_, b_ = dz[keep][ne], dz_plain[keep][ne]
        cols = ne.nonzero()[:, 1]
        print(f"   rdrop {a_[:8].tolist()} ({a_[:8].view(torch.int16).tolist()})\n   plain {b_[:8].tolist()} "
              f"({b_[:8].view(torch.int16).tolist()})\n   columns {cols[:8].tolist()} (mod 4: {(cols % 4).bincount(minlength=4).tolist()}) "
              f"max |diff| {(a_.float() - b_.float()).abs().max().item():.3e} max |value| {b_.float().abs().max().item():.3e}")
    assert n_ne == 0
    # pad rows: zeros in both (ls_xent_bwd multiplies by a zero coefficient, which can leave -0.0)
    assert torch.equal(dz[~keep], torch.zeros_like(dz[~keep])) and torch.equal(dz_plain[~keep], dz[~keep])


def test_two_runs_same_bits_and_log_accumulation(K):
    V, ld = 1004, 1024
    calls = [_inputs(r, V, ld, seed=90 + r) for r in (130, 4 * PARTS + 3)]

    def run():
        acc, acc_kl = torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda")
        outs, grads = [], []
        for lg, tg in calls:
            out, lse = _fwd(K, lg, tg, V, 0.2, 0.5, acc, acc_kl)
            dz = lg.clone()
            K.ls_xent_rdrop_bwd(dz, ld, tg, lg.shape[0], V, 0.2, PAD, 0.5, lse, torch.ones(1, device="cuda"), dz)
            outs.append(out.clone())
            grads.append(dz)
        return acc, acc_kl, outs, grads

    a, b = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16),
                           y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int16))
    want = [sum(o[k].item() for o in a[2]) for k in range(3)]
    assert _relerr(a[0][0].item(), want[0]) <= 1e-6 and _relerr(a[0][1].item(), want[1]) <= 1e-6
    assert _relerr(a[1][0].item(), want[2]) <= 1e-6 and want[2] > 0
    # acc alone / kl alone / call_out alone are each enough
    lg, tg = calls[0]
    only = torch.zeros(1, device="cuda")
    K.ls_xent_rdrop_fwd(lg, ld, tg, lg.shape[0], V, 0.2, PAD, 0.5, None, only, None)
    assert only.item() == a[2][0][2].item()


def test_rejects_bad_arguments(K):
    lg = torch.zeros(4, 1008, dtype=torch.float16, device="cuda")
    tg = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.zeros(3, device="cuda")
    lse = torch.zeros(4, device="cuda")
    g = torch.ones(1, device="cuda")
    big = torch.zeros(2, 4100, dtype=torch.float16, device="cuda")
    odd = torch.zeros(1, 2016 + 1008, dtype=torch.float16, device="cuda").view(-1)[1:1 + 2 * 1008]
    bad = [(lg, 1008, 3, 1004),            # odd rows
           (lg, 1000, 4, 1004),            # ld < V
           (lg, 1006, 4, 1004),            # ld % 4
           (big, 4100, 2, 4097),           # beyond the 4096-column limit
           (odd, 1008, 2, 1004)]           # 2-byte aligned logits
    for t, ld, rows, V in bad:
        with pytest.raises(RuntimeError):
            K.ls_xent_rdrop_fwd(t, ld, tg, rows, V, 0.2, PAD, 0.5, None, None, out)
        with pytest.raises(RuntimeError):
            K.ls_xent_rdrop_bwd(t, ld, tg, rows, V, 0.2, PAD, 0.5, lse, g, t)
    with pytest.raises(RuntimeError):
        K.ls_xent_rdrop_fwd(lg, 1008, tg, 4, 1004, 0.2, PAD, 0.5, None, None, None)   # nowhere to put the sums
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out)) and torch.equal(lg, torch.zeros_like(lg))
    with pytest.raises(ValueError):
        pkg().runtime.label_smoothed_ce_rdrop(lg, tg, 1004, 0.2, PAD, 0.0)


# ------------------------------------------------------------------------------------ plumbing
def _cfg(mm, dropout, **kw):
    c = R.tiny_config(conv_channels=256)
    if not dropout:
        c = R.no_dropout(c)
    c = mm.default_cfg(**c)
    c.update(kw)
    return c


def _sample(mm, cfg, seed=2):
    return mm.data.make_sample([61, 47, 30], [14, 11, 9], img_tokens=17, img_dim=cfg["image_feat_dim"], seed=seed)


def _trainer(mm, cfg, seed=4, **kw):
    model = mm.MMS2UTModel(cfg, device="cuda").init_params(seed=seed)
    tr = mm.trainer.Trainer(model, lr=1e-3, warmup_updates=0, world_size=1, **kw)
    taps = []
    tr.grad_tap = lambda g: taps.append(g.clone())
    return model, tr, taps


def test_duplicate_batch_doubles_every_per_sentence_field():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mm = pkg()
    from test_gpu_multitask import _mt_sample, _tasks
    cfg = _cfg(mm, dropout=False)
    letters, tasks = _tasks(mm, cfg)
    cfg["multitask"] = tasks
    sample = mm.data.make_sample([160, 131, 97], [41, 30, 22], img_tokens=37, img_dim=768, img_mask=True, seed=2)
    sample["multitask"] = _mt_sample(mm, tasks, letters, sample, seed=3)
    batch = mm.runtime.prepare_batch(sample, cfg, "cuda")
    dup = mm.runtime.duplicate_batch(batch)
    B = batch.prev.shape[0]
    seen = 0
    for name in ("src", "enc_len32", "prev", "tgt_mask", "tgt_len32", "target", "imgs", "img_keymask",
                 "tgt_lengths32", "src_lengths"):
        x, y = getattr(batch, name), getattr(dup, name)
        assert x is not None, name            # the sample exercises every field
        assert y.shape == (2 * B, *x.shape[1:]) and y.dtype == x.dtype and y.device == x.device, name
        assert torch.equal(y[:B], x) and torch.equal(y[B:], x), name
        seen += 1
    assert seen == 10
    assert (dup.Te, dup.ntokens, dup.nsentences, dup.n_src_frames) == \
        (batch.Te, batch.ntokens, batch.nsentences, batch.n_src_frames)
    assert set(dup.mt) == set(batch.mt) and len(dup.mt) == 3
    for name, mb in batch.mt.items():
        d = dup.mt[name]
        for k in type(mb).__slots__:
            assert hasattr(d, k) == hasattr(mb, k), (name, k)
            if not hasattr(mb, k):
                continue
            x, y = getattr(mb, k), getattr(d, k)
            if torch.is_tensor(x):
                assert y.shape == (2 * x.shape[0], *x.shape[1:]) and torch.equal(y[:x.shape[0]], x) \
                    and torch.equal(y[x.shape[0]:], x), (name, k)
            else:
                assert y == x or (x is None and y is None), (name, k)
    # a second call reuses the buffers (stable addresses for a captured step) and refreshes them
    ptr = dup.src.data_ptr()
    batch.src.mul_(2)
    dup2 = mm.runtime.duplicate_batch(batch)
    assert dup2.src.data_ptr() == ptr and torch.equal(dup2.src[B:], batch.src)


def test_rdrop_step_without_dropout_is_twice_the_plain_step():
    """Dropout 0, no modality dropout: both passes compute the same logits, so the R-Drop step's
    gradient is twice the plain step's (parity_util's 1e-2 for fp16 gradients: the 2B-row GEMMs sum
    in another order), loss / nll double, the counts do not, and kl stays below what one fp16 ulp
    of difference between the halves could produce."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mm = pkg()
    cfg = _cfg(mm, dropout=False)
    A = 0.5
    model_p, tr_p, taps_p = _trainer(mm, cfg)
    model_r, tr_r, taps_r = _trainer(mm, dict(cfg, rdrop_alpha=A))
    batch = mm.runtime.prepare_batch(_sample(mm, cfg), cfg, "cuda")
    with torch.no_grad():
        model_r.train()
        z = mm.runtime.model_logits(model_r, mm.runtime.duplicate_batch(batch))[:, :cfg["vocab_size"]].float()
    log_p = tr_p.train_step(batch).clone()
    log_r = tr_r.train_step(batch).clone()
    tr_p.sync(), tr_r.sync()
    torch.cuda.synchronize()
    assert log_p.numel() == 5 and log_r.numel() == 6
    lp, lr = log_p.tolist(), log_r.tolist()
    print(f"plain log {lp}\nrdrop log {lr}")
    assert _relerr(lr[0], 2 * lp[0]) <= 1e-3 and _relerr(lr[1], 2 * lp[1]) <= 1e-3
    assert lr[2:5] == lp[2:5] and lr[2] == batch.ntokens and lr[3] == batch.nsentences
    nonpad = int(batch.target.ne(PAD).sum())
    bound = 0.5 * (2.0 ** -10 * z.abs().max().item()) ** 2
    Rr = z.shape[0] // 2
    print(f"kl {lr[5]:.3e} (exactly 0: {lr[5] == 0.0}; halves bit-equal: {torch.equal(z[:Rr], z[Rr:])}); "
          f"bound per row {bound:.3e} x {nonpad} rows")
    assert 0.0 <= lr[5] <= bound * nonpad
    gp, gr = taps_p[0].float(), taps_r[0].float()
    assert torch.isfinite(gr).all()
    err = _rel(gr, 2 * gp)
    worst = max(((n, _rel(gr[o:o + k], 2 * gp[o:o + k])) for n, (o, _, k) in model_p.params.offsets.items()
                 if gp[o:o + k].norm() > 0), key=lambda t: t[1])
    print(f"gradient rel {err:.3e}; worst parameter {worst}")
    assert err <= 1e-2


def test_alpha_zero_is_the_plain_step_bit_for_bit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mm = pkg()
    cfg = _cfg(mm, dropout=True)
    assert "rdrop_alpha" not in cfg
    batch = mm.runtime.prepare_batch(_sample(mm, cfg), cfg, "cuda")
    res = []
    for c in (cfg, dict(cfg, rdrop_alpha=0.0)):
        model, tr, taps = _trainer(mm, c, device_seed=True)
        try:
            logs = [tr.train_step(batch).clone() for _ in range(2)]
            tr.sync()
            torch.cuda.synchronize()
        finally:
            mm.kernels.bind_step_seed(None)
        assert "_rdrop" not in batch.__dict__
        res.append((logs, model.params.flat.clone(), tr.opt.master.clone(), taps))
    (la, pa, ma, ta), (lb, pb, mb, tb) = res
    for x, y in zip(la, lb):
        assert x.numel() == 5 and torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(pa, pb) and torch.equal(ma, mb)
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))


def test_rdrop_step_with_dropout():
    """Dropout 0.1: the two passes see different masks (the counter RNG keys on the element index
    within the 2B tensors), kl > 0, and a fixed seed reproduces the step bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mm = pkg()
    cfg = _cfg(mm, dropout=True, rdrop_alpha=0.5)
    batch = mm.runtime.prepare_batch(_sample(mm, cfg), cfg, "cuda")
    res = []
    for _ in range(2):
        model, tr, taps = _trainer(mm, cfg, device_seed=True)
        try:
            log = tr.train_step(batch).clone()
            tr.sync()
            torch.cuda.synchronize()
        finally:
            mm.kernels.bind_step_seed(None)
        res.append((log, taps[0], model.params.flat.clone()))
    (l0, g0, p0), (l1, g1, p1) = res
    print(f"log {l0.tolist()}")
    assert l0[5].item() > 0 and torch.isfinite(l0).all() and torch.isfinite(g0.float()).all()
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    assert torch.equal(g0, g1) and torch.equal(p0, p1)


def test_criterion_loss_matches_restatement_on_its_own_logits():
    """The criterion path that exposes ``_logits_padded``: with dropout 0.1 the two halves of the
    step's logits differ, and the criterion's loss / nll / kl equal the fp64 restatement applied to
    those very logits to 1e-4."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mm = pkg()
    P = pkg("plugins")
    cfg = _cfg(mm, dropout=True)
    model = P.MM_S2UTTransformerModel(cfg, device="cuda", seed=3)
    task = type("T", (), {"padding_idx": PAD})()
    A = 0.7
    crit = P.SpeechToUnitCriterion(task, cfg["label_smoothing"], False, rdrop_alpha=A)
    sample = _sample(mm, cfg, seed=5)
    model.train()
    V = cfg["vocab_size"]
    model.net.drop.reset(11)
    _, extra = model(**sample["net_input"], target=sample["target"], duplicate_input=True)
    z = extra["_logits_padded"].detach().clone()
    B = sample["target"].shape[0]
    assert extra["_batch"].prev.shape[0] == 2 * B and z.shape[0] == 2 * sample["target"].numel()
    Rr = z.shape[0] // 2
    assert not torch.equal(z[:Rr, :V], z[Rr:, :V])
    model.net.drop.reset(11)
    loss, ss, log = crit(model, sample)
    tgt = sample["target"].reshape(-1).cuda()
    ref = RR.rdrop_loss(z[:, :V].double(), tgt, cfg["label_smoothing"], PAD, A)
    got = (loss.item(), log["nll_loss"].item(), log["rdrop_kl_loss"].item())
    print(f"criterion {got} restatement {[float(x) for x in ref]}")
    for a, b in zip(got, ref):
        assert _relerr(a, float(b)) <= 1e-4
    assert got[2] > 0
    assert ss == sample["ntokens"] == log["sample_size"] == log["ntokens"] and log["nsentences"] == B
    assert float(log["loss"]) == got[0]
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(model.net.params.grad.float()).all()
    # eval mode: un-duplicated, no kl in the log
    model.eval()
    with torch.no_grad():
        _, _, elog = crit(model, sample)
    model.train()
    assert "rdrop_kl_loss" not in elog


def test_rdrop_graph_mode_matches_eager():
    """A = 0.5: capture and two replays against three eager steps on the same device step-seed
    schedule, to the standard tests/test_gpu_graph.py holds the plain step to (logs 1e-4, parameter
    updates 1e-2 relative, loss scale / step count / overflow exact)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mm = pkg()
    Kk = mm.kernels
    cfg = _cfg(mm, dropout=True, rdrop_alpha=0.5)
    batch = mm.runtime.prepare_batch(
        mm.data.make_sample([120, 90], [30, 22], img_tokens=37, img_dim=768, seed=0), cfg, "cuda")
    models = [mm.MMS2UTModel(cfg, device="cuda").init_params(seed=5) for _ in range(2)]
    trs = [mm.trainer.Trainer(models[0], warmup_updates=0, lr=1e-3, graph=True),
           mm.trainer.Trainer(models[1], warmup_updates=0, lr=1e-3, device_seed=True)]
    p0 = models[1].params.flat.float().clone()
    dr = (0.9, 0.9)
    try:
        for i in range(3):
            logs = []
            for k, tr in enumerate(trs):
                if k == 0:
                    log = tr.train_step(batch, draws=[dr])
                else:
                    models[1].np_rng = type("S", (), {"v": list(dr), "random": lambda self: self.v.pop(0)})()
                    log = tr.train_step(batch)
                logs.append(log.clone())
            for tr in trs:
                tr.sync()
            torch.cuda.synchronize()
            print(f"step {i}: graph {logs[0].tolist()} eager {logs[1].tolist()}")
            assert logs[0].numel() == 6 and logs[0][5].item() > 0
            assert _rel(logs[0], logs[1]) < 1e-4, (i, logs)
            assert _relerr(logs[0][5].item(), logs[1][5].item()) < 1e-3, (i, logs)
            oa, ob = trs[0].opt.ost, trs[1].opt.ost
            for j in (Kk.OST_LOSS_SCALE, Kk.OST_STEP, Kk.OST_OVERFLOW):
                assert oa[j].item() == ob[j].item(), (i, j)
            ua, ub = models[0].params.flat.float() - p0, models[1].params.flat.float() - p0
            if ub.norm() > 0:
                assert _rel(ua, ub) < 1e-2, (i, _rel(ua, ub))
        assert len(trs[0].graphs) == 1
    finally:
        Kk.bind_step_seed(None)


def test_rdrop_with_multitask_heads_warns_once_and_doubles_their_losses():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    mm = pkg()
    from test_gpu_multitask import _mt_sample, _tasks
    cfg = _cfg(mm, dropout=False)
    letters, tasks = _tasks(mm, cfg)
    cfg["multitask"] = tasks
    sample = mm.data.make_sample([160, 131, 97], [41, 30, 22], img_tokens=37, img_dim=768, seed=2)
    sample["multitask"] = _mt_sample(mm, tasks, letters, sample, seed=3)
    batch = mm.runtime.prepare_batch(sample, cfg, "cuda")
    model_p, tr_p, _ = _trainer(mm, cfg, seed=9)
    mm.runtime._RDROP_MT_WARNED[0] = False
    with pytest.warns(UserWarning, match="rdrop"):
        model_r, tr_r, _ = _trainer(mm, dict(cfg, rdrop_alpha=0.5), seed=9)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*rdrop.*")          # only once per process
        mm.trainer.Trainer(model_r, world_size=1)
    log_p = tr_p.train_step(batch).tolist()
    aux_p = {k: v.item() for k, v in model_p.last_aux_losses.items()}
    log_r = tr_r.train_step(batch).tolist()
    aux_r = {k: v.item() for k, v in model_r.last_aux_losses.items()}
    print(f"plain {log_p} {aux_p}\nrdrop {log_r} {aux_r}")
    assert set(aux_p) == set(aux_r) and len(aux_p) == 3
    for k in aux_p:
        assert _relerr(aux_r[k], 2 * aux_p[k]) <= 1e-3, k
    assert _relerr(log_r[0], 2 * log_p[0]) <= 1e-3 and log_r[2:5] == log_p[2:5]


def test_fairseq_dropin_criterion_matches_native_trainer(monkeypatch, tmp_path):
    """The fairseq call sequence (tests/fairseq_stub.py) with --rdrop-alpha: the criterion built by
    the task carries the flag and gives the native trainer's loss, kl and sample size on the same
    batch and dropout seed."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fairseq_stub
    from test_gpu_plugins import FUSION_NODROP
    mm = pkg()
    fs, regs, args, c, _ = fairseq_stub.dropin_setup(monkeypatch, tmp_path, FUSION_NODROP, extra="--rdrop-alpha 0.5")
    task = fs.tasks.setup_task(args)
    task.load_dataset("train")
    model = task.build_model(args).half()
    crit = task.impl.build_criterion(args)
    assert crit.rdrop_alpha == 0.5 and model.impl.cfg["rdrop_alpha"] == 0.5
    batches = task.get_batch_iterator(task.dataset("train"), max_tokens=450, max_positions=task.max_positions())
    sample = fs.utils.apply_half(fs.utils.move_to_cuda(batches[0]))
    native, net = model.impl, model.impl.net
    model.train()
    net.drop.reset(7)
    loss, ss, log = crit(native, sample)
    ni = sample["net_input"]
    batch = native._batch(ni.get("src_tokens"), ni["src_lengths"], ni["prev_output_tokens"], ni.get("imgs_list"),
                          ni.get("img_masks_list"), sample["target"], None, extra_input=ni)
    batch.ntokens = int(sample["ntokens"])
    tr = mm.trainer.Trainer(net, lr=1e-3, warmup_updates=0, world_size=1)
    net.drop.reset(7)
    tlog = tr.train_step(batch).tolist()
    tr.sync()
    torch.cuda.synchronize()
    got = (loss.item(), log["nll_loss"].item(), log["rdrop_kl_loss"].item())
    print(f"criterion {got} ss {ss}; trainer log {tlog} (loss bit-equal: {got[0] == tlog[0]})")
    assert got[2] > 0
    assert _relerr(got[0], tlog[0]) <= 1e-6 and _relerr(got[1], tlog[1]) <= 1e-6 and _relerr(got[2], tlog[5]) <= 1e-6
    assert ss == sample["ntokens"] == tlog[2] and log["nsentences"] == tlog[3] == sample["target"].size(0)

"""CPU: the flash-attention test references (tests/attn_ref.py) checked against torch and each other,
so that tests/test_gpu_attention_paths.py measures the kernels and not its own helpers."""
import math

import pytest
import torch

import attn_ref as A

# (causal, Tq, Tk, lens, p): shapes of the kind test_gpu_attention_paths.py runs (randn inputs)
RANDN_CASES = [(False, 20, 40, [40, 21, 1], 0.0), (True, 130, 129, [129, 65, 1], 0.1),
               (False, 24, 72, [72, 37, 1], 0.1), (True, 70, 200, [200, 101, 1], 0.0),
               (False, 33, 257, [257, 0, 129], 0.1)]


def _inputs(B, H, Tq, Tk, hd, seed=3):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Tq, hd, generator=g).half()
    k = torch.randn(B, H, Tk, hd, generator=g).half()
    v = torch.randn(B, H, Tk, hd, generator=g).half()
    do = torch.randn(B, H, Tq, hd, generator=g).half()
    return q, k, v, do


@pytest.mark.parametrize("causal", [False, True])
def test_ref64_matches_torch_sdpa(causal):
    B, H, Tq, Tk, hd = 3, 2, 37, 50, 64
    lens = [50, 26, 1]
    q, k, v, do = _inputs(B, H, Tq, Tk, hd)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    mask = A.valid_mask(lens, Tq, Tk, causal, B)
    scale = hd ** -0.5
    o = torch.nn.functional.scaled_dot_product_attention(qd, kd, vd, attn_mask=mask, scale=scale)
    o.backward(do.double())
    r = A.ref64(q, k, v, do, lens, causal, scale)
    for name, want in (("o", o), ("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        assert float(A.frob_per_head(r[name], want.detach()).max()) < 1e-12, name
    s = (qd.detach() @ kd.detach().transpose(-1, -2)) * scale
    lse = torch.logsumexp(torch.where(mask, s, torch.full_like(s, -math.inf)), -1)
    assert float((r["lse"] - lse).abs().max()) < 1e-12


def test_ref64_dropout_and_empty_rows():
    """Dropout against autograd of the explicit formula; a batch row without keys gives o = 0,
    lse = -inf and no gradient anywhere."""
    B, H, Tq, Tk, hd, p = 3, 2, 9, 12, 64, 0.25
    lens = [12, 0, 5]
    q, k, v, do = _inputs(B, H, Tq, Tk, hd)
    keep = A.keep_flags(77, 4096, B, H, Tq, Tk, p)
    r = A.ref64(q, k, v, do, lens, True, 0.125, keep, p)
    assert torch.equal(r["o"][1], torch.zeros_like(r["o"][1]))
    assert bool(torch.isinf(r["lse"][1]).all()) and bool((r["lse"][1] < 0).all())
    for n in ("dq", "dk", "dv"):
        assert torch.equal(r[n][1], torch.zeros_like(r[n][1])), n
        assert bool(torch.isfinite(r[n]).all())
    live = [0, 2]
    qd, kd, vd = (t[live].double().requires_grad_(True) for t in (q, k, v))
    mask = A.valid_mask([lens[i] for i in live], Tq, Tk, True, 2)
    s = (qd @ kd.transpose(-1, -2)) * 0.125
    P = torch.softmax(torch.where(mask, s, torch.full_like(s, -math.inf)), -1)
    o = (P * keep[live].double() * A.drop_scale(p)) @ vd
    o.backward(do[live].double())
    for name, want in (("o", o), ("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        assert float(A.frob_per_head(r[name][live], want.detach()).max()) < 1e-12, name
    # dK / dV of keys past the length are exactly zero
    assert torch.equal(r["dk"][2, :, 5:], torch.zeros_like(r["dk"][2, :, 5:]))
    assert torch.equal(r["dv"][2, :, 5:], torch.zeros_like(r["dv"][2, :, 5:]))


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("causal,Tq,Tk,lens,p", RANDN_CASES)
def test_emulated_within_project_bounds(hd, causal, Tq, Tk, lens, p):
    """The fp16 rounding points alone stay inside the project's 3e-3 (o) / 5e-3 (gradients) on randn
    inputs, per head; and inside them by enough that 4x the emulated error is a usable bound."""
    B, H = 3, 2
    q, k, v, do = _inputs(B, H, Tq, Tk, hd)
    keep = A.keep_flags(77, 1024, B, H, Tq, Tk, p)
    r = A.ref64(q, k, v, do, lens, causal, hd ** -0.5, keep, p)
    e = A.emulate(q, k, v, do, lens, causal, hd ** -0.5, keep, p)
    for name, bound in (("o", 3e-3), ("dq", 5e-3), ("dk", 5e-3), ("dv", 5e-3)):
        assert float(A.frob_per_head(e[name], r[name]).max()) < bound, name
        err, _ = A.row_err(e[name], r[name])
        assert math.isfinite(float(err.max())), name
    assert torch.equal(torch.isinf(e["lse"]), torch.isinf(r["lse"]))
    err, _ = A.row_err(e["lse"], r["lse"])
    assert float(err.max()) < 1e-5


def test_row_err_names_the_wrong_row():
    ref = torch.randn(2, 3, 50, 64, dtype=torch.float64)
    got = ref.clone()
    got[1, 2, 17] += 0.5 * ref[1, 2, 17].norm() * torch.nn.functional.normalize(torch.randn(64, dtype=torch.float64), dim=0)
    err, row = A.row_err(got, ref)
    val, where = A.worst(err, row)
    assert where == "b=1 h=2 row=17"
    assert 0.2 < val < 1.5
    assert float(err.sum() - err[1, 2]) == 0.0
    # diluted over the head it would read ~ 0.5 / sqrt(50); the row measure keeps it whole
    assert val > 3 * float(A.frob_per_head(got, ref)[1, 2])
    # non-finite reference rows compare exactly
    lse = torch.tensor([[[0.5, -math.inf, 1.0]]], dtype=torch.float64)
    assert float(A.row_err(lse.clone(), lse)[0].max()) == 0.0
    bad = lse.clone()
    bad[0, 0, 1] = 0.0
    assert math.isinf(float(A.row_err(bad, lse)[0].max()))
    nan = torch.full((1, 1, 3, 4), math.nan, dtype=torch.float64)
    assert math.isinf(float(A.row_err(nan, torch.ones(1, 1, 3, 4, dtype=torch.float64))[0].max()))


def test_ulp16_rel():
    r = A.ulp16_rel(torch.tensor([1.0, 1.5, 2.0, 0.0, 1023.9], dtype=torch.float64))
    assert r[0] == 2.0 ** -10 and r[2] == 2.0 ** -10 and r[3] == 0
    assert abs(float(r[1]) - 2.0 ** -10 / 1.5) < 1e-15
    assert 2.0 ** -11 < float(r[4]) <= 2.0 ** -10


@pytest.mark.parametrize("layout,gap", [("bm", 0), ("bm", 3), ("tm", 0)])
def test_padded_buffer_and_sentinel_check(layout, gap):
    B, T, W, ld = 3, 5, 16, 24
    data = torch.randn(B, T, W).half()
    buf = A.Padded(B, T, W, ld=ld, layout=layout, gap_rows=gap, data=data)
    assert torch.equal(buf.view, data)
    if layout == "tm":
        assert (buf.row, buf.sb) == (B * ld, ld)
    else:
        assert (buf.row, buf.sb) == (ld, (T + gap) * ld)
    assert buf.batch_stride == (0 if (layout, gap) == ("bm", 0) else buf.sb)
    assert buf.view.data_ptr() == buf.flat.data_ptr() + 2 * buf.front
    # element (b, t, c) sits where the library's addressing puts it
    assert buf.flat[buf.front + 2 * buf.sb + 4 * buf.row + 7] == data[2, 4, 7]
    assert int(buf.outside.sum()) == buf.flat.numel() - B * T * W
    buf.check()
    buf.view.fill_(1.0)             # writing the whole logical region is fine
    buf.check()
    assert buf.untouched()
    for off in (buf.front - 1, buf.front + W, buf.front + (T - 1) * buf.row + (B - 1) * buf.sb + W):
        buf.check()
        saved = buf.flat[off].clone()
        buf.flat[off] = 0.0         # one out-of-region element altered
        assert not buf.untouched()
        with pytest.raises(AssertionError, match="outside the logical region"):
            buf.check("o")
        buf.flat[off] = saved
    assert buf.untouched()

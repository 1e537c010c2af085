"""GPU: every kernel that draws dropout keep flags, against the independent restatement of the
stream (tests/rng_ref.py), on both sides of each kernel's fast / slow split.

Most kernels hoist a per-site constant out of the hash and fall back to the full mms_keep when the
site's counters straddle a 2^33 boundary (the pair index changes its high word) or when the site's
first counter or row length is odd.  Each consumer below runs at four first counters (WHERE):

  even           4096
  odd            4097
  straddle_even  2^33 falls strictly inside the site, first counter even
  straddle_odd   the same with an odd first counter

For a site of `rows` rows of L counters the boundary lands in row rows // 2 at column L // 2 or
L // 2 + 1 (whichever gives the parity), never in the first or the last row (site_offset).  For the
flash kernels it lands in the middle row of head z = 2 of 6 (z = 144 of 288): the heads before it
take the fast path, that head the slow one, the heads after it the fast path with the new high
word.  Reference masks come from rng_ref, never from K.dropout_mask; mask patterns are compared
exactly, values under the bounds tests/test_gpu_kernels.py sets for the same kernels."""
import math

import numpy as np
import pytest
import torch

import rng_ref
from conftest import pkg

pytestmark = pytest.mark.gpu

B33 = 2 ** 33
WHERE = ["even", "odd", "straddle_even", "straddle_odd"]
SEED = {"even": 77, "odd": 78, "straddle_even": 0x0123456789ABCDEF, "straddle_odd": 2 ** 63 - 1}


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg().kernels


def site_offset(where, rows, L, before=0):
    """First counter of a site of rows x L counters (`before`: counters of the call that precede the
    site, the earlier heads of an attention call).  The straddling forms put 2^33 at row rows // 2,
    column L // 2 (or L // 2 + 1 for the parity) of the site."""
    if where == "even":
        return 4096
    if where == "odd":
        return 4097
    assert rows >= 3 and L >= 4
    k = before + (rows // 2) * L + L // 2
    if (k % 2 == 1) != (where == "straddle_odd"):
        k += 1
    off = B33 - k
    assert off % 2 == (where == "straddle_odd")
    first, last = off + before, off + before + rows * L - 1
    assert first + L <= B33 <= last - L          # not in the first or the last row
    return off


def ref_keep(seed, off, shape, p):
    n = int(np.prod(shape))
    return torch.from_numpy(rng_ref.keep(seed, off, n, p)).view(*shape).cuda()


def ds32(p):
    """The kernels' 1.f / (1.f - p) in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def ulps16(a, b):
    """Largest distance between two fp16 tensors in units in the last place."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs().max().item() if a.numel() else 0


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _away_from_zero(shape, g, lo=0.5, span=1.5, sign=None):
    """fp16 values with lo <= |x| < lo + span (a zero in an output is then a dropped element); sign:
    a broadcastable +-1 tensor, random when None."""
    mag = lo + span * torch.rand(*shape, generator=g, device="cuda")
    if sign is None:
        sign = torch.where(torch.rand(*shape, generator=g, device="cuda") < 0.5, -1.0, 1.0)
    return (mag * sign).half()


def _col_sign(D, g):
    return torch.where(torch.rand(D, generator=g, device="cuda") < 0.5, -1.0, 1.0)


# ============================================================================ the mask kernel
@pytest.mark.parametrize("off", [0, 4097, B33 - 2500, B33 - 2501, 2 ** 40 + 1])
def test_dropout_mask_equals_restatement(K, off):
    n = 5000
    for p in (1e-6, 0.1, 0.25, 0.5, 0.999):        # 1e-6: the threshold clamps to 1
        for seed in (0, 77, 2 ** 63 - 1):
            m = K.dropout_mask(n, p, seed, off, "cuda")
            assert torch.equal(m.bool(), ref_keep(seed, off, (n,), p)), (p, seed, off)
            assert int(m.max()) <= 1


# ============================================================================ elementwise kernels
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("R,D", [(37, 96), (5, 768)])
def test_dropout_fwd(K, R, D, inplace, where):
    """mms2ut_dropout_fwd: half(float(x) * float32(1 / (1 - p))) where kept, exactly 0 where dropped.
    2^33 lands in row R // 2 (18 / 2), column D // 2 or D // 2 + 1."""
    p, seed, off = 0.1, SEED[where], site_offset(where, R, D)
    x = _away_from_zero((R, D), _gen(R))
    keep = ref_keep(seed, off, (R, D), p)
    ref = torch.where(keep, (x.float() * ds32(p)).half(), torch.zeros_like(x))
    x0 = x.clone()
    y = K.dropout(x, p, (seed, off)) if inplace else K.dropout(x, p, (seed, off), out=torch.empty_like(x))
    torch.cuda.synchronize()
    assert torch.equal(y != 0, keep)
    assert torch.equal(y, ref)
    if inplace:
        assert y.data_ptr() == x.data_ptr()
    else:
        assert torch.equal(x, x0)


_P_WHERE = [(0.0, "even")] + [(0.1, w) for w in WHERE]


def _check_embed(x, ref64, keep, p):
    """Kept values within one fp16 ulp of the fp64 reference rounded to fp16 (the kernels may contract
    scale * h + pos into an FMA), dropped ones exactly 0."""
    if p > 0:
        assert torch.equal(x != 0, keep)
        ref64 = ref64 / (1.0 - float(np.float32(p)))
        assert ulps16(x[keep], ref64.half()[keep]) <= 1
    else:
        assert ulps16(x, ref64.half()) <= 1


@pytest.mark.parametrize("p,where", _P_WHERE)
@pytest.mark.parametrize("D", [96, 768])
def test_encoder_embed_fwd(K, D, p, where):
    """mms2ut_encoder_embed_fwd: rows past the length take position row 1, row t takes t + 2.  The
    site is 33 rows of D counters: 2^33 lands in row 16 (b = 1, t = 5).  h and the position table
    share each column's sign, so scale * h + pos never cancels and one ulp covers the fp32 kernel."""
    B, T, lens = 3, 11, [11, 6, 1]
    g = _gen(D)
    sgn = _col_sign(D, g)
    h = _away_from_zero((B * T, D), g, 0.05, 1.0, sgn)
    pos = _away_from_zero((T + 2, D), g, 0.05, 1.0, sgn)
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    scale = float(np.float32(math.sqrt(D)))
    seed, off = SEED[where], site_offset(where, B * T, D)
    x = K.encoder_embed(h, pos, lens_t, B, T, D, scale, p, (seed, off))
    torch.cuda.synchronize()
    t = torch.arange(T, device="cuda")
    pidx = torch.where(t[None, :] < lens_t[:, None].long(), t[None, :] + 2, torch.ones_like(t)[None, :]).reshape(-1)
    ref64 = scale * h.double() + pos.double()[pidx]
    _check_embed(x, ref64, ref_keep(seed, off, (B * T, D), p) if p > 0 else None, p)


@pytest.mark.parametrize("p,where", _P_WHERE)
@pytest.mark.parametrize("D", [96, 768])
def test_scale_dropout_bwd(K, D, p, where):
    """mms2ut_scale_dropout_bwd on the encoder-embed shapes (33 rows of D; 2^33 in row 16)."""
    R = 33
    dx = _away_from_zero((R, D), _gen(D + 1), 0.05, 1.0)
    scale = float(np.float32(math.sqrt(D)))
    seed, off = SEED[where], site_offset(where, R, D)
    dh = K.scale_dropout_bwd(dx, scale, p, (seed, off))
    torch.cuda.synchronize()
    _check_embed(dh, dx.double() * scale, ref_keep(seed, off, (R, D), p) if p > 0 else None, p)


def _tokens(B, T, V, pad, g):
    """Token rows with pads inside and at the end (row 1 also starts with one, and has pads on both
    sides of position 64 where the count loop's second trip begins); row 2 has none."""
    tok = torch.randint(2, V, (B, T), generator=g, device="cuda")
    assert pad < 2
    tok[0, [5, 6, 30]] = pad
    tok[0, T - 4:] = pad
    tok[1, [0, 63, 64, 65]] = pad
    tok[1, T - 2:] = pad
    return tok


@pytest.mark.parametrize("p,where", _P_WHERE)
@pytest.mark.parametrize("D", [96, 768])
def test_token_embed_fwd(K, D, p, where):
    """mms2ut_token_embed_fwd: positions are cumsum(non-pad) + pad, pad rows take position `pad`.
    T = 70: the wave-strided count loop takes a second trip.  210 rows of D counters: 2^33 lands in
    row 105 (b = 1, t = 35)."""
    B, T, V, pad = 3, 70, 40, 1
    g = _gen(D + 2)
    tok = _tokens(B, T, V, pad, g)
    sgn = _col_sign(D, g)
    E = _away_from_zero((V, D), g, 0.05, 1.0, sgn)
    pos = _away_from_zero((T + pad + 1, D), g, 0.05, 1.0, sgn)
    scale = float(np.float32(math.sqrt(D)))
    seed, off = SEED[where], site_offset(where, B * T, D)
    x = K.token_embed(tok, E, pos, B, T, D, pad, scale, p, (seed, off))
    torch.cuda.synchronize()
    nonpad = (tok != pad).long()
    pidx = (torch.cumsum(nonpad, 1) * nonpad + pad).reshape(-1)
    assert pidx.max().item() == T + pad and (pidx == pad).sum().item() == 13
    ref64 = scale * E.double()[tok.reshape(-1)] + pos.double()[pidx]
    _check_embed(x, ref64, ref_keep(seed, off, (B * T, D), p) if p > 0 else None, p)


@pytest.mark.parametrize("where", WHERE)
def test_token_embed_bwd(K, where):
    """token_embed_bwd against index_add of the scaled, masked rows (the bound of
    test_token_embed_bwd); 150 rows of 256 counters, 2^33 in row 75."""
    B, T, D, V, p, pad = 3, 50, 256, 40, 0.1, 1
    g = _gen(7)
    tok = torch.randint(0, V, (B, T), generator=g, device="cuda")
    tok[:, -T // 5:] = pad
    dx = torch.randn(B * T, D, generator=g, device="cuda").half()
    scale = math.sqrt(D)
    seed, off = SEED[where], site_offset(where, B * T, D)
    dE = torch.zeros(V, D, device="cuda")
    K.token_embed_bwd(tok, dx, dE, B, T, D, pad, scale, p, (seed, off))
    torch.cuda.synchronize()
    keep = ref_keep(seed, off, (B * T, D), p)
    x = torch.where(keep, dx.double() * scale / (1 - p), torch.zeros_like(dx, dtype=torch.float64))
    ref = torch.zeros(V, D, device="cuda", dtype=torch.float64).index_add_(0, tok.reshape(-1), x)
    ref[pad] = 0
    assert rel(dE, ref) < 1e-5
    assert torch.equal(dE[pad], torch.zeros_like(dE[pad]))


# ============================================================================ LayerNorm
def _ln_inputs(R, D, seed):
    g_ = _gen(seed)
    x = (2 * torch.randn(R, D, generator=g_, device="cuda") + 0.5).half()
    g = (1 + 0.1 * torch.randn(D, generator=g_, device="cuda")).half()
    b = (0.1 * torch.randn(D, generator=g_, device="cuda")).half()
    return x, g, b, g_


def _dropped(y, keep, p):
    """What a dropout pass over the fp16 tensor y stores."""
    return torch.where(keep, (y.float() * ds32(p)).half(), torch.zeros_like(y))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("D", [768, 96])
def test_layernorm_fwd_dropout(K, D, grouped, where):
    """layernorm(..., p, drop) on the 16-B kernels (D = 768) and the one-wave kernels (D = 96):
    bit-identical to the undropped kernel output times the restated mask, with the counters of the
    unpadded element index; 37 rows, grouped = rows of 10 written 11 apart (the pad rows stay
    untouched).  2^33 lands in row 18."""
    R, p, grp, grp_out = 37, 0.1, 10, 11
    x, g, b, _ = _ln_inputs(R, D, D)
    seed, off = SEED[where], site_offset(where, R, D)
    y0, m0, r0 = K.layernorm(x, g, b)
    want = _dropped(y0, ref_keep(seed, off, (R, D), p), p)
    if grouped:
        out = torch.full((4 * grp_out, D), 7.0, dtype=torch.float16, device="cuda")
        ref = out.clone()
        r = torch.arange(R, device="cuda")
        ref[(r // grp) * grp_out + r % grp] = want
        _, m1, r1 = K.layernorm(x, g, b, out=out, grp=grp, grp_out=grp_out, p=p, drop=(seed, off))
    else:
        out = torch.full((R, D), 7.0, dtype=torch.float16, device="cuda")
        ref = want
        _, m1, r1 = K.layernorm(x, g, b, out=out, p=p, drop=(seed, off))
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(m0, m1) and torch.equal(r0, r1)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("D", [768, 96])
def test_layernorm_bwd_emit(K, D, where):
    """layernorm_bwd(emit=(p, drop)): dxd == dropout(dx) with the restated mask, in the exact form of
    test_layernorm_fwd_bwd (its allowance for the fp16 underflow edge included); 37 rows, 2^33 in
    row 18."""
    R, p = 37, 0.1
    x, g, b, g_ = _ln_inputs(R, D, D + 1)
    _, mean, rstd = K.layernorm(x, g, b)
    dy = torch.randn(R, D, generator=g_, device="cuda").half()
    dres = torch.randn(R, D, generator=g_, device="cuda").half()
    dgb = torch.empty(2 * D, dtype=torch.float16, device="cuda")
    seed, off = SEED[where], site_offset(where, R, D)
    dx = K.layernorm_bwd(dy, x, g, mean, rstd, dgb, dres=dres)
    dx2, dxd = K.layernorm_bwd(dy, x, g, mean, rstd, dgb, dres=dres, emit=(p, (seed, off)))
    torch.cuda.synchronize()
    keep = ref_keep(seed, off, (R, D), p)
    assert torch.equal(dx2, dx)
    ref = torch.where(keep, dx.float() / (1 - p), torch.zeros_like(dx.float()))
    assert (dxd.float() - ref).abs().max().item() <= 2e-3 * ref.abs().max().item() + 1e-3
    mism = (dxd == 0) != (~keep | (dx == 0))
    assert (dx.float().abs()[mism] < 1e-6).all() and (dxd.float().abs()[mism] < 1e-6).all()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("D", [768, 256])
def test_layernorm_bwd_input_dropout(K, D, grouped, where):
    """layernorm_bwd(dy_p, dy_drop): the gradient read through the forward's padded layout and
    dropout is bit-identical to the backward of the gathered, separately dropped gradient (dx and
    gamma / beta grads).  This path exists for D % 256 == 0 only (the library rejects others), so
    both D take the 16-B kernel: 3 and 1 quads per lane.  37 rows, 2^33 in row 18."""
    R, p, grp, grp_out = 37, 0.1, 10, 11
    x, g, b, g_ = _ln_inputs(R, D, D + 2)
    _, mean, rstd = K.layernorm(x, g, b)
    Rout = 4 * grp_out if grouped else R
    dyp = torch.randn(Rout, D, generator=g_, device="cuda").half()
    dres = torch.randn(R, D, generator=g_, device="cuda").half()
    seed, off = SEED[where], site_offset(where, R, D)
    r = torch.arange(R, device="cuda")
    rows = (r // grp) * grp_out + r % grp if grouped else r
    dy = _dropped(dyp[rows].contiguous(), ref_keep(seed, off, (R, D), p), p)
    dgb0, dgb1 = (torch.empty(2 * D, dtype=torch.float16, device="cuda") for _ in range(2))
    dx0 = K.layernorm_bwd(dy, x, g, mean, rstd, dgb0, dres=dres)
    dx1 = K.layernorm_bwd(dyp, x, g, mean, rstd, dgb1, dres=dres, dy_grp=grp if grouped else 0,
                          dy_grp_out=grp_out if grouped else 0, dy_p=p, dy_drop=(seed, off))
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    assert torch.equal(dgb0, dgb1)


# ============================================================================ attention softmax
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("Tk", [30, 101])
def test_attn_softmax_dropout(K, Tk, extra, where):
    """Softmax forward / backward with dropout, Z = 5, Tq = 37 (185 rows of Tk counters: 2^33 lands in
    row 92 = (z 2, q 18)); extra: image key masks with the bias_kv column kept."""
    Z, Tq, p = 5, 37, 0.1
    ldS = (Tk + 7) // 8 * 8
    g = _gen(Tk)
    S = torch.randn(Z * Tq * ldS, device="cuda", generator=g).half()
    km = None
    if extra:
        km = torch.zeros(Z, ldS, dtype=torch.uint8, device="cuda")
        for z in range(Z):
            km[z, max(1, (Tk - 1) * (z + 1) // (Z + 1)):Tk - 1] = 1
    seed, off = SEED[where], site_offset(where, Z * Tq, Tk)
    P, Pd = K.attn_softmax(S, Z, 1, Tq, Tk, ldS, key_mask=km, extra_key=extra, p=p, drop=(seed, off))
    s = S.view(Z, Tq, ldS)[..., :Tk].double()
    valid = torch.ones(Z, Tq, Tk, dtype=torch.bool, device="cuda")
    if km is not None:
        valid = ~km[:, None, :Tk].bool().expand(Z, Tq, Tk)
        s = s.masked_fill(~valid, float("-inf"))
    sf = s.clone().requires_grad_(True)
    pr = torch.softmax(sf, -1)
    keep = ref_keep(seed, off, (Z, Tq, Tk), p)
    m = keep.double()
    Pv, Pdv = P.view(Z, Tq, ldS)[..., :Tk], Pd.view(Z, Tq, ldS)[..., :Tk]
    torch.cuda.synchronize()
    assert rel(Pv, pr) < 2e-3
    assert rel(Pdv, pr * m / (1 - p)) < 2e-3
    assert (Pv[valid] != 0).all()
    assert torch.equal((Pdv != 0)[valid], keep[valid])     # the zero pattern over unmasked keys
    dPd = torch.randn(Z * Tq * ldS, device="cuda", generator=g).half()
    (pr * m / (1 - p)).backward(dPd.view(Z, Tq, ldS)[..., :Tk].double())
    dS = K.attn_softmax_bwd(P, dPd.clone(), Z, 1, Tq, Tk, ldS, p=p, drop=(seed, off))
    torch.cuda.synchronize()
    assert rel(dS.view(Z, Tq, ldS)[..., :Tk], sf.grad.nan_to_num(0.0)) < 3e-3


# ============================================================================ flash attention
def flash_ref(q, k, v, do, lens, scale, mask):
    """o, dq, dk, dv of softmax(scale q k^T, keys < len) * mask @ v in fp64 ([B, H, T, hd] operands,
    mask = keep / (1 - p)), as tests/test_gpu_kernels.py _attn_ref builds it."""
    q, k, v = (t.double().detach().requires_grad_(True) for t in (q, k, v))
    s = scale * q @ k.transpose(-1, -2)
    j = torch.arange(s.shape[-1], device=s.device)
    bad = j[None, None, None, :] >= lens.long()[:, None, None, None]
    o = (torch.softmax(s.masked_fill(bad, float("-inf")), -1) * mask.double()) @ v
    o.backward(do.double())
    return o.detach(), q.grad, k.grad, v.grad


def head_err(a, b):
    """Relative L2 error of each head: [B, H]."""
    a, b = a.double(), b.double()
    return (a - b).flatten(2).norm(dim=-1) / (b.flatten(2).norm(dim=-1) + 1e-12)


def flash_offset(where, B, H, Tq, Tk):
    """First counter of an attention call; the straddling forms put 2^33 in head z = 2 of 6 or 144 of
    288 (both in batch row 1), row Tq // 2, column Tk // 2 or Tk // 2 + 1."""
    z = 2 if B * H == 6 else (B * H) // 2
    return z, site_offset(where, Tq, Tk, before=z * Tq * Tk)


def flash_inputs(B, H, Tq, Tk, hd, dev, seed=5):
    g = torch.Generator(device=dev).manual_seed(seed)
    d = H * hd
    q = torch.randn(B * Tq, d, generator=g, device=dev).half()
    kv = torch.randn(B * Tk, 2 * d, generator=g, device=dev).half()
    do = torch.randn(B * Tq, d, generator=g, device=dev).half()
    return q, kv, do


def heads(x, B, T, H, hd):
    return x.view(B, T, H, hd).transpose(1, 2)


def flash_sensitivity(B, H, Tq, Tk, hd, p, z, lens, q, kv, do, keep):
    """On the reference alone: flipping one keep flag of head z (its middle row, the most probable
    valid key) moves that head's o, dq, dk, dv by more than the bounds they are compared under."""
    d = H * hd
    b, h = z // H, z % H
    sl = lambda x, T: heads(x, B, T, H, hd)[b:b + 1, h:h + 1]
    qh, kh, vh, doh = sl(q, Tq), sl(kv[:, :d], Tk), sl(kv[:, d:], Tk), sl(do, Tq)
    row = Tq // 2
    s = (qh.double() @ kh.double().transpose(-1, -2))[0, 0, row, :int(lens[b])]
    key = int(s.argmax())
    k1 = keep[b:b + 1, h:h + 1].clone()
    k2 = k1.clone()
    k2[0, 0, row, key] = ~k2[0, 0, row, key]
    r1 = flash_ref(qh, kh, vh, doh, lens[b:b + 1], hd ** -0.5, k1.double() / (1 - p))
    r2 = flash_ref(qh, kh, vh, doh, lens[b:b + 1], hd ** -0.5, k2.double() / (1 - p))
    return [head_err(x, y).item() for x, y in zip(r2, r1)]


_FLASH_SHAPES = [(40, 64, 2),      # even / even: the hi_pairs path, fused backward
                 (33, 63, 2),      # odd Tk: no pairs
                 (40, 264, 2),     # Tk > 256: the three-kernel backward
                 (40, 64, 96)]     # 288 heads: persistent blocks walk several heads (next-head prefetch)
_FLASH_BOUNDS = (3e-3, 5e-3, 5e-3, 5e-3)    # o, dq, dk, dv (test_flash_attention_fwd_bwd)


def _flash_general_inputs(B, H, Tq, Tk, hd, dev):
    """Random q / k / v / dO with ragged key lengths; the middle query row of every head carries a 4x
    larger dO (the row whose keep flag the sensitivity check flips)."""
    q, kv, do = flash_inputs(B, H, Tq, Tk, hd, dev)
    do.view(B, Tq, H * hd)[:, Tq // 2] *= 4
    lens = torch.tensor([Tk, Tk - 5, Tk // 2], dtype=torch.int32, device=dev)
    return q, kv, do, lens


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("Tq,Tk,H", _FLASH_SHAPES)
def test_flash_mask_readout(K, Tq, Tk, H, where):
    """The masks the flash kernels generate, read out exactly.  V = identity per head makes
    O[q, k] = Pd[q, k] (Tk <= hd), dO[q, :] = onehot(q) makes dV[k, q] = Pd[q, k] (Tq <= hd, every
    shape here): the zero patterns of O and dV are the forward's and the backward's keep flags."""
    B, hd, p = 3, 64, 0.2
    d = H * hd
    z, off = flash_offset(where, B, H, Tq, Tk)
    seed = SEED[where]
    q, kv, _ = flash_inputs(B, H, Tq, Tk, hd, "cuda")
    q = (0.5 * q.float()).half()      # scores ~ N(0, 1/4): no probability near the fp16 underflow edge
    if Tk <= hd:
        kv[:, d:] = torch.eye(Tk, hd, device="cuda").half()[None, :, None, :].expand(B, Tk, H, hd).reshape(B * Tk, d)
    do = torch.eye(Tq, hd, device="cuda").half()[None, :, None, :].expand(B, Tq, H, hd).reshape(B * Tq, d).contiguous()
    lens_t = torch.full((B,), Tk, dtype=torch.int32, device="cuda")
    o = torch.empty(B * Tq, d, dtype=torch.float16, device="cuda")
    lse = K.mha_fwd(q, kv, kv[:, d:], o, d, 2 * d, 2 * d, d, B, H, Tq, Tk, hd, hd ** -0.5, key_len=lens_t,
                    p=p, drop=(seed, off))
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    K.mha_bwd(q, kv, kv[:, d:], o, d, 2 * d, 2 * d, d, B, H, Tq, Tk, hd, hd ** -0.5, lens_t, False, p,
              (seed, off), lse, do, d, dq, d, dkv, 2 * d, dkv[:, d:], 2 * d)
    torch.cuda.synchronize()
    keep = ref_keep(seed, off, (B, H, Tq, Tk), p)
    if Tk <= hd:
        fwd = heads(o, B, Tq, H, hd)[..., :Tk] != 0                        # [B, H, Tq, Tk]
        bad = (fwd != keep).flatten(2).any(-1).nonzero().tolist()
        assert not bad, f"forward mask differs in heads (b, h) {bad[:8]}; 2^33 is in z = {z}"
    bwd = (heads(dkv[:, d:], B, Tk, H, hd)[..., :Tq] != 0).transpose(-1, -2)   # [B, H, Tq, Tk]
    bad = (bwd != keep).flatten(2).any(-1).nonzero().tolist()
    assert not bad, f"backward mask differs in heads (b, h) {bad[:8]}; 2^33 is in z = {z}"


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("Tq,Tk,H", _FLASH_SHAPES)
def test_flash_values_per_head(K, Tq, Tk, H, where):
    """o, dq, dk, dv of every head (not of the whole batch: one wrong head must not be diluted by the
    right ones) against the fp64 reference with the restated mask, ragged key lengths, under the
    bounds of test_flash_attention_fwd_bwd."""
    B, hd, p = 3, 64, 0.2
    d = H * hd
    z, off = flash_offset(where, B, H, Tq, Tk)
    seed = SEED[where]
    q, kv, do, lens_t = _flash_general_inputs(B, H, Tq, Tk, hd, "cuda")
    o = torch.empty(B * Tq, d, dtype=torch.float16, device="cuda")
    lse = K.mha_fwd(q, kv, kv[:, d:], o, d, 2 * d, 2 * d, d, B, H, Tq, Tk, hd, hd ** -0.5, key_len=lens_t,
                    p=p, drop=(seed, off))
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    K.mha_bwd(q, kv, kv[:, d:], o, d, 2 * d, 2 * d, d, B, H, Tq, Tk, hd, hd ** -0.5, lens_t, False, p,
              (seed, off), lse, do, d, dq, d, dkv, 2 * d, dkv[:, d:], 2 * d)
    torch.cuda.synchronize()
    keep = ref_keep(seed, off, (B, H, Tq, Tk), p)
    ref = flash_ref(heads(q, B, Tq, H, hd), heads(kv[:, :d], B, Tk, H, hd), heads(kv[:, d:], B, Tk, H, hd),
                    heads(do, B, Tq, H, hd), lens_t, hd ** -0.5, keep.double() / (1 - p))
    got = (heads(o, B, Tq, H, hd), heads(dq, B, Tq, H, hd), heads(dkv[:, :d], B, Tk, H, hd),
           heads(dkv[:, d:], B, Tk, H, hd))
    sens = flash_sensitivity(B, H, Tq, Tk, hd, p, z, lens_t, q, kv, do, keep)
    for name, a, r, bound, sn in zip(("o", "dq", "dk", "dv"), got, ref, _FLASH_BOUNDS, sens):
        e = head_err(a, r)
        w = int(e.argmax())
        assert sn > bound, f"{name}: one flipped keep flag moves head {z} by only {sn:.2e}"
        assert e.max().item() < bound, (f"{name}: worst head z = {w} err {e.flatten()[w].item():.2e}; head {z} (2^33 "
                                        f"inside when straddling) err {e.flatten()[z].item():.2e}")


# ============================================================================ GEMM epilogues
@pytest.mark.parametrize("where", WHERE)
def test_gemm_dropout_masks_restated(K, where):
    """test_gemm_dropout_masks_every_tile's (333, 520, 256) case with the mask from rng_ref: ties the
    GEMM epilogue masks to the pinned stream.  333 rows of 520 counters, 2^33 in row 166."""
    M, N, Kd, p = 333, 520, 256, 0.1
    g = _gen(3)
    x = (0.1 * torch.randn(M, Kd, device="cuda", generator=g)).half()
    W = (0.05 * torch.randn(N, Kd, device="cuda", generator=g)).half()
    big = torch.full((N,), 30.0, device="cuda").half()
    zero = torch.zeros(M, N, device="cuda").half()
    z = torch.empty(M, N, device="cuda").half()
    seed, off = SEED[where], site_offset(where, M, N)
    m = ref_keep(seed, off, (M, N), p)
    try:
        for mode in (0, 2, 3, 5):
            K.call("mms2ut_gemm_set_tall", mode)
            for epi, kw in ((K.EPI_RELU_DROP, {}), (K.EPI_DROP_RESID, dict(aux=zero)),
                            (K.EPI_GELU_DROP, dict(out2=z))):
                y = K.linear(x, W, big, epi=epi, p=p, drop=(seed, off), **kw)
                assert torch.equal(y != 0, m), (mode, epi)
    finally:
        K.call("mms2ut_gemm_set_tall", 1)


# ============================================================================ step-seed delta
def test_step_seed_delta(K):
    """With a device delta bound and advanced once by a known increment, dropout_fwd and attn_softmax
    draw from seed + delta (mod 2^64) of the restated stream; unbound, from the seed again."""
    inc, seed, off, p = 0x9E3779B97F4A7C15, 77, 4097, 0.1
    R, D, Z, Tq, Tk, ldS = 37, 96, 5, 37, 30, 32
    x = _away_from_zero((R, D), _gen(11))
    S = torch.randn(Z * Tq * ldS, device="cuda", generator=_gen(12)).half()
    delta = torch.zeros(1, dtype=torch.int64, device="cuda")
    try:
        K.bind_step_seed(delta)
        K.step_seed_advance(delta, inc)
        y = K.dropout(x, p, (seed, off), out=torch.empty_like(x))
        P, Pd = K.attn_softmax(S, Z, 1, Tq, Tk, ldS, p=p, drop=(seed, off))
        torch.cuda.synchronize()
    finally:
        K.bind_step_seed(None)
    assert delta.item() == inc - 2 ** 64          # the increment, read back as a signed 64-bit value
    eff = (seed + inc) % 2 ** 64
    assert torch.equal(y != 0, ref_keep(eff, off, (R, D), p))
    Pv, Pdv = P.view(Z, Tq, ldS)[..., :Tk], Pd.view(Z, Tq, ldS)[..., :Tk]
    assert (Pv != 0).all() and torch.equal(Pdv != 0, ref_keep(eff, off, (Z, Tq, Tk), p))
    y = K.dropout(x, p, (seed, off), out=torch.empty_like(x))
    torch.cuda.synchronize()
    assert torch.equal(y != 0, ref_keep(seed, off, (R, D), p))

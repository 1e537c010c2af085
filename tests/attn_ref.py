"""References and buffers for the flash-attention path tests (tests/test_gpu_attention_paths.py,
CPU self-checks in tests/test_attn_ref.py).  Nothing here calls the library.

* ``ref64``: forward and backward per head in fp64 from the fp16 inputs: masked softmax with key
  lengths and the causal mask (key <= query, both counted from 0), dropout keep flags restated with
  tests/rng_ref.py at counter offset + (z*Tq + q)*Tk + key.  A row without a valid key has o = 0,
  lse = -inf and adds nothing to any gradient.
* ``emulate``: the same math in fp32, rounding to fp16 where the kernels round: the exponentials of a
  64-key tile (relative to the running row maximum) before P.V, the dropped probabilities and dS
  before the dK / dV / dQ products, and the outputs.  Its distance from ``ref64`` sizes tolerances;
  it never sees the code under test.
* ``row_err``: per head, the largest ||got_row - ref_row|| over the head's RMS ||ref_row||.  A head whose
  exact result is zero everywhere (one valid key: dQ = dK = 0) is measured against the tensor's RMS.
* ``Padded``: a logical [B, T, W] fp16 tensor inside a sentinel-filled allocation with a given row
  stride, batch stride and slack; ``check()`` asserts that nothing outside the region changed."""
import math

import numpy as np
import torch

import rng_ref

SENTINEL = 0x7E5A          # an fp16 NaN: a stray read that reaches a result poisons it
KB = 64                    # keys per tile of the kernels' online softmax
MARGIN = 4.0


# ---------------------------------------------------------------------------- dropout flags
def keep_flags(seed, offset, B, H, Tq, Tk, p):
    """bool [B, H, Tq, Tk] (CPU), or None for p == 0."""
    if p <= 0:
        return None
    return torch.from_numpy(rng_ref.keep(seed, offset, B * H * Tq * Tk, p)).view(B, H, Tq, Tk)


def drop_scale(p):
    """The kernels' 1.f / (1.f - p) in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def valid_mask(lens, Tq, Tk, causal, B):
    """bool [B, 1, Tq, Tk]: key < min(len, Tk) and, causal, key <= query.  lens None: every key."""
    key = torch.arange(Tk)
    m = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if lens is not None:
        L = torch.as_tensor(lens, dtype=torch.int64).clamp(max=Tk).view(B, 1, 1, 1)
        m = m & (key.view(1, 1, 1, Tk) < L)
    if causal:
        m = m & (key.view(1, 1, 1, Tk) <= torch.arange(Tq).view(1, 1, Tq, 1))
    return m


# ---------------------------------------------------------------------------- fp64 reference
def ref64(q, k, v, do, lens, causal, scale, keep=None, p=0.0):
    """q, do [B, H, Tq, hd]; k, v [B, H, Tk, hd] (any float dtype, CPU).  -> dict of fp64 tensors
    o, lse [B, H, Tq], dq, dk, dv."""
    q, k, v, do = (t.detach().cpu().double() for t in (q, k, v, do))
    B, H, Tq, _ = q.shape
    Tk = k.shape[2]
    ok = valid_mask(lens, Tq, Tk, causal, B)
    s = (q @ k.transpose(-1, -2)) * scale
    s = torch.where(ok, s, torch.full_like(s, -math.inf))
    m = s.amax(-1, keepdim=True)
    msafe = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.where(ok, torch.exp(s - msafe), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    P = torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))
    lse = torch.where(l > 0, msafe + torch.log(torch.where(l > 0, l, torch.ones_like(l))),
                      torch.full_like(l, -math.inf)).squeeze(-1)
    mk = torch.ones_like(P) if keep is None else keep.double() * drop_scale(p)
    Pd = P * mk
    o = Pd @ v
    dP = (do @ v.transpose(-1, -2)) * mk
    D = (dP * P).sum(-1, keepdim=True)
    dS = P * (dP - D)
    return {"o": o, "lse": lse, "dq": scale * (dS @ k), "dk": scale * (dS.transpose(-1, -2) @ q),
            "dv": Pd.transpose(-1, -2) @ do}


# ---------------------------------------------------------------------------- emulated reference
def _r16(x):
    return x.half().float()


def emulate(q, k, v, do, lens, causal, scale, keep=None, p=0.0):
    """ref64's results as fp32 arithmetic with the kernels' fp16 rounding points would give them."""
    q, k, v, do = (t.detach().cpu().half().float() for t in (q, k, v, do))
    B, H, Tq, hd = q.shape
    Tk = k.shape[2]
    ok = valid_mask(lens, Tq, Tk, causal, B).expand(B, H, Tq, Tk)
    kp = torch.ones(B, H, Tq, Tk, dtype=torch.bool) if keep is None else keep
    ds = drop_scale(p) if keep is not None else 1.0
    s = q @ k.transpose(-1, -2)                       # unscaled, as the kernels keep them
    ninf = torch.full_like(s, -math.inf)
    sm = torch.where(ok, s, ninf)
    m = torch.full((B, H, Tq, 1), -math.inf)
    l = torch.zeros(B, H, Tq, 1)
    o = torch.zeros(B, H, Tq, hd)
    for kb in range(0, Tk, KB):
        st = sm[..., kb:kb + KB]
        mn = torch.maximum(m, st.amax(-1, keepdim=True))
        dead = torch.isinf(mn)
        mz = torch.where(dead, torch.zeros_like(mn), mn)
        alpha = torch.where(dead, torch.ones_like(mn), torch.exp((torch.where(dead, mz, m) - mz) * scale))
        e = torch.exp((st - mz) * scale)               # exp(-inf) = 0 on masked keys
        l = l * alpha + e.sum(-1, keepdim=True)
        pt = _r16(torch.where(kp[..., kb:kb + KB], e, torch.zeros_like(e)))
        o = o * alpha + pt @ v[:, :, kb:kb + KB]
        m = mn
    live = l > 0
    lsafe = torch.where(live, l, torch.ones_like(l))
    o = _r16(torch.where(live, o * (ds / lsafe), torch.zeros_like(o)))
    lse = torch.where(live, torch.where(live, m, torch.zeros_like(m)) * scale + torch.log(lsafe),
                      torch.full_like(l, -math.inf))
    lz = torch.where(live, lse, torch.zeros_like(lse))
    pr = torch.where(ok & live, torch.exp(s * scale - lz), torch.zeros_like(s))
    mk = kp.float() * ds
    Pd = _r16(pr * mk)
    D = (o * do).sum(-1, keepdim=True)
    dS = _r16(pr * ((do @ v.transpose(-1, -2)) * mk - D))
    return {"o": o.double(), "lse": lse.squeeze(-1).double(),
            "dq": _r16(scale * (dS @ k)).double(),
            "dk": _r16(scale * (dS.transpose(-1, -2) @ q)).double(),
            "dv": _r16(Pd.transpose(-1, -2) @ do).double()}


# ---------------------------------------------------------------------------- error measures
def _finite(ref):
    return torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref))


def _or_whole(per_head, whole):
    """per_head [B, H] where it is positive, else the whole tensor's figure: a head whose exact result
    is zero everywhere (a single valid key makes dS, so dQ and dK, cancel to zero) has no scale of
    its own, and what the kernels leave there is rounding noise of the tensor's scale."""
    return torch.where(per_head > 0, per_head, torch.full_like(per_head, float(whole)))


def frob_per_head(got, ref):
    """[B, H] Frobenius ratio per head; a head with an all-zero reference is measured against the
    whole tensor's norm per head.  inf where there is no scale at all but an error."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if got.dim() == 3:
        got, ref = got.unsqueeze(-1), ref.unsqueeze(-1)
    fin = torch.isfinite(ref)
    d = torch.where(fin, got - ref, torch.zeros_like(ref)).flatten(2).norm(dim=-1)
    n = _finite(ref).flatten(2).norm(dim=-1)
    n = _or_whole(n, _finite(ref).norm() / math.sqrt(n.numel()))
    return torch.where(n > 0, d / torch.where(n > 0, n, torch.ones_like(n)),
                       torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))


def head_rms(ref):
    """[B, H]: RMS over a head's rows of ||ref_row|| (finite rows only); for a head whose reference
    is all zero, the same over every row of the tensor."""
    ref = ref.detach().cpu().double()
    if ref.dim() == 3:
        ref = ref.unsqueeze(-1)
    fin = torch.isfinite(ref).all(-1)
    n2 = torch.where(fin, (_finite(ref) ** 2).sum(-1), torch.zeros_like(fin, dtype=torch.float64))
    rms = (n2.sum(-1) / fin.sum(-1).clamp(min=1)).sqrt()
    return _or_whole(rms, (n2.sum() / fin.sum().clamp(min=1)).sqrt())


def row_err(got, ref):
    """Per output row ||got_row - ref_row|| / head_rms(ref), reduced per head.
    got, ref [B, H, T, hd] (or [B, H, T]: rows of one element).  Rows whose reference is not finite
    (lse = -inf) must match exactly, or the error is inf; so is a NaN.
    -> (err [B, H] of the worst row, row [B, H] its index)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if got.dim() == 3:
        got, ref = got.unsqueeze(-1), ref.unsqueeze(-1)
    fin = torch.isfinite(ref)
    d = torch.where(fin, got - ref, torch.where(got == ref, torch.zeros_like(ref), torch.full_like(ref, math.inf)))
    d = torch.nan_to_num(d, nan=math.inf, posinf=math.inf, neginf=math.inf)
    dn = d.norm(dim=-1)                                  # [B, H, T]
    rms = head_rms(ref).unsqueeze(-1)
    e = torch.where(rms > 0, dn / torch.where(rms > 0, rms, torch.ones_like(rms)),
                    torch.where(dn > 0, torch.full_like(dn, math.inf), torch.zeros_like(dn)))
    err, row = e.max(-1)
    return err, row


def ulp16_rel(rms):
    """One fp16 ulp of each value of ``rms`` relative to it (0 where rms == 0)."""
    rms = rms.double()
    pos = rms > 0
    x = torch.where(pos, rms, torch.ones_like(rms)).clamp(min=2.0 ** -14)
    ulp = torch.exp2(torch.floor(torch.log2(x)) - 10)
    return torch.where(pos, ulp / torch.where(pos, rms, torch.ones_like(rms)), torch.zeros_like(rms))


def worst(err, row):
    """(value, 'b=.. h=.. row=..') of the largest entry of a row_err result."""
    i = int(err.flatten().argmax())
    b, h = divmod(i, err.shape[1])
    return float(err[b, h]), f"b={b} h={h} row={int(row[b, h])}"


# ---------------------------------------------------------------------------- padded buffers
def split_heads(x, H):
    """[B, T, H*hd] -> [B, H, T, hd]"""
    B, T, W = x.shape
    return x.reshape(B, T, H, W // H).transpose(1, 2)


class Padded:
    """A logical [B, T, W] fp16 tensor at element (b, t, c) -> front + b*sb + t*ld_row + c of one flat
    allocation whose every element starts as SENTINEL.

    layout "bm" (batch-major): row stride ``ld``, batch stride (T + gap_rows) * ld.
    layout "tm" (time-major):  row stride B * ld, batch stride ld.
    ``front`` / ``tail`` guard elements lie before and after; front is kept a multiple of 8 so the
    region's 16-byte alignment is the allocation's."""

    def __init__(self, B, T, W, ld=None, layout="bm", gap_rows=0, front=64, tail=256, device="cpu", data=None):
        ld = W if ld is None else ld
        assert ld >= W and front % 8 == 0 and layout in ("bm", "tm")
        self.B, self.T, self.W, self.ld, self.layout = B, T, W, ld, layout
        if layout == "bm":
            self.row, self.sb = ld, (T + gap_rows) * ld
        else:
            self.row, self.sb = B * ld, ld
        self.tight = layout == "bm" and gap_rows == 0       # the library's default batch stride
        span = (B - 1) * self.sb + (T - 1) * self.row + W
        self.front = front
        self.flat = torch.full((front + span + tail,), SENTINEL, dtype=torch.int16, device=device).view(torch.float16)
        self.view = torch.as_strided(self.flat, (B, T, W), (self.sb, self.row, 1), front)
        inside = torch.zeros(self.flat.numel(), dtype=torch.bool, device=device)
        torch.as_strided(inside, (B, T, W), (self.sb, self.row, 1), front).fill_(True)
        self.outside = ~inside
        if data is not None:
            self.view.copy_(data.to(device=device, dtype=torch.float16).reshape(B, T, W))

    @property
    def batch_stride(self):
        """What to pass as the batch stride: 0 (the library's default) when rows simply follow."""
        return 0 if self.tight else self.sb

    def untouched(self):
        """True iff every element outside the logical region still holds the sentinel bits."""
        return bool((self.flat.view(torch.int16)[self.outside] == SENTINEL).all())

    def check(self, name="buffer"):
        bits = self.flat.view(torch.int16)
        bad = (self.outside & (bits != SENTINEL)).nonzero().flatten()
        if bad.numel():
            i = int(bad[0]) - self.front
            raise AssertionError(f"{name}: {bad.numel()} element(s) outside the logical region were written; "
                                 f"first at flat offset {i} (row stride {self.row}, batch stride {self.sb}, "
                                 f"width {self.W})")

    def all_sentinel(self):
        return bool((self.flat.view(torch.int16) == SENTINEL).all())

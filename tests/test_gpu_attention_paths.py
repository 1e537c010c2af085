"""GPU: every dispatch path of the flash-attention launchers (csrc/attention.hip) against the fp64
reference of tests/attn_ref.py.

Each case names the path it is there for and asserts it through the host-only plan query
(K.mha_fwd_plan / K.mha_bwd_plan, the code the launchers themselves call) before anything is
compared: a refactor that reroutes a case fails it instead of emptying it.  All eight tensors live in
sentinel-filled allocations with slack behind every row, between batches and around the whole
region; after the run every element outside the logical regions must hold the sentinel bits.

Errors are measured per output row (attn_ref.row_err) and bounded, per case, output and head, by
MARGIN = 4 times the same measure of the emulated reference (fp32 with the kernels' fp16 rounding
points) against the fp64 reference, with a floor of one fp16 ulp of the head's RMS row norm.  randn
cases also keep the project's per-head Frobenius bounds (3e-3 for o, 5e-3 for the gradients)."""
import math
from dataclasses import dataclass, field

import pytest
import torch

import attn_ref as A
from conftest import pkg

pytestmark = pytest.mark.gpu

SEED, OFF = 77, 4096
FROB = {"o": 3e-3, "dq": 5e-3, "dk": 5e-3, "dv": 5e-3}
OUTS = ("o", "lse", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg().kernels


@dataclass
class Case:
    group: str
    name: str
    hd: int
    H: int
    Tq: int
    Tk: int
    fwd: tuple                      # expected (nw, short_k)
    bwd: dict                       # expected fields of the backward plan
    B: int = 3
    lens: object = "ragged"         # "ragged", None, or a list
    causal: bool = False
    p: float = 0.0
    pad_o: int = 8                  # slack columns of o / dq rows (dout rows: always 8, its loads are 16 B)
    pad_kv: int = 8                 # dk / dv row stride: d + pad_kv, or with wide_kv
    wide_kv: bool = False           # 2d + pad_kv (the packed K|V row stride plus slack)
    layout: str = "bm"              # "bm", "gap" (batch-major with 3 slack rows per batch), "tm"
    inputs: str = "randn"           # "randn", "peaked", "rising"
    same_as_full: bool = False      # results equal those of key_len = min(key_len, Tk), bit for bit
    cus: tuple = field(default=None)  # persistent cases: Z = m*G + extra heads on G CUs -> (m, extra, rounds)

    @property
    def id(self):
        return f"{self.group}-{self.name}"


FUSED = lambda nkc, kv16=1: dict(fused=1, nkc=nkc, kv16=kv16, rows_prep=0)
THREE = lambda rows: dict(fused=0, nkc=0, kv16=0, rows_prep=rows)

CASES = [
    # ---- hd 128: four forward variants (+ the 16-wave short one), 3-kernel backward, both prep kernels
    Case("hd128", "20x40", 128, 2, 20, 40, (8, 1), THREE(1)),
    Case("hd128", "20x40-causal-drop", 128, 2, 20, 40, (8, 1), THREE(1), causal=True, p=0.1),
    Case("hd128", "130x129-causal", 128, 2, 130, 129, (16, 0), THREE(1), causal=True),
    Case("hd128", "130x129-drop-H1", 128, 1, 130, 129, (16, 0), THREE(0), p=0.1),
    Case("hd128", "130x100-drop", 128, 2, 130, 100, (16, 1), THREE(1), p=0.1),
    Case("hd128", "100x200-drop", 128, 2, 100, 200, (8, 0), THREE(1), p=0.1),
    Case("hd128", "100x200-causal-H3", 128, 3, 100, 200, (8, 0), THREE(0), causal=True),
    Case("hd128", "140x300-causal-drop", 128, 2, 140, 300, (16, 0), THREE(1), causal=True, p=0.1),
    Case("hd128", "140x300", 128, 2, 140, 300, (16, 0), THREE(1)),
    # ---- rows prep kernel at hd 64 / 96
    Case("rows-prep", "hd64-H4", 64, 4, 70, 257, (8, 0), THREE(1), p=0.1),
    Case("rows-prep", "hd96-H8", 96, 8, 70, 257, (8, 0), THREE(1), causal=True),
    # ---- fused backward, 8-byte dK / dV stores: lddk = lddv = 2d + 4
    Case("fused-kv8", "hd64-Tk72", 64, 2, 150, 72, (16, 1), FUSED(1, 0), p=0.1, wide_kv=True, pad_kv=4),
    Case("fused-kv8", "hd64-Tk200", 64, 2, 70, 200, (8, 0), FUSED(2, 0), causal=True, wide_kv=True, pad_kv=4),
    Case("fused-kv8", "hd96-Tk72", 96, 2, 150, 72, (16, 1), FUSED(1, 0), causal=True, p=0.1, wide_kv=True, pad_kv=4),
    Case("fused-kv8", "hd96-Tk200", 96, 2, 70, 200, (8, 0), FUSED(2, 0), wide_kv=True, pad_kv=4),
    # ---- the same with 16-byte stores: lddk = lddv = 2d + 8
    Case("fused-kv16", "hd64-Tk72", 64, 2, 150, 72, (16, 1), FUSED(1, 1), p=0.1, wide_kv=True),
    Case("fused-kv16", "hd64-Tk200", 64, 2, 70, 200, (8, 0), FUSED(2, 1), causal=True, wide_kv=True),
    Case("fused-kv16", "hd96-Tk72", 96, 2, 150, 72, (16, 1), FUSED(1, 1), causal=True, p=0.1, wide_kv=True),
    Case("fused-kv16", "hd96-Tk200", 96, 2, 70, 200, (8, 0), FUSED(2, 1), wide_kv=True),
    # ---- 3-kernel route at Tk <= 256: o (and dq) rows only 8-byte aligned, ldo = lddq = d + 4.  lddo stays a
    # multiple of 8: every backward route loads dout 16 bytes at a time and the launcher rejects less.
    Case("3k-shortTk", "Tk72", 64, 2, 70, 72, (8, 1), THREE(0), p=0.1, pad_o=4),
    Case("3k-shortTk", "Tk72-causal", 64, 2, 70, 72, (8, 1), THREE(0), causal=True, pad_o=4),
    Case("3k-shortTk", "Tk200", 96, 2, 70, 200, (8, 0), THREE(0), pad_o=4),
    Case("3k-shortTk", "Tk200-causal-H4", 64, 4, 70, 200, (8, 0), THREE(1), causal=True, p=0.1, pad_o=4),
    # ---- persistent rounds of the fused backward: Z heads on G blocks
    Case("persistent", "Z=G", 64, 0, 24, 40, (8, 1), FUSED(1), lens="per-row", p=0.1, cus=(1, 0, 1)),
    Case("persistent", "Z=G+1", 64, 0, 24, 40, (8, 1), FUSED(1), lens="per-row", cus=(1, 1, 2)),
    Case("persistent", "Z=2G", 64, 0, 24, 40, (8, 1), FUSED(1), lens="per-row", causal=True, cus=(2, 0, 2)),
    Case("persistent", "Z=2G+1", 64, 0, 24, 40, (8, 1), FUSED(1), lens="per-row", p=0.1, cus=(2, 1, 3)),
    Case("persistent", "Z=2G+G/2", 64, 0, 24, 40, (8, 1), FUSED(1), lens="per-row", causal=True, p=0.1,
         cus=(2, "half", 3)),
    # ---- key lengths: absent, past Tk (clamped), zero between two non-empty rows
    Case("key-len", "none-fused", 64, 2, 24, 72, (8, 1), FUSED(1), lens=None, same_as_full=True),
    Case("key-len", "none-3k", 64, 2, 140, 257, (16, 0), THREE(0), lens=None, p=0.1, same_as_full=True),
    Case("key-len", "past-fused", 64, 2, 24, 72, (8, 1), FUSED(1), lens=[79, 37, 79], p=0.1, same_as_full=True),
    Case("key-len", "past-3k", 64, 2, 140, 257, (16, 0), THREE(0), lens=[264, 129, 1], causal=True,
         same_as_full=True),
    Case("key-len", "zero-fused", 64, 2, 24, 72, (8, 1), FUSED(1), lens=[72, 0, 37]),
    Case("key-len", "zero-fused-causal-drop", 96, 2, 140, 200, (16, 0), FUSED(2), lens=[200, 0, 101],
         causal=True, p=0.1),
    Case("key-len", "zero-3k", 128, 2, 24, 72, (8, 1), THREE(1), lens=[72, 0, 37]),
    Case("key-len", "zero-3k-causal-drop", 64, 2, 140, 257, (16, 0), THREE(0), lens=[257, 0, 129],
         causal=True, p=0.1),
    # ---- batch strides: time-major (row stride B*ld, batch stride ld) and slack rows between batches
    Case("strides", "tm-fused", 64, 2, 24, 72, (8, 1), FUSED(1), p=0.1, layout="tm"),
    Case("strides", "tm-3k", 64, 2, 140, 257, (16, 0), THREE(0), causal=True, p=0.1, layout="tm"),
    Case("strides", "gap-fused", 96, 2, 70, 200, (8, 0), FUSED(2), causal=True, layout="gap"),
    Case("strides", "gap-3k", 128, 2, 130, 129, (16, 0), THREE(1), p=0.1, layout="gap"),
    # ---- peaked softmax: scaled scores of standard deviation ~ 6
    Case("peaked", "Tk200", 64, 2, 200, 200, (16, 0), FUSED(2), inputs="peaked"),
    Case("peaked", "Tk200-causal", 64, 2, 200, 200, (16, 0), FUSED(2), causal=True, inputs="peaked"),
    Case("peaked", "Tk300", 64, 2, 300, 300, (16, 0), THREE(0), inputs="peaked"),
    Case("peaked", "Tk300-causal-hd128", 128, 2, 300, 300, (16, 0), THREE(1), causal=True, inputs="peaked"),
    # ---- keys in ascending score order: the running maximum rises in every 64-key tile
    Case("rising", "Tk200", 64, 2, 70, 200, (8, 0), FUSED(2), inputs="rising"),
    Case("rising", "Tk200-causal", 64, 2, 200, 200, (16, 0), FUSED(2), causal=True, inputs="rising"),
    Case("rising", "Tk300", 64, 2, 70, 300, (8, 0), THREE(0), inputs="rising", p=0.1),
]


def _shape(c):
    """(B, H, lens) of a case; the persistent cases size Z = B*H from the device's CU count."""
    if c.cus is None:
        B, H = c.B, c.H
    else:
        G = torch.cuda.get_device_properties(0).multi_processor_count
        mult, extra, _ = c.cus
        Z = mult * G + (G // 2 if extra == "half" else extra)
        H = max(h for h in range(1, 33) if Z % h == 0)      # H*hd stays modest
        B = Z // H
    if isinstance(c.lens, str) and c.lens == "ragged":
        lens = [c.Tk, c.Tk // 2 + 1, 1][:B] + [c.Tk] * max(0, B - 3)
    elif isinstance(c.lens, str):                           # "per-row": lengths differ per batch row
        lens = [1 + (7 * b + 3) % c.Tk for b in range(B)]
    else:
        lens = c.lens
    return B, H, lens


def _inputs(c, B, H):
    """q, k, v, do [B, H, T, hd] fp16 on the CPU."""
    g = torch.Generator().manual_seed(5)
    hd = c.hd
    q = torch.randn(B, H, c.Tq, hd, generator=g)
    k = torch.randn(B, H, c.Tk, hd, generator=g)
    v = torch.randn(B, H, c.Tk, hd, generator=g)
    do = torch.randn(B, H, c.Tq, hd, generator=g)
    if c.inputs == "peaked":
        q = 6.0 * q                     # scale * q.k has standard deviation 1 for randn
    elif c.inputs == "rising":
        # queries near one direction per head, keys sorted by their score against the mean query
        q = 3.0 * torch.randn(B, H, 1, hd, generator=g) + 0.3 * q
        score = (k.half().float() @ q.half().float().mean(2, keepdim=True).transpose(-1, -2)).squeeze(-1)
        k = torch.gather(k, 2, score.argsort(-1).unsqueeze(-1).expand_as(k))
    return q.half(), k.half(), v.half(), do.half()


_REF = {}


def _reference(c):
    """Inputs and both references of a case, computed once on the CPU and left unchanged."""
    if c.id not in _REF:
        B, H, lens = _shape(c)
        q, k, v, do = _inputs(c, B, H)
        keep = A.keep_flags(SEED, OFF, B, H, c.Tq, c.Tk, c.p)
        scale = c.hd ** -0.5
        ref = A.ref64(q, k, v, do, lens, c.causal, scale, keep, c.p)
        emu = A.emulate(q, k, v, do, lens, c.causal, scale, keep, c.p)
        if c.inputs == "rising":
            # the property the case is there for: row maxima rise from tile to tile
            s = (q.double() @ k.double().transpose(-1, -2))[0]
            tiles = [s[..., t:t + 64].amax(-1) for t in range(0, c.Tk, 64)]
            rising = torch.stack([b > a for a, b in zip(tiles, tiles[1:])]).double().mean()
            assert rising > 0.9, f"running max rises in only {rising:.2f} of the tile steps"
        if c.inputs == "peaked":
            s = (q.double() @ k.double().transpose(-1, -2))[0] * scale
            assert 5.0 < float(s.std()) < 7.0
        _REF[c.id] = (B, H, lens, (q, k, v, do), ref, emu)
    return _REF[c.id]


def _merge(x):
    """[B, H, T, hd] -> [B, T, H*hd]"""
    B, H, T, hd = x.shape
    return x.transpose(1, 2).reshape(B, T, H * hd)


def _run(K, c, B, H, lens, data):
    """Plans, forward and backward of a case in padded buffers -> (plans, results on the CPU, buffers)."""
    q, k, v, do = data
    d = H * c.hd
    gap = 3 if c.layout == "gap" else 0
    lay = "tm" if c.layout == "tm" else "bm"
    mk = lambda T, ld, data=None: A.Padded(B, T, d, ld=ld, layout=lay, gap_rows=gap, device="cuda", data=data)
    ld_kv = (2 * d if c.wide_kv else d) + c.pad_kv
    bufs = {"q": mk(c.Tq, d + 8, _merge(q)), "k": mk(c.Tk, d + 8, _merge(k)), "v": mk(c.Tk, d + 8, _merge(v)),
            "do": mk(c.Tq, d + 8, _merge(do)), "o": mk(c.Tq, d + c.pad_o), "dq": mk(c.Tq, d + c.pad_o),
            "dk": mk(c.Tk, ld_kv), "dv": mk(c.Tk, ld_kv)}
    lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    b = bufs
    args = (b["q"].view, b["k"].view, b["v"].view, b["o"].view, b["q"].row, b["k"].row, b["v"].row, b["o"].row,
            B, H, c.Tq, c.Tk, c.hd, c.hd ** -0.5)
    fkw = dict(key_len=lens_t, causal=c.causal, p=c.p, drop=(SEED, OFF), sq=b["q"].batch_stride,
               sk=b["k"].batch_stride, sv=b["v"].batch_stride, so=b["o"].batch_stride)
    bkw = dict(sq=fkw["sq"], sk=fkw["sk"], sv=fkw["sv"], so=fkw["so"], sdo=b["do"].batch_stride,
               sdq=b["dq"].batch_stride, sdk=b["dk"].batch_stride, sdv=b["dv"].batch_stride)
    lse0 = torch.empty(B * H * c.Tq, dtype=torch.float32, device="cuda")
    bargs = lambda lse: args + (lens_t, c.causal, c.p, (SEED, OFF), lse, b["do"].view, b["do"].row, b["dq"].view,
                                b["dq"].row, b["dk"].view, b["dk"].row, b["dv"].view, b["dv"].row)
    plans = (K.mha_fwd_plan(*args, **fkw), K.mha_bwd_plan(*bargs(lse0), **bkw))
    for n in ("o", "dq", "dk", "dv"):
        assert bufs[n].all_sentinel()             # the plan queries wrote nothing
    lse = K.mha_fwd(*args, **fkw)
    K.mha_bwd(*bargs(lse), **bkw)
    torch.cuda.synchronize()
    got = {n: A.split_heads(bufs[n].view.cpu(), H) for n in ("o", "dq", "dk", "dv")}
    got["lse"] = lse.cpu().view(B, H, c.Tq)
    return plans, got, bufs


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_attention_path(K, c):
    B, H, lens, data, ref, emu = _reference(c)
    (pf, pb), got, bufs = _run(K, c, B, H, lens, data)
    # 1. the case reaches the path it is there for
    assert (pf["nw"], pf["short_k"]) == c.fwd, f"forward plan {pf}"
    assert pf["grid_y"] == B * H and pf["grid_x"] == -(-c.Tq // (16 * pf["nw"]))
    assert {n: pb[n] for n in c.bwd} == c.bwd, f"backward plan {pb}"
    if c.cus is not None:
        G = torch.cuda.get_device_properties(0).multi_processor_count
        assert B * H == c.cus[0] * G + (G // 2 if c.cus[1] == "half" else c.cus[1])
        assert pb["grid"] == min(B * H, G) and pb["rounds"] == c.cus[2], f"backward plan {pb}, G = {G}"
    # 2. + 4. nothing outside the logical regions was written (inputs included)
    for n, buf in bufs.items():
        buf.check(n)
    # 4. dK / dV of keys at or past the length are exactly zero; a batch row without keys gives
    # o = 0, lse = -inf and dQ = 0, exactly
    if lens is not None:
        for b_, L in enumerate(lens):
            if L == 0:
                assert bool((got["o"][b_] == 0).all()) and bool((got["dq"][b_] == 0).all())
                assert bool((got["lse"][b_] == -math.inf).all())
            for n in ("dk", "dv"):
                tail = got[n][b_, :, min(L, c.Tk):]
                assert bool((tail == 0).all()), f"{n} batch {b_}: keys past length {L} not zero"
    # 3. values, per output row, against the fp64 reference
    report, fails = [], []
    for n in OUTS:
        e_ref, _ = A.row_err(emu[n], ref[n])
        e_got, rows = A.row_err(got[n], ref[n])
        # per head: MARGIN x the emulated reference's error in that head, floored at one fp16 ulp
        floor = A.ulp16_rel(A.head_rms(ref[n]))
        bound = torch.maximum(A.MARGIN * e_ref, floor)
        ratio = e_got / torch.maximum(e_ref, floor / A.MARGIN)
        val, where = A.worst(e_got, rows)
        i = int(e_got.flatten().argmax())
        line = (f"{n}: kernel {val:.3e} at {where}, emulated there {float(e_ref.flatten()[i]):.3e} "
                f"(bound {float(bound.flatten()[i]):.3e}); emulated worst {float(e_ref.max()):.3e}; "
                f"worst kernel/emulated over heads {float(ratio.max()):.2f}")
        report.append(line)
        over = ~(e_got <= bound)
        if bool(over.any()):
            h = int(over.flatten().nonzero()[0])
            fails.append(f"{line}; first head over its bound: b={h // H} h={h % H} "
                         f"(kernel {float(e_got.flatten()[h]):.3e}, emulated {float(e_ref.flatten()[h]):.3e}, "
                         f"bound {float(bound.flatten()[h]):.3e})")
        if c.inputs == "randn" and n in FROB:
            f = float(A.frob_per_head(got[n], ref[n]).max())
            report.append(f"{n}: per-head Frobenius ratio {f:.3e} (bound {FROB[n]:.0e})")
            if not f < FROB[n]:
                fails.append(report[-1])
    print(f"\nATTN_PATHS {c.id}\n  " + "\n  ".join(report))
    assert not fails, f"{c.id}:\n  " + "\n  ".join(fails)
    # key_len absent or past Tk: the very bits of key_len = min(key_len, Tk)
    if c.same_as_full:
        full = [c.Tk] * B if lens is None else [min(L, c.Tk) for L in lens]
        _, got2, bufs2 = _run(K, c, B, H, full, data)
        for n in OUTS:
            assert torch.equal(_bits(got[n]), _bits(got2[n])), f"{n} differs from the key_len = {full} run"
        for n, buf in bufs2.items():
            buf.check(n)


def test_every_listed_path_is_asserted():
    """The case table reaches each path of the launchers at least once (host-side bookkeeping)."""
    fwd = {(c.hd, c.fwd) for c in CASES}
    for nw in (8, 16):
        for short in (0, 1):
            assert (128, (nw, short)) in fwd
    seen = {(c.hd, c.bwd["fused"], c.bwd["nkc"], c.bwd["kv16"], c.bwd["rows_prep"]) for c in CASES}
    for hd in (64, 96):
        for nkc in (1, 2):
            assert (hd, 1, nkc, 0, 0) in seen and (hd, 1, nkc, 1, 0) in seen
        assert (hd, 0, 0, 0, 1) in seen
    assert (128, 0, 0, 0, 1) in seen and (128, 0, 0, 0, 0) in seen
    assert any(c.bwd["fused"] == 0 and c.Tk <= 256 and c.hd <= 96 for c in CASES)
    assert {c.cus[2] for c in CASES if c.cus} == {1, 2, 3}
    assert {"tm", "gap"} <= {c.layout for c in CASES}


# ---------------------------------------------------------------------------- rejection
def _small(K, hd=64, H=2, B=2, Tq=8, Tk=8):
    d = H * hd
    mk = lambda T: A.Padded(B, T, d, ld=d + 8, device="cuda")
    bufs = {n: mk(Tq if n in ("q", "o", "do", "dq") else Tk) for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv")}
    return bufs, d


REJECT = [
    ("ldq", dict(ldq=4), "row strides must be multiples of 8"),
    ("ldo", dict(ldo=2), "row strides must be multiples of 8"),
    ("lddk", dict(lddk=2), "attention bwd: bad strides"),
    ("lddo", dict(lddo=4), "attention bwd: bad strides"),      # dout is loaded 16 bytes at a time
    ("hd80", dict(hd=80), "head_dim 80 not supported"),
    ("p1", dict(p=1.0), "dropout p must be < 1"),
    ("Tk0", dict(Tk=0), "attention: bad sizes"),
    ("null-lse", dict(lse=None), "lse buffer required"),
]


@pytest.mark.parametrize("what,change,msg", REJECT, ids=[r[0] for r in REJECT])
def test_attention_rejects(K, what, change, msg):
    """Host checks of the launchers (and of the plan queries, which share them): the package's error
    with its message, and nothing written."""
    lib = pkg()._lib
    hd = change.get("hd", 64)
    B, H, Tq = 2, 2, 8
    Tk = change.get("Tk", 8)
    bufs, d = _small(K, hd=hd)
    b = bufs
    ld = {n: b[n].row for n in b}
    ld["q"] += change.get("ldq", 0)
    ld["o"] += change.get("ldo", 0)
    ld["dk"] += change.get("lddk", 0)
    ld["do"] += change.get("lddo", 0)
    p = change.get("p", 0.0)
    lse = torch.zeros(B * H * Tq, dtype=torch.float32, device="cuda")
    args = (b["q"].view, b["k"].view, b["v"].view, b["o"].view, ld["q"], ld["k"], ld["v"], ld["o"],
            B, H, Tq, Tk, hd, hd ** -0.5)
    bargs = args + (None, False, p, (SEED, OFF), None if "lse" in change else lse, b["do"].view, ld["do"],
                    b["dq"].view, ld["dq"], b["dk"].view, ld["dk"], b["dv"].view, ld["dv"])
    calls = []
    if what == "null-lse":
        packed = K._attn_args(*args, None, False, p, (SEED, OFF), None)
        stream = torch.cuda.current_stream().cuda_stream
        calls.append(lambda: lib.call("mms2ut_mha_varlen_fwd", packed, stream))
        calls.append(lambda: K.mha_bwd(*bargs))
    elif what in ("lddk", "lddo"):
        calls.append(lambda: K.mha_bwd(*bargs))
        calls.append(lambda: K.mha_bwd_plan(*bargs))
    else:
        calls.append(lambda: K.mha_fwd(*args, p=p, drop=(SEED, OFF)))
        calls.append(lambda: K.mha_fwd_plan(*args, p=p, drop=(SEED, OFF)))
        calls.append(lambda: K.mha_bwd(*bargs))
    for i, f in enumerate(calls):
        want = "attention bwd: null buffers" if what == "null-lse" and i == 1 else msg
        with pytest.raises(lib.HipError, match=want):
            f()
    torch.cuda.synchronize()
    for n in ("o", "dq", "dk", "dv"):
        assert bufs[n].all_sentinel(), f"{n} was written by a rejected call"

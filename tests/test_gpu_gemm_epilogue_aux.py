"""The permuted register epilogue of the NT LDS-DMA GEMMs (csrc/gemm_common.h perm_epilogue: weight rows
permuted in the DMA so a lane owns whole 16-B column runs; residual / pre-activation / gate /
accumulated-C operands loaded into the MFMA layout under the last k-step) against the unpermuted
fp32-staged epilogue (mms2ut_gemm_set_epilogue(1)), bit for bit, and once against the fp32 torch
expression at the tolerance tests/test_gpu_kernels.py uses (2e-3 relative L2).

Shapes are the smallest that reach every path: M = 1 / 17 / 130 / 257 / 400 are row tails of the 16-row
fragment, the 64-row wave tile and the 96 / 128 / 160 / 192-row block tiles; N = 64 / 192 / 320 leave a
block's second 64-column strip past N (that wave returns early); K = 64 / 128 / 192 are one, two and
three k-steps (the operand prefetch sits under the last one, so one k-step has no loop in front of it),
K = 768 is the step's.  The GEMMs are issued unsplit (fixup=False) with the short-M kernel off, so they
run on the 128-row LDS-DMA kernel (default route at these M) or, with mms2ut_gemm_set_tall(2 / 3 / 5),
on the 160 / 192 / 96-row tall kernel, which takes every NT shape when forced.  Dropout streams: an
odd offset (no counter fast path), offsets from the step's range, and one per shape that puts the
2^33 counter boundary in the middle of the matrix (the lanes that straddle it hash with mms_keep4, the
others with mms_keep4_hi)."""
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

STREAMS = ((1234, 0), (77, 7), (5, (1 << 33) - 12345678), (9, 123456789012))
SHAPES = [(1, 64, 64), (17, 192, 128), (130, 320, 192), (257, 768, 768), (400, 768, 768), (400, 64, 768),
          (130, 768, 64), (257, 320, 128), (17, 768, 192), (400, 192, 64), (1, 320, 768), (257, 192, 768),
          (130, 64, 128), (17, 320, 64)]
P_DROP = 0.1
TOL = 2e-3   # tests/test_gpu_kernels.py::test_gemm_epilogues


@pytest.fixture(scope="module")
def K_():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return pkg().kernels


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _both(K_, fn, reps=3):
    """fn() under the register epilogue (reps times, all equal) and under the staged one."""
    outs = []
    try:
        for staged in (0, 1):
            K_.call("mms2ut_gemm_set_epilogue", staged)
            for _ in range(reps if staged == 0 else 1):
                outs.append(fn().clone())
    finally:
        K_.call("mms2ut_gemm_set_epilogue", 0)
    torch.cuda.synchronize()
    ref = outs[-1].view(torch.int16)
    for i, o in enumerate(outs[:-1]):
        assert torch.equal(o.view(torch.int16), ref), f"run {i}: {(o.view(torch.int16) != ref).sum().item()} bits differ"
    return outs[0]


class _Case:
    """Operands of one shape, made once; every form is a closure that returns its output(s)."""

    def __init__(self, K_, M, N, Kd, scale=1.0):
        self.K_, self.M, self.N, self.Kd = K_, M, N, Kd
        g = torch.Generator(device="cuda").manual_seed(1000 * M + 10 * N + Kd)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)
        self.x = (r(M, Kd) * 0.5 * scale).half()
        self.W = (r(N, Kd) * 0.05 * scale).half()
        self.b = (r(N) * 0.1).half()
        self.res = r(M, N + 72).half()[:, 8:8 + N]          # strided view: ldaux = N + 72 > N, 16-B aligned
        self.h = r(M, N).half()                             # fc1 activation: about half of it <= 0
        self.c0 = r(M, N).half()
        self.merge = r(M, 2 * N).half()
        self.out = torch.empty(M, N, dtype=torch.float16, device="cuda")
        self.g = torch.empty(M, N, dtype=torch.float16, device="cuda")
        self.pre = self.x.float() @ self.W.float().t()

    def run(self, epi, *, bias=None, aux=None, out2=None, p=0.0, drop=(0, 0)):
        K_, M, N, Kd = self.K_, self.M, self.N, self.Kd
        K_.gemm(self.x, self.W, self.out, M, N, Kd, lda=Kd, ldb=Kd, ldc=N, epi=epi, bias=bias, aux=aux,
                ldaux=(aux.stride(0) if aux is not None else 0), out2=out2,
                ldo2=(out2.stride(0) if out2 is not None else 0), p=p, seed=drop[0], offset=drop[1], ld_rng=N,
                fixup=False)
        return self.out

    def mask(self, drop):
        return self.K_.dropout_mask(self.M * self.N, P_DROP, drop[0], drop[1], "cuda").view(self.M, self.N).float()

    def acc(self):
        self.out.copy_(self.c0)
        return self.run(self.K_.EPI_F16_ACC)

    def gate(self):
        o = self.run(self.K_.EPI_GATE, bias=self.b, aux=self.merge, out2=self.g)
        return torch.cat([o, self.g])


def _check_forms(K_, M, N, Kd):
    c = _Case(K_, M, N, Kd)
    E = K_
    pre_b = c.pre + c.b.float()
    streams = STREAMS + ((11, (1 << 33) - (M * N // 2 // 8 * 8 + 4)),)   # 2^33 inside the matrix, mid-run
    y = _both(K_, lambda: c.run(E.EPI_F16, bias=c.b))
    assert rel(y, pre_b) < TOL
    y = _both(K_, lambda: c.run(E.EPI_F16))
    assert rel(y, c.pre) < TOL
    y = _both(K_, lambda: c.run(E.EPI_DROP_RESID, bias=c.b, aux=c.res))
    assert rel(y, pre_b + c.res.float()) < TOL
    for drop in streams:   # the replayed mask also pins the counters to the element's true (m, n)
        m = c.mask(drop)
        y = _both(K_, lambda: c.run(E.EPI_RELU_DROP, bias=c.b, p=P_DROP, drop=drop))
        assert rel(y, pre_b.relu() * m / (1 - P_DROP)) < TOL
        y = _both(K_, lambda: c.run(E.EPI_DROP_RESID, bias=c.b, aux=c.res, p=P_DROP, drop=drop))
        assert rel(y, pre_b * m / (1 - P_DROP) + c.res.float()) < TOL
    y = _both(K_, lambda: c.run(E.EPI_RELU_DROP_BWD, aux=c.h, p=P_DROP))
    assert rel(y, c.pre * (c.h > 0) / (1 - P_DROP)) < TOL
    y = _both(K_, c.acc)
    assert rel(y, c.c0.float() + c.pre) < TOL
    y = _both(K_, c.gate)
    gr = torch.sigmoid(pre_b)
    o, t = c.merge[:, :N].float(), c.merge[:, N:].float()
    assert rel(y[M:], gr) < TOL
    assert rel(y[:M], (1 - gr) * t + gr * o) < TOL


@pytest.fixture
def routes(K_):
    """Unsplit NT route: the short-M kernel off, restored afterwards with the tile-height rule."""
    K_.call("mms2ut_gemm_set_skinny", 0)
    try:
        yield
    finally:
        K_.call("mms2ut_gemm_set_skinny", 1)
        K_.call("mms2ut_gemm_set_tall", 1)


@pytest.mark.parametrize("tall", [1, 2, 3, 5])
@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_aux_epilogues_bit_identical(K_, routes, M, N, Kd, tall):
    K_.call("mms2ut_gemm_set_tall", tall)
    _check_forms(K_, M, N, Kd)


@pytest.mark.parametrize("wscale", [40, 1600])
@pytest.mark.parametrize("tall", [1, 2, 3, 5])
def test_overflow_bit_identical(K_, routes, tall, wscale):
    """Large accumulators: operands scaled as tests/test_gpu_gemm_epilogue.py does (x * 60, W * 40: sums of
    a few thousand), and W * 1600, which puts the sums' standard deviation (sqrt(768) * 30 * 80 = 66 k) at
    the fp16 maximum, so about a third of the outputs round to inf: the inf / select paths of every form.
    Bits only."""
    K_.call("mms2ut_gemm_set_tall", tall)
    M, N, Kd = 257, 192, 768
    c = _Case(K_, M, N, Kd)
    c.x = (c.x * 60).half()
    c.W = (c.W * wscale).half()
    E = K_
    _both(K_, lambda: c.run(E.EPI_F16, bias=c.b))
    _both(K_, lambda: c.run(E.EPI_RELU_DROP, bias=c.b, p=P_DROP, drop=(3, 64)))
    y = _both(K_, lambda: c.run(E.EPI_DROP_RESID, bias=c.b, aux=c.res, p=P_DROP, drop=(3, 64)))
    assert wscale == 40 or torch.isinf(y).any()
    _both(K_, lambda: c.run(E.EPI_RELU_DROP_BWD, aux=c.h, p=P_DROP))
    _both(K_, c.acc)
    _both(K_, c.gate)


def test_batched_bit_identical(K_, routes):
    """Batched NT products (per-batch strides of A, B, C and aux, alpha != 1) on the 128-row kernel: the
    permuted epilogue with its operands offset per batch entry.  T = 130 leaves a row tail."""
    g = torch.Generator(device="cuda").manual_seed(5)
    Bh, T, S, hd = 3, 130, 128, 64
    q = torch.randn(Bh, T, hd, device="cuda", generator=g).half()
    k = torch.randn(Bh, S, hd, device="cuda", generator=g).half()
    res = torch.randn(Bh, T, S, device="cuda", generator=g).half()
    out = torch.empty(Bh, T, S, dtype=torch.float16, device="cuda")

    def run(**kw):
        K_.gemm(q, k, out, T, S, hd, lda=hd, ldb=hd, ldc=S, batch=Bh, sA=(T * hd, 0), sB=(S * hd, 0),
                sC=(T * S, 0), alpha=hd ** -0.5, **kw)
        return out
    ref = hd ** -0.5 * q.float() @ k.float().transpose(1, 2)
    y = _both(K_, run)
    assert rel(y, ref) < TOL
    y = _both(K_, lambda: run(epi=K_.EPI_DROP_RESID, aux=res, ldaux=S, sX=(T * S, 0)))
    assert rel(y, ref + res.float()) < TOL
    c0 = res.clone()

    def acc():
        out.copy_(c0)
        return run(epi=K_.EPI_F16_ACC)
    y = _both(K_, acc)
    assert rel(y, ref + c0.float()) < TOL


class _NarrowCase(_Case):
    """_Case with C and out2 in ldc-wide buffers (columns N..ldc hold a sentinel) and the aux operands
    in ldaux-wide ones; GATE's merged operand is 2 N + 4 wide (its second half starts at aux + N, so it
    cannot live in an ldaux = N + 8 row; 2 N + 4 keeps ldaux % 8 == 4).  run() returns the whole C buffer."""
    PAD = 7.0

    def __init__(self, K_, M, N, Kd, ldc, ldaux, fixup):
        super().__init__(K_, M, N, Kd)
        self.ldc, self.fixup = ldc, fixup
        g = torch.Generator(device="cuda").manual_seed(3 * M + N + Kd)
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)
        self.res, self.h, self.z = (r(M, ldaux).half()[:, :N] for _ in range(3))
        self.merge = r(M, 2 * N + 4).half()[:, :2 * N]
        self.cbuf = torch.full((M, ldc), self.PAD, dtype=torch.float16, device="cuda")
        self.o2buf = torch.full((M, ldc), self.PAD, dtype=torch.float16, device="cuda")
        self.out, self.g = self.cbuf[:, :N], self.o2buf[:, :N]

    def run(self, epi, *, bias=None, aux=None, out2=None, p=0.0, drop=(0, 0)):
        M, N, Kd = self.M, self.N, self.Kd
        self.K_.gemm(self.x, self.W, self.cbuf, M, N, Kd, lda=Kd, ldb=Kd, ldc=self.ldc, epi=epi, bias=bias, aux=aux,
                     ldaux=(aux.stride(0) if aux is not None else 0), out2=out2,
                     ldo2=(out2.stride(0) if out2 is not None else 0), p=p, seed=drop[0], offset=drop[1], ld_rng=N,
                     fixup=self.fixup)
        return torch.cat([self.cbuf, self.o2buf]) if out2 is not None else self.cbuf


def _gelu_grad(z):
    return 0.5 * (1 + torch.erf(z * 2 ** -0.5)) + z * torch.exp(-0.5 * z * z) * (2 * torch.pi) ** -0.5


NARROW = [(17, 68, 64, 68, 76, "dma"), (17, 68, 64, 68, 76, "tall"), (17, 68, 512, 68, 76, "skinny"),
          (17, 68, 512, 68, 76, "fixup"), (130, 70, 128, 72, 76, "dma"), (130, 70, 128, 72, 76, "tall")]


@pytest.mark.parametrize("M,N,Kd,ldc,ldaux,route", NARROW)
def test_narrow_store_operand_forms(K_, routes, M, N, Kd, ldc, ldaux, route):
    """The 4- / 8-column store functions epilogue_store / epilogue_store8 (gemm_common.h), the only path
    where vec16 == 0 and on N tails, under the forms that read a row operand or write out2.
    (17, 68, .): ldc = 68 and ldaux = 76 are 4 mod 8, so vec16 == 0 and every group is 4-wide.
    (130, 70, 128): ldc = 72; the forms without aux keep vec16 == 1 and a row is eight 8-wide groups, one
    full 4-wide group (64..67) and a 2-element scalar tail (68, 69); with aux (ldaux = 76) all is 4-wide.
    GATE is left out at N = 70: its second operand sits at aux + N and is read 4-wide, N % 4 == 0.
    Routes (csrc/gemm.hip gemm_dispatch; N % 64 != 0, so reg_epilogue_ok() is false on all of them):
      dma    short-M kernel off, unsplit: `if (dma_ok)` -> launch_dma<true, true> (tall_pick() returns 0
             at these M), staged_epilogue -> epilogue_store8;
      tall   the same with mms2ut_gemm_set_tall(2): `if (dma_ok && a_kc && b_kc && nz == 1)` ->
             launch_tall<5>;
      skinny K = 512 (K % 256 == 0), short-M kernel on, no split asked: `if (splitk == 1 &&
             skinny_eligible(a))` -> launch_skinny (unsplit plan: no workspace is passed);
      fixup  K = 512, short-M kernel off, kernels.gemm asks for 2 splits (_fixup_splits): `if (splitk > 1
             && a->epi != MMS_EPI_F32)` -> fp32 slabs, then splitk_fixup_kernel -> epilogue_store8.
    Per form: bits equal under mms2ut_gemm_set_epilogue(0 / 1), relative L2 against the fp32 torch
    expression below TOL with the mask replayed by dropout_mask (one wrong keep bit of M N <= 9100
    elements moves the L2 by >= 1 / sqrt(9100) = 1e-2), columns N..ldc of C and out2 untouched."""
    E = K_
    K_.call("mms2ut_gemm_set_skinny", 1 if route == "skinny" else 0)
    K_.call("mms2ut_gemm_set_tall", 2 if route == "tall" else 1)
    c = _NarrowCase(K_, M, N, Kd, ldc, ldaux, fixup=(route == "fixup"))
    pre_b = c.pre + c.b.float()
    sc = 1 / (1 - P_DROP)

    def check(fn, ref, ref2=None):
        y = _both(K_, fn)
        assert (y[:, N:] == c.PAD).all()
        assert rel(y[:M, :N], ref) < TOL
        if ref2 is not None:
            assert rel(y[M:, :N], ref2) < TOL

    check(lambda: c.run(E.EPI_F16, bias=c.b), pre_b)
    check(lambda: c.run(E.EPI_RELU_DROP_BWD, aux=c.h, p=P_DROP), c.pre * (c.h > 0) * sc)
    check(c.acc, c.c0.float() + c.pre)
    if N % 4 == 0:
        gr = torch.sigmoid(pre_b)
        o, t = c.merge[:, :N].float(), c.merge[:, N:].float()
        check(lambda: c.run(E.EPI_GATE, bias=c.b, aux=c.merge, out2=c.g), (1 - gr) * t + gr * o, gr)
    for drop in ((77, 7), (11, (1 << 33) - (M * N // 2 // 8 * 8 + 4))):   # odd offset; 2^33 inside the matrix
        m = c.mask(drop)
        check(lambda: c.run(E.EPI_RELU_DROP, bias=c.b, p=P_DROP, drop=drop), pre_b.relu() * m * sc)
        check(lambda: c.run(E.EPI_DROP_RESID, bias=c.b, aux=c.res, p=P_DROP, drop=drop),
              pre_b * m * sc + c.res.float())
        check(lambda: c.run(E.EPI_GELU_DROP, bias=c.b, out2=c.g, p=P_DROP, drop=drop),
              torch.nn.functional.gelu(pre_b) * m * sc, pre_b)
        check(lambda: c.run(E.EPI_GELU_DROP_BWD, aux=c.z, p=P_DROP, drop=drop),
              c.pre * m * sc * _gelu_grad(c.z.float()))


def test_n1004_stays_staged(K_, routes):
    """N = 1004 in a 1024-column row: N % 64 != 0, so every wave of every block takes the staged path on
    unpermuted weight rows (a mixed choice races on the LDS slots, which only repeated runs expose)."""
    M, N, Kd = 257, 1004, 768
    g = torch.Generator(device="cuda").manual_seed(4)
    x = (torch.randn(M, Kd, device="cuda", generator=g) * 0.5).half()
    W = (torch.randn(N, Kd, device="cuda", generator=g) * 0.05).half()
    b = (torch.randn(1024, device="cuda", generator=g) * 0.1).half()
    res = torch.randn(M, 1024, device="cuda", generator=g).half()
    out = torch.zeros(M, 1024, dtype=torch.float16, device="cuda")

    def logits(**kw):
        K_.gemm(x, W, out, M, N, Kd, lda=Kd, ldb=Kd, ldc=1024, bias=b, fixup=False, **kw)
        return out
    y = _both(K_, logits, reps=5)
    pre = x.float() @ W.float().t() + b[:N].float()
    assert rel(y[:, :N], pre) < TOL
    assert not y[:, N:].any()
    y = _both(K_, lambda: logits(epi=K_.EPI_DROP_RESID, aux=res, ldaux=1024, p=P_DROP, seed=77, offset=7, ld_rng=N),
              reps=5)
    m = K_.dropout_mask(M * N, P_DROP, 77, 7, "cuda").view(M, N).float()
    assert rel(y[:, :N], pre * m / (1 - P_DROP) + res[:, :N].float()) < TOL

"""GPU: the forward-only validation scoring kernel (kernels.ls_xent_eval) against torch fp64
log_softmax of the same fp16 logits: label-smoothed loss and nll sums (1e-4 relative, test_ls_xent's
tolerance for the same fp32 row arithmetic), exact ntokens / n_correct counts (argmax over the fp16
values, first index on ties), pad columns [V, ld) never read into the result (they hold 60000, which
would wreck both the loss and the argmax), accumulation over calls, bit-reproducibility, and
agreement with ls_xent_fwd (fp32 against fp64 accumulation of the same row values, 1e-6)."""
import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

EPS, PAD = 0.2, 1
PARTS = 512     # include/mms2ut.h MMS_LS_XENT_PARTS


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    k = pkg().kernels
    assert k.LS_XENT_PARTS == PARTS
    return k


def _inputs(rows, V, ld, seed):
    """fp16 logits [rows, ld] with 60000 in the pad columns; targets: half of them the row's argmax
    (so n_correct is far from 0), the rest random, every 7th pad."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, ld, generator=g).half()
    logits[:, V:] = 60000.0
    target = torch.randint(0, V, (rows,), generator=g)
    am = torch.from_numpy(np.argmax(logits[:, :V].numpy(), axis=1))     # first index on ties
    target[::2] = am[::2]
    target[::7] = PAD
    return logits, target


def _reference(logits, target, V):
    """fp64 {loss, nll, ntokens, n_correct} of the fp16 logits' columns [0, V)."""
    z = logits[:, :V].double()
    lp = torch.log_softmax(z, -1)
    keep = target != PAD
    nll = -lp[keep, target[keep]].sum()
    smooth = -lp[keep].sum()
    ei = EPS / (V - 1)
    loss = (1 - EPS - ei) * nll + ei * smooth
    am = torch.from_numpy(np.argmax(logits[:, :V].numpy(), axis=1))
    return float(loss), float(nll), int(keep.sum()), int((am == target)[keep].sum())


def _eval(K, logits, target, V, stats=None):
    rows, ld = logits.shape
    if stats is None:
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    K.ls_xent_eval(logits, ld, target, rows, V, EPS, PAD, stats)
    return stats


def _relerr(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


@pytest.mark.parametrize("V,ld", [(1004, 1008), (1004, 1024), (37, 40), (260, 264)])
@pytest.mark.parametrize("rows", [1, 3, 333, 4 * PARTS + 5])     # the last one forces the grid-stride
def test_matches_fp64_reference_and_fwd(K, rows, V, ld):
    logits, target = _inputs(rows, V, ld, seed=rows * 7 + V)
    if rows == 1:
        target[0] = int(np.argmax(logits[0, :V].numpy()))        # the one row is not pad
    ref = _reference(logits, target, V)
    lg, tg = logits.cuda(), target.cuda()
    got = _eval(K, lg, tg, V).tolist()
    print(f"rows {rows} V {V} ld {ld}: got {got} ref {ref}")
    assert got[2] == ref[2] and got[3] == ref[3]
    assert ref[2] > 0 and (rows < 333 or 0 < ref[3] < ref[2])     # the inputs exercise both outcomes
    assert _relerr(got[0], ref[0]) < 1e-4 and _relerr(got[1], ref[1]) < 1e-4
    # the training kernel on the same inputs: the same fp32 row values, summed in fp32
    out = torch.zeros(2, device="cuda")
    K.ls_xent_fwd(lg, ld, tg, rows, V, EPS, PAD, out)
    fwd = out.tolist()
    print(f"  ls_xent_fwd {fwd}")
    assert _relerr(fwd[0], got[0]) < 1e-6 and _relerr(fwd[1], got[1]) < 1e-6


def test_ties_go_to_the_lowest_column(K):
    V, ld = 1004, 1008
    # (lower, higher) column of the doubled maximum: within one 4-wide load, across lanes, across
    # the lane's column groups (c), and the last column
    pairs = [(5, 6), (4, 9), (3, 700), (255, 256), (0, V - 1), (1002, V - 1)]
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2 * len(pairs), ld, generator=g).half().clamp_(-4, 4)
    logits[:, V:] = 60000.0
    target = torch.empty(2 * len(pairs), dtype=torch.int64)
    for i, (a, b) in enumerate(pairs):
        logits[2 * i:2 * i + 2, a] = 9.0
        logits[2 * i:2 * i + 2, b] = 9.0
        target[2 * i], target[2 * i + 1] = a, b
    lg = logits.cuda()
    for r in range(len(target)):        # row by row: which rows count is visible exactly
        got = _eval(K, lg[r:r + 1], target[r:r + 1].cuda(), V).tolist()
        assert got[2] == 1.0 and got[3] == (1.0 if r % 2 == 0 else 0.0), (r, pairs[r // 2], got)
    got = _eval(K, lg, target.cuda(), V).tolist()
    assert got[2] == 2 * len(pairs) and got[3] == len(pairs)


@pytest.mark.parametrize("V,ld", [(1004, 1008), (1004, 1024), (37, 40), (260, 264)])
def test_maximum_at_the_last_column(K, V, ld):
    logits, _ = _inputs(5, V, ld, seed=V)
    logits[:, V - 1] = 11.0
    target = torch.full((5,), V - 1, dtype=torch.int64)
    target[3] = V - 2
    got = _eval(K, logits.cuda(), target.cuda(), V).tolist()
    ref = _reference(logits, target, V)
    assert got[2] == 5 and got[3] == 4 == ref[3]
    assert _relerr(got[0], ref[0]) < 1e-4 and _relerr(got[1], ref[1]) < 1e-4


def test_all_pad_adds_exactly_zero(K):
    logits, _ = _inputs(37, 1004, 1008, seed=5)
    target = torch.full((37,), PAD, dtype=torch.int64)
    before = torch.tensor([1.5, 2.25, 3.0, 4.0], dtype=torch.float64, device="cuda")
    stats = _eval(K, logits.cuda(), target.cuda(), 1004, before.clone())
    assert torch.equal(stats, before)
    assert torch.equal(_eval(K, logits.cuda(), target.cuda(), 1004), torch.zeros(4, dtype=torch.float64, device="cuda"))


def test_accumulates_over_calls_bit_reproducibly(K):
    V, ld = 1004, 1024
    calls = [_inputs(r, V, ld, seed=40 + r) for r in (333, 4 * PARTS + 5, 61)]
    calls = [(lg.cuda(), tg.cuda()) for lg, tg in calls]
    single = [_eval(K, lg, tg, V).tolist() for lg, tg in calls]

    def run():
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        for lg, tg in calls:
            _eval(K, lg, tg, V, stats)
        return stats

    a, b = run(), run()
    assert torch.equal(a, b)
    got = a.tolist()
    want = [sum(s[k] for s in single) for k in range(4)]
    assert got[2] == want[2] and got[3] == want[3]
    assert _relerr(got[0], want[0]) < 1e-12 and _relerr(got[1], want[1]) < 1e-12


def test_rejects_bad_arguments(K):
    lg = torch.zeros(4, 1008, dtype=torch.float16, device="cuda")
    tg = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(4, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError):
        K.ls_xent_eval(lg, 1000, tg, 4, 1004, EPS, PAD, st)      # ld < V
    with pytest.raises(RuntimeError):
        K.ls_xent_eval(lg, 1006, tg, 4, 1004, EPS, PAD, st)      # ld % 4
    with pytest.raises(RuntimeError):
        K.ls_xent_eval(lg.view(-1)[1:], 1004, tg, 4, 1004, EPS, PAD, st)   # 2-byte aligned logits
    big = torch.zeros(1, 4100, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError):
        K.ls_xent_eval(big, 4100, tg, 1, 4097, EPS, PAD, st)     # beyond the 4096-column limit
    torch.cuda.synchronize()
    assert torch.equal(st, torch.zeros_like(st))

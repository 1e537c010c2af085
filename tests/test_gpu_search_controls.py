"""GPU: the search-control kernels (log_softmax_step_ext, ngram_block, sample_step) against their
torch statements in generate.py and an fp64 reference, then the controls end to end through
``generate.generate`` and ``mms2ut-generate``.  The sampling stream and the step order are those of
tests/search_controls_ref.py."""
import math

import pytest
import torch

import search_controls_ref as SR
from conftest import pkg

pytestmark = pytest.mark.gpu

PAD, EOS, UNK = 1, 2, 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------ normalisation

@pytest.mark.parametrize("V", [5, 64, 65, 1004])
def test_step_normalisation(V):
    """T = 1, unkpen = 0 is bit-equal to log_softmax_step; the rest within the 1e-5 of
    test_gpu_generate.test_log_softmax_step_masks of the fp32 torch statement of steps 1 to 6,
    with the same -inf pattern."""
    K, G = pkg("kernels"), pkg("generate")
    torch.manual_seed(V)
    for rows in (1, 5, 40):
        z = (torch.randn(rows, V + 3) * 3).half()
        z[rows // 2, V // 2] = float("nan")
        z[0, V - 1] = -math.inf
        z[rows - 1, 0] = -math.inf
        zc = z.cuda()
        for mode in (0, 1, 2):
            base = K.log_softmax_step(zc, V, PAD, EOS, mode)
            same = K.log_softmax_step_ext(zc, V, PAD, EOS, mode, 1.0, 0.0)
            assert torch.equal(base, same)
            for T in (1.0, 0.5, 1.7):
                for unkpen in (0.0, 0.5):
                    lp = K.log_softmax_step_ext(zc, V, PAD, EOS, mode, T, unkpen).cpu()
                    ref = G.normalize_step(z[:, :V], PAD, EOS, mode, T, unkpen)
                    assert torch.equal(torch.isinf(lp), torch.isinf(ref)) and not torch.isnan(lp).any()
                    fin = ~torch.isinf(ref)
                    err = (lp[fin] - ref[fin]).abs().max().item() if fin.any() else 0.0
                    assert err < 1e-5, (rows, mode, T, unkpen, err)
    with pytest.raises(ValueError):
        K.log_softmax_step_ext(zc, V, PAD, EOS, 0, 0.0, 0.0)


# ------------------------------------------------------------------------------ n-gram blocking

LD = 3002


def _histories(N, V, n, step, kind, gen):
    """[N, LD] int64 histories on the GPU, tokens < min(V, 5), columns past `step` <pad>."""
    if kind == "random3":
        h = torch.randint(2, 5, (N, LD), generator=gen)
    elif kind == "periodic":
        h = (torch.arange(LD) % 3 + 2).repeat(N, 1)
        h[1::2] = (torch.arange(LD) % 2 + 3)
    elif kind == "equal":
        h = torch.full((N, LD), 4)
    else:
        h = torch.randint(2, 4, (N, LD), generator=gen)       # tokens 2 and 3; the suffix is 4s
        m = n - 1
        h[:, max(step + 1 - m, 0): step + 1] = 4
        if kind == "first":                                   # the only match at i = 0
            h[:, :m] = 4
        else:                                                 # the only match at the last legal i
            h[:, max(step - m, 0): step + 1] = 4
    if kind != "first":                                       # there the match starts at position 0
        h[:, 0] = EOS
    h[:, step + 1:] = PAD
    return h.cuda()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 6])
def test_ngram_block_matches_torch(n):
    """The -inf pattern and every untouched value, exactly."""
    K, G = pkg("kernels"), pkg("generate")
    gen = torch.Generator().manual_seed(n)
    steps = sorted({s for s in (0, n - 2, n - 1, 62, 63, 64, 65, 300, 2999) if s >= 0})
    hits = 0
    for N in (1, 10, 40):
        for V in (5, 1004):
            lp0 = torch.randn(N, V, generator=gen)
            lp0[torch.rand(N, V, generator=gen) < 0.05] = -math.inf
            lp0 = lp0.cuda()
            for step in steps:
                for kind in ("random3", "periodic", "equal", "first", "last"):
                    h = _histories(N, V, n, step, kind, gen)
                    got = K.ngram_block(h, lp0.clone(), step, n)
                    ref = G.torch_ngram_block(h, lp0.clone(), step, n)
                    assert torch.equal(got, ref), (N, V, step, kind)
                    hits += int((torch.isinf(ref) & ~torch.isinf(lp0)).sum())
                    if kind in ("first", "last") and n > 1 and step >= 2 * n:
                        # exactly one start matches: one banned token per row
                        i = 0 if kind == "first" else step + 1 - n
                        want = lp0.clone()
                        want[torch.arange(N), h[:, i + n - 1]] = -math.inf
                        assert torch.equal(got, want), (N, V, step, kind)
    assert hits > 0
    with pytest.raises(ValueError):
        K.ngram_block(h, lp0.clone(), LD, n)


def test_ngram_block_reads_the_current_buffer_after_a_shrink():
    """The histories after sentences left the batch and beam_advance wrote them to the spare pair."""
    K, G = pkg("kernels"), pkg("generate")
    gen = torch.Generator().manual_seed(0)
    bsz, beam, V, step, L = 6, 4, 64, 70, 90
    tokens = torch.randint(4, 16, (bsz * beam, L), generator=gen).cuda()    # 12 symbols: rows ban different sets
    tokens[:, 0] = EOS
    scores = torch.randn(bsz * beam, L - 1, generator=gen).cuda()
    keep = torch.tensor([0, 2, 5]).cuda()
    nb = keep.numel()
    tokens = tokens.view(bsz, -1)[keep].view(nb * beam, -1)
    scores = scores.view(bsz, -1)[keep].view(nb * beam, -1)
    k = 2 * beam
    cand_scores = torch.randn(nb, k, generator=gen).cuda()
    cand_indices = torch.randint(4, 16, (nb, k), generator=gen).cuda()
    cand_beams = torch.randint(0, beam, (nb, k), generator=gen).cuda()
    ignore = torch.zeros(nb, beam, dtype=torch.bool).cuda()
    mask, _ = K.beam_eos_scan(cand_scores, cand_indices, ignore, EOS)
    spare = (torch.full_like(tokens, PAD), torch.zeros_like(scores))
    K.beam_advance(mask, ignore, cand_scores, cand_indices, cand_beams, tokens, scores, step, spare[0], spare[1])
    cur = spare[0]
    assert not torch.equal(cur[:, : step + 2], tokens[:, : step + 2])
    lp0 = torch.randn(nb * beam, V, generator=gen).cuda()
    for n in (2, 3):
        got = K.ngram_block(cur, lp0.clone(), step + 1, n)
        assert torch.equal(got, G.torch_ngram_block(cur, lp0.clone(), step + 1, n))
        assert torch.isinf(got).any()
        assert not torch.equal(got, G.torch_ngram_block(tokens, lp0.clone(), step + 1, n))


# ------------------------------------------------------------------------------ sampling

def _lprobs(rows, V, P, seed):
    """fp32 [rows, V] rows of un-renormalised log-probabilities (total e^-0.05) with -inf at <pad>
    and at a tenth of the tokens, such that in fp64 no running sum of the descending order lies
    within 1e-4 of P (rows that do are drawn again)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    while len(out) < rows:
        z = torch.randn(V, generator=g) * 3
        m = torch.rand(V, generator=g) < 0.1
        m[PAD] = True
        m[0] = False
        z[m] = -math.inf
        lp = (torch.log_softmax(z, -1) - 0.05).float()
        if P > 0:
            c = torch.sort(lp.double(), descending=True, stable=True)[0].exp().cumsum(-1)
            if ((c - P).abs() < 1e-4).any():
                continue
        out.append(lp)
    return torch.stack(out)


def _reference(lp, topk, topp):
    """fp64: (order [rows, V] of the kept set's order, running sums C, kept [rows])."""
    rows, V = lp.shape
    if topk > 0 or topp > 0:
        order = torch.sort(-lp.double(), dim=-1, stable=True)[1]
    else:
        order = torch.arange(V).repeat(rows, 1)
    C = lp.double().gather(-1, order).exp().cumsum(-1)
    if topk > 0:
        kept = torch.full((rows,), min(topk, V))
    elif topp > 0:
        if topp > 0:
            assert not ((C - topp).abs() < 1e-4).any()        # asserted before the GPU is touched
        kept = ((C < topp).sum(-1) + 1).clamp(max=V)
    else:
        kept = torch.full((rows,), V)
    return order, C, kept


VARIANTS = [("topk", 1), ("topk", 2), ("topk", 10), ("topk", 32), ("topp", 0.1), ("topp", 0.9), ("topp", 1.0),
            ("full", 0)]


@pytest.mark.parametrize("variant,arg", VARIANTS)
def test_sample_draw(variant, arg):
    """The drawn j satisfies C_{j-1} - eps <= u * total <= C_j + eps against fp64 running sums C of
    exp(lprob) over the kept set, the returned lprob is the row's own bit for bit, and no token of
    probability 0 is drawn.

    eps, for a kept set of n tokens with total = C_n.  The kernel's p_j = expf(lprob_j) is within
    1 ulp of exp(lprob_j) (the HIP math API's bound for expf): a relative 2^-23.  Its running sum is
    a recursive fp32 sum of at most n non-negative terms in some order, whose relative error is at
    most (n - 1) * 2^-24 to first order whatever the order (Higham, Accuracy and Stability of
    Numerical Algorithms, §4.2).  So every kernel C_j is within g * total of the exact one,
    g = (n - 1) * 2^-24 + 2^-23.  The threshold u * total carries total's error g * total and one
    rounding of the product, 2^-24 * total.  The kernel picks C_{j-1} <= thr < C_j on its own
    values, so on exact ones the two sides move by at most g * total + (g + 2^-24) * total:
    eps = (2 g + 2^-24) * total, times 1.01 for the second-order terms."""
    K = pkg("kernels")
    topk = arg if variant == "topk" else -1
    topp = arg if variant == "topp" else -1.0
    seed, step = 11, 37
    for V in (5, 64, 65, 1004, 4096):
        for rows in (1, 10, 40):
            lp = _lprobs(rows, V, topp, seed=V + rows)
            order, C, kept = _reference(lp, topk, topp)
            ids = torch.arange(rows) * 3 + 1
            prev = torch.randn(rows, 4)
            sc, tok, bm, out_lp, out_kept = K.sample_step(lp.cuda(), prev.cuda()[:, 2], ids.cuda(), rows, 1, V, step,
                                                          seed, topk, topp)
            sc, tok, out_lp, out_kept = sc.cpu().view(-1), tok.cpu().view(-1), out_lp.cpu().view(-1), \
                out_kept.cpu().view(-1)
            assert out_kept.tolist() == kept.tolist(), (V, rows)
            assert torch.equal(bm.cpu(), torch.zeros(rows, 1, dtype=torch.long))
            own = lp.gather(-1, tok.view(-1, 1)).view(-1)
            assert torch.equal(out_lp, own) and torch.equal(sc, own + prev[:, 2])
            assert not torch.isinf(own).any()
            for r in range(rows):
                n = int(kept[r])
                j = order[r, :n].tolist().index(int(tok[r]))
                total = float(C[r, n - 1])
                g = (n - 1) * 2.0 ** -24 + 2.0 ** -23
                eps = 1.01 * (2 * g + 2.0 ** -24) * total
                ut = SR.uniform(seed, int(ids[r]), step, 0) * total
                lo = float(C[r, j - 1]) if j > 0 else 0.0
                assert lo - eps <= ut <= float(C[r, j]) + eps, (V, rows, r, j, lo, ut, float(C[r, j]), eps)


@pytest.mark.parametrize("P", [0.1, 0.5, 0.9, 1.0])
def test_sample_topp_cut(P):
    """No fp64 running sum lies within 1e-4 of P (asserted on the reference first; the kernel's
    fp32 sums are within (16 + 256) * 2^-24 < 2e-5 of them), so the kept count must match exactly."""
    K = pkg("kernels")
    cases = [(V, _lprobs(40, V, P, seed=int(P * 100) + V)) for V in (5, 64, 1004, 4096)]
    refs = [_reference(lp, -1, P) for _, lp in cases]
    for (V, lp), (_, _, kept) in zip(cases, refs):
        out_kept = K.sample_step(lp.cuda(), None, torch.arange(40).cuda(), 40, 1, V, 0, 1, -1, P)[4]
        assert out_kept.cpu().view(-1).tolist() == kept.tolist(), V
        if V > 5 and P < 1.0:
            assert int(kept.min()) < V                      # the cut is exercised


def test_sample_stream():
    K, G = pkg("kernels"), pkg("generate")
    bsz, beam, V = 6, 3, 65
    lp = _lprobs(bsz * beam, V, 0.9, seed=3).cuda()
    prev = torch.randn(bsz * beam).cuda()
    ids = torch.tensor([4, 9, 0, 7, 2, 31]).cuda()
    for step, pv in ((0, None), (5, prev)):
        for kw in ({}, {"topk": 4}, {"topp": 0.9}):
            a = K.sample_step(lp, pv, ids, bsz, beam, V, step, 7, **kw)
            b = K.sample_step(lp, pv, ids, bsz, beam, V, step, 7, **kw)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            c = K.sample_step(lp, pv, ids, bsz, beam, V, step, 8, **kw)
            assert not torch.equal(a[1], c[1])
            assert torch.equal(a[2].cpu(), torch.arange(beam).repeat(bsz, 1))
            # the torch statement (fp64 running sums) draws the same tokens
            t = G.torch_sample_step(lp, pv, ids, bsz, beam, V, step, 7, **kw)
            assert torch.equal(a[1], t[1]) and torch.equal(a[0], t[0])
            # permuting the batch with its ids permutes the draws
            perm = torch.tensor([3, 0, 5, 1, 4, 2]).cuda()
            lpp = lp.view(bsz, beam, V)[perm].reshape(bsz * beam, V)
            pvp = None if pv is None else pv.view(bsz, beam)[perm].reshape(-1)
            p = K.sample_step(lpp, pvp, ids[perm], bsz, beam, V, step, 7, **kw)
            assert torch.equal(p[1], a[1][perm]) and torch.equal(p[0], a[0][perm])
    # step 0 draws every slot from the sentence's first row
    first = K.sample_step(lp, None, ids, bsz, beam, V, 0, 7)
    rows0 = lp.view(bsz, beam, V)[:, 0]
    assert torch.equal(first[3], rows0.gather(-1, first[1]))
    with pytest.raises(NotImplementedError, match="4096"):
        K.sample_step(torch.zeros(1, 4097).cuda(), None, ids[:1], 1, 1, 4097, 0, 1)
    with pytest.raises(ValueError):
        K.sample_step(lp, None, ids, bsz, beam, V, 0, 1, topk=3, topp=0.5)


# ------------------------------------------------------------------------------ end to end

class NoControlsDecoder:
    """The incremental decoder without ngram_block / sample_step: the generator then runs
    generate.torch_ngram_block / torch_sample_step (everything else stays on the HIP path)."""

    def __init__(self, dec):
        self.dec = dec

    def step(self, *a, **k):
        return self.dec.step(*a, **k)

    def reorder(self, *a, **k):
        return self.dec.reorder(*a, **k)

    def beam_topk(self, *a, **k):
        return self.dec.beam_topk(*a, **k)

    def beam_eos_scan(self, *a, **k):
        return self.dec.beam_eos_scan(*a, **k)

    def beam_advance(self, *a, **k):
        return self.dec.beam_advance(*a, **k)


@pytest.fixture(scope="module")
def tiny():
    from test_gpu_generate import _setup
    from test_gpu_generate_cli import _edit
    mm, cfg, P, model, batch, _, _ = _setup(lengths=(120, 57, 200, 57, 88), seed=5)
    model.params.load_state_dict(_edit(P))
    return mm.generate, model, batch


@pytest.fixture(scope="module")
def plain():
    """The unedited tiny model: flat distributions (every hypothesis runs to max_len), so top-k
    sampling has real choices at every step."""
    from test_gpu_generate import _setup
    mm, cfg, P, model, batch, _, _ = _setup()
    return mm.generate, model, batch


def _same(a, b, beam):
    assert len(a) == len(b)
    for hs, rs in zip(a, b):
        assert len(hs) == len(rs) == beam
        for h, r in zip(hs, rs):
            assert torch.equal(h["tokens"], r["tokens"]) and h["score"] == r["score"]
            assert torch.equal(h["positional_scores"], r["positional_scores"])


BEAM, MAX_LEN_B = 4, 12


@pytest.mark.parametrize("kw", [{"no_repeat_ngram_size": 2},
                                {"sampling": True, "sampling_topk": 5, "seed": 7}], ids=["ngram2", "sampling_topk5"])
def test_generate_kernel_path_matches_torch_fallback(tiny, plain, monkeypatch, kw):
    """n-gram blocking on the sharpened model (sentences end at different steps: the batch shrinks);
    sampling on the unedited one (on the sharpened one </s> holds all the mass at step 0 and every
    other probability underflows fp32, so there is nothing to draw from)."""
    G, model, batch = plain if kw.get("sampling") else tiny
    assert hasattr(G.IncrementalDecoder, "ngram_block") and hasattr(G.IncrementalDecoder, "sample_step")
    ids = torch.tensor([10, 3, 7]) if kw.get("sampling") else None
    hip = G.generate(model, batch, beam_size=BEAM, max_len_a=0.0, max_len_b=MAX_LEN_B, sample_ids=ids, **kw)
    real = G.IncrementalDecoder
    monkeypatch.setattr(G, "IncrementalDecoder", lambda *a, **k: NoControlsDecoder(real(*a, **k)))
    ref = G.generate(model, batch, beam_size=BEAM, max_len_a=0.0, max_len_b=MAX_LEN_B, sample_ids=ids, **kw)
    torch.cuda.synchronize()
    _same(hip, ref, BEAM)
    if kw.get("sampling"):
        assert len({tuple(h["tokens"].tolist()) for hs in hip for h in hs}) > len(hip)    # the samples differ
    if "no_repeat_ngram_size" in kw:
        for hs in hip:
            for h in hs:
                assert not SR.has_repeated_ngram([EOS] + h["tokens"].tolist(), 2)


def test_generate_defaults_unchanged(tiny):
    G, model, batch = tiny
    c0 = G.graph_captures()
    plain = G.generate(model, batch, beam_size=BEAM, max_len_a=0.0, max_len_b=MAX_LEN_B)
    c1 = G.graph_captures()
    dflt = G.generate(model, batch, beam_size=BEAM, max_len_a=0.0, max_len_b=MAX_LEN_B, temperature=1.0,
                      unk_penalty=0.0, no_repeat_ngram_size=0, sampling=False, sampling_topk=-1, sampling_topp=-1.0,
                      seed=1, sample_ids=None)
    c2 = G.graph_captures()
    _same(plain, dflt, BEAM)
    assert c1 - c0 == c2 - c1 > 0


def test_cli_search_controls(tmp_path):
    from manifest_corpus import write_corpus
    from test_gpu_generate_cli import _checkpoint, _cli, _fusion_yaml
    d = tmp_path / "data"
    d.mkdir()
    c = write_corpus(str(d), split="valid")
    ckpt, _, _, _, _ = _checkpoint(tmp_path, d, _fusion_yaml(tmp_path, c["feat_dir"]))

    def h_lines(out):
        return [l for l in (out / "generate-valid.txt").read_text().splitlines() if l.startswith("H-")]

    assert _cli(d, ckpt, tmp_path / "a", extra="--no-repeat-ngram-size 3 --unkpen 0.5 --temperature 0.8") == 0
    assert len(h_lines(tmp_path / "a")) == 5
    for l in h_lines(tmp_path / "a"):
        units = l.split("\t")[2].split()
        assert not SR.has_repeated_ngram(units, 3)
    sampled = "--sampling --sampling-topk 10 --nbest 3 --seed 7"
    assert _cli(d, ckpt, tmp_path / "b", extra=sampled) == 0
    assert len(h_lines(tmp_path / "b")) == 15
    assert _cli(d, ckpt, tmp_path / "c", extra=sampled) == 0          # the stream replays
    assert h_lines(tmp_path / "c") == h_lines(tmp_path / "b")
    for bad, word in (("--sampling --sampling-topk 3 --sampling-topp 0.5", "exclude"), ("--temperature 0", "--temperature"),
                      ("--sampling-topk 3", "require --sampling")):
        with pytest.raises(SystemExit) as e:
            _cli(d, ckpt, tmp_path / "bad", extra=bad)
        assert word in str(e.value)

"""GPU: the scoring kernels (csrc/score.hip: ngram_stats, edit_distance) against the plain-Python oracle
(scoring_oracle.py), exact integers; the closing line of mms2ut-generate for ``--scoring bleu`` and
``--scoring wer`` recomputed from the ids in the written file; and the WER tool end to end.

The batches are built so that every path runs: both launch shapes (256 threads up to 1024 sort keys or
512 reference tokens, 1024 threads above), lengths around the sort's powers of two, the trims' corner
rows, unknowns on both sides, and the 4096-token limit."""
import functools

import numpy as np
import pytest
import torch

import scoring_oracle as O
from conftest import pkg

pytestmark = pytest.mark.gpu

PAD, EOS, UNK = 1, 2, 3
GRID = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000)
SHORT = tuple(g for g in GRID if g <= 257)      # ld_ref + ld_pred <= 1024: the 256-thread launches
LIMIT = 4096


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tokens(rng, n, nsym, p_unk=0.05):
    """n tokens over nsym symbols (ids from 4), a few of them <unk>."""
    t = rng.integers(4, 4 + nsym, n)
    t[rng.random(n) < p_unk] = UNK
    return [int(x) for x in t]


@functools.lru_cache(maxsize=None)
def bleu_batch(grid, seed):
    """64 (ref, pred) pairs: core lengths from the grid over 3-6 symbols (repeats make the clipping
    matter), pads on both ends, </s> and pads behind, <unk> on both sides, the trims' corner rows.
    -> (pairs, the oracle's ten integers)."""
    rng = np.random.default_rng(seed)
    pairs = [([EOS], [EOS]), ([PAD, EOS], [5, 6, EOS]), ([5, 6, EOS], [PAD, EOS]), ([PAD, PAD, PAD], [PAD, PAD]),
             ([], [5, EOS]), ([5, EOS], []), ([EOS, EOS], [PAD, 5, PAD, EOS, PAD]), ([UNK, EOS], [UNK, EOS])]
    while len(pairs) < 64:
        nsym = int(rng.integers(3, 7))
        m = int(rng.choice(grid))
        n = m if rng.random() < 0.3 else int(rng.choice(grid))

        def wrap(core):
            left = [PAD] * int(rng.integers(0, 3))
            right = [EOS] * int(rng.integers(0, 2)) + [PAD] * int(rng.integers(0, 3))
            return left + core + right

        ref = _tokens(rng, m, nsym)
        if m == n and rng.random() < 0.5:           # a noisy copy: long shared n-grams
            pred = [t if rng.random() > 0.1 else int(rng.integers(4, 4 + nsym)) for t in ref]
        else:
            pred = _tokens(rng, n, nsym)
        pairs.append((wrap(ref), wrap(pred)))
    return pairs, O.bleu_stats(pairs, PAD, EOS, UNK)


@functools.lru_cache(maxsize=None)
def wer_batch(grid, seed):
    """Pairs over the grid's lengths plus empty / non-empty, non-empty / empty, empty / empty and identical
    sequences -> (pairs, the oracle's distances)."""
    rng = np.random.default_rng(seed)
    same = _tokens(rng, int(max(grid)), 4, p_unk=0.0)
    pairs = [([], [5, 6, 7]), ([5, 6, 7], []), ([], []), (same, list(same)), ([UNK, 5], [UNK, 5])]
    for m in grid:
        for n in (m, int(rng.choice(grid)), int(rng.choice(grid))):
            nsym = int(rng.integers(3, 7))
            pairs.append((_tokens(rng, m, nsym), _tokens(rng, n, nsym)))
    return pairs, [O.levenshtein(r, p, UNK) for r, p in pairs]


@functools.lru_cache(maxsize=None)
def long_pair():
    rng = np.random.default_rng(7)
    a = [int(x) for x in rng.integers(4, 8, LIMIT)]
    b = [t if rng.random() > 0.2 else int(rng.integers(4, 8)) for t in a[3:]] + [int(x) for x in rng.integers(4, 8, 3)]
    assert len(a) == len(b) == LIMIT
    return a, b


def _ngram(pairs, stats=None):
    S, K = pkg("scoring"), pkg("kernels")
    if stats is None:
        stats = torch.zeros(10, dtype=torch.int64, device="cuda")
    K.ngram_stats(*S.upload_pairs([r for r, _ in pairs], [p for _, p in pairs], PAD, "cuda"), stats, PAD, EOS, UNK)
    return stats


def test_ngram_stats_worked_example():
    S = pkg("scoring")
    assert _ngram(O.EXAMPLE_PAIRS).tolist() == O.EXAMPLE_STATS
    sc = S.BleuScorer(PAD, EOS, UNK)
    sc.add_batch(*S.upload_pairs([r for r, _ in O.EXAMPLE_PAIRS], [p for _, p in O.EXAMPLE_PAIRS], PAD, "cuda"))
    assert sc.result_string() == O.EXAMPLE_STRING
    # without an unk the target's 3 matches the hypothesis' 3
    K = pkg("kernels")
    st = torch.zeros(10, dtype=torch.int64, device="cuda")
    K.ngram_stats(*S.upload_pairs([r for r, _ in O.EXAMPLE_PAIRS], [p for _, p in O.EXAMPLE_PAIRS], PAD, "cuda"), st,
                  PAD, EOS, None)
    assert st.tolist() == O.bleu_stats(O.EXAMPLE_PAIRS, PAD, EOS, None)


@pytest.mark.parametrize("grid", [SHORT, GRID], ids=["short", "full"])
def test_ngram_stats_random_batch(grid):
    pairs, want = bleu_batch(grid, 11)
    assert want[2] > 0 and want[8] > 0 and want[2] < want[3]          # matches at every order, and clipping
    got = _ngram(pairs).tolist()
    assert got == want
    assert _ngram(pairs).tolist() == got                              # a second run: the same bits


def test_ngram_stats_single_pairs_of_the_corner_rows():
    pairs, _ = bleu_batch(SHORT, 11)
    for r, p in pairs[:8]:
        assert _ngram([(r, p)]).tolist() == O.bleu_stats([(r, p)], PAD, EOS, UNK), (r, p)


def test_ngram_stats_4096_tokens():
    a, b = long_pair()
    want = O.bleu_stats([(a, b)], PAD, EOS, UNK)
    assert want[0] == want[1] == LIMIT and want[8] > 0
    assert _ngram([(a, b)]).tolist() == want


def test_ngram_stats_arbitrary_int32_tokens():
    """Tokens are not 16-bit units: the extremes of int32, negative ids, -999 itself."""
    rng = np.random.default_rng(3)
    vals = [-2 ** 31, 2 ** 31 - 1, -1, 0, -999, 70000, 65536 + 5, 5]
    a = [int(x) for x in rng.choice(vals, 300)]
    b = [int(x) for x in rng.choice(vals, 280)]
    assert _ngram([(a, b), (b, a)]).tolist() == O.bleu_stats([(a, b), (b, a)], PAD, EOS, UNK)


def test_ngram_stats_accumulates_across_batches():
    pairs, want = bleu_batch(GRID, 11)
    stats = _ngram(pairs[:20])
    _ngram(pairs[20:], stats)
    assert stats.tolist() == want
    assert _ngram([], stats).tolist() == want                          # an empty batch is a no-op


def test_length_limit_is_an_error_and_leaves_the_totals():
    K, L = pkg("kernels"), pkg("_lib")
    assert K.SCORE_MAX_LEN == LIMIT
    ok = torch.full((1, LIMIT), 5, dtype=torch.int32, device="cuda")
    over = torch.full((1, LIMIT + 1), 5, dtype=torch.int32, device="cuda")
    n_ok = torch.tensor([LIMIT], dtype=torch.int32, device="cuda")
    n_over = torch.tensor([LIMIT + 1], dtype=torch.int32, device="cuda")
    stats = torch.arange(10, dtype=torch.int64, device="cuda")
    totals = torch.tensor([7, 9], dtype=torch.int64, device="cuda")
    for ref, rl, pred, pl in ((over, n_over, ok, n_ok), (ok, n_ok, over, n_over)):
        with pytest.raises(L.HipError, match=f"limit of {LIMIT}"):
            K.ngram_stats(ref, rl, pred, pl, stats, PAD, EOS, UNK)
        with pytest.raises(L.HipError, match=f"limit of {LIMIT}"):
            K.edit_distance(ref, rl, pred, pl, totals, UNK)
    torch.cuda.synchronize()
    assert stats.tolist() == list(range(10)) and totals.tolist() == [7, 9]


@pytest.mark.parametrize("grid", [SHORT, GRID], ids=["short", "full"])
def test_edit_distance_batch(grid):
    S, K = pkg("scoring"), pkg("kernels")
    pairs, want = wer_batch(grid, 5)
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    up = S.upload_pairs([r for r, _ in pairs], [p for _, p in pairs], PAD, "cuda")
    dist = K.edit_distance(*up, totals, UNK, want_dist=True)
    assert dist.tolist() == want
    assert want[3] == 0 and want[4] == 1                               # identical; the target's unk never matches
    assert totals.tolist() == [sum(want), sum(len(r) for r, _ in pairs)]
    assert K.edit_distance(*up, totals, UNK) is None                   # no per-pair output: totals only
    assert totals.tolist() == [2 * sum(want), 2 * sum(len(r) for r, _ in pairs)]
    sc = S.WerScorer(UNK)
    sc.add_batch(*up)
    assert sc.result_string() == O.wer_string(sum(want), sum(len(r) for r, _ in pairs))


def test_edit_distance_4096_by_4096():
    S, K = pkg("scoring"), pkg("kernels")
    a, b = long_pair()
    want = O.levenshtein(a, b, UNK)
    assert 0 < want < LIMIT
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    dist = K.edit_distance(*S.upload_pairs([a, a, []], [b, a, b], PAD, "cuda"), totals, UNK, want_dist=True)
    assert dist.tolist() == [want, 0, LIMIT] and totals.tolist() == [want + LIMIT, 2 * LIMIT]


# ---------------------------------------------------------------------------------- the command-line tools

@pytest.fixture(scope="module")
def decoded(tmp_path_factory):
    """The five-utterance corpus and the edited tiny checkpoint of test_gpu_generate_cli."""
    from manifest_corpus import write_corpus
    from test_gpu_generate_cli import _checkpoint, _fusion_yaml
    tmp = tmp_path_factory.mktemp("scoring_cli")
    d = tmp / "data"
    d.mkdir()
    c = write_corpus(str(d), split="valid")
    ckpt = _checkpoint(tmp, d, _fusion_yaml(tmp, c["feat_dir"]))[0]
    return tmp, d, ckpt


def _pairs_of_file(text):
    """(target ids, best hypothesis ids) per sentence, both ending in </s>, from the T- and D- lines."""
    C, M = pkg("generate_cli"), pkg("manifest")
    dic = M.UnitDictionary.for_codes(1000)
    tgt = {int(l[2:].split("\t")[0]): l.split("\t")[1] for l in text.splitlines() if l.startswith("T-")}
    units = C.extract_units(text)
    assert sorted(tgt) == list(range(len(units)))
    return [(dic.encode_line(tgt[i]).tolist(), dic.encode_line(units[i]).tolist()) for i in sorted(tgt)]


def _expected(scoring, pairs):
    if scoring == "bleu":
        return O.bleu_string(O.bleu_stats(pairs, PAD, EOS, UNK))
    pairs = [(r[:-1], p[:-1]) for r, p in pairs]
    return O.wer_string(sum(O.levenshtein(r, p, UNK) for r, p in pairs), sum(len(r) for r, _ in pairs))


@pytest.mark.parametrize("extra", ["", "--scoring bleu --nbest 2", "--scoring wer", "--scoring wer --nbest 2"])
def test_cli_closing_line(decoded, extra):
    from test_gpu_generate_cli import BEAM, _cli
    tmp, d, ckpt = decoded
    out = tmp / ("out_" + extra.replace("-", "").replace(" ", "_"))
    assert _cli(d, ckpt, out, extra=extra) == 0
    text = (out / "generate-valid.txt").read_text()
    pairs = _pairs_of_file(text)
    assert len(pairs) == 5 and all(r[-1] == EOS and p[-1] == EOS for r, p in pairs)
    want = _expected("wer" if "wer" in extra else "bleu", pairs)
    assert text.splitlines()[-1] == f"Generate valid with beam={BEAM}: {want}"
    assert text.splitlines()[-2].startswith("Translated 5 sentences (")
    # --nbest prints more hypotheses; the pairs above are the best ones, so the score is that of --nbest 1
    assert sum(l.startswith("D-") for l in text.splitlines()) == (10 if "--nbest 2" in extra else 5)


def test_wer_tool(tmp_path, capsys):
    W = pkg("wer_cli")
    ref, hyp = tmp_path / "ref.txt", tmp_path / "hyp.txt"
    refs = ["a man rides a  horse", "two dogs play in the snow", "ein mann", "the end"]
    hyps = ["a man rides the horse ", "two dogs are playing in snow", "", "the end"]
    ref.write_text("\n".join(refs) + "\n")
    hyp.write_text("\n".join(hyps) + "\n")
    assert W.main(["--reference", str(ref), "--hypothesis", str(hyp)]) == 0
    got = capsys.readouterr().out.splitlines()
    assert got == O.wer_tool_lines([W.tokenize(l) for l in refs], [W.tokenize(l) for l in hyps])
    assert got == ["WER: 40.0%", "Errors: 6", "Reference words: 15"]

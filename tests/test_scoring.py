"""CPU: the host side of the scorers (scoring.py), ``--scoring`` on the mms2ut-generate command line and
the WER tool up to its device call (wer_cli.py), against the plain-Python oracle (scoring_oracle.py).
fairseq and jiwer are absent: their semantics are restated from the published sources."""
import pytest

import scoring_oracle as O
from conftest import pkg


def test_oracle_worked_example():
    stats = O.bleu_stats(O.EXAMPLE_PAIRS, O.EXAMPLE_PAD, O.EXAMPLE_EOS, O.EXAMPLE_UNK)
    assert stats == O.EXAMPLE_STATS
    assert O.bleu_string(stats) == O.EXAMPLE_STRING
    # without the unk rule pair 3 matches completely: the target's 3 is what keeps it from matching
    assert O.bleu_stats(O.EXAMPLE_PAIRS, O.EXAMPLE_PAD, O.EXAMPLE_EOS, None)[2] == 14
    trimmed = [(O.trim(r, 1, 2), O.trim(p, 1, 2)) for r, p in O.EXAMPLE_PAIRS]
    assert [O.levenshtein(r, p) for r, p in trimmed] == [1, 2, 0, 1]
    assert [O.levenshtein(r, p, unk=3) for r, p in trimmed] == [1, 2, 1, 1]


def test_oracle_trims():
    assert O.trim([1, 2], 1, 2) == [] and O.trim([2], 1, 2) == [2] and O.trim([1, 1, 1], 1, 2) == []
    assert O.trim([], 1, 2) == [] and O.trim([2, 2], 1, 2) == [2]
    assert O.trim([1, 1, 5, 1, 6, 2, 1], 1, 2) == [5, 1, 6]


def test_oracle_levenshtein_known_answers():
    assert O.levenshtein([], []) == 0 and O.levenshtein([], [1, 2, 3]) == 3 and O.levenshtein([4, 5], []) == 2
    assert O.levenshtein(list(b"kitten"), list(b"sitting")) == 3
    assert O.levenshtein(list(b"intention"), list(b"execution")) == 5


def test_bleu_scorer_worked_example():
    S = pkg("scoring")
    sc = S.BleuScorer.from_stats(O.EXAMPLE_STATS)
    assert sc.result_string() == O.EXAMPLE_STRING
    assert sc.stats() == dict(zip(S.BLEU_STATS, O.EXAMPLE_STATS))
    assert sc.precision() == [13 / 17, 7 / 13, 4 / 10, 2 / 7] and sc.brevity() == 1
    assert sc.result_string(order=2) == O.bleu_string(O.EXAMPLE_STATS, order=2)
    assert sc.result_string(order=2).startswith("BLEU2 = ") and sc.result_string(order=2).count("/") == 1


def test_bleu_scorer_brevity_penalty():
    S = pkg("scoring")
    stats = [20, 10, 8, 10, 5, 9, 3, 8, 2, 7]
    sc = S.BleuScorer.from_stats(stats)
    assert sc.result_string() == O.bleu_string(stats)
    assert "(BP=0.368, ratio=0.500, syslen=10, reflen=20)" in sc.result_string()


def test_bleu_scorer_zero_precision_scores_zero():
    S = pkg("scoring")
    stats = [9, 9, 5, 9, 2, 8, 1, 7, 0, 6]                  # no 4-gram matches: ln 0 = -inf
    sc = S.BleuScorer.from_stats(stats)
    assert sc.score() == 0.0
    assert sc.result_string() == "BLEU4 = 0.00, 55.6/25.0/14.3/0.0 (BP=1.000, ratio=1.000, syslen=9, reflen=9)"
    assert sc.result_string() == O.bleu_string(stats)


def test_bleu_scorer_empty_prediction_rule():
    S = pkg("scoring")
    for stats in ([5, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0] * 10, [0, 4, 0, 4, 0, 3, 0, 2, 0, 1]):
        sc = S.BleuScorer.from_stats(stats)
        assert sc.score() == 0.0
        assert sc.result_string() == (f"BLEU4 = 0.00, 0.0/0.0/0.0/0.0 (BP=0.000, ratio=0.000, syslen={stats[1]}, "
                                      f"reflen={stats[0]})")
        assert sc.result_string() == O.bleu_string(stats)


def test_wer_scorer_string():
    S = pkg("scoring")
    assert S.WerScorer.from_stats(5, 17).result_string() == "WER: 29.41" == O.wer_string(5, 17)
    assert S.WerScorer.from_stats(0, 0).result_string() == "WER: 0.00"
    assert S.WerScorer.from_stats(30, 20).result_string() == "WER: 150.00"
    assert S.WerScorer.from_stats(5, 17).score() == 100.0 * 5 / 17


def test_sentence_pair_per_scorer():
    S = pkg("scoring")
    target, hypo = [7, 3, 8, 2, 1, 1], [7, 9, 2]
    assert S.sentence_pair("bleu", target, hypo, 1, 2) == ([7, 3, 8, 2], [7, 9, 2])
    assert S.sentence_pair("wer", target, hypo, 1, 2) == ([7, 3, 8], [7, 9])
    assert S.sentence_pair("wer", [2], [2], 1, 2) == ([], [])


def test_upload_pairs_layout():
    S = pkg("scoring")
    ref, rl, pred, pl = S.upload_pairs([[5, 6, 7], [], [8]], [[9], [10, 11], []], 1, "cpu")
    assert ref.tolist() == [[5, 6, 7], [1, 1, 1], [8, 1, 1]] and rl.tolist() == [3, 0, 1]
    assert pred.tolist() == [[9, 1], [10, 11], [1, 1]] and pl.tolist() == [1, 2, 0]
    assert all(t.dtype.is_floating_point is False and t.element_size() == 4 for t in (ref, rl, pred, pl))
    ref, rl, pred, pl = S.upload_pairs([[], []], [[], []], 0, "cpu")
    assert tuple(ref.shape) == (2, 0) and tuple(pred.shape) == (2, 0) and rl.tolist() == pl.tolist() == [0, 0]


def test_scoring_flag():
    P = pkg("plugins")
    a = P.merge_generate_args(P.parse_generate_args(["/data", "--path", "c.pt"]), None)
    assert a.scoring == "bleu" and P.GENERATE_DEFAULTS["scoring"] == "bleu"
    a = P.merge_generate_args(P.parse_generate_args(["/data", "--path", "c.pt", "--scoring", "wer"]), None)
    assert a.scoring == "wer"
    # the default belongs to the run: a saved value never overrides it
    import argparse
    a = P.merge_generate_args(P.parse_generate_args(["/data", "--path", "c.pt"]), argparse.Namespace(scoring="wer"))
    assert a.scoring == "bleu"
    with pytest.raises(SystemExit) as e:
        P.parse_generate_args(["/data", "--path", "c.pt", "--scoring", "sacrebleu"])
    assert "sacrebleu" in str(e.value) and "bleu" in str(e.value) and "wer" in str(e.value)


def test_build_scorer():
    S = pkg("scoring")
    b = S.build_scorer("bleu", 1, 2, 3)
    assert isinstance(b, S.BleuScorer) and (b.pad, b.eos, b.unk) == (1, 2, 3)
    assert isinstance(S.build_scorer("wer", 1, 2, 3), S.WerScorer)
    with pytest.raises(SystemExit, match="bleu, wer"):
        S.build_scorer("chrf", 1, 2, 3)


def test_wer_tool_tokenisation():
    W = pkg("wer_cli")
    assert W.tokenize("  a  man   rides a\thorse \n") == ["a", "man", "rides", "a\thorse"]   # one tab is no run
    assert W.tokenize("a \t b") == ["a", "b"] and W.tokenize("") == [] and W.tokenize("   ") == []
    refs, hyps = W.encode([["a", "b", "a"], ["c"]], [["b", "a"], ["d", "c"]])
    assert refs == [[1, 2, 1], [3]] and hyps == [[2, 1], [4, 3]]


def test_wer_tool_file_errors(tmp_path):
    W = pkg("wer_cli")
    ref, hyp = tmp_path / "ref.txt", tmp_path / "hyp.txt"
    ref.write_text("a man rides\nthe  dog\n")
    hyp.write_text("a man  rides\n\n")
    assert W.read_pairs(str(ref), str(hyp)) == ([["a", "man", "rides"], ["the", "dog"]], [["a", "man", "rides"], []])
    hyp.write_text("a man rides\n")
    with pytest.raises(SystemExit, match="2 lines.*1"):
        W.read_pairs(str(ref), str(hyp))
    ref.write_text("a man rides\n  \nthe dog\n")
    hyp.write_text("x\ny\nz\n")
    with pytest.raises(SystemExit, match="line 2 is empty"):
        W.read_pairs(str(ref), str(hyp))


def test_wer_tool_output_format():
    W = pkg("wer_cli")
    assert W.format_result(157, 1033) == ["WER: 15.2%", "Errors: 157", "Reference words: 1033"]
    assert W.format_result(3, 2) == ["WER: 150.0%", "Errors: 3", "Reference words: 2"]
    assert W.format_result(3, 2) == O.wer_tool_lines([["a", "b"]], [["c", "d", "e"]])

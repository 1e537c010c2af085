"""CPU: the host side of mms2ut-generate (generate_cli.py) — fairseq-generate's line format, the
unit extraction that replaces the reference's grep/sed/sort/cut (2_inference_all.sh:91-93), and the
command line with its fall-back to the checkpoint's saved args.  fairseq is absent: the format is
restated from fairseq_cli/generate.py, not pinned against the library."""
import argparse
import math

import pytest
import torch

from conftest import pkg

LN2 = math.log(2)


def _dict():
    return pkg("manifest").UnitDictionary.for_codes(1000)


def test_hypothesis_lines():
    C = pkg("generate_cli")
    hypo = {"tokens": torch.tensor([4 + 17, 4 + 999, 4 + 0, 2]), "score": -1.25,
            "positional_scores": torch.tensor([-0.5, -2.0, -0.25, -2.25])}
    h, d, p = C.format_hypothesis(12, hypo, _dict())
    assert h == f"H-12\t{-1.25 / LN2}\t17 999 0"            # score / ln 2, str(); units without </s>
    assert d == "D" + h[1:]
    tag, pos = p.split("\t")
    assert tag == "P-12"
    assert pos.split(" ") == ["{:.4f}".format(x / LN2) for x in (-0.5, -2.0, -0.25, -2.25)]   # </s> included
    lines = C.format_sentence(3, "5 6 7", [hypo, dict(hypo, score=-2.0)], _dict(), nbest=2)
    assert [l.split("\t")[0] for l in lines] == ["T-3", "H-3", "D-3", "P-3", "H-3", "D-3", "P-3"]
    assert lines[0] == "T-3\t5 6 7"
    assert lines[4].split("\t")[1] == str(-2.0 / LN2)
    # a hypothesis that is </s> alone prints an empty unit string
    assert C.format_hypothesis(0, {"tokens": torch.tensor([2]), "score": -3.0,
                                   "positional_scores": torch.tensor([-3.0])}, _dict())[1].endswith("\t")


def _shell_extract(text):
    """grep "^D\\-" | sed 's/^D-//ig' | sort -nk1 | cut -f3, restated: numeric sort on the leading
    number of the line, the whole line as the tie-break."""
    rows = [l[2:] for l in text.splitlines() if l.startswith("D-")]
    rows.sort(key=lambda r: (float(r.split("\t")[0]), r))
    return [r.split("\t")[2] for r in rows]


def _text(ids, nbest):
    lines = []
    for i in ids:
        lines.append(f"T-{i}\t1 2 3")
        for n in range(nbest):
            units = f"{i} {n} 7"
            lines += [f"H-{i}\t{-0.5 - n}\t{units}", f"D-{i}\t{-0.5 - n}\t{units}", f"P-{i}\t-0.1000 -0.2000"]
    lines.append("Translated 12 sentences (40 tokens) in 0.1s (120.00 sentences/s, 400.00 tokens/s)")
    return "\n".join(lines) + "\n"


def test_extract_units_numeric_order():
    C = pkg("generate_cli")
    ids = [10, 2, 0, 11, 1, 9, 3, 12, 4, 8, 5, 7, 6]              # out of order, ids >= 10
    text = _text(ids, nbest=1)
    got = C.extract_units(text)
    assert got == [f"{i} 0 7" for i in range(13)]
    assert got == _shell_extract(text)
    lexical = [f"{i} 0 7" for i in sorted(ids, key=str)]
    assert got != lexical                                         # the case needs the numeric sort


def test_extract_units_takes_best_of_nbest():
    C = pkg("generate_cli")
    got = C.extract_units(_text([10, 2, 0, 11, 1], nbest=2))
    assert got == [f"{i} 0 7" for i in (0, 1, 2, 10, 11)]          # the first D- line of every id only


REFERENCE_ARGV = ("/data --config-yaml config.yaml --task multimodal_speech_to_speech --target-is-code "
                  "--target-code-size 1000 --vocoder code_hifigan --path /ckpt/checkpoint_last.pt "
                  "--gen-subset valid --max-tokens 8000 --beam 10 --max-len-a 1 "
                  "--required-batch-size-multiple 1 --multitask-config-yaml /mt.yaml "
                  "--multimodal-translation-config-yaml /mm.yaml --user-dir /src/mm_s2ut "
                  "--results-path /out").split()


def test_reference_command_line_parses():
    P = pkg("plugins")
    a = P.merge_generate_args(P.parse_generate_args(REFERENCE_ARGV), None)
    assert a.data == "/data" and a.path == "/ckpt/checkpoint_last.pt" and a.results_path == "/out"
    assert (a.gen_subset, a.max_tokens, a.beam, a.max_len_a) == ("valid", 8000, 10, 1.0)
    assert a.multitask_config_yaml == "/mt.yaml" and a.multimodal_translation_config_yaml == "/mm.yaml"
    assert a.target_is_code and a.target_code_size == 1000
    # fairseq-generate's defaults where a flag is omitted
    assert (a.max_len_b, a.lenpen, a.min_len, a.nbest) == (200, 1.0, 1, 1)
    b = P.merge_generate_args(P.parse_generate_args(["/data", "--path", "c.pt"]), None)
    assert (b.beam, b.max_len_a, b.max_len_b, b.lenpen, b.min_len, b.nbest, b.gen_subset) == \
        (5, 0.0, 200, 1.0, 1, 1, "test")
    assert b.noise_config_yaml is None and not b.skip_invalid_size_inputs_valid_test


def test_saved_args_fill_missing_flags():
    P = pkg("plugins")
    saved = argparse.Namespace(task="multimodal_speech_to_speech", multimodal_translation_config_yaml="/saved/mm.yaml",
                               config_yaml="saved.yaml", target_code_size=500, encoder_layers=2, data="/train",
                               beam=3, gen_subset="train_dev", max_tokens=40000, noise_config_yaml="/saved/noise.yaml")
    given = P.parse_generate_args(["/data", "--path", "c.pt", "--config-yaml", "config.yaml", "--max-tokens", "800"])
    a = P.merge_generate_args(given, saved)
    assert a.multimodal_translation_config_yaml == "/saved/mm.yaml"      # omitted: from the checkpoint
    assert a.target_code_size == 500 and a.encoder_layers == 2
    assert a.config_yaml == "config.yaml" and a.data == "/data"          # given: the command line wins
    # run flags are fairseq-generate's, never the training run's
    assert (a.beam, a.gen_subset, a.max_tokens, a.noise_config_yaml) == (5, "test", 800, None)
    given = P.parse_generate_args(["/data", "--path", "c.pt", "--multimodal-translation-config-yaml", "/mine.yaml",
                                   "--target-code-size", "1000"])
    a = P.merge_generate_args(given, saved)
    assert a.multimodal_translation_config_yaml == "/mine.yaml" and a.target_code_size == 1000


def test_batch_size_multiple_refused(capsys):
    P = pkg("plugins")
    with pytest.raises(SystemExit):
        P.parse_generate_args(["/data", "--path", "c.pt", "--required-batch-size-multiple", "8"])
    assert "required-batch-size-multiple" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        P.merge_generate_args(P.parse_generate_args(["/data", "--path", "c.pt", "--nbest", "6"]), None)

"""GPU: mms2ut-train with a valid split — validation records, checkpoint_best.pt / checkpoint_last.pt,
``best`` across a resume, and the warning when the split is missing."""
import argparse
import json
import os
import shutil

import pytest
import torch

from conftest import pkg
from test_gpu_plugins import TINY
from test_plugins import FUSION_YAML

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _corpus(tmp_path, valid=True):
    """A train split; valid = its first four utterances (same WAVs, the image features copied:
    writing a second corpus would overwrite WAVs of the same names)."""
    from manifest_corpus import write_corpus
    d = tmp_path / "data"
    d.mkdir()
    c = write_corpus(str(d), frames=(150, 97, 200, 61, 88, 131, 45, 170), di=768, ti=12, split="train")
    if valid:
        lines = (d / "train.tsv").read_text().splitlines()
        (d / "valid.tsv").write_text("\n".join(lines[:5]) + "\n")
        for suffix in (".pth", "_mask.pth"):
            shutil.copy(os.path.join(c["feat_dir"], "train" + suffix), os.path.join(c["feat_dir"], "valid" + suffix))
    y = tmp_path / "mm.yaml"
    y.write_text(FUSION_YAML.replace('["/feats/vit_base_patch16_384"]', f'["{c["feat_dir"]}"]'))
    return d, y


def _argv(d, y, save_dir, extra=""):
    return (f"{d} --task multimodal_speech_to_speech --arch mm_s2ut_transformer --criterion speech_to_unit "
            f"--config-yaml config.yaml --target-is-code --target-code-size 1000 "
            f"--share-decoder-input-output-embed --fp16 --multimodal-translation-config-yaml {y} {TINY} "
            f"--max-tokens 600 --max-tokens-valid 300 --log-interval 6 --warmup-updates 4 --lr 1e-3 "
            f"--train-subset train --valid-subset valid --save-dir {save_dir} {extra}").split()


def _records(capsys):
    cap = capsys.readouterr()
    recs = [json.loads(l) for l in cap.out.splitlines() if l.startswith("{")]
    return [r for r in recs if "subset" in r], [r for r in recs if "subset" not in r], cap.err


def _load(path):
    with torch.serialization.safe_globals([argparse.Namespace]):
        return torch.load(path, map_location="cpu", weights_only=True)


def test_cli_validates_and_keeps_the_best_checkpoint(tmp_path, capsys):
    C, P = pkg("generate_cli"), pkg("plugins")
    d, y = _corpus(tmp_path)
    sd = tmp_path / "ck"
    run = "--max-update 6 --validate-interval-updates 2 --report-accuracy"
    assert pkg("cli").main(_argv(d, y, sd, run)) == 0
    valid, train, err = _records(capsys)
    assert "validation is disabled" not in err
    assert len(valid) >= 3 and {2, 4, 6} <= {r["num_updates"] for r in valid}
    assert [r["num_updates"] for r in train] == [6] and "accuracy" not in train[0]
    for r in valid:
        assert r["subset"] == "valid" and r["ntokens"] > 0 and r["nsentences"] == 4
        assert r["loss"] > 0 and r["nll_loss"] > 0 and r["ppl"] == 2.0 ** r["nll_loss"]
        assert 0.0 <= r["accuracy"] <= 100.0
    losses = [r["loss"] for r in valid]
    assert [r["best_loss"] for r in valid] == [min(losses[:i + 1]) for i in range(len(losses))]
    best_path, last_path = sd / "checkpoint_best.pt", sd / "checkpoint_last.pt"
    assert best_path.exists() and last_path.exists()
    assert sorted(os.listdir(sd)) == ["checkpoint_best.pt", "checkpoint_last.pt"]
    best = C.load_checkpoint(str(best_path))                   # mms2ut-generate's loader
    assert best["extra_state"]["best"] == min(losses)
    assert best["extra_state"]["val_loss"] == best["extra_state"]["best"]
    last = _load(last_path)
    assert last["extra_state"]["best"] == min(losses) and last["extra_state"]["val_loss"] == losses[-1]
    assert last["extra_state"]["num_updates"] == 6
    args = P.merge_generate_args(argparse.Namespace(path=str(best_path), data=str(d)), best["args"])
    _, model = C.build_model(args, best, torch.device("cuda", 0))
    assert not model.net.training

    # resumed at --max-update: nothing to train, checkpoint_best.pt is not rewritten
    content, mtime = best_path.read_bytes(), os.stat(best_path).st_mtime_ns
    assert pkg("cli").main(_argv(d, y, sd, run)) == 0
    valid2, _, _ = _records(capsys)
    assert valid2 == []
    assert os.stat(best_path).st_mtime_ns == mtime and best_path.read_bytes() == content
    assert _load(last_path)["extra_state"]["best"] == min(losses)

    # resumed with a restored best no validation can reach: two more updates validate and keep it
    last["extra_state"]["best"] = 0.0
    torch.save(last, last_path)
    assert pkg("cli").main(_argv(d, y, sd, run.replace("--max-update 6", "--max-update 8"))) == 0
    valid3, _, _ = _records(capsys)
    assert valid3 and valid3[-1]["num_updates"] == 8 and all(r["best_loss"] == 0.0 for r in valid3)
    assert os.stat(best_path).st_mtime_ns == mtime and best_path.read_bytes() == content
    assert _load(last_path)["extra_state"]["best"] == 0.0 and _load(last_path)["extra_state"]["num_updates"] == 8


def test_cli_without_the_valid_split_warns_and_trains(tmp_path, capsys):
    d, y = _corpus(tmp_path, valid=False)
    sd = tmp_path / "ck"
    assert pkg("cli").main(_argv(d, y, sd, "--max-update 3 --validate-interval-updates 1")) == 0
    valid, train, err = _records(capsys)
    assert valid == [] and [r["num_updates"] for r in train] == [3]
    assert err.count("validation is disabled") == 1 and "valid.tsv" in err
    assert os.listdir(sd) == ["checkpoint_last.pt"]

"""Validation / checkpoint policy of mms2ut-train on the host (validation.ValidationPolicy): the new
flags and their fairseq defaults, checkpoint_best.pt's rule (ties overwrite, NaN never best),
--patience, the extra_state round trip, the validate / save decisions at every kind of boundary and
the valid record's format."""
import argparse
import math

import pytest

from conftest import pkg
from test_plugins import CANONICAL


def _parse(extra=""):
    return pkg("plugins").build_parser().parse_args(["/d", "--fp16"] + extra.split())


def _policy(extra="", enabled=True):
    return pkg("validation").ValidationPolicy(_parse(extra), enabled=enabled)


def _stats(loss=3.0, nll=2.0, acc=25.0, ntok=40, nsent=5):
    return {"loss": loss, "nll_loss": nll, "ppl": 2.0 ** nll, "accuracy": acc, "ntokens": ntok, "nsentences": nsent}


def test_new_flags_have_fairseq_defaults():
    a = _parse("--max-tokens 1234")
    assert a.max_tokens_valid == 1234
    assert a.validate_interval == 1 and a.validate_interval_updates == 0 and a.validate_after_updates == 0
    assert a.disable_validation is False and a.skip_invalid_size_inputs_valid_test is False
    assert a.best_checkpoint_metric == "loss" and a.maximize_best_checkpoint_metric is False
    assert a.patience == -1 and a.report_accuracy is False and a.no_epoch_checkpoints is False
    b = _parse("--max-tokens 1234 --max-tokens-valid 99 --best-checkpoint-metric accuracy "
               "--maximize-best-checkpoint-metric --patience 3 --report-accuracy --no-epoch-checkpoints "
               "--validate-interval 2 --validate-interval-updates 50 --validate-after-updates 10 "
               "--disable-validation --skip-invalid-size-inputs-valid-test")
    assert b.max_tokens_valid == 99 and b.best_checkpoint_metric == "accuracy" and b.patience == 3
    assert b.maximize_best_checkpoint_metric and b.report_accuracy and b.no_epoch_checkpoints
    assert (b.validate_interval, b.validate_interval_updates, b.validate_after_updates) == (2, 50, 10)
    assert b.disable_validation and b.skip_invalid_size_inputs_valid_test
    for m in ("loss", "nll_loss", "ppl", "accuracy"):
        assert _parse(f"--best-checkpoint-metric {m}").best_checkpoint_metric == m
    with pytest.raises(SystemExit):
        _parse("--best-checkpoint-metric bleu")


def test_canonical_command_still_parses():
    a = pkg("plugins").build_parser().parse_args(CANONICAL.format(yaml="mm.yaml").split())
    assert a.valid_subset == "valid" and a.train_subset == "train"
    assert a.max_tokens_valid == a.max_tokens == 40000
    p = pkg("validation").ValidationPolicy(a)
    assert p.metric == "loss" and not p.maximize and p.patience == -1 and p.enabled


def test_minimise_ties_overwrite():
    p = _policy()
    wrote = [p.update(_stats(loss=v))[0] for v in (3.0, 2.0, 2.0, 2.5)]
    assert wrote == [True, True, True, False]
    assert p.best == 2.0 and p.val_loss == 2.5


def test_maximise_mirrored():
    p = _policy("--best-checkpoint-metric accuracy --maximize-best-checkpoint-metric")
    wrote = [p.update(_stats(acc=v))[0] for v in (10.0, 20.0, 20.0, 15.0)]
    assert wrote == [True, True, True, False]
    assert p.best == 20.0


def test_nan_is_never_best():
    for extra in ("", "--maximize-best-checkpoint-metric"):
        p = _policy(extra)
        assert p.update(_stats(loss=float("nan")))[0] is False and p.best is None   # not even as the first
        assert p.update(_stats(loss=float("inf")))[0] is False and p.best is None
        assert p.update(_stats(loss=3.0))[0] is True
        assert p.update(_stats(loss=float("nan")))[0] is False and p.best == 3.0


def test_patience_counts_consecutive_non_improvements():
    p = _policy("--patience 2")
    stops = [p.update(_stats(loss=v))[1] for v in (3.0, 3.5, 2.9, 2.9, 3.0)]
    # 3.5: one run; 2.9 improves and resets; 2.9 (a tie is no improvement): one; 3.0: two -> stop
    assert stops == [False, False, False, False, True]
    q = _policy("--patience 2")
    assert [q.update(_stats(loss=v))[1] for v in (3.0, 3.1, 3.2)] == [False, False, True]
    off = _policy()     # --patience -1
    assert not any(off.update(_stats(loss=v))[1] for v in (1.0, 2.0, 3.0, 4.0, 5.0))
    mx = _policy("--patience 1 --best-checkpoint-metric accuracy --maximize-best-checkpoint-metric")
    assert [mx.update(_stats(acc=v))[1] for v in (10.0, 11.0, 10.5)] == [False, False, True]


def test_extra_state_round_trip():
    p = _policy("--patience 2")
    p.update(_stats(loss=2.0))
    p.update(_stats(loss=2.4))
    es = p.extra_state()
    assert es == {"val_loss": 2.4, "best": 2.0}
    q = _policy("--patience 2")
    q.load_extra_state(dict(es, num_updates=7))
    assert q.best == 2.0 and q.run_best is None and q.num_runs == 0     # patience state is the run's own
    assert q.update(_stats(loss=2.2)) == (False, False)                  # worse than the restored best
    assert q.best == 2.0
    assert q.update(_stats(loss=1.9))[0] is True and q.best == 1.9
    old = _policy()
    old.load_extra_state({"num_updates": 7, "train_iterator": {"epoch": 2}})   # a checkpoint without "best"
    assert old.best is None and old.update(_stats(loss=9.0))[0] is True
    none = _policy()
    none.load_extra_state(None)
    assert none.best is None


def test_boundaries_validate_interval_updates():
    p = _policy("--validate-interval-updates 3")
    got = {u: p.boundary(u) for u in range(1, 8)}
    assert [u for u, (v, s) in got.items() if v] == [3, 6]
    assert not any(s for v, s in got.values())
    assert [u for u in range(0, 8) if p.is_update_boundary(u)] == [3, 6]


def test_boundaries_save_interval_updates():
    p = _policy("--save-interval-updates 4")
    got = {u: p.boundary(u) for u in range(1, 10)}
    assert [u for u, (v, s) in got.items() if v] == [4, 8]      # every mid-epoch save validates first
    assert [u for u, (v, s) in got.items() if s] == [4, 8]
    assert [u for u in range(0, 10) if p.is_update_boundary(u)] == [4, 8]


def test_boundaries_epoch_end_and_stop():
    p = _policy()
    assert p.boundary(5, epoch=1, end_of_epoch=True) == (True, True)
    assert p.boundary(7, epoch=2) == (False, False)
    q = _policy("--validate-interval 2")
    assert q.boundary(5, epoch=1, end_of_epoch=True) == (False, True)    # checkpoint_last at every epoch end
    assert q.boundary(10, epoch=2, end_of_epoch=True) == (True, True)
    # the stop validates; its checkpoint is the one written after the loop
    assert _policy().boundary(9, epoch=3, stop=True) == (True, False)
    # an interval that fell on the epoch's last step is not validated / saved twice at the epoch end
    r = _policy("--save-interval-updates 4")
    assert r.boundary(4, epoch=1) == (True, True)
    assert r.boundary(4, epoch=1, end_of_epoch=True) == (False, False)
    assert r.boundary(6, epoch=2, end_of_epoch=True) == (True, True)


def test_boundaries_validate_after_updates_and_disable():
    p = _policy("--validate-interval-updates 2 --save-interval-updates 2 --validate-after-updates 5")
    assert p.boundary(2) == (False, False) and p.boundary(4) == (False, False)
    assert p.boundary(3, epoch=1, end_of_epoch=True) == (False, True)
    assert p.boundary(4, epoch=1, stop=True) == (False, False)
    assert p.boundary(6) == (True, True)
    d = _policy("--validate-interval-updates 2 --save-interval-updates 4 --disable-validation")
    assert not d.enabled
    assert d.boundary(2) == (False, False) and d.boundary(4) == (False, True)
    assert d.boundary(5, epoch=1, end_of_epoch=True) == (False, True) and d.boundary(6, stop=True) == (False, False)
    off = _policy("--validate-interval-updates 2", enabled=False)    # no valid split / --synthetic
    assert off.boundary(2) == (False, False) and off.boundary(3, end_of_epoch=True) == (False, True)


def test_valid_stats_and_record_format():
    T = pkg("trainer")
    ln2 = math.log(2.0)
    st = T.valid_stats(loss=80.0 * ln2, nll=60.0 * ln2, ntokens=40, n_correct=10, nsentences=5)
    assert st["ntokens"] == 40 and st["nsentences"] == 5
    assert st["loss"] == pytest.approx(2.0, rel=1e-12) and st["nll_loss"] == pytest.approx(1.5, rel=1e-12)
    assert st["ppl"] == pytest.approx(2.0 ** 1.5, rel=1e-12) and st["accuracy"] == 25.0
    empty = T.valid_stats(0.0, 0.0, 0, 0, 0)
    assert all(math.isnan(empty[k]) for k in ("loss", "nll_loss", "ppl", "accuracy"))
    p = _policy()
    p.update(st)
    rec = p.record("valid", 2, 6, st)
    assert list(rec) == ["subset", "epoch", "num_updates", "loss", "nll_loss", "ppl", "ntokens", "nsentences",
                         "best_loss"]
    assert rec["subset"] == "valid" and rec["epoch"] == 2 and rec["num_updates"] == 6
    assert rec["best_loss"] == rec["loss"] == st["loss"]
    q = _policy("--report-accuracy --best-checkpoint-metric nll_loss")
    q.update(st)
    rec = q.record("valid", 1, 3, st)
    assert rec["accuracy"] == 25.0 and rec["best_nll_loss"] == st["nll_loss"] and "best_loss" not in rec


def test_policy_from_old_namespace():
    """Args saved by a run before these flags existed: every default applies."""
    p = pkg("validation").ValidationPolicy(argparse.Namespace(save_interval_updates=0))
    assert p.metric == "loss" and p.patience == -1 and p.enabled and p.boundary(3) == (False, False)

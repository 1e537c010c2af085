"""Validation / checkpoint policy of ``mms2ut-train``: fairseq's ``validate_and_save``,
``checkpoint_utils.save_checkpoint`` ("best" bookkeeping) and ``should_stop_early`` as one host-only
object.  No device, no files: the CLI asks it what to do at each boundary and does the work.

  * when to validate / save (``boundary``): epoch ends (``--validate-interval``),
    ``--validate-interval-updates``, every mid-epoch ``--save-interval-updates`` save, the stop;
    never before ``--validate-after-updates``; ``--disable-validation``
  * checkpoint_best.pt (``update``): written when there is no best yet or the metric
    ``is_better`` than the best, ties included (``<=``, ``>=`` with
    ``--maximize-best-checkpoint-metric``); a non-finite metric is never better
  * ``--patience N``: stop after N consecutive validations without a strict improvement over the
    run's own best (not restored on resume, as fairseq's function attribute)
  * ``extra_state`` round trip: ``val_loss`` and ``best``
"""
import math

METRICS = ("loss", "nll_loss", "ppl", "accuracy")


class ValidationPolicy:
    def __init__(self, args, enabled=True):
        g = lambda k, d: getattr(args, k, d)   # noqa: E731
        self.metric = g("best_checkpoint_metric", "loss")
        if self.metric not in METRICS:
            raise ValueError(f"--best-checkpoint-metric {self.metric!r}: one of {', '.join(METRICS)}")
        self.maximize = bool(g("maximize_best_checkpoint_metric", False))
        self.patience = int(g("patience", -1))
        self.validate_interval = max(1, int(g("validate_interval", 1)))
        self.validate_interval_updates = int(g("validate_interval_updates", 0))
        self.validate_after_updates = int(g("validate_after_updates", 0))
        self.save_interval_updates = int(g("save_interval_updates", 0) or 0)
        self.report_accuracy = bool(g("report_accuracy", False))
        self.enabled = bool(enabled) and not g("disable_validation", False)
        self.best = None        # best metric any checkpoint_best.pt holds (restored on resume)
        self.val_loss = None    # the last validation's metric
        self.run_best = None    # patience: this run's own best
        self.num_runs = 0       # patience: consecutive validations without improvement
        self.validated_at = self.saved_at = None   # update counts of the last validation / save

    # ------------------------------------------------------------------ decisions
    def is_better(self, a, b):
        """checkpoint_best.pt's rule: ties overwrite (fairseq save_checkpoint)."""
        return a >= b if self.maximize else a <= b

    def is_update_boundary(self, num_updates):
        """Does this update count end on a validate / save interval?  (The loop reads the exact
        count from the device only where this, the log interval or the stop can be true.)"""
        return any(n > 0 and num_updates > 0 and num_updates % n == 0
                   for n in (self.validate_interval_updates, self.save_interval_updates))

    def boundary(self, num_updates, epoch=1, end_of_epoch=False, stop=False):
        """-> (do_validate, do_save) after update ``num_updates`` (fairseq validate_and_save;
        validate first, then save).  ``stop``: --max-update is reached; the checkpoint of the stop
        is the one written after the loop, so a stop asks for no save here."""
        after = num_updates >= self.validate_after_updates
        siu, viu = self.save_interval_updates, self.validate_interval_updates
        do_save = bool(end_of_epoch or (siu > 0 and num_updates > 0 and num_updates % siu == 0 and after))
        do_validate = ((not end_of_epoch and do_save)
                       or (end_of_epoch and epoch % self.validate_interval == 0)
                       or stop
                       or (viu > 0 and num_updates > 0 and num_updates % viu == 0))
        do_validate = bool(do_validate and self.enabled and after)
        # the caller does what is returned: an epoch end that falls on an update already validated /
        # saved (an interval hit on the epoch's last step) does not repeat it
        do_validate = do_validate and num_updates != self.validated_at
        do_save = do_save and not stop and num_updates != self.saved_at
        if do_validate:
            self.validated_at = num_updates
        if do_save:
            self.saved_at = num_updates
        return do_validate, do_save

    def update(self, stats):
        """Take one validation's stats (of the first --valid-subset) -> (write_best, stop_early)."""
        v = float(stats[self.metric])
        self.val_loss = v
        finite = math.isfinite(v)
        write = finite and (self.best is None or self.is_better(v, self.best))
        if write:
            self.best = v
        stop = False
        if self.patience > 0:     # fairseq should_stop_early: strict improvement resets the count
            improved = finite and (self.run_best is None or
                                   (v > self.run_best if self.maximize else v < self.run_best))
            if improved:
                self.run_best, self.num_runs = v, 0
            else:
                self.num_runs += 1
                stop = self.num_runs >= self.patience
        return write, stop

    # ------------------------------------------------------------------ checkpoint round trip
    def extra_state(self):
        return {"val_loss": self.val_loss, "best": self.best}

    def load_extra_state(self, es):
        """``best`` of a restored checkpoint (absent in older files: no best yet).  The patience
        state is the run's own and starts fresh."""
        b = (es or {}).get("best")
        self.best = float(b) if b is not None and math.isfinite(float(b)) else None
        self.val_loss = (es or {}).get("val_loss")

    # ------------------------------------------------------------------ logging
    def record(self, subset, epoch, num_updates, stats):
        """The JSON record of one validation (base-2 per-token values, as the training records)."""
        rec = {"subset": subset, "epoch": epoch, "num_updates": num_updates, "loss": stats["loss"],
               "nll_loss": stats["nll_loss"], "ppl": stats["ppl"]}
        if self.report_accuracy:
            rec["accuracy"] = stats["accuracy"]
        rec.update(ntokens=stats["ntokens"], nsentences=stats["nsentences"])
        rec[f"best_{self.metric}"] = self.best
        return rec

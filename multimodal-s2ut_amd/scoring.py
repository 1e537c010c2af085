"""Scorers over generated token sequences: what fairseq-generate prints on its last line.

``BleuScorer`` mirrors fairseq ``scoring/bleu.py`` ``Scorer`` (the built-in token BLEU over libbleu's
``bleu_add`` statistics, the default of ``--scoring``), ``WerScorer`` mirrors ``scoring/wer.py``
``WerScorer`` (``--scoring wer``).  The statistics are integers computed and accumulated on the device
(``kernels.ngram_stats`` / ``kernels.edit_distance``, csrc/score.hip); ``add_batch`` only launches, and
the first ``stats()`` / ``score()`` / ``result_string()`` does the one host read.  The score and its
string are formed on the host from those integers in Python floats, exactly as fairseq does.

fairseq is not importable here: these semantics are restated from its published source and are not
pinned against the library (as generate_cli.py's output format).
"""
import math

import torch

BLEU_STATS = ("reflen", "predlen", "match1", "count1", "match2", "count2", "match3", "count3", "match4", "count4")
SCORERS = ("bleu", "wer")


def upload_pairs(refs, preds, pad, device):
    """Host token lists -> device (ref [n, ld_ref], ref_len [n], pred [n, ld_pred], pred_len [n]) int32,
    right-padded with ``pad``, as one pinned host buffer and one copy."""
    n = len(refs)
    assert len(preds) == n
    ldr, ldp = max([len(r) for r in refs] + [0]), max([len(p) for p in preds] + [0])
    host = torch.full((n * (ldr + ldp + 2),), int(pad), dtype=torch.int32)
    views = (host[:n * ldr].view(n, ldr), host[n * ldr:n * ldr + n],
             host[n * (ldr + 1):n * (ldr + 1 + ldp)].view(n, ldp), host[n * (ldr + 1 + ldp):])
    for i, (r, p) in enumerate(zip(refs, preds)):
        views[0][i, :len(r)] = torch.as_tensor(r, dtype=torch.int32)
        views[2][i, :len(p)] = torch.as_tensor(p, dtype=torch.int32)
        views[1][i], views[3][i] = len(r), len(p)
    device = torch.device(device)
    if device.type == "cuda" and host.numel():
        host = host.pin_memory()
    dev = host.to(device, non_blocking=True)
    return (dev[:n * ldr].view(n, ldr), dev[n * ldr:n * ldr + n],
            dev[n * (ldr + 1):n * (ldr + 1 + ldp)].view(n, ldp), dev[n * (ldr + 1 + ldp):])


class BleuScorer:
    """fairseq ``scoring.bleu.Scorer(pad, eos, unk)``.

    Where fairseq would divide by zero (``predlen == 0`` in ``brevity``, ``reflen == 0`` in the ratio of
    ``result_string``: nothing scored, or only empty sequences) this reports score 0.00, BP 0.000 and ratio
    0.000 instead of raising."""

    def __init__(self, pad, eos, unk=None):
        self.pad, self.eos, self.unk = int(pad), int(eos), -1 if unk is None else int(unk)
        self._dev = None          # int64 [10] on the device, allocated by the first add_batch
        self._host = [0] * 10     # what was read back (or given to from_stats)
        self._dirty = False

    @classmethod
    def from_stats(cls, stats, pad=1, eos=2, unk=3):
        """A scorer over ten given integers (BLEU_STATS order): the host formulas without a device."""
        s = cls(pad, eos, unk)
        s._host = [int(x) for x in stats]
        assert len(s._host) == 10
        return s

    def add_batch(self, ref, ref_len, pred, pred_len):
        """Device int32 ref [n, ld_ref], ref_len [n], pred [n, ld_pred], pred_len [n]: launch only."""
        from . import kernels as K
        if self._dev is None:
            self._dev = torch.tensor(self._host, dtype=torch.int64, device=ref.device)
        K.ngram_stats(ref, ref_len, pred, pred_len, self._dev, self.pad, self.eos, self.unk)
        self._dirty = True

    def stats(self):
        """-> {name: int} of the ten statistics; the one device -> host read."""
        if self._dirty:
            self._host = [int(x) for x in self._dev.cpu().tolist()]
            self._dirty = False
        return dict(zip(BLEU_STATS, self._host))

    def precision(self):
        s = self.stats()
        return [s[f"match{n}"] / s[f"count{n}"] if s[f"count{n}"] > 0 else 0 for n in (1, 2, 3, 4)]

    def brevity(self):
        s = self.stats()
        if s["predlen"] == 0:
            return 0.0
        return min(1, math.exp(1 - s["reflen"] / s["predlen"]))

    def score(self, order=4):
        if self.stats()["predlen"] == 0 or self.stats()["reflen"] == 0:
            return 0.0
        psum = sum(math.log(p) if p > 0 else float("-Inf") for p in self.precision()[:order])
        return self.brevity() * math.exp(psum / order) * 100

    def result_string(self, order=4):
        assert 1 <= order <= 4, "BLEU scores for order > 4 aren't supported"
        s = self.stats()
        fmt = "BLEU{} = {:2.2f}, {:2.1f}" + "/{:2.1f}" * (order - 1) + " (BP={:.3f}, ratio={:.3f}, syslen={}, reflen={})"
        degenerate = s["predlen"] == 0 or s["reflen"] == 0
        return fmt.format(order, self.score(order=order), *[p * 100 for p in self.precision()[:order]],
                          0.0 if degenerate else self.brevity(), 0.0 if degenerate else s["predlen"] / s["reflen"],
                          s["predlen"], s["reflen"])


class WerScorer:
    """fairseq ``scoring.wer.WerScorer``: 100 * (sum of edit distances) / (sum of reference lengths) over
    the pairs added, 0 where no reference token was added.  ``unk``: a reference token that never matches."""

    def __init__(self, unk=None):
        self.unk = -1 if unk is None else int(unk)
        self._dev = None          # int64 [2] on the device: distance, ref_length
        self._host = [0, 0]
        self._dirty = False

    @classmethod
    def from_stats(cls, distance, ref_length):
        s = cls()
        s._host = [int(distance), int(ref_length)]
        return s

    def add_batch(self, ref, ref_len, pred, pred_len, want_dist=False):
        """Layout as BleuScorer.add_batch; launch only.  -> the int32 [n] distances with want_dist."""
        from . import kernels as K
        if self._dev is None:
            self._dev = torch.tensor(self._host, dtype=torch.int64, device=ref.device)
        self._dirty = True
        return K.edit_distance(ref, ref_len, pred, pred_len, self._dev, self.unk, want_dist=want_dist)

    def stats(self):
        if self._dirty:
            self._host = [int(x) for x in self._dev.cpu().tolist()]
            self._dirty = False
        return {"distance": self._host[0], "ref_length": self._host[1]}

    def score(self):
        s = self.stats()
        return 100.0 * s["distance"] / s["ref_length"] if s["ref_length"] > 0 else 0

    def result_string(self):
        return "WER: {:.2f}".format(self.score())


def build_scorer(name, pad, eos, unk):
    """``--scoring`` -> scorer."""
    if name == "bleu":
        return BleuScorer(pad, eos, unk)
    if name == "wer":
        return WerScorer(unk)
    raise SystemExit(f"unknown --scoring {name!r}; the scorers are {', '.join(SCORERS)}")


def sentence_pair(name, target, tokens, pad, eos):
    """What fairseq-generate scores for one sentence, as two lists of ids: ``target`` the sample's padded
    target row, ``tokens`` the best hypothesis (both end in </s>).  bleu: the rows with pad stripped; wer:
    the unit strings split on spaces, i.e. both without </s>."""
    ref = [t for t in target if t != pad]
    hyp = list(tokens)
    if name == "wer":
        ref = ref[:-1] if ref and ref[-1] == eos else ref
        hyp = hyp[:-1] if hyp and hyp[-1] == eos else hyp
    return ref, hyp

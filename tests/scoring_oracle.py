"""Plain-Python restatements for the scoring tests: libbleu's bleu_add (trims, clipped n-gram matches),
fairseq's BLEU / WER result strings, and a Levenshtein distance whose row update is vectorised.
fairseq is not importable here; restated from its published source (scoring/bleu.py, clib/libbleu,
scoring/wer.py)."""
import math
from collections import Counter

import numpy as np

UNK_REPLACED = -999


def trim(seq, pad, eos):
    """libbleu bleu_trim: bleu_rtrim (eos / pad from the right while end > 0), then bleu_ltrim (pad)."""
    s = list(seq)
    if s:
        end = len(s) - 1
        while end > 0 and (s[end] == eos or s[end] == pad):
            end -= 1
        s = s[:end + 1]
    start = 0
    while start < len(s) and s[start] == pad:
        start += 1
    return s[start:]


def replace_unk(ref, unk):
    return [UNK_REPLACED if (unk is not None and unk >= 0 and t == unk) else t for t in ref]


def bleu_add(stats, ref, pred, pad, eos, unk):
    """Adds one pair into stats = [reflen, predlen, match1, count1, ..., match4, count4] (in place)."""
    r, p = trim(replace_unk(ref, unk), pad, eos), trim(pred, pad, eos)
    stats[0] += len(r)
    stats[1] += len(p)
    for n in range(1, 5):
        if len(p) < n:
            continue
        stats[2 * n + 1] += len(p) - n + 1
        if len(r) < n:
            continue
        cr = Counter(tuple(r[i:i + n]) for i in range(len(r) - n + 1))
        cp = Counter(tuple(p[i:i + n]) for i in range(len(p) - n + 1))
        stats[2 * n] += sum(min(c, cr[g]) for g, c in cp.items())
    return stats


def bleu_stats(pairs, pad, eos, unk):
    stats = [0] * 10
    for ref, pred in pairs:
        bleu_add(stats, ref, pred, pad, eos, unk)
    return stats


def bleu_string(stats, order=4):
    """fairseq scoring/bleu.py Scorer.result_string over the ten integers (zero divisions: 0.00 / 0.000)."""
    reflen, predlen = stats[0], stats[1]
    prec = [stats[2 * n] / stats[2 * n + 1] if stats[2 * n + 1] > 0 else 0 for n in range(1, 5)]
    if reflen == 0 or predlen == 0:
        score = brevity = ratio = 0.0
    else:
        brevity = min(1, math.exp(1 - reflen / predlen))
        psum = sum(math.log(p) if p > 0 else float("-Inf") for p in prec[:order])
        score = brevity * math.exp(psum / order) * 100
        ratio = predlen / reflen
    fmt = "BLEU{} = {:2.2f}, {:2.1f}"
    for _ in range(1, order):
        fmt += "/{:2.1f}"
    fmt += " (BP={:.3f}, ratio={:.3f}, syslen={}, reflen={})"
    return fmt.format(order, score, *[p * 100 for p in prec[:order]], brevity, ratio, predlen, reflen)


def levenshtein(ref, pred, unk=None):
    """Unit-cost edit distance over exactly the given tokens (the reference's unk never matches).  Row i from
    row i - 1: t[j] = min(prev[j] + 1, prev[j - 1] + cost) and then d[j] = min(t[j], d[j - 1] + 1), which
    is j + the running minimum of t[j] - j."""
    a = np.asarray(replace_unk(ref, unk), dtype=np.int64)
    b = np.asarray(list(pred), dtype=np.int64)
    n = len(b)
    ar = np.arange(n + 1, dtype=np.int64)
    d = ar.copy()
    for i in range(1, len(a) + 1):
        t = np.empty(n + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(d[1:] + 1, d[:-1] + (b != a[i - 1]))
        d = np.minimum.accumulate(t - ar) + ar
    return int(d[n])


def wer_string(distance, ref_length):
    return "WER: {:.2f}".format(100.0 * distance / ref_length if ref_length > 0 else 0)


def wer_tool_lines(refs, hyps):
    """The three output lines of the WER tool over word lists."""
    vocab = {}
    ids = lambda words: [vocab.setdefault(w, len(vocab)) for w in words]
    dist = sum(levenshtein(ids(r), ids(h)) for r, h in zip(refs, hyps))
    n = sum(len(r) for r in refs)
    return [f"WER: {100.0 * dist / n:.1f}%", f"Errors: {dist}", f"Reference words: {n}"]


# the issue's worked example: pad 1, eos 2, unk 3
EXAMPLE_PAD, EXAMPLE_EOS, EXAMPLE_UNK = 1, 2, 3
EXAMPLE_PAIRS = [([5, 6, 7, 8, 9, 10, 11, 2], [5, 6, 7, 8, 9, 9, 11, 2]),
                 ([4, 4, 4, 5, 2, 1, 1], [4, 4, 5, 5, 6, 2]),
                 ([7, 3, 8, 9, 2], [7, 3, 8, 9, 2]),
                 ([12, 13, 2], [12, 2])]
EXAMPLE_STATS = [17, 17, 13, 17, 7, 13, 4, 10, 2, 7]
EXAMPLE_STRING = "BLEU4 = 46.58, 76.5/53.8/40.0/28.6 (BP=1.000, ratio=1.000, syslen=17, reflen=17)"

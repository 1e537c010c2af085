"""``mms2ut-wer``: the reference's mm_s2ut/scripts/wer.py as its README calls it,

    python scripts/mms2ut_wer.py --reference data/test.txt --hypothesis outputs/transcripts.txt

the word error rate of ASR transcripts (mms2ut_transcript.py) against reference text, with the edit
distances from the HIP kernel (kernels.edit_distance).  Line i of --hypothesis is scored against line i
of --reference; the result is wer.py's non-concatenated formula, the sum of the lines' edit distances
over the sum of the reference lines' word counts:

    WER: {100 * wer:.1f}%
    Errors: {sum of distances}
    Reference words: {N}

Words are what jiwer's default transform yields (jiwer is not installed: restated from its published
source, not pinned against it): runs of whitespace collapse to one space, the line is stripped and split
on single spaces.  An empty reference line is an error, as in jiwer; an empty hypothesis line is all
deletions.  The README's split of the errors into insertions, deletions and substitutions is not
printed: it is not unique among the optimal alignments, and jiwer's choice cannot be pinned here."""
import argparse
import re
import sys

_SPACES = re.compile(r"\s\s+")


def tokenize(line):
    """jiwer's default transform of one sentence (RemoveMultipleSpaces, Strip, ReduceToListOfListOfWords)."""
    return [w for w in _SPACES.sub(" ", line).strip().split(" ") if w]


def read_lines(path):
    with open(path, encoding="utf-8") as f:
        return f.read().splitlines()


def read_pairs(reference, hypothesis):
    """The two files -> (reference word lists, hypothesis word lists), paired by line."""
    refs, hyps = read_lines(reference), read_lines(hypothesis)
    if len(refs) != len(hyps):
        raise SystemExit(f"mms2ut-wer: {reference} has {len(refs)} lines, {hypothesis} has {len(hyps)}: "
                         "the files are paired line by line")
    refs, hyps = [tokenize(l) for l in refs], [tokenize(l) for l in hyps]
    for i, r in enumerate(refs):
        if not r:
            raise SystemExit(f"mms2ut-wer: {reference} line {i + 1} is empty: a reference needs at least one word")
    return refs, hyps


def encode(refs, hyps):
    """Word lists -> lists of int32 ids over the joint vocabulary (ids from 1 in order of appearance; 0 pads)."""
    vocab = {}
    return tuple([[vocab.setdefault(w, len(vocab) + 1) for w in s] for s in side] for side in (refs, hyps))


def wer_totals(refs, hyps, device="cuda", batch_pairs=4096):
    """-> (sum of edit distances, sum of reference words) of the word lists, the distances on the device."""
    import torch
    from . import kernels as K
    from . import scoring as S
    ref_ids, hyp_ids = encode(refs, hyps)
    limit = K.SCORE_MAX_LEN
    for name, side in (("reference", ref_ids), ("hypothesis", hyp_ids)):
        for i, s in enumerate(side):
            if len(s) > limit:
                raise SystemExit(f"mms2ut-wer: {name} line {i + 1} has {len(s)} words; the limit is {limit}")
    scorer = S.WerScorer()
    if ref_ids and not torch.cuda.is_available():
        raise SystemExit("mms2ut-wer: needs a GPU")
    for a in range(0, len(ref_ids), batch_pairs):
        scorer.add_batch(*S.upload_pairs(ref_ids[a:a + batch_pairs], hyp_ids[a:a + batch_pairs], 0, device))
    st = scorer.stats()
    return st["distance"], st["ref_length"]


def format_result(distance, ref_words):
    return [f"WER: {100.0 * distance / ref_words if ref_words else 0.0:.1f}%", f"Errors: {distance}",
            f"Reference words: {ref_words}"]


def main(argv=None):
    ap = argparse.ArgumentParser("mms2ut-wer", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="reference text, one sentence per line")
    ap.add_argument("--hypothesis", required=True, help="transcripts, one per line, in the same order")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    refs, hyps = read_pairs(args.reference, args.hypothesis)
    print("\n".join(format_result(*wer_totals(refs, hyps, args.device))))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Timing of the scoring kernels (kernels.ngram_stats, kernels.edit_distance) and of a whole
mms2ut-generate run.

    python scripts/scoring_bench.py [--repeats 20] [--out FILE]        the kernels
    python scripts/scoring_bench.py --cli [--tree DIR] [--repeats 7]   mms2ut-generate's wall time

Kernels: HIP events on the stream the kernels run on, warm-up first, median (min .. max) of the repeats
(the scheme of scripts/units_bench.py), the inputs resident on the device, at (a) 1000 pairs of about 150
units over 1000 symbols, a test split, and (b) 64 pairs of 4096 tokens over 4 symbols.  Next to each the
plain-Python oracle of the tests (tests/scoring_oracle.py) on the same input, once, time.perf_counter on
this machine's CPU.

--cli: time.perf_counter around generate_cli.main over the five-utterance corpus and the tiny edited
checkpoint of tests/test_gpu_generate_cli.py, after one untimed run that pays the kernels' first launches.
--tree DIR takes the package and the tests from another checkout (with its library built), so that two
commits are compared by running this script once per tree, interleaved."""
import argparse
import importlib
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli_wall(args):
    tree = os.path.abspath(args.tree or ROOT)
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    import pathlib
    from manifest_corpus import write_corpus
    import test_gpu_generate_cli as T
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        d = tmp / "data"
        d.mkdir()
        c = write_corpus(str(d), split="valid")
        ckpt = T._checkpoint(tmp, d, T._fusion_yaml(tmp, c["feat_dir"]))[0]
        ts = []
        for i in range(args.repeats + 1):
            t0 = time.perf_counter()
            T._cli(d, ckpt, tmp / f"out{i}")
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        last = (tmp / f"out{args.repeats}" / "generate-valid.txt").read_text().splitlines()[-1]
    ts = ts[1:]
    return [f"scoring_bench --cli: {tree}; {args.repeats} runs after one warm-up; {torch.cuda.get_device_name(0)}",
            f"  mms2ut-generate, 5 utterances, wall           {statistics.median(ts):9.2f} ms ({min(ts):.2f} .. {max(ts):.2f})",
            f"  last line: {last}"]


def kernels(args):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]
    import numpy as np
    import scoring_oracle as O
    from asr_bench import timed
    K = importlib.import_module("multimodal-s2ut_amd.kernels")
    S = importlib.import_module("multimodal-s2ut_amd.scoring")
    rng = np.random.default_rng(1)
    lines = [f"scoring_bench: warm-up {args.warmup}, {args.repeats} repeats; {torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)

    def noisy(ref, nsym):
        return [t if rng.random() > 0.15 else int(rng.integers(4, 4 + nsym)) for t in ref]

    split = [[int(x) for x in rng.integers(4, 1004, int(rng.integers(100, 201)))] + [2] for _ in range(1000)]
    long = [[int(x) for x in rng.integers(4, 8, 4096)] for _ in range(64)]
    cases = (("1000 pairs of ~150 units, 1000 symbols", [(r, noisy(r[:-1], 1000) + [2]) for r in split], 1000),
             ("64 pairs of 4096 tokens, 4 symbols", [(r, noisy(r, 4)) for r in long], 4))
    for name, pairs, n_oracle in cases:
        up = S.upload_pairs([r for r, _ in pairs], [p for _, p in pairs], 1, "cuda")
        stats = torch.zeros(10, dtype=torch.int64, device="cuda")
        totals = torch.zeros(2, dtype=torch.int64, device="cuda")
        for what, fn in (("ngram_stats", lambda: K.ngram_stats(*up, stats, 1, 2, 3)),
                         ("edit_distance", lambda: K.edit_distance(*up, totals, 3))):
            med, lo, hi = timed(fn, args.warmup, args.repeats)
            lines.append(f"  {what + ', ' + name:<60s} {med:9.3f} ms ({lo:.3f} .. {hi:.3f})")
            print(lines[-1], flush=True)
        sub = pairs[:n_oracle]
        t0 = time.perf_counter()
        want = O.bleu_stats(sub, 1, 2, 3)
        t1 = time.perf_counter()
        dist = sum(O.levenshtein(r, p, 3) for r, p in sub)
        t2 = time.perf_counter()
        scale = len(pairs) / len(sub)
        lines.append(f"  {'host oracle bleu_stats, ' + name:<60s} {(t1 - t0) * 1e3 * scale:9.1f} ms"
                     + (f" ({len(sub)} pairs timed, scaled)" if scale != 1 else ""))
        lines.append(f"  {'host oracle levenshtein, ' + name:<60s} {(t2 - t1) * 1e3 * scale:9.1f} ms"
                     + (f" ({len(sub)} pairs timed, scaled)" if scale != 1 else ""))
        print("\n".join(lines[-2:]), flush=True)
        if scale == 1:                                     # the timed kernels ran warmup + repeats times
            runs = args.warmup + args.repeats
            assert stats.tolist() == [runs * x for x in want], "ngram_stats differs from the oracle"
            assert totals.tolist() == [runs * dist, runs * sum(len(r) for r, _ in pairs)], "edit_distance differs"
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cli", action="store_true", help="time mms2ut-generate instead of the kernels")
    ap.add_argument("--tree", default=None, help="--cli: the checkout to take the package and tests from")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("scoring_bench needs a GPU: a CPU run gives no timing")
    if args.repeats is None:
        args.repeats = 7 if args.cli else 20
    lines = cli_wall(args) if args.cli else kernels(args)
    if args.cli:
        print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Per-step GPU time of fairseq-generate's search controls (kernels.log_softmax_step_ext,
kernels.ngram_block, kernels.sample_step) at a decode step's shapes.

    python scripts/search_controls_bench.py [--rows 400] [--vocab 1004] [--step 300] [--out FILE]

HIP events on the stream the kernels run on (scripts/asr_bench.timed): warm-up first, then the median
(min .. max) over the repeats of `--calls` back-to-back launches, divided by `--calls`.  Inputs are
resident on the device.  rows = sentences x beam (40 x 10), histories of `step` + 1 random units over
`--ngram-symbols` symbols (the number of bans per row is printed; the kernel's time is the scan of
the history, not the few stores).  Next to each kernel the torch
statement of generate.py on the same input, the path a decoder without the kernel takes."""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=1004)
    ap.add_argument("--step", type=int, default=300)
    ap.add_argument("--ngram", type=int, default=3)
    ap.add_argument("--ngram-symbols", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("search_controls_bench needs a GPU: a CPU run gives no timing")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
    from asr_bench import timed
    K = importlib.import_module("multimodal-s2ut_amd.kernels")
    G = importlib.import_module("multimodal-s2ut_amd.generate")
    N, V, step, beam = args.rows, args.vocab, args.step, args.beam
    bsz = N // beam
    torch.manual_seed(0)
    logits = (torch.randn(N, K.round_up(V, 64), device="cuda") * 3).half()
    lprobs = K.log_softmax_step(logits, V, 1, 2, 0)
    tokens = torch.randint(4, 4 + args.ngram_symbols, (N, step + 202), device="cuda")
    tokens[:, 0] = 2
    prev = torch.randn(N, step + 201, device="cuda")
    ids = torch.arange(bsz, device="cuda")
    work = lprobs.clone()
    lines = [f"search_controls_bench: {N} rows (beam {beam}), V {V}, step {step}; warm-up {args.warmup}, "
             f"{args.repeats} repeats of {args.calls} calls; {torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)

    def many(fn):
        def run():
            for _ in range(args.calls):
                fn()
        return run

    cases = [
        ("log_softmax_step (T 1, unkpen 0)", lambda: K.log_softmax_step(logits, V, 1, 2, 0, out=work)),
        ("log_softmax_step_ext (T 0.8, unkpen 0.5)",
         lambda: K.log_softmax_step_ext(logits, V, 1, 2, 0, 0.8, 0.5, out=work)),
        (f"ngram_block n = {args.ngram}", lambda: K.ngram_block(tokens, work, step, args.ngram)),
        (f"torch_ngram_block n = {args.ngram}", lambda: G.torch_ngram_block(tokens, work, step, args.ngram)),
        ("sample_step, whole row", lambda: K.sample_step(lprobs, prev[:, step - 1], ids, bsz, beam, V, step, 1)),
        ("sample_step, top-k 10",
         lambda: K.sample_step(lprobs, prev[:, step - 1], ids, bsz, beam, V, step, 1, topk=10)),
        ("sample_step, top-p 0.9",
         lambda: K.sample_step(lprobs, prev[:, step - 1], ids, bsz, beam, V, step, 1, topp=0.9)),
        ("torch_sample_step, top-k 10",
         lambda: G.torch_sample_step(lprobs, prev[:, step - 1], ids, bsz, beam, V, step, 1, topk=10)),
        ("torch_sample_step, top-p 0.9",
         lambda: G.torch_sample_step(lprobs, prev[:, step - 1], ids, bsz, beam, V, step, 1, topp=0.9)),
        ("beam_topk k = 20 (the beam search's selection)",
         lambda: K.beam_topk(lprobs, prev[:, step - 1], bsz, beam, V, 2 * beam, False)),
    ]
    for name, fn in cases:
        med, lo, hi = timed(many(fn), args.warmup, args.repeats)
        c = args.calls
        lines.append(f"  {name:<50s} {1e3 * med / c:9.2f} us ({1e3 * lo / c:.2f} .. {1e3 * hi / c:.2f})")
        print(lines[-1], flush=True)
    banned = int(torch.isinf(K.ngram_block(tokens, lprobs.clone(), step, args.ngram)).sum()) - int(
        torch.isinf(lprobs).sum())
    lines.append(f"  ngram_block bans {banned / N:.2f} tokens per row on this input")
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

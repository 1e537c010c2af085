"""``mms2ut-generate``: the reference's fairseq-generate call (scripts/textless/2_inference.sh:34-44,
2_inference_all.sh:66-75) on the HIP path — a checkpoint written by ``mms2ut-train`` and one
manifest split in, ``generate-{subset}.txt`` and ``generate-{subset}.unit`` out.

    python scripts/mms2ut_generate.py DATA --config-yaml config.yaml \\
        --task multimodal_speech_to_speech --target-is-code --target-code-size 1000 \\
        --path CKPT --gen-subset valid --max-tokens 8000 --beam 10 --max-len-a 1 \\
        --required-batch-size-multiple 1 --results-path DIR

The architecture comes from the checkpoint's saved ``args``; task and data flags not given on the
command line fall back to the saved ones (``plugins.merge_generate_args``).  One process, one GPU.
fairseq-generate's search controls are accepted with its defaults: ``--temperature``, ``--unkpen``,
``--no-repeat-ngram-size``, and ``--sampling`` with ``--sampling-topk`` / ``--sampling-topp`` (a
replayable stream keyed by ``--seed`` and the sentence's row in the manifest; ``--nbest`` prints the
sampled hypotheses).

Output lines follow fairseq ``fairseq_cli/generate.py`` (restated from its published source;
fairseq is not importable here, so the format is not pinned against the library).  Per sentence,
with ``{id}`` its 0-based row in ``{subset}.tsv``:

    T-{id}\\t{tgt_text}
    H-{id}\\t{score}\\t{units}          per hypothesis (``--nbest``), score = hypo score / ln 2
    D-{id}\\t{score}\\t{units}
    P-{id}\\t{positional scores / ln 2, "{:.4f}", space-joined}

The file ends with the ``Translated ...`` line and ``Generate {subset} with beam={beam}: {result}``,
``{result}`` the string of ``--scoring``'s scorer over the best hypothesis of every sentence
(scoring.py): ``bleu`` (the default) fairseq's token BLEU4 of the hypothesis' tokens against the target
row, ``wer`` the unit error rate of the unit strings.  The statistics are accumulated on the device,
one launch per batch, and read once after the last batch.

There is no ``S-`` line (the speech tasks have no source dictionary).  ``{units}`` is the
hypothesis without its final ``</s>``.  ``generate-{subset}.unit`` holds column 3 of the best
``D-`` line of every sentence in id order: what the reference's
``grep "^D\\-" | sed 's/^D-//ig' | sort -nk1 | cut -f3`` (2_inference_all.sh:91-93) extracts, and
what ``mms2ut_generate_waveform.py --in-code-file`` reads.
"""
import argparse
import logging
import math
import os
import sys
import time

import torch

from .plugins import REGISTRY, merge_generate_args, parse_generate_args, search_controls

log = logging.getLogger("mms2ut.generate")
LN2 = math.log(2)


def hypo_units(tokens, tgt_dict):
    """A hypothesis' tokens without the final </s>, as the dictionary's symbols joined by spaces."""
    ids = [int(t) for t in tokens]
    if ids and ids[-1] == tgt_dict.eos():
        ids = ids[:-1]
    return " ".join(tgt_dict.symbols[i] for i in ids)


def format_hypothesis(sample_id, hypo, tgt_dict):
    """fairseq-generate's H- / D- / P- lines of one hypothesis dict (tokens, score, positional_scores)."""
    score = hypo["score"] / LN2
    units = hypo_units(hypo["tokens"], tgt_dict)
    pos = " ".join("{:.4f}".format(float(x) / LN2) for x in hypo["positional_scores"])
    return [f"H-{sample_id}\t{score}\t{units}", f"D-{sample_id}\t{score}\t{units}", f"P-{sample_id}\t{pos}"]


def format_sentence(sample_id, tgt_text, hypos, tgt_dict, nbest=1):
    """The T- line and the lines of the first ``nbest`` hypotheses (sorted by score)."""
    lines = [f"T-{sample_id}\t{tgt_text}"]
    for h in hypos[:nbest]:
        lines += format_hypothesis(sample_id, h, tgt_dict)
    return lines


def extract_units(text):
    """The text of a generate-*.txt -> one unit string per sentence, in numeric id order: column 3
    of the first (best) ``D-`` line of every id."""
    best = {}
    for line in text.splitlines():
        if not line.startswith("D-"):
            continue
        cols = line[2:].split("\t")
        sid = int(cols[0])
        if sid not in best:
            best[sid] = cols[2] if len(cols) > 2 else ""
    return [best[i] for i in sorted(best)]


def load_checkpoint(path):
    """The file ``cli._save`` writes: {"model": MM_S2UTTransformerModel keys, "args": Namespace, ...},
    read with ``weights_only=True`` (argparse.Namespace allow-listed, as ``cli._restore``)."""
    if not os.path.exists(path):
        raise SystemExit(f"mms2ut-generate: --path {path} not found")
    with torch.serialization.safe_globals([argparse.Namespace]):
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    for key in ("model", "args"):
        if not isinstance(ckpt, dict) or ckpt.get(key) is None:
            raise SystemExit(f"mms2ut-generate: {path} has no {key!r} entry (not an mms2ut-train checkpoint)")
    return ckpt


def build_model(args, ckpt, device):
    """task + model from the merged args, weights from the checkpoint (optimizer state is not
    read).  Keys the model does not have (auxiliary multitask decoders when no
    --multitask-config-yaml is given) are ignored; keys it lacks are an error."""
    if args.task not in REGISTRY["task"]:
        raise SystemExit(f"mms2ut-generate: unknown task {args.task!r}; have {sorted(REGISTRY['task'])}")
    task = REGISTRY["task"][args.task].setup_task(args)
    model = task.build_model(args, device=device)
    missing = model.load_state_dict(ckpt["model"], strict=False)
    if missing:
        raise SystemExit(f"mms2ut-generate: {args.path} lacks {len(missing)} model keys: {', '.join(missing)}")
    model.eval()
    return task, model


def load_split(args, task, cfg):
    """The generation split: never a training split (no shuffling, the '*' transforms), no
    multitask text targets; image features only for a fusion model."""
    from . import manifest as M
    fus = task.multimodal_translation_config
    feat = getattr(fus, "image_feat_path", None) if (fus is not None and cfg["fusion"]) else None
    data_cfg = M.load_data_config(os.path.join(args.data, getattr(args, "config_yaml", None) or "config.yaml"))
    return M.MultiModalS2SManifest(args.data, args.gen_subset, M.UnitDictionary.for_codes(task.vocab_size - 4),
                                   data_cfg=data_cfg, image_feat_path=feat, is_train=False,
                                   max_source_positions=cfg.get("max_source_positions", 6000),
                                   max_target_positions=cfg.get("max_target_positions", 1024),
                                   noise=getattr(task, "noise", None))


def main(argv=None):
    from . import generate as G
    from . import manifest as M
    from . import scoring as S
    given = parse_generate_args(argv)
    ckpt = load_checkpoint(given.path)
    args = merge_generate_args(given, ckpt["args"])
    if args.max_tokens is None:
        raise SystemExit("mms2ut-generate: --max-tokens is required")
    if not torch.cuda.is_available():
        raise SystemExit("mms2ut-generate: needs a GPU")
    dev = torch.device("cuda", 0)
    task, model = build_model(args, ckpt, dev)
    del ckpt
    net = model.net
    ds = load_split(args, task, net.cfg)
    batches = ds.batches(args.max_tokens, skip_invalid=args.skip_invalid_size_inputs_valid_test)
    kept = {int(i) for b in batches for i in b}
    skipped = [ds.ids[i] for i in range(len(ds)) if i not in kept]
    if skipped:
        log.warning("%d samples exceed the size limits and are skipped: %s", len(skipped), " ".join(skipped))
    out = sys.stdout
    txt_path = unit_path = None
    if args.results_path:
        os.makedirs(args.results_path, exist_ok=True)
        txt_path = os.path.join(args.results_path, f"generate-{args.gen_subset}.txt")
        unit_path = os.path.join(args.results_path, f"generate-{args.gen_subset}.unit")
        out = open(txt_path, "w", buffering=1)
    lines = []
    nsent = ntok = 0
    pad, eos = ds.tgt_dict.pad(), ds.tgt_dict.eos()
    scorer = S.build_scorer(args.scoring, pad, eos, M.UNK)
    try:
        cfg = dict(net.cfg, multitask=None)      # the auxiliary heads are not run: no text targets
        torch.cuda.synchronize(dev)
        t0, captures0 = time.perf_counter(), G.graph_captures()
        controls = search_controls(args)         # the sampling stream is keyed by the manifest index
        for batch, sample in M.DeviceLoader(ds, batches, cfg, dev, seed=getattr(args, "seed", 1) or 1):
            # the search of task.build_generator / inference_step, on the loader's device batch
            hypos = G.generate(net, batch, beam_size=args.beam, max_len_a=args.max_len_a, max_len_b=args.max_len_b,
                               len_penalty=args.lenpen, min_len=args.min_len,
                               sample_ids=sample["id"] if args.sampling else None, **controls)
            for i, sid in enumerate(sample["id"].tolist()):
                if not hypos[i]:             # n-gram blocking banned </s> at every step it could end
                    raise SystemExit(f"mms2ut-generate: sentence {sid} has no finished hypothesis "
                                     f"(--no-repeat-ngram-size {args.no_repeat_ngram_size} bans its </s>)")
                block = format_sentence(sid, ds.tgt_texts[sid], hypos[i], ds.tgt_dict, args.nbest)
                print("\n".join(block), file=out)
                lines += block
                nsent += 1
                ntok += len(hypos[i][0]["tokens"])
            # the first hypothesis of every sentence against its target (--nbest prints more, scores the same)
            pairs = [S.sentence_pair(args.scoring, t, h[0]["tokens"].tolist(), pad, eos)
                     for t, h in zip(sample["target"].tolist(), hypos)]
            scorer.add_batch(*S.upload_pairs([r for r, _ in pairs], [p for _, p in pairs], pad, dev))
        torch.cuda.synchronize(dev)
        dt = max(time.perf_counter() - t0, 1e-9)
        log.info("%d batches, step graph captured %d times", len(batches), G.graph_captures() - captures0)
        tail = ["Translated {:,} sentences ({:,} tokens) in {:.1f}s ({:.2f} sentences/s, {:.2f} tokens/s)".format(
                    nsent, ntok, dt, nsent / dt, ntok / dt),
                f"Generate {args.gen_subset} with beam={args.beam}: {scorer.result_string()}"]
        print("\n".join(tail), file=out)
    finally:
        if out is not sys.stdout:
            out.close()
    if unit_path:
        with open(unit_path, "w") as f:
            f.write("".join(u + "\n" for u in extract_units("\n".join(lines))))
    return 0


if __name__ == "__main__":
    sys.exit(main())

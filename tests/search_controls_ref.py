"""A per-sentence Python restatement of fairseq's search with its controls, for the tests of
``generate.SequenceGenerator``'s temperature, unk penalty, n-gram blocking and sampling search.

Restated from fairseq's published ``sequence_generator.py`` (``_generate``, ``finalize_hypos``),
``search.py`` (``BeamSearch.step``, ``Sampling.step``) and ``ngram_repeat_block.py`` (its CPU path:
python lists and dicts).  fairseq is not installed, so parity with the library itself is unpinned.
It shares no code with the product: lists and numpy here, batched tensors there.

The order inside a step is fairseq's:

1. ``logits / temperature`` in fp16, then log_softmax (fp64 here, rounded to fp32);
2. NaN -> -inf;  3. ``<pad>`` -> -inf;  4. ``lprobs[unk] -= unk_penalty``;
5. at ``step >= max_len`` everything but ``</s>`` -> -inf;  6. at ``step < min_len`` ``</s>`` -> -inf;
7. n-gram blocking;  8. candidate selection (beam top-2·beam, or ``beam`` sampled candidates).

The sampling stream: ``u = (h >> 8) * 2^-24`` with ``h`` the 32-bit hash of csrc/common.h for the
counter pair ``c = id * 2^32 + step * 2^8 + slot`` — the word whose halves are ``rng_ref.u16`` of
the counters ``2c`` and ``2c + 1``.  The draw is taken in fp64: the smallest j of the kept set with
``C_j > u * C_last``.
"""
import math

import numpy as np

import rng_ref

NEG = -math.inf


def uniform(seed, sent_id, step, slot):
    c = (int(sent_id) << 32) + (int(step) << 8) + int(slot)
    lo = int(rng_ref.u16(seed, 2 * c)[0])
    hi = int(rng_ref.u16(seed, 2 * c + 1)[0])
    return (((hi << 16) | lo) >> 8) * 2.0 ** -24


def step_lprobs(z, step, max_len, min_len, temperature=1.0, unk_penalty=0.0, pad=1, eos=2, unk=3):
    """Steps 1 to 6 for one row of fp16-representable logits -> list of python floats (fp32 values)."""
    z = np.asarray(z, dtype=np.float16)
    if temperature != 1.0:
        z = (z.astype(np.float32) / np.float32(temperature)).astype(np.float16)
    z = z.astype(np.float64)
    z[np.isnan(z)] = NEG
    m = z.max()
    lp = z - (m + math.log(np.exp(z - m).sum()))
    lp = [float(np.float32(x)) for x in lp]
    lp[pad] = NEG
    lp[unk] = float(np.float32(lp[unk]) - np.float32(unk_penalty))
    if step >= max_len:
        lp = [x if v == eos else NEG for v, x in enumerate(lp)]
    elif step < min_len:
        lp[eos] = NEG
    return lp


def banned_tokens(h, n):
    """fairseq's CPU n-gram blocking for one history h (position 0 is </s>): the tokens that would
    complete an n-gram h already holds."""
    step = len(h) - 1
    if step + 2 - n < 0:
        return []
    grams = {}
    for i in range(len(h) - n + 1):
        grams.setdefault(tuple(h[i:i + n - 1]), []).append(h[i + n - 1])
    return grams.get(tuple(h[step + 2 - n:step + 1]), [])


def kept_order(lp, topk=-1, topp=-1.0):
    """The kept set of one row in its order -> list of token ids."""
    V = len(lp)
    if topk <= 0 and topp <= 0:
        return list(range(V))
    order = sorted(range(V), key=lambda v: (-lp[v], v))
    if topk > 0:
        return order[:min(topk, V)]
    run, below = 0.0, 0
    for v in order:
        run += math.exp(lp[v])
        below += run < topp
    return order[:min(V, below + 1)]


def draw(lp, u, topk=-1, topp=-1.0):
    """-> (token, j, kept, running sums): the smallest j with C_j > u * C_last."""
    order = kept_order(lp, topk, topp)
    C, run = [], 0.0
    for v in order:
        run += math.exp(lp[v])
        C.append(run)
    thr = u * C[-1]
    j = sum(1 for c in C if c <= thr)
    j = min(j, len(order) - 1)
    return order[j], j, len(order), C


def search(logits_fn, bsz, V, beam, max_len, pad=1, eos=2, unk=3, min_len=1, len_penalty=1.0,
           normalize_scores=True, temperature=1.0, unk_penalty=0.0, ngram=0, sampling=False, topk=-1, topp=-1.0,
           seed=1, ids=None):
    """``logits_fn(sent, prefix) -> V logits`` (prefix starts with </s>).  Returns per sentence the
    hypotheses {"tokens", "score", "positional_scores"} sorted by score."""
    ids = list(range(bsz)) if ids is None else list(ids)
    cand_size = 2 * beam
    hyps = {s: [([eos], [])] * beam for s in range(bsz)}
    ignore = {s: [False] * beam for s in range(bsz)}
    finalized = [[] for _ in range(bsz)]
    finished = [False] * bsz
    for step in range(max_len + 1):
        live = [s for s in range(bsz) if not finished[s]]
        newly, cands = [], {}
        for s in live:
            rows = []
            for toks, _ in hyps[s]:
                lp = step_lprobs(logits_fn(s, toks), step, max_len, min_len, temperature, unk_penalty, pad, eos, unk)
                if ngram > 0:
                    for t in banned_tokens(toks, ngram):
                        lp[t] = NEG
                rows.append(lp)
            if sampling:
                c = []
                for j in range(beam):
                    row = rows[0] if step == 0 else rows[j]
                    base = 0.0 if step == 0 else hyps[s][j][1][step - 1]
                    tok = draw(row, uniform(seed, ids[s], step, j), topk, topp)[0]
                    c.append((row[tok] + base, j, tok))
            else:
                flat = []
                for j in range(1 if step == 0 else beam):
                    base = 0.0 if step == 0 else hyps[s][j][1][step - 1]
                    flat += [(rows[j][v] + base, j * V + v) for v in range(V)]
                flat.sort(key=lambda t: (-t[0], t[1]))
                c = [(sc, idx // V, idx % V) for sc, idx in flat[:min(cand_size, len(flat) - 1)]]
            eos_mask = [tok == eos and sc != NEG for sc, _, tok in c]
            for p in range(beam):
                if ignore[s][p]:
                    eos_mask[p] = False
            for p in range(beam):
                if eos_mask[p] and len(finalized[s]) < beam:
                    sc, j, _ = c[p]
                    cum = hyps[s][j][1][:step] + [sc]
                    finalized[s].append({
                        "tokens": hyps[s][j][0][1:step + 1] + [eos],
                        "score": sc / (step + 1) ** len_penalty if normalize_scores else sc,
                        "positional_scores": [cum[0]] + [cum[i] - cum[i - 1] for i in range(1, len(cum))]})
            if any(eos_mask[:beam]) and (len(finalized[s]) == beam or step == max_len):
                newly.append(s)
            cands[s] = (c, eos_mask)
        for s in newly:
            finished[s] = True
        if all(finished) or step >= max_len:
            break
        for s in live:
            if finished[s]:
                continue
            c, eos_mask = cands[s]
            masked = [eos_mask[p] or (p < beam and ignore[s][p]) for p in range(len(c))]
            act = sorted(range(len(c)), key=lambda p: masked[p] * cand_size + p)[:beam]
            ignore[s] = [masked[p] for p in act]
            hyps[s] = [(hyps[s][c[p][1]][0][:step + 1] + [c[p][2]], hyps[s][c[p][1]][1][:step] + [c[p][0]])
                       for p in act]
    for s in range(bsz):
        finalized[s].sort(key=lambda e: -e["score"])
    return finalized


def has_repeated_ngram(tokens, n):
    grams = [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]
    return len(grams) != len(set(grams))

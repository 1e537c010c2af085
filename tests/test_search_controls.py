"""CPU: fairseq-generate's search controls in ``generate.SequenceGenerator`` — temperature, unk
penalty, n-gram blocking and the sampling search — on the toy decoder of test_generate_search with
the torch fallbacks (``normalize_step``, ``torch_ngram_block``, ``torch_sample_step``), against the
per-sentence restatement tests/search_controls_ref.py: identical tokens, scores to fp32 rounding.

With n = 1 every token of the history is banned, position 0's ``</s>`` included, so no hypothesis
can end: both sides then return no hypotheses (fairseq's rule, not special-cased)."""
import math

import pytest
import torch

import search_controls_ref as SR
from conftest import pkg
from test_generate_search import EOS, PAD, ToyDecoder, toy_logits

UNK = 3


def _logits(sent, prefix, V, sharp):
    """The toy decoder's row as fp16 logits (what a decoder hands to the step normalisation)."""
    return torch.tensor(toy_logits(sent, prefix, V, sharp), dtype=torch.float16)


class ControlsToyDecoder(ToyDecoder):
    """ToyDecoder whose step takes the temperature and the unk penalty, as IncrementalDecoder.step."""

    def step(self, tokens_last, step, mode, temperature=1.0, unk_penalty=0.0):
        G = pkg("generate")
        rows = []
        for n, t in enumerate(tokens_last.tolist()):
            self.pref[n].append(t)
            rows.append(self.row(self.sent[n // self.beam], self.pref[n]))
        return G.normalize_step(torch.stack(rows), PAD, EOS, mode, temperature, unk_penalty)

    def row(self, sent, prefix):
        return _logits(sent, prefix, self.V, self.sharp)


def _compare(got, ref, beam, max_len):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert len(g) == len(r) <= beam
        for a, b in zip(g, r):
            assert a["tokens"].tolist() == b["tokens"]
            assert a["tokens"][-1] == EOS and len(a["tokens"]) <= max_len + 1
            assert math.isclose(a["score"], b["score"], rel_tol=1e-5, abs_tol=1e-5)
            assert torch.allclose(a["positional_scores"], torch.tensor(b["positional_scores"]), atol=1e-4)


def _run(bsz, beam, V, max_len, sharp, ids=None, **kw):
    G = pkg("generate")
    gen_kw = {{"ngram": "no_repeat_ngram_size", "topk": "sampling_topk", "topp": "sampling_topp"}.get(k, k): v
              for k, v in kw.items()}
    gen = G.SequenceGenerator(beam_size=beam, **gen_kw)
    got = gen.generate(ControlsToyDecoder(bsz, beam, V, sharp), bsz, max_len, V, torch.device("cpu"),
                       sample_ids=None if ids is None else torch.tensor(ids))
    ref = SR.search(lambda s, p: _logits(s, p, V, sharp).tolist(), bsz, V, beam, max_len, ids=ids, **kw)
    return got, ref


@pytest.mark.parametrize("V", [7, 64])
@pytest.mark.parametrize("beam", [1, 3, 5])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_ngram_blocking_matches_restatement(V, beam, n):
    max_len = 9
    got, ref = _run(3, beam, V, max_len, 1.5, ngram=n, unk_penalty=0.5, temperature=0.7)
    _compare(got, ref, beam, max_len)
    for hs in got:
        if n == 1:
            assert hs == []                         # </s> is in every history: nothing can end
        for h in hs:
            assert not SR.has_repeated_ngram([EOS] + h["tokens"].tolist(), n)
    if n > 1:
        assert all(len(hs) > 0 for hs in got)


@pytest.mark.parametrize("V,beam,max_len,min_len,T,unkpen", [
    (7, 3, 6, 1, 0.7, 0.5), (64, 5, 8, 3, 0.7, 0.0), (64, 1, 5, 5, 1.0, 0.5), (7, 5, 1, 1, 0.7, 0.5),
    (64, 3, 4, 6, 1.7, 0.5)])
def test_temperature_unkpen_and_length_edges(V, beam, max_len, min_len, T, unkpen):
    """min_len at, below and above max_len (the forced </s> wins at step == max_len), max_len 1."""
    got, ref = _run(2, beam, V, max_len, 2.0, min_len=min_len, temperature=T, unk_penalty=unkpen)
    _compare(got, ref, beam, max_len)
    for hs in got:
        assert len(hs) == beam
        assert all(len(h["tokens"]) >= min(min_len, max_len) + 1 for h in hs)


def test_unk_penalty_moves_only_unk():
    G = pkg("generate")
    z = (torch.randn(4, 64) * 2).half()
    z[1, 9] = float("nan")
    a = G.normalize_step(z, PAD, EOS, 0, 0.7, 0.0)
    b = G.normalize_step(z, PAD, EOS, 0, 0.7, 0.5)
    assert torch.equal(a[:, UNK] - 0.5, b[:, UNK])
    keep = [v for v in range(64) if v != UNK]
    assert torch.equal(a[:, keep], b[:, keep]) and torch.isinf(b[:, PAD]).all() and b[1, 9] == -math.inf
    forced = G.normalize_step(z, PAD, EOS, 1, 0.7, 0.5)
    assert torch.isinf(forced[:, UNK]).all() and torch.equal(forced[:, EOS], a[:, EOS])


@pytest.mark.parametrize("V", [7, 64])
@pytest.mark.parametrize("beam", [1, 3, 5])
@pytest.mark.parametrize("variant", [{}, {"topk": 2}, {"topk": 5}, {"topp": 0.6}, {"topp": 1.0}])
def test_sampling_matches_restatement(V, beam, variant):
    max_len = 8
    got, ref = _run(3, beam, V, max_len, 1.0, ids=[5, 0, 11], sampling=True, seed=7, temperature=0.7,
                    unk_penalty=0.5, **variant)
    _compare(got, ref, beam, max_len)
    assert all(len(hs) == beam for hs in got)


def test_sampling_with_ngram_blocking_matches_restatement():
    got, ref = _run(2, 3, 64, 9, 1.0, sampling=True, topk=5, ngram=2, seed=3)
    _compare(got, ref, 3, 9)
    for hs in got:
        for h in hs:
            assert not SR.has_repeated_ngram([EOS] + h["tokens"].tolist(), 2)


def test_sampling_does_not_depend_on_the_batch():
    """A sentence keeps its samples when the batch is permuted and its id moves with it."""
    G = pkg("generate")
    V, beam, max_len = 64, 3, 8

    class Perm(ControlsToyDecoder):
        def __init__(self, order):
            super().__init__(len(order), beam, V, 1.0)
            self.sent = list(order)

    def run(order):
        gen = G.SequenceGenerator(beam_size=beam, sampling=True, sampling_topp=0.9, seed=5)
        return gen.generate(Perm(order), len(order), max_len, V, torch.device("cpu"), sample_ids=torch.tensor(order))

    a, b = run([0, 1, 2, 3]), run([2, 0, 3, 1])
    for pos, s in enumerate([2, 0, 3, 1]):
        assert [h["tokens"].tolist() for h in b[pos]] == [h["tokens"].tolist() for h in a[s]]
    other = G.SequenceGenerator(beam_size=beam, sampling=True, sampling_topp=0.9, seed=6).generate(
        Perm([0, 1, 2, 3]), 4, max_len, V, torch.device("cpu"), sample_ids=torch.arange(4))
    assert [h["tokens"].tolist() for hs in other for h in hs] != [h["tokens"].tolist() for hs in a for h in hs]


class LoopDecoder(ControlsToyDecoder):
    """Hand-built logits that force a loop: after 4 comes 5, after anything else 4; </s> only
    becomes likely late."""

    def row(self, sent, prefix):
        z = [-0.25 * v for v in range(self.V)]
        z[5 if prefix[-1] == 4 else 4] = 6.0
        z[EOS] = 0.8 * len(prefix) - 6.0
        return torch.tensor(z, dtype=torch.float16)


@pytest.mark.parametrize("n", [2, 3, 4])
def test_forced_loop_is_broken(n):
    G = pkg("generate")
    V, beam, max_len = 16, 3, 14
    looped = G.SequenceGenerator(beam_size=beam).generate(LoopDecoder(1, beam, V, 1.0), 1, max_len, V,
                                                          torch.device("cpu"))
    assert SR.has_repeated_ngram(looped[0][0]["tokens"].tolist(), n)     # the loop is there without blocking
    got = G.SequenceGenerator(beam_size=beam, no_repeat_ngram_size=n).generate(
        LoopDecoder(1, beam, V, 1.0), 1, max_len, V, torch.device("cpu"))
    assert len(got[0]) == beam
    for h in got[0]:
        assert not SR.has_repeated_ngram([EOS] + h["tokens"].tolist(), n)


def test_torch_ngram_block_rule():
    G = pkg("generate")
    tok = torch.tensor([[2, 4, 5, 4, 5, 4, 1, 1], [2, 4, 4, 4, 4, 4, 1, 1], [2, 6, 7, 8, 9, 6, 1, 1]])
    for n in (1, 2, 3, 4, 6, 7):
        for step in range(0, 6):
            lp = G.torch_ngram_block(tok, torch.zeros(3, 12), step, n)
            for r in range(3):
                banned = sorted(set(SR.banned_tokens(tok[r, :step + 1].tolist(), n)))
                assert torch.isinf(lp[r]).nonzero().view(-1).tolist() == banned, (n, step, r)


def test_stream_matches_restatement():
    G = pkg("generate")
    ids = torch.tensor([0, 1, 7, 2 ** 31 - 1])
    for seed in (1, 7, 2 ** 40 + 3):
        for step in (0, 1, 300, 2999):
            slots = torch.tensor([0, 1, 2, 255])
            u = G.sample_uniform(seed, ids, step, slots)
            want = [SR.uniform(seed, int(i), step, int(s)) for i, s in zip(ids, slots)]
            assert u.tolist() == want
    # neighbouring slots do not share a draw
    u = G.sample_uniform(1, torch.zeros(8, dtype=torch.long), 0, torch.arange(8))
    assert len(set(u.tolist())) == 8


def test_argument_errors():
    G = pkg("generate")
    for kw in ({"temperature": 0.0}, {"temperature": -1.0}, {"sampling": True, "sampling_topk": 3, "sampling_topp": 0.5},
               {"sampling_topk": 3}, {"sampling": True, "beam_size": 257}, {"no_repeat_ngram_size": -1}):
        with pytest.raises(ValueError):
            G.SequenceGenerator(**kw)


def test_flags_in_both_parsers():
    P = pkg("plugins")
    line = ("--temperature 0.8 --unkpen 0.5 --no-repeat-ngram-size 3 --sampling --sampling-topk 10 "
            "--sampling-topp 0.9").split()
    a = P.build_parser().parse_args(["data"] + line)
    g = P.build_generate_parser().parse_args(["data", "--path", "x.pt"] + line)
    for ns in (a, g):
        assert (ns.temperature, ns.unkpen, ns.no_repeat_ngram_size, ns.sampling, ns.sampling_topk,
                ns.sampling_topp) == (0.8, 0.5, 3, True, 10, 0.9)
    d = P.GENERATE_DEFAULTS
    assert (d["temperature"], d["unkpen"], d["no_repeat_ngram_size"], d["sampling"], d["sampling_topk"],
            d["sampling_topp"]) == (1.0, 0.0, 0, False, -1, -1.0)
    # the run flags never come from the checkpoint's saved args
    import argparse
    saved = argparse.Namespace(temperature=0.3, sampling=True, no_repeat_ngram_size=4, beam=2)
    m = P.merge_generate_args(P.build_generate_parser().parse_args(["data", "--path", "x.pt"]), saved)
    assert (m.temperature, m.sampling, m.no_repeat_ngram_size) == (1.0, False, 0)
    assert P.search_controls(m) == {"temperature": 1.0, "unk_penalty": 0.0, "no_repeat_ngram_size": 0,
                                    "sampling": False, "sampling_topk": -1, "sampling_topp": -1.0, "seed": 1}
    for bad in (["--temperature", "0"], ["--sampling", "--sampling-topk", "3", "--sampling-topp", "0.5"],
                ["--sampling-topk", "3"]):
        given = P.build_generate_parser().parse_args(["data", "--path", "x.pt"] + bad)
        with pytest.raises(SystemExit) as e:
            P.merge_generate_args(given, None)
        assert "mms2ut-generate: --" in str(e.value)

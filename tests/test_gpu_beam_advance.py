"""GPU: the beam-search bookkeeping kernels (beam_eos_scan, beam_advance) against the torch helper
they replace (generate.TorchBookkeeping) on the same device tensors.  Everything is integers or
copied floats: every output is compared with torch.equal, histories on the columns the step
defines (tokens [:, :step+2], scores [:, :step+1])."""
import math

import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

EOS = 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _inputs(bsz, beam, k, step, max_len, seed):
    g = torch.Generator().manual_seed(seed)
    N = bsz * beam
    # history cells distinct per (row, column): a gather from the wrong row or column shows
    tokens = (torch.arange(N).view(N, 1) * 4096 + torch.arange(max_len + 2).view(1, -1) + 4).long()
    scores = -(torch.arange(N).view(N, 1) * 1024.0 + torch.arange(max_len + 1).view(1, -1) + 0.5)
    cand_beams = torch.randint(0, beam, (bsz, k), generator=g)             # shared parents occur
    cand_indices = torch.randint(4, 1004, (bsz, k), generator=g)
    is_eos = torch.rand(bsz, k, generator=g) < 0.4
    cand_scores = -torch.rand(bsz, k, generator=g) * 9
    if bsz >= 2:
        is_eos[0, :beam] = True                                             # every first-beam candidate ends
        is_eos[1] = False                                                   # none does
    cand_indices[is_eos] = EOS
    dead = is_eos & (torch.rand(bsz, k, generator=g) < 0.3)                 # </s> at -inf does not count
    if bsz >= 2:
        dead[0, :beam] = False
    cand_scores[dead] = -math.inf
    ignore = torch.rand(bsz, beam, generator=g) < 0.25
    if bsz >= 2:
        ignore[0] = False
    return [t.cuda() for t in (cand_scores.float(), cand_indices, cand_beams, ignore, tokens, scores.float())]


CASES = [(1, 1, 2, 0, 3), (1, 3, 6, 0, 5), (3, 4, 8, 5, 12), (5, 10, 20, 11, 12), (2, 4, 5, 0, 6),
         (7, 5, 10, 300, 700)]


@pytest.mark.parametrize("bsz,beam,k,step,max_len", CASES)
def test_kernels_match_torch_bookkeeping(bsz, beam, k, step, max_len):
    G, K = pkg("generate"), pkg("kernels")
    cand_scores, cand_indices, cand_beams, ignore, tokens, scores = _inputs(bsz, beam, k, step, max_len,
                                                                             seed=bsz * 100 + k)
    ref = G.TorchBookkeeping(bsz, beam, tokens.device)
    mask_ref, n_ref = ref.beam_eos_scan(cand_scores, cand_indices, ignore, EOS)
    mask, count = K.beam_eos_scan(cand_scores, cand_indices, ignore, EOS)
    assert mask.dtype == torch.bool and torch.equal(mask, mask_ref)
    assert count.dtype == torch.int32 and int(count) == int(n_ref)
    if bsz >= 2:
        assert int(mask[0, :beam].sum()) == beam and int(mask[1].sum()) == 0

    tok_in, sc_in = tokens.clone(), scores.clone()
    tok_out = torch.full_like(tokens, -7)
    sc_out = torch.full_like(scores, 7.0)
    new_ignore, active = K.beam_advance(mask, ignore, cand_scores, cand_indices, cand_beams, tok_in, sc_in, step,
                                        tok_out, sc_out)
    ign_ref, act_ref, tok_ref, sc_ref = ref.beam_advance(mask_ref.clone(), ignore.clone(), cand_scores,
                                                         cand_indices, cand_beams, tokens.clone(), scores.clone(),
                                                         step)
    torch.cuda.synchronize()
    assert new_ignore.dtype == torch.bool and torch.equal(new_ignore, ign_ref)
    assert active.dtype == torch.int64 and torch.equal(active, act_ref)
    assert torch.equal(tok_out[:, : step + 2], tok_ref[:, : step + 2])
    assert torch.equal(sc_out[:, : step + 1], sc_ref[:, : step + 1])
    # out of place: the inputs are read only, and nothing past the step's columns is written
    assert torch.equal(tok_in, tokens) and torch.equal(sc_in, scores)
    assert bool((tok_out[:, step + 2:] == -7).all()) and bool((sc_out[:, step + 1:] == 7.0).all())


def test_same_output_on_every_run():
    K = pkg("kernels")
    bsz, beam, k, step, max_len = 5, 10, 20, 11, 12
    cand_scores, cand_indices, cand_beams, ignore, tokens, scores = _inputs(bsz, beam, k, step, max_len, seed=1)
    outs = []
    for _ in range(3):
        mask, count = K.beam_eos_scan(cand_scores, cand_indices, ignore, EOS)
        to, so = torch.zeros_like(tokens), torch.zeros_like(scores)
        ni, act = K.beam_advance(mask, ignore, cand_scores, cand_indices, cand_beams, tokens, scores, step, to, so)
        outs.append((mask, count, ni, act, to, so))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


def test_refused_shapes():
    """k above one wave's worth of candidates, or an in-place update, is an error, not a fallback."""
    K, L = pkg("kernels"), pkg("_lib")
    bsz, beam, k, step, max_len = 2, 17, 34, 1, 4
    cand_scores, cand_indices, cand_beams, ignore, tokens, scores = _inputs(bsz, beam, k, step, max_len, seed=2)
    mask, _ = K.beam_eos_scan(cand_scores, cand_indices, ignore, EOS)
    with pytest.raises(L.HipError):
        K.beam_advance(mask, ignore, cand_scores, cand_indices, cand_beams, tokens, scores, step,
                       torch.empty_like(tokens), torch.empty_like(scores))
    bsz, beam, k = 2, 4, 8
    cand_scores, cand_indices, cand_beams, ignore, tokens, scores = _inputs(bsz, beam, k, step, max_len, seed=3)
    mask, _ = K.beam_eos_scan(cand_scores, cand_indices, ignore, EOS)
    with pytest.raises(L.HipError):
        K.beam_advance(mask, ignore, cand_scores, cand_indices, cand_beams, tokens, scores, step, tokens, scores)

"""GPU: Trainer.validate — a split's label-smoothed loss / nll / accuracy accumulated on the device.

  * parity with the fp32 oracle's summed LS-CE over two batches (2e-3 relative, the tolerance
    test_gpu_model.py applies to the same quantities) and fairseq's definitions of the returned stats;
  * eval mode switches dropout and modality dropout off and still fuses the images: a model with
    dropout 0.1 and modality_dropout 1.0 validates to the same floats as the same weights without;
  * validation does not disturb training: 4 updates with a validation after updates 1 and 3 leave
    bit-identical parameters, fp32 masters, Adam moments and optimizer stats to 4 updates without
    (dropout 0.1, device step seed on), eagerly and in HIP-graph mode (validating between replays)."""
import math

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import ref_model as R
from parity_util import round16

pytestmark = pytest.mark.gpu

SHAPES = (([61, 47, 30], [14, 11, 9]), ([53, 40], [12, 8]))
IMG_TOKENS = 17


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _samples(mm, cfg):
    out = []
    for s, (L, T) in enumerate(SHAPES):
        sample = mm.data.make_sample(L, T, img_tokens=IMG_TOKENS, img_dim=cfg["image_feat_dim"], seed=2 + s)
        ni = sample["net_input"]
        ni["src_tokens"] = ni["src_tokens"].half().float()
        ni["imgs_list"][0] = ni["imgs_list"][0].half().float()
        out.append(sample)
    return out


def _trainer(mm, ocfg, P=None, **kw):
    model = mm.MMS2UTModel(mm.default_cfg(**ocfg), device="cuda:0")
    if P is None:
        model.init_params(seed=4)
    else:
        model.params.load_state_dict(P, strict=True)
    return mm.trainer.Trainer(model, lr=1e-3, warmup_updates=2, world_size=1, **kw), model


def test_validate_matches_oracle_summed_loss():
    mm = pkg()
    ocfg = R.no_dropout(R.tiny_config(conv_channels=256))
    P = round16(R.init_params(ocfg, seed=5, include_unused=False))
    tr, model = _trainer(mm, ocfg, P)
    samples = _samples(mm, ocfg)
    batches = [mm.runtime.prepare_batch(s, model.cfg, "cuda:0") for s in samples]
    got = tr.validate(iter(batches))
    assert model.training                                  # train mode restored
    ref_loss = ref_nll = 0.0
    with torch.no_grad():
        for s in samples:
            lo, nl, _ = R.model_forward(P, s, ocfg)
            ref_loss += float(lo)
            ref_nll += float(nl)
    ntok = sum(int(s["ntokens"]) for s in samples)
    assert got["ntokens"] == ntok and got["nsentences"] == sum(len(L) for L, _ in SHAPES)
    ln2 = math.log(2.0)
    loss_sum, nll_sum = got["loss"] * ntok * ln2, got["nll_loss"] * ntok * ln2
    print(f"validate loss {loss_sum:.6f} nll {nll_sum:.6f}; oracle {ref_loss:.6f} {ref_nll:.6f}; "
          f"accuracy {got['accuracy']:.3f}")
    assert abs(loss_sum - ref_loss) / ref_loss < 2e-3
    assert abs(nll_sum - ref_nll) / ref_nll < 2e-3
    assert got["ppl"] == 2.0 ** got["nll_loss"]
    # accuracy: the eval-mode logits' own argmax against the targets (--report-accuracy's definition)
    V, pad = model.cfg["vocab_size"], model.cfg["padding_idx"]
    model.eval()
    hits = 0
    with torch.no_grad():
        for b in batches:
            lg = mm.runtime.model_logits(model, b)[:, :V].float().cpu().numpy()
            tg = b.target.reshape(-1).cpu().numpy()
            hits += int(((np.argmax(lg, axis=1) == tg) & (tg != pad)).sum())
    model.train()
    assert got["accuracy"] == 100.0 * hits / ntok
    # the same pass again: the same bits; one batch fewer: fewer tokens
    assert tr.validate(iter(batches)) == got
    assert tr.validate(batches[:1])["ntokens"] == int(samples[0]["ntokens"])
    empty = tr.validate([])
    assert empty["ntokens"] == 0 and math.isnan(empty["loss"])


def test_eval_mode_ignores_dropout_and_modality_dropout():
    mm = pkg()
    on = R.tiny_config(conv_channels=256, modality_dropout=1.0, audio_dropout=0.5)
    off = R.no_dropout(R.tiny_config(conv_channels=256))
    assert on["dropout"] == 0.1 and off["dropout"] == 0.0 and off["modality_dropout"] < 0
    P = round16(R.init_params(off, seed=6, include_unused=False))
    results = []
    for ocfg in (on, off):
        tr, model = _trainer(mm, ocfg, P)
        batches = [mm.runtime.prepare_batch(s, model.cfg, "cuda:0") for s in _samples(mm, ocfg)]
        results.append(tr.validate(batches))
    assert results[0] == results[1], results
    # the images reach the result: other image features, another loss
    tr, model = _trainer(mm, on, P)
    samples = _samples(mm, on)
    for s in samples:
        s["net_input"]["imgs_list"][0] = s["net_input"]["imgs_list"][0].flip(1) * 0.5
    other = tr.validate([mm.runtime.prepare_batch(s, model.cfg, "cuda:0") for s in samples])
    assert other["loss"] != results[0]["loss"]


def _train(mm, validate_after, steps=4, **kw):
    ocfg = R.tiny_config(conv_channels=256)          # dropout 0.1 everywhere
    tr, model = _trainer(mm, ocfg, None, device_seed=True, **kw)
    samples = _samples(mm, ocfg)
    batch = mm.runtime.prepare_batch(samples[0], model.cfg, "cuda:0")
    vbatches = [mm.runtime.prepare_batch(s, model.cfg, "cuda:0") for s in samples]
    np.random.seed(11)                               # the modality-dropout draws of the training forwards
    vals = []
    for step in range(1, steps + 1):
        tr.train_step(batch)
        if step in validate_after:
            # no sync first: the deferred optimizer chunks of this update are still pending
            before = (np.random.get_state()[1].copy(), np.random.get_state()[2], model.drop.seed, model.drop.offset,
                      tr.seed_delta.clone())
            vals.append(tr.validate(vbatches))
            after = (np.random.get_state()[1], np.random.get_state()[2], model.drop.seed, model.drop.offset,
                     tr.seed_delta)
            assert np.array_equal(before[0], after[0]) and before[1:4] == after[1:4]
            assert torch.equal(before[4], after[4])
            assert model.training
    st = tr.opt.stats()
    tr.sync()
    torch.cuda.synchronize()
    return (model.params.flat.clone(), tr.opt.master.clone(), tr.opt.exp_avg_sq.clone(), st), vals, tr


@pytest.mark.parametrize("graph", [False, True])
def test_validation_does_not_disturb_training(graph):
    mm = pkg()
    a, _, _ = _train(mm, (), graph=graph)
    b, vals, tr = _train(mm, (1, 3), graph=graph)
    assert len(vals) == 2 and all(math.isfinite(v["loss"]) and v["ntokens"] > 0 for v in vals)
    assert vals[0]["loss"] != vals[1]["loss"]        # the weights moved between the two validations
    if graph:
        assert len(tr.graphs) == 1                   # one capture, replayed around the validations
    assert a[3] == b[3]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])

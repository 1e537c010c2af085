"""GPU: mms2ut-generate end to end, and the HIP search bookkeeping against the torch bookkeeping on
a real search.

The tiny random model is edited so that the search finishes sentences at different steps:
``decoder.layer_norm.weight`` x 6 (sharp distributions) and row 2 (``</s>``) of
``decoder.embed_tokens.weight`` x 5 (the tied output projection then favours ``</s>`` more with every
step).  Without the ``</s>`` scaling the fp32 oracle search (oracle/ref_generate.py) runs every
hypothesis to max_len, and neither finalisation nor the removal of finished sentences is exercised.
With it the oracle finishes the five sentences of ``_setup`` with best-hypothesis lengths 6, 5, 9,
5, 4 (top-1 / top-2 score gaps >= 0.16, against the decoder's <= 0.03 log-prob error), and on the
manifest corpus of the CLI test (oracle init seed 11, the same scale 5) with lengths 5, 5, 5, 5, 4:
the batch of sentences 1 and 3 shrinks."""
import argparse
import math

import pytest
import torch

from conftest import pkg
from oracle import ref_generate as RG
from oracle import ref_model as R
from test_gpu_generate import _setup
from test_gpu_plugins import TINY
from test_plugins import FUSION_YAML

pytestmark = pytest.mark.gpu

LAYER_NORM_SCALE, EOS_ROW_SCALE = 6.0, 5.0
BEAM, MAX_LEN_B = 4, 12


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _edit(P):
    P["decoder.layer_norm.weight"] = (P["decoder.layer_norm.weight"] * LAYER_NORM_SCALE).half().float()
    E = P["decoder.embed_tokens.weight"].clone()
    E[2] = (E[2] * EOS_ROW_SCALE).half().float()
    P["decoder.embed_tokens.weight"] = E
    return P


class TorchPathDecoder:
    """The incremental decoder without beam_eos_scan / beam_advance: the generator then runs
    generate.TorchBookkeeping (candidate selection stays the HIP beam_topk on both paths)."""

    def __init__(self, dec):
        self.dec = dec

    def step(self, *a, **k):
        return self.dec.step(*a, **k)

    def reorder(self, *a, **k):
        return self.dec.reorder(*a, **k)

    def beam_topk(self, *a, **k):
        return self.dec.beam_topk(*a, **k)


def test_kernel_path_matches_torch_path_on_a_search(monkeypatch):
    mm, cfg, P, model, batch, enc_ref, pad_ref = _setup(lengths=(120, 57, 200, 57, 88), seed=5)
    model.params.load_state_dict(_edit(P))
    G = mm.generate
    assert hasattr(G.IncrementalDecoder, "beam_advance") and hasattr(G.IncrementalDecoder, "beam_eos_scan")
    hip = G.generate(model, batch, beam_size=BEAM, max_len_a=0.0, max_len_b=MAX_LEN_B)
    real = G.IncrementalDecoder
    monkeypatch.setattr(G, "IncrementalDecoder", lambda *a, **k: TorchPathDecoder(real(*a, **k)))
    ref = G.generate(model, batch, beam_size=BEAM, max_len_a=0.0, max_len_b=MAX_LEN_B)
    torch.cuda.synchronize()
    assert len(hip) == len(ref) == 5
    for hs, rs in zip(hip, ref):
        assert len(hs) == len(rs) == BEAM
        for h, r in zip(hs, rs):
            assert torch.equal(h["tokens"], r["tokens"]) and h["score"] == r["score"]
            assert torch.equal(h["positional_scores"], r["positional_scores"])
    step_fn = RG.full_recompute_step(P, cfg, enc_ref, pad_ref, BEAM)
    oracle = RG.beam_search(step_fn, 5, cfg["vocab_size"], BEAM, MAX_LEN_B)
    for s in range(5):
        assert hip[s][0]["tokens"].tolist() == oracle[s][0]["tokens"], (s, hip[s][0], oracle[s][0])
    # sentences finish at different steps: the batch shrinks during this search
    assert len({len(hs[0]["tokens"]) for hs in hip}) >= 3


def _fusion_yaml(tmp_path, feat_dir):
    y = tmp_path / "mm.yaml"
    y.write_text(FUSION_YAML.replace('["/feats/vit_base_patch16_384"]', f'["{feat_dir}"]')
                 .replace("image_feat_dim: [768]", "image_feat_dim: [16]")
                 .replace("SA_image_dropout: 0.1", "SA_image_dropout: 0.0")
                 .replace("SA_attention_dropout: 0.1", "SA_attention_dropout: 0.0"))
    return y


def _checkpoint(tmp_path, data, fusion_yaml=None, edit=True, name="checkpoint_last.pt", extra=""):
    """A tiny model built through the task from parser args, saved in the layout cli._save writes."""
    P = pkg("plugins")
    argv = (f"{data} --task multimodal_speech_to_speech --arch mm_s2ut_transformer --criterion speech_to_unit "
            f"--config-yaml config.yaml --target-is-code --target-code-size 1000 "
            f"--share-decoder-input-output-embed --dropout 0.0 --attention-dropout 0.0 --relu-dropout 0.0 --fp16 "
            f"{TINY} {extra}")
    if fusion_yaml is not None:
        argv += f" --multimodal-translation-config-yaml {fusion_yaml}"
    a = P.build_parser().parse_args(argv.split())
    task = P.REGISTRY["task"][a.task].setup_task(a)
    model = task.build_model(a)
    if edit:
        ocfg = R.no_dropout(R.tiny_config(image_feat_dim=16))
        Pp = {k: v.half().float() for k, v in R.init_params(ocfg, seed=11, include_unused=False).items()}
        model.load_state_dict(_edit(Pp), strict=True)
    state = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()},
             "args": argparse.Namespace(**{k: v for k, v in vars(a).items()
                                           if isinstance(v, (int, float, str, bool, type(None)))})}
    path = tmp_path / name
    torch.save(state, path)
    return path, a, task, model, state


def _cli(data, ckpt, out, extra=""):
    argv = (f"{data} --config-yaml config.yaml --task multimodal_speech_to_speech --target-is-code "
            f"--target-code-size 1000 --vocoder code_hifigan --path {ckpt} --gen-subset valid --max-tokens 260 "
            f"--beam {BEAM} --max-len-a 0 --max-len-b {MAX_LEN_B} --required-batch-size-multiple 1 "
            f"--results-path {out} {extra}").split()
    return pkg("generate_cli").main(argv)


def test_cli_end_to_end(tmp_path):
    from manifest_corpus import write_corpus
    C, G, M = pkg("generate_cli"), pkg("generate"), pkg("manifest")
    d = tmp_path / "data"
    d.mkdir()
    c = write_corpus(str(d), split="valid")                      # five WAVs, image rows ti=9, di=16
    # the fusion YAML is not on the generate command line: it comes from the checkpoint's args
    ckpt, a, task, model, _ = _checkpoint(tmp_path, d, _fusion_yaml(tmp_path, c["feat_dir"]))
    out = tmp_path / "out"
    assert _cli(d, ckpt, out) == 0
    text = (out / "generate-valid.txt").read_text()
    lines = text.splitlines()
    by = {t: [l for l in lines if l.startswith(t + "-")] for t in "THDP"}
    assert all(len(by[t]) == 5 for t in "THDP") and not any(l.startswith("S-") for l in lines)
    tsv = M.load_samples_from_tsv(str(d), "valid")
    for l in by["T"]:
        sid, tgt = l[2:].split("\t")
        assert tgt == tsv[int(sid)]["tgt_text"]
    assert lines[-2].startswith("Translated 5 sentences (") and "sentences/s" in lines[-2]
    assert lines[-1].startswith(f"Generate valid with beam={BEAM}")
    units = (out / "generate-valid.unit").read_text().splitlines()
    assert units == C.extract_units(text) and len(units) == 5

    # the same search called directly on the same DeviceLoader batches
    net = model.net
    model.eval()
    a.gen_subset = "valid"
    ds = C.load_split(a, task, net.cfg)
    batches = ds.batches(260)
    assert len(batches) >= 3
    best = {}
    for batch, sample in M.DeviceLoader(ds, batches, dict(net.cfg, multitask=None), "cuda:0"):
        hyps = G.generate(net, batch, beam_size=BEAM, max_len_a=0.0, max_len_b=MAX_LEN_B)
        for sid, hs in zip(sample["id"].tolist(), hyps):
            best[sid] = hs[0]
    assert sorted(best) == list(range(5))
    hscore = {int(l[2:].split("\t")[0]): l.split("\t")[1] for l in by["H"]}
    for i in range(5):
        assert units[i] == C.hypo_units(best[i]["tokens"], ds.tgt_dict)
        assert hscore[i] == str(best[i]["score"] / math.log(2))
    assert len({len(best[i]["tokens"]) for i in range(5)}) >= 2   # a batch shrinks (module docstring)


def test_cli_missing_key_names_it(tmp_path):
    from manifest_corpus import write_corpus
    d = tmp_path / "data"
    d.mkdir()
    write_corpus(str(d), split="valid")
    ckpt, _, _, _, state = _checkpoint(tmp_path, d, edit=False)
    del state["model"]["decoder.layers.1.fc1.weight"]
    broken = tmp_path / "broken.pt"
    torch.save(state, broken)
    with pytest.raises(SystemExit) as e:
        _cli(d, broken, tmp_path / "out")
    assert "decoder.layers.1.fc1.weight" in str(e.value)


def test_cli_audio_only_checkpoint(tmp_path):
    """No fusion YAML in the checkpoint or on the command line: no image features are read."""
    from manifest_corpus import write_corpus
    import shutil
    d = tmp_path / "data"
    d.mkdir()
    c = write_corpus(str(d), split="valid")
    shutil.rmtree(c["feat_dir"])
    ckpt, _, _, _, _ = _checkpoint(tmp_path, d, edit=False)
    out = tmp_path / "out"
    assert _cli(d, ckpt, out, extra="--max-len-b 3") == 0
    units = (out / "generate-valid.unit").read_text().splitlines()
    assert len(units) == 5 and all(len(u.split()) <= 3 for u in units)


def test_cli_multitask_checkpoint(tmp_path):
    """Auxiliary multitask decoder weights in the checkpoint: loaded when --multitask-config-yaml is
    given, ignored when it is not; never run, so both decode the same units (and no text targets
    are read: the tasks' data directories hold none for this split)."""
    from manifest_corpus import write_corpus
    d = tmp_path / "data"
    d.mkdir()
    c = write_corpus(str(d), split="valid")
    mtd = tmp_path / "mt"
    mtd.mkdir()
    (mtd / "dict.txt").write_text("".join(f"{ch} 1\n" for ch in "abcdefgh"))
    mt = tmp_path / "config_multitask.yaml"
    mt.write_text(f"source_letter:\n  decoder_type: transformer\n  dict: {mtd}/dict.txt\n  data: {mtd}\n"
                  f"  encoder_layer: 2\n  loss_weight: 8.0\n  decoder_args:\n    decoder_layers: 1\n"
                  f"target_ctc:\n  decoder_type: ctc\n  dict: {mtd}/dict.txt\n  data: {mtd}\n  encoder_layer: 1\n"
                  f"  loss_weight: 1.0\n")
    ckpt, _, _, _, state = _checkpoint(tmp_path, d, _fusion_yaml(tmp_path, c["feat_dir"]), edit=False,
                                       extra=f"--multitask-config-yaml {mt}")
    assert "source_letter_decoder.embed_tokens.weight" in state["model"] and "target_ctc_decoder.proj.weight" in \
        state["model"]
    assert _cli(d, ckpt, tmp_path / "with", extra=f"--max-len-b 3 --multitask-config-yaml {mt}") == 0
    assert _cli(d, ckpt, tmp_path / "without", extra="--max-len-b 3") == 0
    a = (tmp_path / "with" / "generate-valid.unit").read_text()
    assert len(a.splitlines()) == 5 and a == (tmp_path / "without" / "generate-valid.unit").read_text()

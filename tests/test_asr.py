"""CPU: the wav2vec2 CTC restatement (tests/asr_ref.py) against torch's own modules, the loader of
multimodal-s2ut_amd/asr.py (key names, weight-norm namings, .bin and safetensors, unsupported configs),
greedy CTC decoding on hand-written sequences, the transcript CLI's ordering and output format (with a
stub model), and the margin condition the GPU end-to-end test relies on."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import asr_ref as AR
from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def A():
    return pkg("asr")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ restatement

@pytest.mark.parametrize("k", [128, 16, 15])
@pytest.mark.parametrize("style", ["g_v", "param"])
def test_pos_conv_matches_torch_weight_norm(k, style):
    """fold_pos + pos_conv against weight_norm(Conv1d(..., groups), dim=2), with the even-kernel trim."""
    g = _gen(k)
    d, groups, T = 32, 2, 21
    conv = nn.Conv1d(d, d, k, padding=k // 2, groups=groups)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(d, d // groups, k, generator=g))
        conv.bias.copy_(torch.randn(d, generator=g))
    conv = nn.utils.parametrizations.weight_norm(conv, name="weight", dim=2)
    with torch.no_grad():
        conv.parametrizations.weight.original0.copy_(torch.rand(1, 1, k, generator=g) + 0.5)
    g0, v0 = conv.parametrizations.weight.original0.detach(), conv.parametrizations.weight.original1.detach()
    assert tuple(g0.shape) == (1, 1, k)
    h = torch.randn(T, d, generator=g)
    with torch.no_grad():
        y = conv(h.t()[None])[0].t()
    if k % 2 == 0:
        assert y.shape[0] == T + 1
        y = y[:-1]
    want = h + F.gelu(y)
    names = ("weight_g", "weight_v") if style == "g_v" else \
        ("parametrizations.weight.original0", "parametrizations.weight.original1")
    p = "wav2vec2.encoder.pos_conv_embed.conv."
    W = AR.pos_weight({p + names[0]: g0, p + names[1]: v0})
    torch.testing.assert_close(W, conv.weight.detach(), rtol=1e-5, atol=1e-6)
    got = AR.pos_conv(h, W, conv.bias.detach(), groups)
    assert got.shape == (T, d)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)


def test_attention_matches_sdpa():
    g = _gen(3)
    T, H, hd = 19, 2, 64
    qkv = torch.randn(T, 3 * H * hd, generator=g)
    q, k, v = (qkv[:, i * H * hd:(i + 1) * H * hd].reshape(T, H, hd).transpose(0, 1)[None] for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v)[0].transpose(0, 1).reshape(T, H * hd)
    torch.testing.assert_close(AR.attention(qkv, H), want, rtol=1e-4, atol=1e-5)


def test_normalise_matches_numpy():
    x = AR.to_float(AR.make_wave(4000, 5, dc=0.4))
    xn = x.numpy().astype(np.float64)
    want = (xn - xn.mean()) / np.sqrt(xn.var() + 1e-7)
    np.testing.assert_allclose(AR.normalise(x).numpy(), want, rtol=0, atol=2e-5)


def test_gelu_and_layer_pieces_match_torch():
    g = _gen(4)
    x = torch.randn(9, 64, generator=g)
    torch.testing.assert_close(AR.gelu(x), F.gelu(x))
    W, b = torch.randn(72, 64, 3, generator=g), torch.randn(72, generator=g)
    conv = nn.Conv1d(64, 72, 3, stride=2)
    with torch.no_grad():
        conv.weight.copy_(W)
        conv.bias.copy_(b)
        want = conv(x.t()[None])[0].t()
    torch.testing.assert_close(AR.conv_strided(x, W, b, 2), want)


@pytest.mark.parametrize("n,frames", [(400, 1), (719, 1), (8000, 24), (12345, 38), (48000, 149)])
def test_frame_count(A, n, frames):
    assert AR.frame_count(n) == frames
    assert A.frame_counts(n, AR.KERNELS, AR.STRIDES)[-1] == frames
    sd = AR.make_state_dict(AR.SMALL, 0)
    if n <= 8000:
        with torch.no_grad():
            assert AR.forward(sd, AR.SMALL, AR.to_float(AR.make_wave(n, 1))).shape == (frames, 32)


def test_receptive_field_and_short_input(A):
    assert A.receptive_field(AR.KERNELS, AR.STRIDES) == 400
    m = A.Wav2Vec2CTC(AR.make_state_dict(AR.SMALL, 0), AR.SMALL, AR.VOCAB, device="cpu")
    assert m.min_samples == 400
    with pytest.raises(ValueError, match="receptive field"):
        m._wave(np.zeros(399, dtype=np.float32))
    with pytest.raises(ValueError, match="16000"):
        m._wave(np.zeros(4000, dtype=np.float32), sr=22050)
    assert m._wave(np.zeros(400, dtype=np.float32), sr=16000).numel() == 400


# ------------------------------------------------------------------------------------------ loader

def _same_model(a, b):
    assert torch.equal(a.pos_w, b.pos_w) and torch.equal(a.head_w, b.head_w) and torch.equal(a.conv[0].w, b.conv[0].w)
    assert torch.equal(a.conv[3].w, b.conv[3].w) and torch.equal(a.layers[1]["wqkv"], b.layers[1]["wqkv"])


def test_loader_weight_norm_namings_and_fold(A):
    sd = AR.make_state_dict(AR.SMALL, 2, style="g_v")
    p = "wav2vec2.encoder.pos_conv_embed.conv."
    sd2 = {k: v for k, v in sd.items() if not k.startswith(p + "weight_")}
    sd2[p + "parametrizations.weight.original0"] = sd[p + "weight_g"]
    sd2[p + "parametrizations.weight.original1"] = sd[p + "weight_v"]
    a = A.Wav2Vec2CTC(sd, AR.SMALL, AR.VOCAB, device="cpu")
    b = A.Wav2Vec2CTC(sd2, AR.SMALL, AR.VOCAB, device="cpu")
    _same_model(a, b)
    folded = A.fold_pos_conv_weight_norm(sd)
    torch.testing.assert_close(folded[p + "weight"], AR.pos_weight(sd))
    assert p + "weight_g" not in folded and p + "weight_v" not in folded
    # q | k | v stacked in that order, the head padded to a multiple of 8 rows
    l = "wav2vec2.encoder.layers.1.attention."
    want = torch.cat([sd[l + f"{n}_proj.weight"] for n in "qkv"]).half()
    assert torch.equal(a.layers[1]["wqkv"], want)
    assert a.conv[0].w.shape == (10, 64) and torch.equal(a.conv[0].w[:, 5], sd[
        "wav2vec2.feature_extractor.conv_layers.0.conv.weight"][5, 0])


@pytest.mark.parametrize("fmt", ["bin", "safetensors"])
def test_from_pretrained_formats(A, tmp_path, fmt):
    sd = AR.make_state_dict(AR.SMALL, 3)
    AR.write_model_dir(str(tmp_path), sd, AR.SMALL, fmt, tokenizer_cfg={"word_delimiter_token": "|",
                                                                       "clean_up_tokenization_spaces": False})
    m = A.Wav2Vec2CTC.from_pretrained(str(tmp_path), device="cpu")
    _same_model(m, A.Wav2Vec2CTC(sd, AR.SMALL, AR.VOCAB, device="cpu"))
    assert m.cleanup is False and m.delimiter == "|" and m.blank == 0 and m.sampling_rate == 16000
    if fmt == "safetensors":
        got = A.read_safetensors(os.path.join(str(tmp_path), "model.safetensors"))
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_safetensors_reader_rejects_bad_files(A, tmp_path):
    p = tmp_path / "x.safetensors"
    p.write_bytes(b"\x00\x01")
    with pytest.raises(ValueError, match="not a safetensors"):
        A.read_safetensors(str(p))
    AR.write_safetensors(str(p), {"a": torch.arange(6, dtype=torch.float32).reshape(2, 3)})
    raw = p.read_bytes()
    p.write_bytes(raw[:-4])
    with pytest.raises(ValueError, match="offsets"):
        A.read_safetensors(str(p))


@pytest.mark.parametrize("extra,what", [
    ({"feat_extract_norm": "group"}, "feat_extract_norm"), ({"do_stable_layer_norm": False}, "do_stable_layer_norm"),
    ({"add_adapter": True}, "adapter"), ({"hidden_act": "relu"}, "hidden_act"),
    ({"feat_extract_activation": "relu"}, "feat_extract_activation"), ({"num_attention_heads": 4}, "head dim"),
    ({"conv_bias": False}, "conv_bias")])
def test_unsupported_configs(A, extra, what):
    with pytest.raises(NotImplementedError, match=what):
        A.parse_config(dict(AR.SMALL, **extra))


def test_checkpoint_shapes_and_keys_are_checked(A):
    sd = AR.make_state_dict(AR.SMALL, 0)
    bad = dict(sd)
    bad["lm_head.weight"] = torch.zeros(31, 128)
    with pytest.raises(ValueError, match="lm_head.weight"):
        A.Wav2Vec2CTC(bad, AR.SMALL, AR.VOCAB, device="cpu")
    del bad["wav2vec2.encoder.layer_norm.bias"]
    bad["lm_head.weight"] = sd["lm_head.weight"]
    with pytest.raises(KeyError, match="encoder.layer_norm.bias"):
        A.Wav2Vec2CTC(bad, AR.SMALL, AR.VOCAB, device="cpu")
    with pytest.raises(ValueError, match="vocab.json"):
        A.Wav2Vec2CTC(sd, AR.SMALL, {"a": 0, "b": 1}, device="cpu")
    with pytest.raises(NotImplementedError, match="do_normalize"):
        A.Wav2Vec2CTC(sd, AR.SMALL, AR.VOCAB, preprocessor_cfg={"do_normalize": False}, device="cpu")


def test_read_wav_first_channel(A, tmp_path):
    pcm = AR.make_wave(500, 9)
    AR.write_wav(str(tmp_path / "m.wav"), pcm)
    x, sr = A.read_wav(str(tmp_path / "m.wav"))
    assert sr == 16000 and x.dtype == np.float32 and np.array_equal(x, pcm.astype(np.float32) / 32768.0)
    AR.write_wav(str(tmp_path / "s.wav"), pcm, sr=22050, channels=2)
    x2, sr2 = A.read_wav(str(tmp_path / "s.wav"))
    assert sr2 == 22050 and np.array_equal(x2, x)


# ------------------------------------------------------------------------------------------ decoding

def _ids(s):
    """'_' is the blank, '|' the delimiter."""
    return [0 if c == "_" else AR.VOCAB[c] for c in s]


@pytest.mark.parametrize("frames,text", [
    ("AA_A", "AA"), ("A", "A"), ("____", ""), ("", ""), ("|HHE_LL_LO||_||WO_RLD|", "HELLO  WORLD"),
    ("||A|", "A"), ("_A_|_|_B_", "A  B"), ("AAAA", "A"), ("A_A_A", "AAA"), ("DO|N'T", "DO N'T")])
def test_greedy_decode_known_answers(A, frames, text):
    inv = {i: t for t, i in AR.VOCAB.items()}
    assert A.greedy_decode(_ids(frames), inv, 0) == text
    assert AR.decode(_ids(frames)) == text


def test_cleanup_is_switchable(A):
    vocab = {t: i for i, t in enumerate(["<pad>", "|", "'"] + list("itswer"))}     # the list is lower-case
    inv = {i: t for t, i in vocab.items()}
    ids = [vocab[c] for c in "it|'s|we|'re"]
    assert A.greedy_decode(ids, inv, 0, cleanup=True) == "it's we're"
    assert A.greedy_decode(ids, inv, 0, cleanup=False) == "it 's we 're"
    assert AR.decode(ids, vocab, cleanup=True) == "it's we're" and AR.decode(ids, vocab, cleanup=False) == "it 's we 're"
    assert A.collapse([5, 5, 0, 5, 4, 4, 0, 0, 6], 0) == [5, 5, 4, 6]


def test_do_lower_case_and_added_tokens(A, tmp_path):
    """tokenizer_config.json's do_lower_case lower-cases the decoded string; tokens that the tokenizer keeps
    in added_tokens.json complete vocab.json (without them the loader names that file)."""
    inv = {i: t for t, i in AR.VOCAB.items()}
    assert A.greedy_decode(_ids("HI|THERE"), inv, 0, lower=True) == "hi there"
    sd = AR.make_state_dict(AR.SMALL, 3)
    base = {t: i for t, i in AR.VOCAB.items() if t not in ("<s>", "</s>")}
    AR.write_model_dir(str(tmp_path), sd, AR.SMALL, "bin", vocab=base, tokenizer_cfg={"do_lower_case": True})
    with pytest.raises(ValueError, match="added_tokens.json"):
        A.Wav2Vec2CTC.from_pretrained(str(tmp_path), device="cpu")
    with open(tmp_path / "added_tokens.json", "w") as f:
        json.dump({"<s>": 1, "</s>": 2}, f)
    m = A.Wav2Vec2CTC.from_pretrained(str(tmp_path), device="cpu")
    assert m.lower and m.id_to_token == inv


# ------------------------------------------------------------------------------------------ CLI

class _StubModel:
    sampling_rate = 16000

    def __init__(self):
        self.batches = []

    def transcribe_many(self, waves, batch_size=8, sr=None, cleanup=None):
        self.batches.append(len(waves))
        return [f"LEN {len(w)}" for w in waves]


def test_cli_orders_files_and_joins_lines(A, tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("mms2ut_transcript", os.path.join(ROOT, "scripts", "mms2ut_transcript.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    for i in (10, 9, 0, 2, 1):
        AR.write_wav(str(wavs / f"{i}_pred.wav"), AR.make_wave(400 + i, i))
    stub = _StubModel()
    seen = {}
    monkeypatch.setattr(A.Wav2Vec2CTC, "from_pretrained", classmethod(lambda cls, path, device="cuda": seen.update(
        path=path, device=device) or stub))
    out = tmp_path / "t.txt"
    assert cli.main(["--model-path", "MODEL", "--tts-wav-dir", str(wavs), "--transcript-txt", str(out),
                     "--batch-size", "2", "--device", "cpu"]) == 0
    assert seen == {"path": "MODEL", "device": "cpu"}
    assert out.read_text() == "LEN 400\nLEN 401\nLEN 402\nLEN 409\nLEN 410"      # 9 before 10, no trailing newline
    assert stub.batches == [2, 2, 1]
    AR.write_wav(str(wavs / "11_pred.wav"), AR.make_wave(400, 0), sr=22050)
    with pytest.raises(ValueError, match="sample rate"):
        cli.main(["--model-path", "MODEL", "--tts-wav-dir", str(wavs), "--transcript-txt", str(out)])
    (wavs / "transcript.txt").write_text("x")
    with pytest.raises(ValueError, match="'transcript.txt': file names must start with an integer"):
        cli.main(["--model-path", "MODEL", "--tts-wav-dir", str(wavs), "--transcript-txt", str(out)])


# ------------------------------------------------------------------------------------------ margins

@pytest.mark.parametrize("fx", AR.E2E_FIXTURES, ids=lambda f: f"{f[0]}-n{f[2]}-bias{f[4]}")
def test_margin_condition_of_the_e2e_fixtures(fx):
    """On the reference alone: at most MARGIN_CAP of a fixture's frames have an fp32 top-2 logit margin
    below 2 x allowance (allowance = TOL_FACTOR x the emulation floor), so the GPU test's argmax
    comparison covers at least three quarters of the frames."""
    _, _, ref, emu = AR.reference(*fx)
    floor = float((emu - ref).abs().max())
    allowance = AR.TOL_FACTOR * floor
    share = float((AR.margins(ref) < 2 * allowance).float().mean())
    blank = float((ref.argmax(1) == 0).float().mean())
    print(f"{fx}: floor {floor:.3e}, allowance {allowance:.3e}, share below 2x allowance {share:.3f}, blank frames {blank:.2f}")
    assert floor > 0 and torch.isfinite(ref).all()
    assert share <= AR.MARGIN_CAP

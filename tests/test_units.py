"""CPU: the HuBERT restatement (tests/hubert_ref.py) against the goldens of the ``transformers`` library's
own HubertModel (scripts/gen_hf_golden.py), and the host side of multimodal-s2ut_amd/units.py: config
validation, the loader, the centroid files, the CLI, and the margin condition that keeps the GPU
end-to-end test from hiding failures.  Nothing here imports ``transformers`` or needs a GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import asr_ref as AR
import hubert_ref as HR
from conftest import GOLDEN, ROOT, pkg

HF_TOL = 5e-5      # fp32 on both sides, only the summation order differs; features of std 1, abs-max ~5


@pytest.fixture(scope="module")
def U():
    return pkg("units")


@pytest.fixture(scope="module")
def K():
    return pkg("kernels")


def check_checksums(gold, sd, what):
    """The seeded state dict must be the one the golden was made from; a drift is reported as such."""
    want = {k[4:]: gold[k] for k in gold.files if k.startswith("sum_")}
    assert sorted(want) == sorted(sd), f"{what}: the seeded state dict's keys differ from the golden's"
    have = HR.checksums(sd)
    drift = [k for k in want if not np.allclose(have[k], want[k], rtol=1e-9, atol=1e-12)]
    assert not drift, (f"{what}: the seeded weight generator drifted from the one the golden was written with (checksum "
                       f"mismatch in {drift[:3]}...); regenerate with scripts/gen_hf_golden.py. This is not a parity failure.")


# ------------------------------------------------------------------------------------------ HF goldens

@pytest.mark.parametrize("variant", ["plain", "norm", "bias"])
def test_restatement_matches_hf_golden(variant):
    gold = np.load(os.path.join(GOLDEN, f"hubert_hf_small_{variant}.npz"))
    cfg = dict(HR.SMALL, conv_bias=variant == "bias")
    sd = HR.make_state_dict(cfg, 0)
    check_checksums(gold, sd, f"hubert_hf_small_{variant}")
    km, normalize = int(gold["km_layer"]), bool(gold["normalize"])
    assert km == HR.KM_LAYER["small"] and normalize == (variant == "norm")
    for n, ws in HR.WAVES:
        want = {}
        with torch.no_grad():
            hk = HR.forward(sd, cfg, AR.to_float(AR.make_wave(n, ws)), km, normalize=normalize, want=want)
        pairs = [("hk", hk, gold[f"hk_{n}"]), ("h0", want["h0"][::4], gold[f"h0_{n}"])]
        if n == 8000:
            pairs.append(("layer0", want["layer0"][::16], gold[f"layer0_{n}"]))
        for name, got, ref in pairs:
            ref = torch.from_numpy(ref)
            assert got.shape == ref.shape
            err = float((got - ref).abs().max())
            print(f"{variant} n{n} {name}: max-abs vs HF {err:.2e} (scale {float(ref.abs().max()):.2f}, std "
                  f"{float(ref.std()):.2f})")
            assert err <= HF_TOL, (variant, n, name, err)


def test_checksum_mismatch_is_reported_as_drift():
    gold = np.load(os.path.join(GOLDEN, "hubert_hf_small_plain.npz"))
    sd = HR.make_state_dict(HR.SMALL, 1)                # another seed: same keys, other weights
    with pytest.raises(AssertionError, match="drifted"):
        check_checksums(gold, sd, "seed 1")


# ------------------------------------------------------------------------------------------ config

def test_parse_config(U, K):
    c = U.parse_config({})
    assert c["feat_extract_norm"] == "group" and c["hidden_size"] == 768 and c["feat_proj_layer_norm"] is True
    assert U.parse_config(dict(HR.SMALL, conv_bias=True))["conv_bias"] is True
    assert U.parse_config(dict(HR.SMALL, feat_proj_layer_norm=False))["feat_proj_layer_norm"] is False
    for over, word in (({"feat_extract_norm": "layer"}, "feat_extract_norm"), ({"do_stable_layer_norm": True}, "do_stable_layer_norm"),
                       ({"hidden_act": "relu"}, "hidden_act"), ({"feat_extract_activation": "relu"}, "feat_extract_activation"),
                       ({"add_adapter": True}, "add_adapter"), ({"num_attention_heads": 4}, "head dim")):
        assert 32 not in K.FLASH_HD
        with pytest.raises(NotImplementedError, match=word):
            U.parse_config(dict(HR.SMALL, **over))
    for over in ({"conv_kernel": [10, 3]}, {"conv_stride": [5] * 6}, {"num_conv_pos_embedding_groups": 3}):
        with pytest.raises(ValueError):
            U.parse_config(dict(HR.SMALL, **over))
    for km in (-1, 4):
        with pytest.raises(ValueError, match="km_layer"):
            U.check_km_layer(km, U.parse_config(HR.SMALL))
        with pytest.raises(ValueError, match="km_layer"):
            U.HubertUnits(HR.make_state_dict(HR.SMALL, 0), HR.SMALL, np.zeros((4, 128), np.float32), km, device="cpu")
    assert [U.check_km_layer(k, U.parse_config(HR.SMALL)) for k in (0, 3)] == [0, 3]


# ------------------------------------------------------------------------------------------ loader

def _weights(m):
    out = {"pos_w": m.pos_w, "pos_b": m.pos_b, "fp_w": m.fp_w, "enc_g": m.enc_g, "c_hi": m.c_hi, "c_lo": m.c_lo,
           "c_norm": m.c_norm}
    for i, c in enumerate(m.conv):
        out[f"conv{i}"] = c.w
    for l, L in enumerate(m.layers):
        out.update({f"l{l}.{k}": v for k, v in L.items()})
    return out


def test_loader_prefixes_and_weight_norm_namings(U):
    cents = np.random.default_rng(0).standard_normal((20, 128)).astype(np.float32)
    base = _weights(U.HubertUnits(HR.make_state_dict(HR.SMALL, 0), HR.SMALL, cents, 2, device="cpu"))
    assert len([k for k in base if k.startswith("l")]) == 2 * 12        # km_layer 2 of 3: the third layer is not loaded
    for prefix in ("", "hubert.", "wav2vec2."):
        for style in ("param", "g_v"):
            sd = HR.make_state_dict(HR.SMALL, 0, prefix=prefix, style=style)
            sd["lm_head.weight"] = torch.zeros(32, 128)                 # a head: ignored
            got = _weights(U.HubertUnits(sd, HR.SMALL, cents, 2, device="cpu"))
            assert sorted(got) == sorted(base)
            for k in base:
                assert torch.equal(got[k], base[k]), (prefix, style, k)
    sd = HR.make_state_dict(HR.SMALL, 0)
    # a layer past km_layer may be absent altogether
    U.HubertUnits({k: v for k, v in sd.items() if "encoder.layers.2." not in k}, HR.SMALL, cents, 2, device="cpu")
    miss = {k: v for k, v in sd.items() if k != "encoder.layers.1.final_layer_norm.bias"}
    with pytest.raises(KeyError, match="encoder.layers.1.final_layer_norm.bias"):
        U.HubertUnits(miss, HR.SMALL, cents, 2, device="cpu")
    bad = dict(sd)
    bad["feature_projection.projection.weight"] = torch.zeros(128, 65)
    with pytest.raises(ValueError, match="feature_projection.projection.weight"):
        U.HubertUnits(bad, HR.SMALL, cents, 2, device="cpu")
    with pytest.raises(KeyError, match="conv_layers.0.conv.weight"):
        U.HubertUnits({"x." + k: v for k, v in sd.items()}, HR.SMALL, cents, 2, device="cpu")
    with pytest.raises(KeyError, match="conv_layers.0.conv.bias"):      # conv_bias true, a checkpoint without
        U.HubertUnits(sd, dict(HR.SMALL, conv_bias=True), cents, 2, device="cpu")
    with pytest.raises(ValueError, match="feature width 128"):
        U.HubertUnits(sd, HR.SMALL, cents[:, :64], 2, device="cpu")
    with pytest.raises(NotImplementedError):                            # asr.py keeps refusing this family
        pkg("asr").parse_config(HR.SMALL)


def test_centroid_files(U, tmp_path):
    cents = np.random.default_rng(1).standard_normal((12, 128))
    np.save(tmp_path / "km.npy", cents)
    a = U.load_centroids(str(tmp_path / "km.npy"))
    assert a.dtype == np.float32 and a.shape == (12, 128) and np.array_equal(a, cents.astype(np.float32))
    np.save(tmp_path / "flat.npy", cents.reshape(-1))
    with pytest.raises(ValueError, match="centroids"):
        U.load_centroids(str(tmp_path / "flat.npy"))


def test_joblib_centroid_file(U, tmp_path):
    joblib = pytest.importorskip("joblib")
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(2)
    km = cluster.MiniBatchKMeans(n_clusters=5, n_init=1, random_state=0).fit(rng.standard_normal((200, 16)))
    joblib.dump(km, tmp_path / "km.bin")
    np.save(tmp_path / "km.npy", km.cluster_centers_)
    assert np.array_equal(U.load_centroids(str(tmp_path / "km.bin")), U.load_centroids(str(tmp_path / "km.npy")))
    joblib.dump({"no": "centres"}, tmp_path / "other.bin")
    with pytest.raises(ValueError, match="cluster_centers_"):
        U.load_centroids(str(tmp_path / "other.bin"))


def test_kmeans_pack_carries_22_bits(K):
    Cm = torch.randn(37, 128, generator=torch.Generator().manual_seed(0)) * 3.0
    hi, lo, cn = K.kmeans_pack(Cm)
    assert hi.shape == lo.shape == (48, 128) and not hi[37:].any() and not lo[37:].any()
    back = hi[:37].double() + lo[:37].double() / 2048.0
    rel = float(((back - Cm.double()).abs() / Cm.abs().double().clamp_min(2.0 ** -14)).max())
    print(f"kmeans_pack: hi + lo / 2^11 relative error {rel:.2e}")
    assert rel <= 2.0 ** -21
    assert torch.equal(cn, Cm.double().pow(2).sum(1).float())
    with pytest.raises(ValueError, match="fp16's range"):
        K.kmeans_pack(torch.full((2, 8), 1e5))
    with pytest.raises(ValueError, match="multiple of 8"):
        K.kmeans_pack(torch.zeros(2, 12))


def test_kmeans_chunk_rule(K):
    """Host side of kmeans_assign's launch: 64 centroids per block while that gives at most 512 blocks (one
    5 s utterance: 4 x 16), 256 from there on (16 utterances: 63 x 4); a given chunk is checked."""
    assert K.kmeans_chunks(249, 1000) == (64, 16)
    assert K.kmeans_chunks(2048, 1000) == (64, 16) and K.kmeans_chunks(2049, 1000) == (256, 4)
    assert K.kmeans_chunks(3984, 1000) == (256, 4)
    assert K.kmeans_chunks(1, 1) == (64, 1) and K.kmeans_chunks(10 ** 6, 1) == (256, 1)
    assert K.kmeans_chunks(249, 1000, 128) == (128, 8)
    with pytest.raises(pkg("_lib").HipError, match="multiple of 64"):
        K.kmeans_chunks(249, 1000, 100)


# ------------------------------------------------------------------------------------------ CLI

class _StubModel:
    sampling_rate, min_samples = 16000, 400

    def __init__(self):
        self.batches = []

    def units_many(self, waves, batch_size=8):
        self.batches.append(len(waves))
        return [([len(w), 7, 7, 3], [len(w), 7, 3]) for w in waves]


def test_cli_manifest_order_and_lines(U, tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("mms2ut_quantize_units",
                                                  os.path.join(ROOT, "scripts", "mms2ut_quantize_units.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    root = tmp_path / "audio"
    (root / "sub").mkdir(parents=True)
    names = ["b.wav", "sub/a.wav", "c.wav"]
    for i, nm in enumerate(names):
        AR.write_wav(str(root / nm), AR.make_wave(400 + i, i))
    man = tmp_path / "train.tsv"
    man.write_text(f"{root}\n" + "".join(f"{nm}\t{400 + i}\n" for i, nm in enumerate(names)))
    (tmp_path / "model").mkdir()
    stub, seen = _StubModel(), {}
    monkeypatch.setattr(U.HubertUnits, "from_pretrained", classmethod(
        lambda cls, path, km, km_layer=11, device="cuda": seen.update(path=path, km=km, layer=km_layer, device=device) or stub))
    out = tmp_path / "train.km"
    argv = ["--feature_type", "hubert", "--acoustic_model_path", str(tmp_path / "model"), "--kmeans_model_path", "KM",
            "--layer", "11", "--manifest_path", str(man), "--out_quantized_file_path", str(out), "--extension", ".wav",
            "--batch-size", "2", "--device", "cpu"]
    assert cli.main(argv) == 0
    assert seen == {"path": str(tmp_path / "model"), "km": "KM", "layer": 11, "device": "cpu"}
    assert out.read_text() == "b|400 7 7 3\na|401 7 7 3\nc|402 7 7 3\n"          # manifest order, basenames
    assert stub.batches == [2, 1]
    assert cli.main(argv + ["--reduce"]) == 0
    assert out.read_text() == "b|400 7 3\na|401 7 3\nc|402 7 3\n"
    for bad, word in ((["--feature_type", "cpc"] + argv[2:], "feature_type"),
                      (argv[:3] + [str(tmp_path / "hubert_base_ls960.pt")] + argv[4:], r"\.pt")):
        with pytest.raises(SystemExit):
            cli.main(bad)
    (tmp_path / "hubert_base_ls960.pt").write_bytes(b"x")
    with pytest.raises(SystemExit):                                         # a file, not an HF directory
        cli.main(argv[:3] + [str(tmp_path / "hubert_base_ls960.pt")] + argv[4:])
    AR.write_wav(str(root / "short.wav"), AR.make_wave(399, 0))
    man.write_text(f"{root}\nshort.wav\t399\n")
    with pytest.raises(ValueError, match="short.wav.*receptive field"):
        cli.main(argv)
    AR.write_wav(str(root / "fast.wav"), AR.make_wave(800, 0), sr=22050)
    man.write_text(f"{root}\nfast.wav\t800\n")
    with pytest.raises(ValueError, match="fast.wav: sample rate"):
        cli.main(argv)
    man.write_text(f"{root}\nb.wav 400\n")
    with pytest.raises(ValueError, match="n_samples"):
        cli.main(argv)


def test_cli_names_the_pt_format(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("mms2ut_quantize_units",
                                                  os.path.join(ROOT, "scripts", "mms2ut_quantize_units.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(SystemExit):
        cli.main(["--feature_type", "hubert", "--acoustic_model_path", str(tmp_path / "m.pt"), "--kmeans_model_path", "KM",
                  "--layer", "11", "--manifest_path", "x", "--out_quantized_file_path", "y"])
    assert ".pt checkpoint format is out of scope" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------ margins

@pytest.mark.parametrize("n,ws", HR.WAVES)
def test_margin_condition_of_the_e2e_fixtures(n, ws):
    """On the reference alone: with a = TOL_FACTOR x (emulation - fp32 max-abs at km_layer), at most
    MARGIN_CAP of a fixture's frames are unsafe, i.e. have a centroid c with s_c - s_c1 < 2 (2 a |C_c -
    C_c1|_1): the GPU test's unit comparison covers at least three quarters of the frames."""
    _, _, ref, emu = HR.reference("small", n, ws)
    cents = HR.make_centroids("small")
    a = HR.TOL_FACTOR * float((emu - ref).abs().max())
    safe = HR.safe_frames(ref, cents, a)
    share = 1.0 - float(safe.float().mean())
    wins = HR.assign(ref, cents).unique().numel()
    print(f"n{n}: {ref.shape[0]} frames, a {a:.2e}, unsafe share {share:.3f}, distinct units {wins}")
    assert share <= HR.MARGIN_CAP
    if n == 48000:
        assert ref.shape[0] == 149 and wins >= 10

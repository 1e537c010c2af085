"""CPU: the noise augmentation's host side (--noise-config-yaml): the tests' numpy restatement
against fixtures written by the reference's own add_noise_v2 (scripts/gen_noise_golden.py), config
parsing and validation, the per-utterance draws, and the wiring through the manifest, the task and
the fairseq collater.  The mixing kernels are tested in tests/test_gpu_noise.py."""
import os

import numpy as np
import pytest
import torch

import noise_util as NU
from conftest import pkg
from manifest_corpus import write_corpus


def _clips(tmp_path, lengths=(700, 2403, 9000), seed=5):
    M = pkg("manifest")
    rng = np.random.default_rng(seed)
    d = tmp_path / "noise"
    d.mkdir(exist_ok=True)
    paths, clips = [], []
    for i, L in enumerate(lengths):
        c = rng.integers(-3000, 3000, L).astype(np.int16)
        M.write_wav(str(d / f"n{i}.wav"), c)
        paths.append(str(d / f"n{i}.wav"))
        clips.append(c)
    return paths, clips


def _yaml(path, noise_wav, **kw):
    lines = ["noise_wav:"] + [f"  - {p}" for p in noise_wav] + [f"{k}: {v}" for k, v in kw.items()]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_golden_set_is_complete():
    names = [n for n, _ in NU.golden_cases()]
    assert names == ["a", "b", "c", "d", "e", "f"]
    g = dict(NU.golden_cases())
    assert g["a"]["peak"] < 1.0 < g["b"]["peak"]                    # normalisation off in a, on in b
    assert len(g["c"]["clean"]) > 2 * len(g["c"]["clips"][int(g["c"]["ids"][0])])
    assert len(g["d"]["clean"]) == len(g["d"]["clips"][int(g["d"]["ids"][0])]) and g["d"]["start"] == 0
    assert g["e"]["noise_num"] == 3 and len({len(g["e"]["clips"][int(i)]) for i in g["e"]["ids"]}) > 1
    assert len(g["f"]["clean"]) == 400


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f"])
def test_restatement_matches_reference(name):
    g = dict(NU.golden_cases())[name]
    x = g["clean"].astype(np.float32) / np.float32(32768.0)
    out = NU.mix_normalised(x, NU.noise_signal(g["clips"], g["ids"]), int(g["start"]), g["f"])
    err = float(np.abs(out.astype(np.float64) - g["out"].astype(np.float64)).max())
    print(f"case {name}: err {err:.3e}, d {float(g['d']):.3e}, tol {NU.golden_tol(g):.3e}")
    assert err <= NU.golden_tol(g)
    # the batch form (x 2^15 in and out, params row) is the same arithmetic
    via = NU.mix_waves([g["clean"].astype(np.float32)], g["clips"], NU.golden_params(g))[0]
    assert np.array_equal(via, out * np.float32(32768.0))


def test_factor_is_the_reference_formula():
    """The generator stored f from the reference's three torch operations on the SNR it drew."""
    FE = pkg("frontend")
    for _, g in NU.golden_cases():
        lo, hi = g["snr_range"]
        aug = FE.NoiseAugment([], 0.0, [float(lo), float(hi)], 0)
        u = 0.0 if hi == lo else (float(g["snr"]) - lo) / (hi - lo)
        snr, f = aug.factor([np.float32(u)] * 3)
        assert f.dtype == np.float32 and f.shape == (3,)
        if np.all(snr == g["snr"]):
            assert np.all(f == g["f"])
        assert np.abs(f.astype(np.float64) - float(g["f"])).max() <= 1e-6


def test_config_defaults_and_validation(tmp_path):
    M, FE = pkg("manifest"), pkg("frontend")
    paths, clips = _clips(tmp_path)
    y = tmp_path / "empty.yaml"
    y.write_text("{}\n")
    assert M.load_noise_config(str(y)) == {"noise_wav": [], "noise_prob": 0.0, "noise_snr": 0.0, "noise_num": 0}
    aug = FE.NoiseAugment.from_config_dict(M.load_noise_config(str(y)))
    assert not aug.active and len(aug.lengths) == 0
    cfg = M.load_noise_config(_yaml(tmp_path / "n.yaml", paths, noise_prob=0.5, noise_snr="[0, 20]", noise_num=2))
    assert cfg == {"noise_wav": paths, "noise_prob": 0.5, "noise_snr": [0, 20], "noise_num": 2}
    aug = FE.NoiseAugment.from_config_dict(cfg)
    assert aug.active and aug.lengths.tolist() == [700, 2403, 9000] and (aug.snr_low, aug.snr_high) == (0, 20)
    assert all(c.dtype == np.int16 and np.array_equal(c, r) for c, r in zip(aug.clips, clips))
    # scalar SNR: [s, s] (the reference crashes on the [0] index)
    s = FE.NoiseAugment(paths, 1.0, 7.5, 1)
    assert (s.snr_low, s.snr_high) == (7.5, 7.5)
    p = s.draws([1000], np.random.RandomState(0))
    f = p[0, 2:3].view(np.float32)[0]
    assert f == (1 / (10 ** (torch.tensor([7.5]) / 20) + 1)).numpy()[0]
    # undefined in the reference: refused at construction
    with pytest.raises(ValueError):
        FE.NoiseAugment(paths, 0.3, [0, 10], 0)
    with pytest.raises(ValueError):
        FE.NoiseAugment([], 0.3, [0, 10], 1)
    with pytest.raises(ValueError):
        FE.NoiseAugment(paths, 0.3, [0, 10, 20], 1)
    with pytest.raises(NotImplementedError):
        FE.NoiseAugment(paths, 0.3, [0, 10], 5)
    FE.NoiseAugment(paths, 0.3, [0, 10], 4)
    FE.NoiseAugment([], 0.0, 0.0, 0)            # inactive: nothing is checked or read, as the reference
    # noise files: 16-bit PCM, mono, 16 kHz
    import wave
    bad = tmp_path / "bad"
    bad.mkdir()
    M.write_wav(str(bad / "8k.wav"), clips[0], sample_rate=8000)
    for name, ch, width in (("stereo.wav", 2, 2), ("u8.wav", 1, 1)):
        with wave.open(str(bad / name), "wb") as w:
            w.setnchannels(ch)
            w.setsampwidth(width)
            w.setframerate(16000)
            w.writeframes(bytes(400))
    for name in ("8k.wav", "stereo.wav", "u8.wav"):
        with pytest.raises(ValueError):
            FE.NoiseAugment([str(bad / name)], 1.0, [0, 10], 1)


def test_draws(tmp_path):
    FE = pkg("frontend")
    paths, _ = _clips(tmp_path)
    n = [400, 1601, 2403, 4000, 6007, 700, 9000, 20000] * 8
    for K in (1, 3):
        aug = FE.NoiseAugment(paths, 0.5, [0, 20], K)
        a, b = aug.draws(n, np.random.RandomState(3)), aug.draws(n, np.random.RandomState(3))
        assert a.dtype == np.int32 and a.shape == (len(n), 3 + K) and np.array_equal(a, b)
        assert not np.array_equal(a, aug.draws(n, np.random.RandomState(4)))
        assert 0 < a[:, 0].sum() < len(n) and np.all(a[a[:, 0] == 0] == 0)
        assert aug.check(a, n) == K
        for row, T in zip(a, n):
            if not row[0]:
                continue
            assert np.all((0 <= row[3:]) & (row[3:] < 3))
            L = int(aug.lengths[row[3:]].min())
            Lt = NU.tiled_length(T, L)
            assert 0 <= row[1] and row[1] + T <= Lt
            if T == Lt:
                assert row[1] == 0
            f = row[2:3].view(np.float32)[0]
            assert 1 / (10 ** (20 / 20) + 1) - 1e-6 <= f <= 0.5
        applied = a[a[:, 0] == 1]
        assert len(set(applied[:, 3].tolist())) == 3 and len(set(applied[:, 2].tolist())) > 1
    one = FE.NoiseAugment(paths, 1.0, [0, 20], 1).draws(n, np.random.RandomState(1))
    assert one[:, 0].all()
    # T == Lt happens for T == L and for whole multiples of L
    exact = FE.NoiseAugment(paths[:1], 1.0, [0, 20], 1).draws([700, 1400, 2100], np.random.RandomState(1))
    assert exact[:, 0].all() and not exact[:, 1].any()
    assert not FE.NoiseAugment(paths, 0.0, [0, 20], 1).active
    # the host refuses what the kernel would index with
    aug = FE.NoiseAugment(paths, 1.0, [0, 20], 1)
    good = aug.draws([1000, 1000], np.random.RandomState(0))
    for col, val in ((3, 3), (3, -1), (1, -1), (1, 1 << 20)):
        bad = good.copy()
        bad[1, col] = val
        with pytest.raises(ValueError):
            aug.check(bad, [1000, 1000])
    with pytest.raises(ValueError):
        aug.check(good.astype(np.int64), [1000, 1000])
    with pytest.raises(ValueError):
        aug.check(np.zeros((2, 3 + 5), np.int32), [1000, 1000])


def test_registry(tmp_path):
    FE = pkg("frontend")
    paths, _ = _clips(tmp_path)
    aug = FE.NoiseAugment(paths, 1.0, [0, 20], 1)
    assert aug.key == FE.NoiseAugment(paths, 1.0, [0, 20], 1).key != FE.NoiseAugment(paths, 1.0, [0, 10], 1).key
    assert FE.noise_bank(FE.register_noise_bank(aug.key, aug)) is aug
    with pytest.raises(KeyError):
        FE.noise_bank("noise-none")


def test_noise_prob_zero_changes_nothing(monkeypatch, tmp_path):
    """noise_prob 0: the manifest's and the collater's output equals a run without the flag, and
    src_noise is absent; with noise_prob 1 the collater attaches the draws and the bank's key."""
    import fairseq_stub
    from test_plugins import FUSION_YAML
    paths, _ = _clips(tmp_path)
    FE = pkg("frontend")
    samples = {}
    for tag, prob in (("off", None), ("zero", 0.0), ("one", 1.0)):
        sub = tmp_path / tag
        sub.mkdir()
        extra = "" if prob is None else \
            f"--noise-config-yaml {_yaml(sub / 'noise.yaml', paths, noise_prob=prob, noise_snr='[0, 20]', noise_num=2)}"
        fs, regs, args, c, _ = fairseq_stub.dropin_setup(monkeypatch, sub, FUSION_YAML, extra=extra)
        task = fs.tasks.setup_task(args)
        ds = task.load_dataset("train")
        assert (ds.man.noise is not None) == (prob == 1.0)
        samples[tag] = list(task.get_batch_iterator(ds, max_tokens=450, max_positions=task.max_positions()))
        host, waves = ds.man.collate([0, 1, 2])
        samples[tag + "_host"] = (host["net_input"]["src_lengths"], host["target"], waves)

    def same(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, torch.Tensor):
            return torch.equal(a, b)
        if isinstance(a, np.ndarray):
            return np.array_equal(a, b)
        if isinstance(a, str):                       # audio paths: each run has its own corpus copy
            return os.path.basename(a) == os.path.basename(b)
        return a == b

    assert same(samples["off"], samples["zero"]) and same(samples["off_host"], samples["zero_host"])
    assert all("src_noise" not in s["net_input"] for s in samples["zero"])
    for s_on, s_off in zip(samples["one"], samples["off"]):
        sn = s_on["net_input"].pop("src_noise")
        assert same(s_on, s_off)                     # the waveforms travel clean; the GPU mixes them
        B = len(s_on["id"])
        assert sn["params"].dtype == torch.int32 and sn["params"].shape == (B, 3 + 2) and sn["n_mix"] == 2
        assert sn["params"][:, 0].all()
        assert fs.utils.apply_half({"p": sn["params"]})["p"].dtype == torch.int32
        aug = FE.noise_bank(sn["bank"])
        assert aug.check(sn["params"].numpy(), np.diff(s_on["net_input"]["src_wave_offsets"].numpy())) == 2


def test_task_resolves_relative_yaml_and_reaches_every_split(tmp_path):
    P, M = pkg("plugins"), pkg("manifest")
    d = tmp_path / "data"
    d.mkdir()
    paths, _ = _clips(tmp_path)
    for split in ("train", "valid", "test"):
        write_corpus(str(d), frames=(60, 41), split=split, di=16, ti=3)
    _yaml(d / "noise.yaml", paths, noise_prob=0.25, noise_snr="[5, 15]", noise_num=1)
    argv = (f"{d} --task multimodal_speech_to_speech --arch mm_s2ut_transformer --criterion speech_to_unit "
            f"--target-is-code --target-code-size 1000 --fp16 --noise-config-yaml noise.yaml")
    task = P.REGISTRY["task"]["multimodal_speech_to_speech"].setup_task(P.build_parser().parse_args(argv.split()))
    assert task.noise.active and task.noise.noise_prob == 0.25 and task.noise.noise_wav == paths
    for split in ("train", "valid", "test"):       # one noise config for every split, as the reference
        man = task.load_dataset(split)
        assert man.noise is task.noise
    # without the flag nothing is attached
    task0 = P.REGISTRY["task"]["multimodal_speech_to_speech"].setup_task(
        P.build_parser().parse_args(argv.split()[:-2]))
    assert task0.noise is None and task0.load_dataset("train").noise is None
    with pytest.raises(FileNotFoundError):
        P.REGISTRY["task"]["multimodal_speech_to_speech"].setup_task(
            P.build_parser().parse_args(argv.replace("noise.yaml", "missing.yaml").split()))
    # multi-channel source audio with noise enabled is refused (the reference mixes per channel)
    import wave
    with wave.open(os.path.join(str(d), "wav", os.listdir(os.path.join(str(d), "wav"))[0]), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(bytes(4 * 16000))
    man = task.load_dataset("train")
    bad = [i for i, p in enumerate(man.audio_paths) if M.read_wav_info(p)[2] == 2]
    assert bad
    with pytest.raises(NotImplementedError):
        man.item(bad[0])
    task0.load_dataset("train").item(bad[0])       # still folded to mono when noise is off

"""CPU: S2UT data preparation (multimodal-s2ut_amd/prepare.py) — the resampler's tap table against the
float64 restatement (tests/resample_ref.py), the filter's pass band and stop band, output lengths and
refusals, and the host tools: write_manifest, prep_s2ut_data (loaded back through MultiModalS2SManifest),
convert_dir's copy path (no GPU) and the three scripts' usage errors."""
import functools
import math
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

import resample_ref as RR
from conftest import ROOT, pkg

# rate pair -> (o, n, width, K) for the default filter
TABLE = {(48000, 16000): (3, 1, 203, 409), (44100, 16000): (441, 160, 187, 815),
         (22050, 16000): (441, 320, 94, 629), (8000, 16000): (1, 2, 68, 137), (24000, 16000): (3, 2, 102, 207)}


@functools.lru_cache(maxsize=None)
def ref_taps(orig, new):
    return RR.taps(orig, new)


def _ulps(a, b):
    """distance in units of the last place between two fp32 arrays of one sign pattern"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("pair", sorted(TABLE))
def test_taps_match_restatement(pair):
    P = pkg("prepare")
    h, width, o, n = P.resample_taps(*pair)
    hr, wr, o_r, n_r = ref_taps(*pair)
    assert (o, n, width, h.shape[1]) == TABLE[pair] == (o_r, n_r, wr, hr.shape[1])
    assert h.dtype == np.float32 and h.shape == (n, 2 * width + o)
    r32 = hr.astype(np.float32)
    # 1 ulp of fp32; where the two round to different signs around 0 the values themselves are compared
    ok = (_ulps(h, r32) <= 1) | (np.abs(h.astype(np.float64) - hr) <= 2.0 ** -149)
    assert ok.all(), f"{(~ok).sum()} taps differ by more than 1 ulp"
    assert np.abs(hr).sum(1).max() <= 2.6


def test_taps_hann_and_options():
    P = pkg("prepare")
    h, width, o, n = P.resample_taps(5, 3, lowpass_filter_width=2, window="hann")
    hr, wr, _, _ = RR.taps(5, 3, lpw=2, window="hann")
    assert (o, n, width) == (5, 3, wr) and h.shape == hr.shape == (3, 2 * wr + 5)
    assert ((_ulps(h, hr.astype(np.float32)) <= 1) | (np.abs(h - hr) <= 2.0 ** -149)).all()
    with pytest.raises(ValueError, match="window"):
        P.resample_taps(5, 3, window="blackman")


def test_filter_pass_and_stop_band():
    """On the restatement alone, 22050 -> 16000, 0.25 s sines, the middle half of the output."""
    h, width, o, n = ref_taps(22050, 16000)
    L = 22050 // 4
    t = np.arange(L) / 22050.0
    db = {}
    for f in (1000.0, 7000.0, 8600.0, 9000.0, 10000.0):
        y = RR.resample(np.sin(2 * np.pi * f * t), h, width, o, n)
        mid = y[len(y) // 4: 3 * len(y) // 4]
        db[f] = 20 * math.log10(math.sqrt((mid ** 2).mean()) / math.sqrt(0.5) + 1e-300)
    print("rms gain dB:", db)
    assert abs(db[1000.0]) <= 1e-3 and abs(db[7000.0]) <= 1e-3
    assert max(db[8600.0], db[9000.0], db[10000.0]) <= -140.0


def test_lengths_and_refusals():
    P = pkg("prepare")
    for pair, (o, n, width, K) in TABLE.items():
        h = ref_taps(*pair)[0]
        for L in (1, o - 1, o, o + 1, 4001):
            if L < 1:
                continue
            want = math.ceil(n * L / o)
            assert P.out_len(L, o, n) == want
            if K * want < 3e6:            # the restatement itself, where it is cheap
                assert len(RR.resample(np.ones(L), h, width, o, n)) == want
    with pytest.raises(ValueError, match="cap"):
        P.resample_taps(44101, 16000)
    with pytest.raises(ValueError, match="positive"):
        P.resample_taps(0, 16000)


def test_empty_clip_raises():
    """identity needs no device; the check comes before anything is uploaded"""
    P = pkg("prepare")
    rs = P.Resampler(16000, 16000, device="cpu")
    with pytest.raises(ValueError, match="empty"):
        rs([np.ones(4, np.float32), np.zeros(0, np.float32)])
    with pytest.raises(ValueError, match="empty"):
        rs.to_int16([np.zeros(0, np.float32)])


def test_kernel_plan_limits():
    """the library's tile plan needs no device: whole frames, and the table cap is the host's"""
    K, P = pkg("kernels"), pkg("prepare")
    with open(os.path.join(ROOT, "include", "mms2ut.h")) as f:
        header = f.read()
    define = lambda name: eval(re.search(rf"#define {name}\s+(.+)", header).group(1))
    assert K.RESAMPLE_MAX_TAPS == P.MAX_TAPS == define("MMS_RESAMPLE_MAX_TAPS")
    assert K.RESAMPLE_TILE == define("MMS_RESAMPLE_TILE")
    assert K.resample_tile(1, 2, 137) == K.RESAMPLE_TILE       # two phases, nothing to round: the nominal tile
    with pytest.raises(pkg("_lib").HipError, match="exceed the LDS window"):
        K.resample_tile(1, 1, define("MMS_RESAMPLE_LDS_FLOATS") + 1)
    for (o, n, width, taps) in TABLE.values():
        tile = K.resample_tile(o, n, taps)
        assert tile % n == 0 and tile >= 4 * n
        assert (tile // n - 1) * o + taps <= 16384      # MMS_RESAMPLE_LDS_FLOATS
    with pytest.raises(pkg("_lib").HipError, match="cap"):
        K.resample_tile(44101, 16000, 44475)


# ------------------------------------------------------------------------------------------ host tools

def _wav(path, samples, rate=16000, channels=1, width=2):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.asarray(samples).astype({1: np.uint8, 2: "<i2"}[width]).tobytes())


def test_write_manifest_round_trip(tmp_path):
    P, U = pkg("prepare"), pkg("units")
    root = tmp_path / "wav"
    lens = {"b/2.wav": 700, "a/10.wav": 1601, "a/9.wav": 1, "3.wav": 4000}
    for rel, n in lens.items():
        _wav(str(root / rel), np.arange(n) % 100)
    (root / "notes.txt").write_text("not audio")
    dest = tmp_path / "manifest" / "train.tsv"
    assert P.write_manifest(str(root), str(dest), ext="wav") == 4
    lines = dest.read_text().splitlines()
    assert lines[0] == os.path.realpath(root)
    assert lines[1:] == [f"{rel}\t{lens[rel]}" for rel in sorted(lens)]
    got_root, files = U.read_manifest(str(dest))
    assert got_root == os.path.realpath(root) and files == sorted(lens)
    with pytest.raises(ValueError, match="no files"):
        P.write_manifest(str(root), str(dest), ext=".flac")


@pytest.fixture()
def s2ut_dirs(tmp_path):
    rng = np.random.default_rng(5)
    src, tgt = tmp_path / "16khz_wav", tmp_path / "units"
    lens = {"1": 1600, "2": 4001, "3": 799, "10": 16000, "21": 480}
    for stem, n in lens.items():
        _wav(str(src / "train" / f"{stem}.wav"), rng.integers(-3000, 3000, n))
    units = {"1": "5 5 5 7 7 5", "2": "1 2 3", "10": "9 9 9 9", "21": "4 4 8 8 8 4 0 0"}     # no units for "3"
    tgt.mkdir()
    (tgt / "train.txt").write_text("".join(f"{k}|{v}\n" for k, v in units.items()))
    return src, tgt, lens, units


@pytest.mark.parametrize("reduce", [False, True])
def test_prep_s2ut_data(s2ut_dirs, tmp_path, reduce):
    P, Mf = pkg("prepare"), pkg("manifest")
    src, tgt, lens, units = s2ut_dirs
    out = tmp_path / "format_data"
    rep = P.prep_s2ut_data(str(src), str(tgt), ["train"], str(out), reduce_unit=reduce,
                           vocoder_checkpoint="/voc/model.pt", vocoder_cfg="/voc/config.json")
    assert rep == {"train": {"written": 4, "missing": ["3"]}}
    assert "1 with missing target data" in P.report_lines(rep)[0] and "3" in P.report_lines(rep)[0]
    rows = [ln.split("\t") for ln in (out / "train.tsv").read_text().splitlines()]
    assert rows[0] == ["id", "src_audio", "src_n_frames", "tgt_text", "tgt_n_frames"]
    want_units = {"1": "5 7 5", "2": "1 2 3", "10": "9", "21": "4 8 4 0"} if reduce else units
    assert [r[0] for r in rows[1:]] == ["1", "2", "10", "21"]               # natural numeric order
    for r in rows[1:]:
        assert r[1] == os.path.abspath(src / "train" / f"{r[0]}.wav")
        assert r[2] == str(lens[r[0]] // 160)
        assert r[3] == want_units[r[0]] and r[4] == str(len(want_units[r[0]].split()))

    import yaml
    cfg = yaml.safe_load((out / "config.yaml").read_text())
    assert cfg["input_channels"] == 1 and cfg["input_feat_per_channel"] == 80
    assert cfg["vocoder"] == {"type": "code_hifigan", "config": "/voc/config.json", "checkpoint": "/voc/model.pt"}
    assert cfg["transforms"] == {"*": ["utterance_cmvn"], "_train": ["utterance_cmvn", "specaugment"]}

    d = Mf.UnitDictionary.for_codes(1000)
    ds = Mf.MultiModalS2SManifest(str(out), "train", d)
    assert len(ds) == 4 and ds.ids == ["1", "2", "10", "21"]
    assert ds.n_frames.tolist() == [lens[s] // 160 for s in ds.ids]
    assert ds.tgt_n_frames.tolist() == [len(want_units[s].split()) for s in ds.ids]
    assert ds.cmvn and ds.specaugment is not None
    sa = ds.specaugment
    assert (sa.fn, sa.ff, sa.tn, sa.tt, sa.tp) == (1, 27, 1, 100, 1.0)
    it = ds.item(2)
    assert len(it["wave"]) == lens["10"]
    assert it["target"].tolist() == [int(u) + 4 for u in want_units["10"].split()] + [Mf.EOS]
    assert Mf.feature_transforms(ds.data_cfg, "train", True) == ["utterance_cmvn", "specaugment"]
    assert Mf.feature_transforms(ds.data_cfg, "valid", False) == ["utterance_cmvn"]
    ev = Mf.MultiModalS2SManifest(str(out), "train", d, is_train=False)
    assert ev.cmvn and ev.specaugment is None


def test_prep_s2ut_data_refuses_other_rates(s2ut_dirs, tmp_path):
    P = pkg("prepare")
    src, tgt, _, _ = s2ut_dirs
    _wav(str(src / "train" / "2.wav"), np.zeros(2205), rate=22050)
    with pytest.raises(ValueError, match=r"2\.wav: 22050 Hz.*mms2ut_resample"):
        P.prep_s2ut_data(str(src), str(tgt), ["train"], str(tmp_path / "out"))
    with pytest.raises(FileNotFoundError):
        P.prep_s2ut_data(str(src), str(tgt), ["valid"], str(tmp_path / "out"))


def test_convert_dir_copies_16k_mono_without_gpu(tmp_path):
    P = pkg("prepare")
    rng = np.random.default_rng(6)
    src, dst = tmp_path / "src", tmp_path / "dst"
    clips = {"train/1.wav": 1601, "train/deep/er/2.wav": 1, "valid/7.wav": 4000}
    for rel, n in clips.items():
        _wav(str(src / rel), rng.integers(-32768, 32768, n))
    rep = P.convert_dir(str(src), str(dst), num_workers=2)
    assert rep == {"files": 3, "copied": 3, "resampled": {}}
    for rel in clips:
        assert (dst / rel).read_bytes() == (src / rel).read_bytes()
    _wav(str(src / "train" / "8bit.wav"), np.full(100, 128), width=1)
    with pytest.raises(ValueError, match=r"8bit\.wav.*16-bit"):
        P.convert_dir(str(src), str(tmp_path / "dst2"))
    (src / "train" / "8bit.wav").unlink()
    (src / "train" / "speech.wav").write_bytes(b"ID3\x03" + bytes(200))          # an mp3 under a .wav name
    with pytest.raises(ValueError, match=r"speech\.wav"):
        P.convert_dir(str(src), str(tmp_path / "dst3"))


@pytest.mark.parametrize("script", ["mms2ut_resample.py", "mms2ut_manifest.py", "mms2ut_prep_s2ut_data.py"])
def test_scripts_usage(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)], capture_output=True, text=True)
    assert r.returncode != 0
    assert "usage:" in r.stderr

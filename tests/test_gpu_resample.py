"""GPU: the resampling kernel (csrc/resample.hip, mms2ut_resample_f32) against the float64 restatement in
tests/resample_ref.py, within the fp32 dot-product bound computed from the taps,
    |y_dev - y_ref| <= (K + 2) 2^-24 (max_i sum_c |h[i][c]|) max|x|,
at every clip length where the indexing changes (1, 2, around the filter half-width, around one input
frame, around the kernel's output tile, 4001); clip isolation and determinism bit for bit; the identity
rate; the int16 output of the same launch; and the tools end to end (convert_dir -> write_manifest ->
prep_s2ut_data -> MultiModalS2SManifest)."""
import functools
import math
import os
import wave

import numpy as np
import pytest
import torch

import resample_ref as RR
from conftest import pkg

pytestmark = pytest.mark.gpu

HANN = dict(lowpass_filter_width=2, window="hann")
CASES = {"48000-16000": (48000, 16000, {}), "22050-16000": (22050, 16000, {}), "8000-16000": (8000, 16000, {}),
         "24000-16000": (24000, 16000, {}), "5-3-hann": (5, 3, HANN)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def ref_taps(name):
    orig, new, kw = CASES[name]
    return RR.taps(orig, new, lpw=kw.get("lowpass_filter_width", RR.LPW), window=kw.get("window", "kaiser"))


@functools.lru_cache(maxsize=None)
def resampler(name):
    orig, new, kw = CASES[name]
    return pkg("prepare").Resampler(orig, new, device="cuda", **kw)


def lengths(name):
    """every clip length at which the kernel's indexing takes another path"""
    _, width, o, n = ref_taps(name)
    K = 2 * width + o
    tile = pkg("kernels").resample_tile(o, n, K)          # outputs per block, a multiple of n
    full = tile // n * o                                  # the input length that fills exactly one tile
    want = [1, 2, width - 1, width, width + 1, o - 1, o, o + 1, tile - 1, tile, tile + 1, full - 1, full, full + 1, 4001]
    return sorted({L for L in want if L >= 1})


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_restatement(name):
    h, width, o, n = ref_taps(name)
    K = h.shape[1]
    rs = resampler(name)
    assert (rs.width, rs.o, rs.n, rs.K) == (width, o, n, K)
    rng = np.random.default_rng(11)
    clips = [rng.uniform(-1, 1, L).astype(np.float32) for L in lengths(name)]
    outs = [t.cpu().numpy() for t in rs(clips)]
    worst = 0.0
    for x, y in zip(clips, outs):
        ref = RR.resample(x, h, width, o, n)
        assert y.dtype == np.float32 and len(y) == len(ref) == math.ceil(n * len(x) / o)
        tol = RR.bound(h, K, np.abs(x).max())
        err = np.abs(y.astype(np.float64) - ref).max()
        worst = max(worst, err / tol)
        assert err <= tol, f"{name}: clip of {len(x)} samples: |err| {err:.3e} > bound {tol:.3e}"
    print(f"{name}: K {K}, lengths {lengths(name)}, worst |err| / bound = {worst:.2e}")


@pytest.mark.parametrize("name", ["22050-16000", "48000-16000", "5-3-hann"])
def test_clips_are_isolated_and_runs_repeat(name):
    """a 1-sample and a width-sample clip between two full-scale clips: a read past a clip's edge would pull
    +-1 samples into outputs whose own inputs are small"""
    _, width, o, n = ref_taps(name)
    rs = resampler(name)
    rng = np.random.default_rng(12)
    square = lambda L: np.where(np.arange(L) % 7 < 3, 1.0, -1.0).astype(np.float32)
    small = lambda L: rng.uniform(-1e-3, 1e-3, L).astype(np.float32)
    clips = [small(4001), square(900), small(1), small(width), square(1301), small(2 * o + 1), small(o + 1)]
    batch = [t.cpu().numpy() for t in rs(clips)]
    again = [t.cpu().numpy() for t in rs(clips)]
    for k, x in enumerate(clips):
        alone = rs([x])[0].cpu().numpy()
        assert _same_bits(batch[k], alone), f"clip {k} ({len(x)} samples) differs between batch and alone"
        assert _same_bits(batch[k], again[k]), f"clip {k} differs between two runs"
    for k in (2, 3):                                      # nothing leaked in from the full-scale neighbours
        assert np.abs(batch[k]).max() <= 2.6e-3


def test_identity_returns_input_bits():
    rs = pkg("prepare").Resampler(16000, 16000, device="cuda")
    rng = np.random.default_rng(13)
    clips = [rng.uniform(-40000, 40000, L).astype(np.float32) for L in (1, 4001, 160)]
    clips[1][:3] = [0.0, -0.0, np.float32(1e-42)]
    for x, y in zip(clips, rs(clips)):
        assert y.is_cuda and _same_bits(y.cpu().numpy(), x)


@pytest.mark.parametrize("name", ["22050-16000", "8000-16000"])
def test_int16_is_rint_clip_of_the_same_launch(name):
    K = pkg("kernels")
    rs = resampler(name)
    rng = np.random.default_rng(14)
    loud = np.where(np.arange(3000) % 50 < 25, 32767.0, -32768.0).astype(np.float32)      # overshoots: clips
    clips = [rng.integers(-32768, 32768, 4001).astype(np.float32), loud, rng.integers(-5, 6, 777).astype(np.float32)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    x = torch.from_numpy(np.concatenate(clips)).cuda()
    y, out_off, y16 = K.resample(x, off, rs.taps, rs.o, rs.n, rs.width, int16=True)
    y, y16 = y.cpu().numpy(), y16.cpu().numpy()
    assert y16.dtype == np.int16 and y16.shape == y.shape and out_off[-1] == len(y)
    assert (y > 32767.5).any() and (y < -32768.5).any(), "the case must contain values that clip"
    assert np.array_equal(y16, np.clip(np.rint(y), -32768, 32767).astype(np.int16))
    for a, b in zip(rs.to_int16(clips), np.split(y16, out_off[1:-1])):
        assert a.dtype == torch.int16 and np.array_equal(a.cpu().numpy(), b)
    y_only, _, none = K.resample(x, off, rs.taps, rs.o, rs.n, rs.width)
    assert none is None and _same_bits(y_only.cpu().numpy(), y)


def test_wrapper_refuses_bad_arguments():
    K = pkg("kernels")
    rs = resampler("24000-16000")
    x = torch.zeros(10, device="cuda")
    with pytest.raises(ValueError, match="empty"):
        K.resample(x, [0, 4, 4, 10], rs.taps, rs.o, rs.n, rs.width)
    with pytest.raises(ValueError, match="in_off"):
        K.resample(x, [0, 4, 11], rs.taps, rs.o, rs.n, rs.width)
    with pytest.raises(ValueError, match="taps"):
        K.resample(x, [0, 10], rs.taps.t().contiguous(), rs.o, rs.n, rs.width)
    with pytest.raises(ValueError, match="fp32"):
        K.resample(x.double(), [0, 10], rs.taps, rs.o, rs.n, rs.width)


def test_tools_end_to_end(tmp_path):
    """three stereo 22050 Hz WAVs -> convert_dir -> write_manifest -> prep_s2ut_data -> the training loader"""
    P, Mf, U = pkg("prepare"), pkg("manifest"), pkg("units")
    h, width, o, n = ref_taps("22050-16000")
    rng = np.random.default_rng(15)
    src, dst = tmp_path / "wav", tmp_path / "16khz_wav"
    os.makedirs(src / "train")
    refs = {}
    for stem, L in (("1", 2000), ("2", 3001), ("3", 4410)):
        st = rng.integers(-12000, 12000, (L, 2)).astype("<i2")
        with wave.open(str(src / "train" / f"{stem}.wav"), "wb") as w:
            w.setnchannels(2)
            w.setsampwidth(2)
            w.setframerate(22050)
            w.writeframes(st.tobytes())
        mono = st.astype(np.float32).mean(axis=1, dtype=np.float32)
        refs[stem] = np.clip(np.rint(RR.resample(mono, h, width, o, n)), -32768, 32767)
    rep = P.convert_dir(str(src), str(dst), batch_size=2, num_workers=2)
    assert rep == {"files": 3, "copied": 0, "resampled": {22050: 3}}
    for stem, ref in refs.items():
        got, sr, ch = Mf.read_wav_info(str(dst / "train" / f"{stem}.wav"))
        assert (sr, ch) == (16000, 1) and len(got) == len(ref)
        assert np.abs(got - ref).max() <= 1, f"{stem}.wav: more than 1 LSB from the restatement"
    tsv = tmp_path / "manifest" / "train.tsv"
    assert P.write_manifest(str(dst / "train"), str(tsv)) == 3
    root, files = U.read_manifest(str(tsv))
    assert root == os.path.realpath(dst / "train") and files == ["1.wav", "2.wav", "3.wav"]
    (tmp_path / "manifest" / "train.txt").write_text("1|3 3 4\n2|7\n3|1 2 2 2 9\n")
    out = tmp_path / "format_data"
    rep = P.prep_s2ut_data(str(dst), str(tmp_path / "manifest"), ["train"], str(out), reduce_unit=True,
                           vocoder_checkpoint="model.pt", vocoder_cfg="config.json")
    assert rep == {"train": {"written": 3, "missing": []}}
    ds = Mf.MultiModalS2SManifest(str(out), "train", Mf.UnitDictionary.for_codes(1000))
    assert ds.ids == ["1", "2", "3"] and ds.n_frames.tolist() == [len(refs[s]) // 160 for s in ds.ids]
    assert [ds.item(i)["target"].tolist() for i in range(3)] == [[7, 8, 2], [11, 2], [5, 6, 13, 2]]
    assert np.array_equal(ds.item(0)["wave"], Mf.read_wav(str(dst / "train" / "1.wav"))[0])

"""GPU: the noise-augmentation kernels (csrc/noise.hip, mms2ut_noise_mix_f32) against the numpy
restatement in tests/noise_util.py (bit for bit: the fp64 sums are exact for 16-bit samples and
every later operation is one fp32 rounding on both sides), against fixtures written by the
reference's own add_noise_v2 (|err| <= 4 d + 1 ulp of the peak, d = the reference's own fp32
distance from the exact result, stored per case), and through both data paths: the DeviceLoader
and the fairseq drop-in's wave_net_input_src."""
import numpy as np
import pytest
import torch

import noise_util as NU
from conftest import pkg
from manifest_corpus import write_corpus
from oracle import ref_model as R

pytestmark = pytest.mark.gpu

LENS = (6007, 4000, 2403, 1601, 400)            # offsets 6007, 10007, 12410, 14011: none a multiple of 4
CLIP_LENS = (700, 2403, 9000)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(17)
    waves = [rng.integers(-9000, 9000, T).astype(np.float32) for T in LENS]
    clips = [rng.integers(-2500, 2500, L).astype(np.int16) for L in CLIP_LENS]
    return waves, clips


def _bits(f):
    return int(np.array([f], dtype=np.float32).view(np.int32)[0])


def _mix(waves, clips, params):
    """mms2ut_noise_mix_f32 on the utterances laid back to back -> list of fp32 arrays."""
    K = pkg("kernels")
    params = np.ascontiguousarray(params, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    wb = {"wave": torch.from_numpy(np.concatenate(waves).astype(np.float32)).cuda(),
          "wave_off": torch.from_numpy(off).cuda(), "B": len(waves)}
    bank = torch.from_numpy(np.concatenate(clips)).cuda()
    boff = torch.from_numpy(np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)).cuda()
    K.noise_mix(wb, bank, boff, torch.from_numpy(params).cuda(), params.shape[1] - 3)
    torch.cuda.synchronize()
    out = wb["wave"].cpu().numpy()
    return [out[off[b]:off[b + 1]] for b in range(len(waves))]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# rows {apply, start, f, ids}: T > L with eight wraps and start + T == Lt; T < L ending on the clip's
# last sample; apply 0 in the middle (then T == L there, with the neighbour off); a 400-sample tail
PARAMS_K1 = [
    [[1, 293, _bits(0.31), 0], [1, 5000, _bits(0.07), 2], [0, 0, 0, 0], [1, 802, _bits(0.5), 1], [1, 150, _bits(0.2), 0]],
    [[1, 0, _bits(0.45), 0], [0, 0, 0, 0], [1, 0, _bits(0.12), 1], [0, 0, 0, 0], [1, 300, _bits(0.35), 0]],
    [[1, 2993, _bits(0.25), 2], [1, 806, _bits(0.4), 1], [1, 1500, _bits(0.3), 2], [1, 0, _bits(0.09), 2],
     [1, 2003, _bits(0.5), 1]],
]
# K = 3: L = the shortest chosen clip (700 / 2403 / 9000)
PARAMS_K3 = [
    [[1, 293, _bits(0.31), 0, 1, 2], [1, 806, _bits(0.2), 2, 1, 1], [0, 0, 0, 0, 0, 0], [1, 7399, _bits(0.5), 2, 2, 2],
     [1, 300, _bits(0.4), 1, 0, 2]],
    [[0, 0, 0, 0, 0, 0], [1, 0, _bits(0.3), 1, 2, 0], [1, 0, _bits(0.15), 1, 1, 2], [1, 100, _bits(0.45), 0, 0, 0],
     [0, 0, 0, 0, 0, 0]],
]


@pytest.mark.parametrize("params", PARAMS_K1 + PARAMS_K3)
def test_bit_identical_to_restatement(data, params):
    waves, clips = data
    params = np.array(params, dtype=np.int32)
    ref = NU.mix_waves(waves, clips, params)
    got = _mix(waves, clips, params)
    for b, (g, r, w) in enumerate(zip(got, ref, waves)):
        assert np.all(np.isfinite(g))
        if params[b, 0] == 0:
            assert _same_bits(g, w), f"utterance {b}: apply 0 must leave the samples untouched"
        else:
            assert not np.array_equal(g, w)
            assert _same_bits(g, r), f"utterance {b}: max |diff| {np.abs(g - r).max()}"


def test_normalising_bit_identical(data):
    """A quiet clip with a few full-scale spikes: the gain lifts them past 1, so max|y| > 1 and the
    true division by the folded maximum is exercised (K = 1 and the floor-mean noise of K = 2)."""
    waves, clips = data
    spiky = (np.arange(2403) % 7 - 3).astype(np.int16)
    spiky[100::300] = 32767
    spiky[250::300] = -32768
    for row in ([1, 57, _bits(0.5), 0], [1, 57, _bits(0.5), 0, 1]):
        params = np.array([row, row], dtype=np.int32)
        pair = [waves[3], waves[4]]
        ref = NU.mix_waves(pair, [spiky, clips[1]], params)
        got = _mix(pair, [spiky, clips[1]], params)
        if len(row) == 4:
            assert all(np.abs(r).max() == 32768.0 for r in ref)       # normalised to the peak
        assert all(_same_bits(g, r) for g, r in zip(got, ref))


def test_golden_cases():
    """The reference's own output (scripts/gen_noise_golden.py): a T < L, b normalising, c two
    wraps, d T == L, e three clips of different lengths (floor-mean path), f one fbank frame."""
    for name, g in NU.golden_cases():
        got = _mix([g["clean"].astype(np.float32)], g["clips"], NU.golden_params(g))[0]
        err = float(np.abs(got.astype(np.float64) / 32768.0 - g["out"].astype(np.float64)).max())
        print(f"case {name}: err {err:.3e}, d {float(g['d']):.3e}, tol {NU.golden_tol(g):.3e}")
        assert err <= NU.golden_tol(g), name


def test_placement_independence(data):
    waves, clips = data
    rng = np.random.default_rng(3)
    row = [1, 4321, _bits(0.27), 2]
    alone = _mix([waves[1]], clips, [row])[0]
    for lead in (1601, 402, 403, 400):              # the utterance starts 1, 2, 3 and 0 samples past a 16-B boundary
        pre = rng.integers(-9000, 9000, lead).astype(np.float32)
        batch = [pre, waves[1], waves[3]]
        p = [[1, 10, _bits(0.4), 1], row, [1, 0, _bits(0.1), 0]]
        a, b = _mix(batch, clips, p), _mix(batch, clips, p)
        assert all(_same_bits(x, y) for x, y in zip(a, b))       # run to run
        assert _same_bits(a[1], alone), f"offset {lead}"
    row3 = [1, 17, _bits(0.33), 1, 2, 0]
    alone3 = _mix([waves[1]], clips, [row3])[0]
    assert _same_bits(_mix([waves[4][:399], waves[1]], clips, [[0, 0, 0, 0, 0, 0], row3])[1], alone3)


def test_degenerate_inputs(data):
    waves, clips = data
    f = np.float32(0.3)
    zero = np.zeros(1601, np.float32)
    out = _mix([zero, waves[3]], clips, [[1, 5, _bits(f), 1], [1, 5, _bits(f), 1]])
    assert np.all(out[0] == 0) and np.all(np.isfinite(out[1]))
    silent = [np.zeros(2000, np.int16), clips[1]]
    out = _mix([waves[3], waves[4]], silent, [[1, 399, _bits(f), 0], [1, 0, _bits(f), 0]])
    for g, w in zip(out, (waves[3], waves[4])):
        # seg g = 0 exactly and max|y| < 1: out = x (1 - f), no NaN from the huge gain
        assert _same_bits(g, (w * np.float32(2.0 ** -15)) * (np.float32(1.0) - f) * np.float32(32768.0))
    out = _mix([zero], silent, [[1, 0, _bits(f), 0]])
    assert np.all(out[0] == 0)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    mm = pkg()
    M, FE = mm.manifest, mm.frontend
    root = tmp_path_factory.mktemp("noise_corpus")
    c = write_corpus(str(root), frames=(38, 21, 30, 21, 26), di=768, ti=5, split="valid")   # noise only
    rng = np.random.default_rng(9)
    paths, clips = [], []
    for i, L in enumerate((3001, 7000, 1234)):
        clips.append(rng.integers(-4000, 4000, L).astype(np.int16))
        paths.append(str(root / f"noise{i}.wav"))
        M.write_wav(paths[-1], clips[-1])
    cfg = mm.default_cfg(**R.tiny_config(conv_channels=256))

    def loader(prob, num=2):
        aug = None if prob is None else FE.NoiseAugment(paths, prob, [0, 15], num)
        ds = M.MultiModalS2SManifest(str(root), "valid", M.UnitDictionary.for_codes(1000), is_train=False,
                                     image_feat_path=c["feat_dir"], noise=aug)
        return ds, aug, ds.batches(max_tokens=80)

    return {"c": c, "clips": clips, "cfg": cfg, "loader": loader}


def _replay(aug, b, n_samples, seed=1, epoch=1):
    """The loader's per-batch stream (manifest.DeviceLoader._to_device)."""
    return aug.draws(n_samples, np.random.RandomState((seed * 1000003 + epoch * 7919 + b) % 2 ** 32))


def test_device_loader_end_to_end(corpus):
    mm = pkg()
    M, FE = mm.manifest, mm.frontend
    fe = FE.FbankFrontend("cuda:0")
    ds, aug, batches = corpus["loader"](1.0)
    ds0, _, _ = corpus["loader"](None)
    dsz, _, _ = corpus["loader"](0.0)
    assert len(batches) >= 2 and ds.specaugment is None
    noisy = [b.src.clone() for b, _ in M.DeviceLoader(ds, batches, corpus["cfg"], "cuda:0")]
    clean = [b.src.clone() for b, _ in M.DeviceLoader(ds0, batches, corpus["cfg"], "cuda:0")]
    zero = [b.src.clone() for b, _ in M.DeviceLoader(dsz, batches, corpus["cfg"], "cuda:0")]
    for b, idx in enumerate(batches):
        _, waves = ds0.collate(idx)
        params = _replay(aug, b, [len(w) for w in waves])
        assert params[:, 0].all()
        ref = fe(fe.upload(NU.mix_waves(waves, corpus["clips"], params)))
        torch.cuda.synchronize()
        err = float((noisy[b].float() - ref.float()).abs().max())
        moved = float((noisy[b].float() - clean[b].float()).abs().max())
        print(f"batch {b}: |noisy - restatement| {err:.3e}, |noisy - clean| {moved:.3f}")
        assert noisy[b].shape == ref.shape and err <= 5e-3
        assert moved > 0.1
        assert torch.equal(zero[b], clean[b])


def test_fairseq_dropin_equals_device_loader(corpus):
    mm = pkg()
    M, FE = mm.manifest, mm.frontend
    ds, aug, batches = corpus["loader"](1.0, num=1)
    key = FE.register_noise_bank(aug.key, aug)
    loaded = [b.src.clone() for b, _ in M.DeviceLoader(ds, batches, corpus["cfg"], "cuda:0")]
    for b, idx in enumerate(batches):
        _, waves = ds.collate(idx)
        flat = torch.from_numpy(np.concatenate(waves).astype(np.float32).view(np.int32))
        off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64))
        params = torch.from_numpy(_replay(aug, b, [len(w) for w in waves]))
        for dev in ("cpu", "cuda:0"):               # fairseq moves the sample to the GPU before the forward
            ni = {"src_waves": flat.to(dev), "src_wave_offsets": off.to(dev), "src_cmvn": True,
                  "src_noise": {"params": params.to(dev), "n_mix": 1, "bank": key}}
            out = FE.wave_net_input_src(ni, "cuda:0")
            torch.cuda.synchronize()
            assert torch.equal(out, loaded[b])
            assert torch.equal(ni["src_waves"].cpu(), flat)          # the sample's waveforms stay clean
        ni.pop("src_noise")
        assert not torch.equal(FE.wave_net_input_src(ni, "cuda:0"), loaded[b])

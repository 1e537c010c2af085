"""GPU: the top-k beam decode of speech units (csrc/units.hip kmeans_topk, csrc/units_beam.hip) and
HubertUnits.decode built on them.

units_beam is integer and float32 work with every rounding pinned, so it must equal its host restatement
units.beam_decode_host bit for bit (tests/test_units_beam.py ties that one to the reference's own decode).

kmeans_topk is compared with a float64 evaluation of the reference's formula sqrt(|x|^2 - 2 x.C + |C|^2) on
the same fp16-rounded rows.  The yardstick is the reference's own float32 torch expression on the CPU: its
max-abs distance from float64 over these inputs is measured, and the kernel may be 4 x as far (another
accumulation order; the hi/lo centroid images carry 22 bits).  The indices must equal the float64 order on
every row whose first top_k + 1 float64 distances lie pairwise further apart than twice that bound; at most
5 % of the rows may fail that condition, which is asserted on the inputs before the kernel is looked at."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import asr_ref as AR
import hubert_ref as HR
from conftest import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIST_FACTOR, EXEMPT_CAP = 4.0, 0.05
GOLD = ["a", "b", "c", "one", "open"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def U():
    return pkg("units")


@pytest.fixture(scope="module")
def K():
    return pkg("kernels")


# ------------------------------------------------------------------------------------------ units_beam

def _beam_check(U, K, idx, val, lens, beamsize):
    """units_beam on idx / val [B, Tmax, k] (numpy) against the host restatement, utterance by utterance."""
    B, Tm, _ = idx.shape
    lens32 = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    args = (torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV), lens32)
    code, merged, count, bad = K.units_beam(*args, beamsize=beamsize)
    again = K.units_beam(*args, beamsize=beamsize)
    assert all(torch.equal(a, b) for a, b in zip(again, (code, merged, count, bad)))      # bitwise reproducible
    assert bad.tolist() == [0] * B
    out = []
    for b in range(B):
        T = Tm if lens is None else lens[b]
        want = U.beam_decode_host(idx[b, :T], val[b, :T], beamsize)
        assert code[b, :T].tolist() == want
        assert int(count[b]) == len(U.merge(want)) and merged[b, :int(count[b])].tolist() == U.merge(want)
        assert not code[b, T:].any() and not merged[b, int(count[b]):].any()
        out.append(want)
    return out


def _random_topk(B, Tm, k, vocab, seed):
    """Frames whose k candidates come from a small vocabulary (so runs and repeated tokens exist), with
    ascending positive distances."""
    r = np.random.default_rng(seed)
    idx = np.stack([np.stack([r.permutation(vocab)[:k] for _ in range(Tm)]) for _ in range(B)]).astype(np.int32)
    val = np.sort(r.random((B, Tm, k), dtype=np.float32) * np.float32(3.0) + np.float32(0.25), axis=2)
    return idx, val


@pytest.mark.parametrize("case", GOLD)
def test_units_beam_golden(U, K, case):
    g = np.load(os.path.join(GOLDEN, f"units_beam_{case}.npz"))
    want, = _beam_check(U, K, g["idx"][None], g["val"][None], None, int(g["beamsize"]))
    assert want == g["beam_code"].tolist()                       # and so the device equals the reference's own run


def test_units_beam_packed_batch(U, K):
    """1, 37 and 64 frames in one Tmax = 64 tensor at the defaults; the padding frames hold NaN distances,
    which nothing may read."""
    lens = [1, 37, 64]
    idx, val = _random_topk(3, 64, 10, 14, 11)
    for b, T in enumerate(lens):
        val[b, T:] = np.nan
        idx[b, T:] = -7
    beams = _beam_check(U, K, idx, val, lens, 200)
    assert any(beams[b] != idx[b, :lens[b], 0].tolist() for b in (1, 2))      # the beam does not just follow the nearest


@pytest.mark.parametrize("top_k,beamsize", [(32, 64), (8, 256)])
def test_units_beam_at_the_limits(U, K, top_k, beamsize):
    idx, val = _random_topk(1, 20, top_k, 40, top_k)
    _beam_check(U, K, idx, val, None, beamsize)


def test_units_beam_flags_and_refuses(K):
    idx, val = _random_topk(3, 6, 4, 9, 3)
    val[0, 2] = 0.0                                   # a frame on its 4 nearest centroids: the divisor is 0
    val[1, 5, 3] = np.inf
    val[2, 5, 3] = np.inf                             # past lens[2]
    lens = torch.tensor([6, 6, 5], dtype=torch.int32, device=DEV)
    bad = K.units_beam(torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV), lens, beamsize=5)[3]
    assert bad.tolist() == [1, 1, 0]
    i32, f32 = torch.zeros(1, 2, 33, dtype=torch.int32, device=DEV), torch.ones(1, 2, 33, device=DEV)
    with pytest.raises(NotImplementedError, match="32"):
        K.units_beam(i32, f32)
    with pytest.raises(NotImplementedError, match="2048"):
        K.units_beam(i32[..., :10].contiguous(), f32[..., :10].contiguous(), beamsize=205)
    with pytest.raises(ValueError):
        K.units_beam(i32[..., :10].contiguous(), f32[..., :9].contiguous())


# ------------------------------------------------------------------------------------------ kmeans_topk

def _gen(seed):
    return torch.Generator().manual_seed(seed)


_SHAPES = {
    # R = 70: a partial 64-row block and a partial wave; d = 24: a k-step tail; Kc = 100: off the 16-grid
    "tail": dict(B=1, Tm=70, lens=None, d=24, Kc=100, chunk=None, seed=1),
    # the real widths, 16 chunks of 64 centroids, two utterances of 5 and 33 frames
    "wide": dict(B=2, Tm=33, lens=[5, 33], d=768, Kc=1000, chunk=64, seed=2),
}
_REF = {}


def _spaced_inputs(R, d, Kc, seed, rays=4):
    """Rows and centroids whose distances are evenly spaced, so that the index check can cover (nearly) every
    row at top_k = 32: with random centroids the 33 nearest of 1000 lie about 1e-2 apart at random, and a third
    of the rows would have two of them closer than the bound.

    The first half of the width holds `rays` directions w_g on disjoint coordinates (orthogonal exactly),
    each of squared length P; the second half a dense vector z.  Centroid c = a_c w_(c mod rays) + s_c z with
    a_c, s_c rising evenly in c; row r = -beta_r w_(r mod rays) + gamma_r z' (z' another dense vector).  Then
      d^2(r, c) = beta^2 P + gamma^2 |z'|^2 + a_c^2 P + s_c^2 |z|^2 - 2 gamma s_c z.z'
    for the centroids off the row's own ray, rising smoothly in c (its own ray's lie further out): the gaps
    are regular, the order differs from row to row by the ray left out, and every distance still hangs on a
    dot product over the dense half, which differs from centroid to centroid and needs the lo image."""
    g = _gen(seed)
    h, per = d // 2, d // 2 // rays
    W = torch.zeros(rays, d, dtype=torch.float64)
    for q in range(rays):
        w = torch.randn(per, generator=g, dtype=torch.float64)
        W[q, q * per:(q + 1) * per] = w * (per ** 0.5 / w.norm())
    z, zp = torch.zeros(2, d, dtype=torch.float64)
    z[h:], zp[h:] = 0.5 * torch.randn(d - h, generator=g, dtype=torch.float64), 0.5 * torch.randn(d - h, generator=g, dtype=torch.float64)
    c, r = torch.arange(Kc, dtype=torch.float64), torch.arange(R, dtype=torch.float64)
    Cm = (1.0 + 3.3 * c / Kc)[:, None] * W[torch.arange(Kc) % rays] + (1.0 + 0.3 * c / Kc)[:, None] * z[None]
    X = -(0.3 + 0.4 * r / R)[:, None] * W[torch.arange(R) % rays] + (0.5 + r / R)[:, None] * zp[None]
    return X.half(), Cm.float()


def _topk_reference(name):
    """Computed once per shape on the CPU and left unchanged: the inputs, the float64 distances of the
    fp16-rounded rows, and the reference expression's own float32 error e32 against them."""
    if name not in _REF:
        s = _SHAPES[name]
        R = s["B"] * s["Tm"]
        X, Cm = _spaced_inputs(R, s["d"], s["Kc"], s["seed"])
        valid = (torch.ones(s["B"], s["Tm"], dtype=torch.bool) if s["lens"] is None else
                 torch.arange(s["Tm"])[None] < torch.tensor(s["lens"])[:, None]).reshape(-1)
        x64, c64 = X.double(), Cm.double()
        d64 = torch.sqrt(x64.pow(2).sum(1, keepdim=True) - 2 * x64 @ c64.t() + c64.pow(2).sum(1)[None])
        feature, C, Cnorm = X.float(), Cm.t().contiguous(), Cm.pow(2).sum(1)[None]
        d32 = torch.sqrt(feature.pow(2).sum(1, keepdim=True) - 2 * torch.matmul(feature, C) + Cnorm)
        e32 = float((d32.double() - d64)[valid].abs().max())
        _REF[name] = (X.reshape(s["B"], s["Tm"], s["d"]), Cm, valid, d64, e32)
    return _REF[name]


@pytest.mark.parametrize("top_k", [1, 10, 32])
@pytest.mark.parametrize("name", list(_SHAPES))
def test_kmeans_topk_kernel(K, name, top_k):
    s = _SHAPES[name]
    X3, Cm, valid, d64, e32 = _topk_reference(name)
    bound = DIST_FACTOR * e32
    order = d64.argsort(dim=1, stable=True)
    srt = d64.gather(1, order)
    first = srt[:, :min(top_k + 1, s["Kc"])]
    sure = ((first[:, 1:] - first[:, :-1]) > 2.0 * bound).all(1) & valid
    exempt = 1.0 - float(sure[valid].float().mean())
    assert e32 > 0 and exempt <= EXEMPT_CAP, (name, top_k, e32, exempt)       # the inputs, before the kernel
    packed = tuple(t.to(DEV) for t in K.kmeans_pack(Cm))
    lens32 = None if s["lens"] is None else torch.tensor(s["lens"], dtype=torch.int32, device=DEV)
    idx, dist, bad = K.kmeans_topk(X3.to(DEV), *packed, lens32, top_k=top_k, chunk=s["chunk"])
    assert idx.shape == dist.shape == (s["B"], s["Tm"], top_k) and bad.tolist() == [0] * s["B"]
    again = K.kmeans_topk(X3.to(DEV), *packed, lens32, top_k=top_k, chunk=s["chunk"])
    assert all(torch.equal(a, b) for a, b in zip(again, (idx, dist, bad)))     # bitwise reproducible
    i2, v2 = idx.cpu().reshape(-1, top_k).long(), dist.cpu().reshape(-1, top_k).double()
    assert not i2[~valid].any() and not v2[~valid].any()                       # rows past the length get nothing
    assert bool(((i2 >= 0) & (i2 < s["Kc"])).all())
    assert bool((i2[valid].sort(1).values.diff(dim=1) > 0).all())             # top_k distinct centroids
    err_own = float((v2 - d64.gather(1, i2))[valid].abs().max())              # the distance of the centroid it names
    err_rank = float((v2 - srt[:, :top_k])[valid].abs().max())                 # and the j-th smallest distance
    print(f"kmeans_topk {name} top_k {top_k}: reference fp32 error {e32:.3e}, bound {bound:.3e}, kernel "
          f"{err_own:.3e} (own index) / {err_rank:.3e} (rank); rows exempt from the index check {exempt:.4f}")
    assert err_own <= bound and err_rank <= bound
    assert bool((v2[valid].diff(dim=1) >= 0).all())                            # ascending
    assert torch.equal(i2[sure], order[:, :top_k][sure])
    # the first index is kmeans_assign's code, bit for bit, whatever the chunking
    code = K.kmeans_assign(X3.to(DEV), *packed, lens32, chunk=s["chunk"])[0]
    assert torch.equal(idx[..., 0], code)
    if s["chunk"] is None:
        other = K.kmeans_topk(X3.to(DEV), *packed, lens32, top_k=top_k, chunk=256)
        assert all(torch.equal(a, b) for a, b in zip(other, (idx, dist, bad)))     # the chunking changes nothing


def test_kmeans_topk_ties_zero_distance_and_limits(K):
    g = _gen(3)
    Cm = (2.0 * torch.randn(100, 64, generator=g)).half().float()
    Cm[3] = torch.randint(-2, 3, (64,), generator=g).float()  # small integers: its norm and dot products are exact
    Cm[7] = Cm[3]                                             # exact duplicates: the lower index first
    Cm[70] = Cm[3]                                            # ... also across the chunk boundary
    X = torch.stack([Cm[3], Cm[99]]).half()
    packed = tuple(t.to(DEV) for t in K.kmeans_pack(Cm))
    idx, dist, bad = K.kmeans_topk(X[None].to(DEV), *packed, top_k=3)
    assert idx[0, 0].tolist() == [3, 7, 70] and idx[0, 1, 0].item() == 99
    assert dist[0, 0].tolist() == [0.0, 0.0, 0.0] and bad.tolist() == [1]      # three distances that sum to 0
    assert 0.0 <= float(dist[0, 1, 0]) < 0.05 < float(dist[0, 1, 1])          # a frame on a centroid: never NaN
    assert K.kmeans_topk(X[None, 1:].to(DEV), *packed, top_k=3)[2].tolist() == [0]
    Xb = torch.stack([X[1], X[1]])
    Xb[1, 5] = float("inf")
    assert K.kmeans_topk(Xb[None].to(DEV), *packed, torch.tensor([1], dtype=torch.int32, device=DEV),
                         top_k=2)[2].tolist() == [0]          # past the length
    assert K.kmeans_topk(Xb[None].to(DEV), *packed, top_k=2)[2].tolist() == [1]
    with pytest.raises(NotImplementedError, match="32"):
        K.kmeans_topk(X[None].to(DEV), *packed, top_k=33)
    with pytest.raises(ValueError):
        K.kmeans_topk(X[None].to(DEV), *packed, top_k=0)
    small = tuple(t.to(DEV) for t in K.kmeans_pack(Cm[:5]))
    with pytest.raises(ValueError, match="centroids"):
        K.kmeans_topk(X[None].to(DEV), *small, top_k=6)
    idx5 = K.kmeans_topk(X[None].to(DEV), *small, top_k=5)[0]                  # top_k = Kc: every centroid
    assert sorted(idx5[0, 0].tolist()) == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------ the model

_MODELS = {}


def _model(U):
    if "small" not in _MODELS:
        cfg = HR.CFGS["small"]
        _MODELS["small"] = U.HubertUnits(HR.make_state_dict(cfg, 0), cfg, HR.make_centroids("small").numpy(),
                                         HR.KM_LAYER["small"], {"do_normalize": False}, device=DEV)
    return _MODELS["small"]


def test_decode_end_to_end(U):
    m = _model(U)
    waves = [AR.to_float(AR.make_wave(n, ws)) for n, ws in HR.WAVES[:2]]
    outs = m.decode_many(waves, batch_size=2)
    units = m.units_many(waves, batch_size=2)
    for out, (code, merged) in zip(outs, units):
        T = len(code)
        assert out["code"] == code and out["merged_code"] == merged
        assert out["topk_code"].shape == out["topk_distance"].shape == (T, 10)
        assert out["topk_code"].dtype == np.int32 and out["topk_distance"].dtype == np.float32
        want = U.beam_decode_host(out["topk_code"], out["topk_distance"], 200)
        assert out["beam_code"] == want and out["beam_merged_code"] == U.merge(want)
        print(f"  decode {T} frames: greedy {len(merged)} merged units, beam {len(out['beam_merged_code'])}")
    one = m.decode(waves[1])
    solo = m.units(waves[1])
    assert one["code"] == solo[0] and one["beam_code"] == U.beam_decode_host(one["topk_code"], one["topk_distance"], 200)
    plain = m.decode(waves[1], beamsearch=False, top_k=3)
    assert "beam_code" not in plain and plain["code"] == solo[0] and plain["topk_code"].shape[1] == 3
    with pytest.raises(NotImplementedError, match="2048"):
        m.decode(waves[1], top_k=10, beamsize=300)


def test_decode_non_finite_guard(U):
    """A projection scaled far past fp16's range: the guard raises, no units come back."""
    sd = dict(HR.make_state_dict(HR.SMALL, 0))
    sd["feature_projection.projection.weight"] = sd["feature_projection.projection.weight"] * 3e4
    m = U.HubertUnits(sd, HR.SMALL, HR.make_centroids("small").numpy(), 2, device=DEV)
    for beamsearch in (True, False):
        with pytest.raises(U.NonFiniteFeatures, match="non-finite"):
            m.decode(AR.to_float(AR.make_wave(8000, 1)), beamsearch=beamsearch)


def test_quantize_cli_beamsearch(U, tmp_path):
    """--beamsearch --reduce writes the beam-merged units, --beamsearch the beam code; without the flag the
    file is what units_many gives, as before."""
    spec = importlib.util.spec_from_file_location("mms2ut_quantize_units", os.path.join(ROOT, "scripts", "mms2ut_quantize_units.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(HR.SMALL))
    AR.write_safetensors(str(mdir / "model.safetensors"), HR.make_state_dict(HR.SMALL, 0, prefix="hubert."))
    np.save(tmp_path / "km.npy", HR.make_centroids("small").numpy())
    root = tmp_path / "audio"
    root.mkdir()
    pcms = {"b": AR.make_wave(9000, 21), "a": AR.make_wave(400, 22), "c": AR.make_wave(16000, 23)}
    for nm, pcm in pcms.items():
        AR.write_wav(str(root / f"{nm}.wav"), pcm)
    (tmp_path / "m.tsv").write_text(f"{root}\n" + "".join(f"{nm}.wav\t{len(p)}\n" for nm, p in pcms.items()))
    m = _model(U)
    first, last = [AR.to_float(p) for p in list(pcms.values())[:2]], [AR.to_float(pcms["c"])]
    beams = m.decode_many(first, 2, True, 5, 40) + m.decode_many(last, 2, True, 5, 40)
    plain = m.units_many(first, 2) + m.units_many(last, 2)
    want = {("--beamsearch", "--reduce"): [r["beam_merged_code"] for r in beams],
            ("--beamsearch",): [r["beam_code"] for r in beams],
            (): [p[0] for p in plain], ("--reduce",): [p[1] for p in plain]}
    for flags, units in want.items():
        out = tmp_path / ("out" + "".join(flags) + ".km")
        assert cli.main(["--feature_type", "hubert", "--acoustic_model_path", str(mdir), "--kmeans_model_path",
                         str(tmp_path / "km.npy"), "--layer", "2", "--manifest_path", str(tmp_path / "m.tsv"),
                         "--out_quantized_file_path", str(out), "--batch-size", "2", "--device", DEV, "--top_k", "5",
                         "--beamsize", "40", *flags]) == 0
        assert out.read_text().splitlines() == [f"{nm}|" + " ".join(map(str, u)) for nm, u in zip(pcms, units)]
    assert any(r["beam_code"] != p[0] for r, p in zip(beams, plain))          # the two outputs are not one and the same

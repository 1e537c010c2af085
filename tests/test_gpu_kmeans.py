"""GPU: codebook training (csrc/kmeans.hip, multimodal-s2ut_amd/kmeans.py, scripts/mms2ut_learn_kmeans.py) against
the float64 restatement in tests/kmeans_ref.py and scikit-learn's recorded fits (tests/golden/kmeans_small.npz).
Nothing here needs scikit-learn.

The kernels one by one against float64 on the same fp16 rows; whole fits on the golden's inputs (n_steps_ equal to
scikit-learn's, centres within TOL_FACTOR (3) x the floor tests/test_kmeans.py measures: the fp32 variant's
distance from the float64 restatement; every check prints floor and ratio; a second fit bit-identical); and the
tool end to end on a tiny random HuBERT."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import asr_ref as AR
import hubert_ref as HR
import kmeans_ref as KR
from conftest import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(GOLDEN, "kmeans_small.npz"))
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def K():
    return pkg("kernels")


@pytest.fixture(scope="module")
def KM():
    return pkg("kmeans")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(R, d, Kc, seed):
    """fp16 rows that sit among fp32 centroids (tests/test_gpu_units.py's inputs)."""
    g = _gen(seed)
    Cm = torch.randn(Kc, d, generator=g)
    X = (Cm[torch.randint(0, Kc, (R,), generator=g)] + 0.5 * torch.randn(R, d, generator=g)).half()
    return X, Cm


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)


# ------------------------------------------------------------------------------------------ norms, gather

@pytest.mark.parametrize("N,d", [(1, 8), (1001, 72), (257, 768), (70, 1032)])
def test_row_norms_and_gather(K, N, d):
    """One wave per row, 512 columns a pass: d below one pass, off its grid, 1.5 and 2 + passes; the last block of
    four rows part empty.  A lane adds at most 8 * ceil(d / 512) exact products in fp32 before the sum goes on in
    double, and the result is rounded once: relative error <= (8 * ceil(d / 512) + 1) * 2^-24."""
    X = (3.0 * torch.randn(N, d, generator=_gen(N + d))).half()
    Xd = X.to(DEV)
    norms = K.kmeans_row_norms(Xd)
    want = X.double().pow(2).sum(1)
    rel = float(((norms.cpu().double() - want).abs() / want).max())
    bound = (8 * -(-d // 512) + 1) * EPS32
    print(f"row norms N{N} d{d}: relative error {rel:.2e}, bound {bound:.2e}")
    assert rel <= bound
    idx = torch.randint(0, N, (2 * N + 3,), generator=_gen(1))
    idx[0], idx[1], idx[2], idx[-1] = 0, N - 1, N - 1, 0          # repeats, both ends
    rows, nb = K.kmeans_gather(Xd, _i32(idx), norms)
    assert torch.equal(rows.cpu(), X[idx]) and torch.equal(nb, norms[idx.to(DEV)])
    wide = K.kmeans_gather(Xd, _i32(idx), wide=True)
    assert wide.dtype == torch.float32 and torch.equal(wide.cpu(), X[idx].float())
    assert torch.equal(K.kmeans_row_norms(Xd), norms)


# ------------------------------------------------------------------------------------------ fold, inertia

@pytest.mark.parametrize("R,d,Kc", [(1, 8, 1), (257, 64, 37), (1000, 768, 100), (300, 128, 1000), (2100, 72, 1000)])
def test_train_fold_codes_and_inertia(K, R, d, Kc):
    """Codes equal to kmeans_assign's on the same rows (one chunk and several; 2100 rows of 1000 centroids take
    the chunks of 256);
    best scores within TOL_FACTOR x the fp32 emulation's distance from float64; the inertia equal to the double
    sum of max(|x|^2 + best, 0) over the kernel's own values up to the order of a double sum, and within the
    scores' and norms' allowance of float64's."""
    X, Cm = _rows(R, d, Kc, R + d + Kc)
    Xd = X.to(DEV)
    packed = tuple(t.to(DEV) for t in K.kmeans_pack(Cm))
    norms = K.kmeans_row_norms(Xd)
    code, best, inertia, bad = K.kmeans_train_assign(Xd, norms, *packed)
    assert torch.equal(code, K.kmeans_assign(Xd[None], *packed)[0][0]) and int(bad) == 0
    S = HR.scores(X.float(), Cm)                                       # float64
    allow = HR.TOL_FACTOR * float((HR.kmeans_emulation(X, Cm).double() - S).abs().max())
    at = S[torch.arange(R), code.cpu().long()]
    err = float((best.cpu().double() - at).abs().max())
    own = float(torch.clamp(norms.cpu().double() + best.cpu().double(), min=0).sum())
    want = float(torch.clamp(X.double().pow(2).sum(1) + S.min(1).values, min=0).sum())
    slack = R * (allow + float(norms.max()) * (8 * -(-d // 512) + 1) * EPS32)
    print(f"train fold R{R} d{d} Kc{Kc}: score allowance {allow:.3e}, error {err:.3e}; inertia {float(inertia):.6f}, "
          f"from its own rows {own:.6f}, float64 {want:.6f} (slack {slack:.3e})")
    assert allow > 0 and err <= allow
    assert abs(float(inertia) - own) <= 1e-12 * own
    assert abs(float(inertia) - want) <= slack
    again = K.kmeans_train_assign(Xd, norms, *packed)
    assert all(torch.equal(a, b) for a, b in zip(again, (code, best, inertia, bad)))


def test_train_fold_flags_non_finite(K):
    X, Cm = _rows(300, 64, 30, 9)
    X[17, 3] = float("inf")
    packed = tuple(t.to(DEV) for t in K.kmeans_pack(Cm))
    Xd = X.to(DEV)
    assert int(K.kmeans_train_assign(Xd, K.kmeans_row_norms(Xd), *packed)[3]) == 1


# ------------------------------------------------------------------------------------------ accumulate

def _ordered_sums(X, code, Kc):
    """Per centroid the fp32 sum of its rows, added one by one in row order, and the counts."""
    Xf = X.float().numpy()
    sums, cnt = np.zeros((Kc, X.shape[1]), np.float32), np.zeros(Kc, np.int32)
    for c in range(Kc):
        rows = Xf[code == c]
        cnt[c] = len(rows)
        if len(rows):
            sums[c] = np.cumsum(rows, axis=0, dtype=np.float32)[-1]
    return sums, cnt


@pytest.mark.parametrize("d", [8, 64, 768])
@pytest.mark.parametrize("Kc", [1, 5, 37, 100])
@pytest.mark.parametrize("R", [1, 63, 65, 1000])
def test_accumulate(K, R, Kc, d):
    """Rows below, at and past a 64-row scan step and many steps; centroid counts off every grid; one, 1.5 and 3
    waves of columns.  Batches: all rows on one centroid; every centroid empty but two; fewer rows than centroids
    (where there are two centroids or more), each on its own centroid; random codes.  Sums and counts bit-identical
    across two runs and equal to the fp32 sum in row order."""
    g = _gen(R + Kc + d)
    X = (2.0 * torch.randn(R, d, generator=g)).half()
    few = min(R, max(Kc - 1, 1))
    batches = {"one centroid": (R, np.full(R, Kc // 2)),
               "all empty but two": (R, np.where(np.arange(R) % 3 == 0, 0, Kc - 1)),
               "fewer rows than centroids": (few, torch.randperm(Kc, generator=g)[:few].numpy()),
               "random": (R, torch.randint(0, Kc, (R,), generator=g).numpy())}
    for name, (r, code) in batches.items():
        Xb = X[:r].contiguous()
        want, wcnt = _ordered_sums(Xb, code, Kc)
        assert wcnt.sum() == r and (name != "one centroid" or wcnt.max() == r)
        sums, cnt = K.kmeans_accumulate(Xb.to(DEV), _i32(code), Kc)
        assert np.array_equal(cnt.cpu().numpy(), wcnt), name
        assert np.array_equal(sums.cpu().numpy().view(np.int32), want.view(np.int32)), name
        s2, c2 = K.kmeans_accumulate(Xb.to(DEV), _i32(code), Kc)
        assert torch.equal(s2.view(torch.int32), sums.view(torch.int32)) and torch.equal(c2, cnt), name


# ------------------------------------------------------------------------------------------ update and repack

@pytest.mark.parametrize("Kc,d", [(1, 8), (37, 72), (100, 768)])
def test_update_and_repack(K, Kc, d):
    """New centres equal to the float64 expression rounded once; counts exact past 2^24; a centroid without rows
    keeps its bits; the images bit-equal to kernels.kmeans_pack of the same fp32 centres; no host read needed: the
    flag stays 0.  Then the images alone, and the flag on a centre outside fp16's range."""
    g = _gen(Kc + d)
    C = torch.randn(Kc, d, generator=g)
    counts = torch.randint(0, 1 << 26, (Kc,), generator=g)
    cnt = torch.randint(0, 50, (Kc,), generator=g, dtype=torch.int32)
    cnt[::3] = 0
    counts[:1] = 0
    sums = 20.0 * torch.randn(Kc, d, generator=g)
    new = ((C.double() * counts.double()[:, None] + sums.double()) / (counts + cnt).double().clamp(min=1)[:, None]).float()
    want = torch.where(cnt[:, None] > 0, new, C)
    Cd, cd, bad = C.to(DEV), counts.to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    images = K.kmeans_images(Kc, d, DEV)
    K.kmeans_update(Cd, images, bad, cd, sums.to(DEV), cnt.to(DEV))
    assert torch.equal(Cd.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(cd.cpu(), counts + cnt) and int(bad) == 0
    for got, ref in zip(images, K.kmeans_pack(want)):
        assert got.dtype == ref.dtype and torch.equal(got.cpu().view(torch.int16 if ref.dtype == torch.float16 else torch.int32),
                                                      ref.view(torch.int16 if ref.dtype == torch.float16 else torch.int32))
    only = K.kmeans_images(Kc, d, DEV)
    K.kmeans_update(Cd, only, bad)
    assert all(torch.equal(a, b) for a, b in zip(only, images)) and torch.equal(Cd.cpu(), want) and int(bad) == 0
    Cd[Kc - 1, d - 1] = 1e5
    K.kmeans_update(Cd, only, bad)
    assert int(bad) == 1


# ------------------------------------------------------------------------------------------ k-means++

@pytest.mark.parametrize("name", [n for n in KR.CASES if KR.CASES[n]["init"] == "k-means++"])
def test_kmeanspp_rows(K, name):
    """The rows k-means++ takes on the device, per init of the golden's seeds, equal to the restatement's."""
    X, kw = KR.case_inputs(name)
    Xd = torch.from_numpy(X).to(DEV)
    for i, rec in enumerate(KR.reference(name)["inits"]):
        Xs = Xd if rec["sub"] is None else K.kmeans_gather(Xd, _i32(rec["sub"]))
        chosen = K.kmeans_pp(Xs, kw["n_clusters"], rec["first"], torch.from_numpy(rec["u"]).to(DEV))
        print(f"{name} init {i}: {chosen.tolist()}")
        assert chosen.tolist() == rec["chosen"].tolist()
        assert torch.equal(K.kmeans_pp(Xs, kw["n_clusters"], rec["first"], torch.from_numpy(rec["u"]).to(DEV)), chosen)


def test_kmeanspp_many_blocks_and_trials(K):
    """More rows than the pick kernel's 1024 threads and the distance kernel's 16-row blocks divide, 100 centres
    (6 trials), d of 1.5 passes: the rows equal the restatement's, which are distinct rows of distinct blobs."""
    X = KR.blobs(3001, 100, 72, 7)[0]
    first, u = KR.pp_draws(np.random.RandomState(11), len(X), 100)
    want = KR.plusplus(X, 100, first, u)
    assert np.array_equal(want, KR.plusplus(X, 100, first, u, np.float32)) and u.shape == (99, 6)
    got = K.kmeans_pp(torch.from_numpy(X).to(DEV), 100, first, torch.from_numpy(u).to(DEV))
    assert got.tolist() == want.tolist()


# ------------------------------------------------------------------------------------------ whole fits

def _fit(KM, name, **over):
    X, kw = KR.case_inputs(name)
    kw = dict(kw, **over)
    km = KM.UnitKMeans(kw.pop("n_clusters"), **kw)
    return km.fit(torch.from_numpy(X).to(DEV)), X


@pytest.mark.parametrize("name", list(KR.CASES))
def test_fit_matches_sklearn_and_restatement(KM, name):
    km, X = _fit(KM, name)
    r, fl = KR.reference(name), KR.floor(name)
    err = float(np.abs(km.cluster_centers_.astype(np.float64) - r["cluster_centers_"]).max())
    gerr = float(np.abs(km.cluster_centers_.astype(np.float64) - GOLD[f"{name}.cluster_centers_"]).max())
    ierr = abs(km.inertia_ - r["inertia_"]) / r["inertia_"]
    print(f"{name}: n_steps_ {km.n_steps_} (scikit-learn {int(GOLD[f'{name}.n_steps_'])}); centres floor {fl:.3e}, from "
          f"float64 {err:.3e} ({err / fl:.2f}x), from scikit-learn {gerr:.3e} ({gerr / fl:.2f}x); inertia_ relative "
          f"error {ierr:.3e}")
    assert km.n_steps_ == int(GOLD[f"{name}.n_steps_"]) == r["n_steps_"] and km.n_iter_ == r["n_iter_"]
    assert km.cluster_centers_.dtype == np.float32 and km.cluster_centers_.shape == r["cluster_centers_"].shape
    assert err <= KR.TOL_FACTOR * fl and gerr <= KR.TOL_FACTOR * fl
    assert ierr <= KR.TOL_FACTOR * 100 * EPS32                         # tests/test_kmeans.py's bound for inertia_
    if "chosen" in r["inits"][0]:
        assert int(np.argmin(km.init_inertias_)) == r["best_init"]
    again, _ = _fit(KM, name)
    assert np.array_equal(again.cluster_centers_.view(np.int32), km.cluster_centers_.view(np.int32))
    assert again.n_steps_ == km.n_steps_ and again.inertia_ == km.inertia_
    want = KR.sqdist(X, km.cluster_centers_).argmin(1)
    assert np.array_equal(km.predict(torch.from_numpy(X).to(DEV)), want)


def test_fit_does_not_depend_on_the_polling(KM, monkeypatch):
    """The stopping rule runs on the device: reading its state after every step or every 32 gives the same bits."""
    a, _ = _fit(KM, "pp_5")
    monkeypatch.setattr(KM, "POLL", 1)
    b, _ = _fit(KM, "pp_5")
    assert a.n_steps_ == b.n_steps_ == 20 and a.inertia_ == b.inertia_
    assert np.array_equal(a.cluster_centers_.view(np.int32), b.cluster_centers_.view(np.int32))


def test_fit_refuses_bad_input(KM):
    km = KM.UnitKMeans(4)
    with pytest.raises(ValueError, match="multiple of 8"):
        km.fit(torch.zeros(10, 12, dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="n_clusters"):
        km.fit(torch.zeros(3, 16, dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="fp16"):
        km.fit(torch.zeros(10, 16, device=DEV))
    X = torch.zeros(10, 16, dtype=torch.float16, device=DEV)
    X[3, 2] = float("inf")
    with pytest.raises(KM.NonFiniteCentres):
        km.fit(X)


# ------------------------------------------------------------------------------------------ end to end

def test_sample_features_samples_files_and_names_a_non_finite_one(KM, tmp_path):
    """sample_pct takes random.Random(seed).sample of the manifest's files, in the sampled order; a projection
    scaled far past fp16's range (tests/test_gpu_units.py's guard test) raises, naming the file."""
    import random
    U = pkg("units")
    root = tmp_path / "audio"
    root.mkdir()
    pcms = {nm: AR.make_wave(8000, 30 + i) for i, nm in enumerate("abcd")}
    for nm, pcm in pcms.items():
        AR.write_wav(str(root / f"{nm}.wav"), pcm)
    (tmp_path / "m.tsv").write_text(f"{root}\n" + "".join(f"{nm}.wav\t{len(p)}\n" for nm, p in pcms.items()))
    m = U.HubertUnits(HR.make_state_dict(HR.SMALL, 0), HR.SMALL, None, 2, device=DEV)
    picked = random.Random(5).sample([f"{nm}.wav" for nm in pcms], 2)
    feats = KM.sample_features(m, str(tmp_path / "m.tsv"), 0.5, seed=5, batch_size=2)
    want = m.features_batch([AR.to_float(pcms[f[0]]) for f in picked])[0]
    assert feats.shape == (48, 128) and torch.equal(feats, want.reshape(48, 128))
    assert KM.sample_features(m, str(tmp_path / "m.tsv"), 1.0).shape == (96, 128)
    sd = dict(HR.make_state_dict(HR.SMALL, 0))
    sd["feature_projection.projection.weight"] = sd["feature_projection.projection.weight"] * 3e4
    wild = U.HubertUnits(sd, HR.SMALL, None, 2, device=DEV)
    with pytest.raises(U.NonFiniteFeatures, match=r"a\.wav"):
        KM.sample_features(wild, str(tmp_path / "m.tsv"), 1.0)

def test_learn_kmeans_cli_end_to_end(KM, tmp_path):
    """The tool on an HF-layout directory of the small random HuBERT and three synthetic WAVs writes a .npy;
    HubertUnits.from_pretrained with that file quantises the same WAVs, and every frame's unit is the argmin
    against the saved centres on the model's own features."""
    U = pkg("units")
    spec = importlib.util.spec_from_file_location("mms2ut_learn_kmeans", os.path.join(ROOT, "scripts", "mms2ut_learn_kmeans.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    mdir = tmp_path / "model"
    mdir.mkdir()
    (mdir / "config.json").write_text(json.dumps(HR.SMALL))
    AR.write_safetensors(str(mdir / "model.safetensors"), HR.make_state_dict(HR.SMALL, 0, prefix="hubert."))
    root = tmp_path / "audio"
    root.mkdir()
    pcms = {"b": AR.make_wave(12345, 21), "a": AR.make_wave(8000, 22), "c": AR.make_wave(48000, 23)}
    for nm, pcm in pcms.items():
        AR.write_wav(str(root / f"{nm}.wav"), pcm)
    (tmp_path / "m.tsv").write_text(f"{root}\n" + "".join(f"{nm}.wav\t{len(p)}\n" for nm, p in pcms.items()))
    out, fpath = tmp_path / "km.npy", tmp_path / "feats.npy"
    assert cli.main(["--num_clusters", "8", "--feature_type", "hubert", "--acoustic_model_path", str(mdir), "--layer", "2",
                     "--manifest_path", str(tmp_path / "m.tsv"), "--out_kmeans_model_path", str(out), "--batch_size", "64",
                     "--max_iter", "5", "--n_init", "2", "--seed", "3", "--out_features_path", str(fpath),
                     "--device", DEV]) == 0
    cents, feats = np.load(out), np.load(fpath)
    assert cents.shape == (8, 128) and cents.dtype == np.float32 and feats.shape == (38 + 24 + 149, 128)
    m = U.HubertUnits.from_pretrained(str(mdir), str(out), 2, DEV)
    waves = [AR.to_float(p) for p in pcms.values()]
    Fb, lens, code = m.forward_batch(waves)[:3]                         # one batch, as the tool ran them
    got = np.concatenate([code[b, :T].cpu().numpy() for b, T in enumerate(lens)])
    own = torch.cat([Fb[b, :T] for b, T in enumerate(lens)]).cpu().numpy()
    assert np.array_equal(own, feats)                                  # the features the codebook was trained on
    assert m.units_many(waves, 3) == [(code[b, :T].tolist(), HR.merge(code[b, :T].tolist())) for b, T in enumerate(lens)]
    D = KR.sqdist(own, cents)
    top = np.sort(D, axis=1)
    print(f"learn-kmeans end to end: {len(got)} frames, units used {len(set(got.tolist()))}, least top-2 gap "
          f"{float((top[:, 1] - top[:, 0]).min()):.3e}")
    assert np.array_equal(got, D.argmin(1)) and len(set(got.tolist())) > 1
    feats_only = U.HubertUnits.from_pretrained(str(mdir), None, 2, DEV)
    assert torch.equal(feats_only.features(waves[0]), m.features(waves[0]))
    with pytest.raises(RuntimeError, match="without centroids"):
        feats_only.units(waves[0])
    again = tmp_path / "again.npy"
    assert cli.main(["--num_clusters", "8", "--feature_type", "hubert", "--features_path", str(fpath),
                     "--out_kmeans_model_path", str(again), "--batch_size", "64", "--max_iter", "5", "--n_init", "2",
                     "--seed", "3", "--device", DEV]) == 0
    assert np.array_equal(np.load(again), cents)

"""CPU: the codebook-training restatement (tests/kmeans_ref.py) against scikit-learn -- always against the golden
of scripts/gen_kmeans_golden.py, and against a live fit where scikit-learn is importable -- and the host side of
multimodal-s2ut_amd/kmeans.py and scripts/mms2ut_learn_kmeans.py.

Tolerances are measured (the convention of tests/test_gpu_units.py): centres may be at most TOL_FACTOR (3) x as
far from the float64 restatement as the restatement's fp32 variant is (scikit-learn's own arithmetic on fp32
input); every check prints its floor and ratio.  n_steps_ must be equal.  Two tests assert the properties of the
inputs that make those comparisons sound: the fp32 and float64 runs take the same k-means++ rows, and every
decision of the stopping rule in the early-stopping cases is taken by a margin the fp32 error cannot bridge."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest

import kmeans_ref as KR
from conftest import GOLDEN, ROOT, pkg

GOLD = np.load(os.path.join(GOLDEN, "kmeans_small.npz"))


ref, floor = KR.reference, KR.floor


def _cli():
    spec = importlib.util.spec_from_file_location("mms2ut_learn_kmeans", os.path.join(ROOT, "scripts", "mms2ut_learn_kmeans.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _compare(name, centers, n_steps, inertia, what):
    r = ref(name)
    fl = floor(name)
    err = float(np.abs(np.asarray(centers, np.float64) - r["cluster_centers_"]).max())
    ifl = abs(ref(name, True)["inertia_"] - r["inertia_"]) / r["inertia_"]
    ierr = abs(float(inertia) - r["inertia_"]) / r["inertia_"]
    print(f"{name} vs {what}: n_steps_ {r['n_steps_']} / {int(n_steps)}; centres floor {fl:.3e}, error {err:.3e} "
          f"({err / fl:.2f}x); inertia_ relative floor {ifl:.3e}, error {ierr:.3e}")
    assert r["n_steps_"] == int(n_steps)
    assert fl > 0 and err <= KR.TOL_FACTOR * fl
    # inertia_ is a sum of batch_size fp32 distances per step: scikit-learn adds them in an order that depends on
    # its threads, so the bound is fp32's: 2^-24 per distance at the blobs' scale |x|^2 / distance (about 100)
    assert ierr <= KR.TOL_FACTOR * 100 * 2.0 ** -24
    return err


@pytest.mark.parametrize("name", list(KR.CASES))
def test_restatement_matches_golden(name):
    X, kw = KR.case_inputs(name)
    args = json.loads(str(GOLD[f"{name}.args"]))
    assert np.array_equal(GOLD["X." + args["data"]], X)       # the golden was written for these inputs
    assert {k: v for k, v in args.items() if k != "data"} == {k: v for k, v in kw.items() if k != "init"}
    if f"{name}.init" in GOLD:
        assert np.array_equal(GOLD[f"{name}.init"], kw["init"])
    _compare(name, GOLD[f"{name}.cluster_centers_"], GOLD[f"{name}.n_steps_"], GOLD[f"{name}.inertia_"], "golden")


@pytest.mark.parametrize("name", list(KR.CASES))
def test_restatement_matches_live_sklearn(name):
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("gen_kmeans_golden", os.path.join(ROOT, "scripts", "gen_kmeans_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    X, kw = KR.case_inputs(name)
    km = gen.sklearn_fit(X, kw)
    _compare(name, km.cluster_centers_, km.n_steps_, km.inertia_, "scikit-learn")


def test_golden_covers_the_cases():
    r = {n: ref(n) for n in KR.CASES}
    bs, isz, n_steps = KR.sizes(200, 5, 100, 6)
    assert isz == 200 and r["pp_small"]["inits"][0]["sub"] is None          # n below init_size: no seeding subset
    assert all(i["sub"] is not None for i in r["pp_100"]["inits"] + r["explicit_100"]["inits"])
    assert r["pp_none"]["n_steps_"] == KR.sizes(3000, 12, 256, 4)[2] == 46  # never stopped
    for n in KR.EARLY:
        assert 2 < r[n]["n_steps_"] < 46                                     # the rule did stop these
    assert len({r[n]["best_init"] for n in KR.CASES if "pp" in n}) > 1       # not always the first init


def test_kmeanspp_rows_equal_in_fp32_and_float64():
    """For every seed used, the fp32 and the float64 restatement take identical k-means++ rows: the inputs do not
    put a seeding decision within rounding."""
    n = 0
    for name in KR.CASES:
        for a, b in zip(ref(name)["inits"], ref(name, True)["inits"]):
            if "chosen" in a:
                assert np.array_equal(a["chosen"], b["chosen"]) and len(set(a["chosen"].tolist())) == len(a["chosen"])
                n += 1
        assert ref(name)["best_init"] == ref(name, True)["best_init"]
    assert n >= 3 + 3 + 4 + 2


@pytest.mark.parametrize("name", KR.EARLY)
def test_early_stopping_decisions_have_margin(name):
    """Every ewa < ewa_min decision of the float64 run is taken by a relative margin larger than TOL_FACTOR x the
    fp32 variant's relative batch-inertia error, so n_steps_ cannot depend on the arithmetic's last bits."""
    r, r32 = ref(name), ref(name, True)
    assert len(r["batch_inertia"]) == len(r32["batch_inertia"])
    ierr = max(abs(a - b) / a for a, b in zip(r["batch_inertia"], r32["batch_inertia"]))
    margin = min(abs(e - m) / m for e, m in r["decisions"])
    print(f"{name}: {len(r['decisions'])} decisions, least relative margin {margin:.3e}, fp32 inertia error {ierr:.3e}")
    assert ierr > 0 and len(r["decisions"]) >= 5 and margin > KR.TOL_FACTOR * ierr


# ---------------------------------------------------------------------------------------------- host code

def _fitted(name="pp_small"):
    r = ref(name)
    _, kw = KR.case_inputs(name)
    return types.SimpleNamespace(cluster_centers_=r["cluster_centers_"].astype(np.float32), n_steps_=r["n_steps_"],
                                 n_iter_=r["n_iter_"], inertia_=r["inertia_"], counts_=np.ones(kw["n_clusters"], np.int64),
                                 init="k-means++", max_iter=kw["max_iter"], batch_size=kw["batch_size"],
                                 max_no_improvement=kw["max_no_improvement"], n_init=kw["n_init"], seed=kw["seed"])


def test_save_centroids_npy_round_trip(tmp_path):
    KM, U = pkg("kmeans"), pkg("units")
    km = _fitted()
    KM.save_centroids(str(tmp_path / "km.npy"), km)
    got = U.load_centroids(str(tmp_path / "km.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, km.cluster_centers_)


def test_save_centroids_pickle_round_trip_and_predict(tmp_path):
    joblib = pytest.importorskip("joblib")
    pytest.importorskip("sklearn")
    KM, U = pkg("kmeans"), pkg("units")
    km = _fitted()
    path = str(tmp_path / "km.bin")
    KM.save_centroids(path, km)
    assert np.array_equal(U.load_centroids(path), km.cluster_centers_)
    sk = joblib.load(path)
    X = KR.case_inputs("pp_small")[0].astype(np.float32)
    want = KR.sqdist(X, km.cluster_centers_).argmin(1)
    assert np.array_equal(sk.predict(X), want) and len(set(want.tolist())) == 5
    assert sk.n_steps_ == km.n_steps_ and sk.inertia_ == km.inertia_


def test_save_centroids_without_joblib(tmp_path, monkeypatch):
    import builtins
    KM = pkg("kmeans")
    real = builtins.__import__

    def fake(name, *a, **k):
        if name == "joblib":
            raise ImportError(name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", fake)
    with pytest.raises(ImportError, match=r"\.npy"):
        KM.save_centroids(str(tmp_path / "km.bin"), _fitted())


def test_unsupported_options_raise():
    KM = pkg("kmeans")
    with pytest.raises(NotImplementedError, match="reassignment_ratio"):
        KM.UnitKMeans(10, reassignment_ratio=0.01)
    with pytest.raises(NotImplementedError, match="tol"):
        KM.UnitKMeans(10, tol=1e-3)
    with pytest.raises(NotImplementedError, match="sample weights"):
        KM.UnitKMeans(10).fit(None, sample_weight=np.ones(3))
    with pytest.raises(NotImplementedError, match="init"):
        KM.UnitKMeans(10, init="random")
    with pytest.raises(ValueError, match="init of shape"):
        KM.UnitKMeans(10, init=np.zeros((9, 8)))
    with pytest.raises(NotImplementedError, match="reassignment_ratio"):
        KR.fit(np.zeros((4, 8)), 2, reassignment_ratio=0.5)


def test_cli_argument_errors(tmp_path, capsys):
    cli = _cli()
    base = ["--num_clusters", "10", "--out_kmeans_model_path", str(tmp_path / "km.npy")]
    model = ["--checkpoint_path", str(tmp_path), "--layer", "2", "--manifest_path", str(tmp_path / "m.tsv")]
    for argv, msg in [
            (base + ["--feature_type", "mfcc"] + model, "only 'hubert'"),
            (base + ["--feature_type", "hubert"], "--checkpoint_path, --layer and --manifest_path are required"),
            (base + ["--feature_type", "hubert", "--acoustic_model_path", str(tmp_path / "m.pt"), "--layer", "2",
                     "--manifest_path", "x"], "not a directory"),
            (base + ["--feature_type", "hubert", "--reassignment_ratio", "0.01"] + model, "--reassignment_ratio must be 0"),
            (base + ["--feature_type", "hubert", "--tol", "0.1"] + model, "--tol must be 0"),
            (base + ["--feature_type", "hubert", "--sample_pct", "0"] + model, "--sample_pct"),
            (base + ["--feature_type", "hubert", "--init", "random"] + model, "--init"),
            (["--num_clusters", "0", "--out_kmeans_model_path", "x", "--feature_type", "hubert"] + model, "--num_clusters")]:
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err

"""Writes tests/golden/kmeans_small.npz: scikit-learn MiniBatchKMeans fits (fairseq cluster_kmeans.py's settings:
tol 0, reassignment_ratio 0, compute_labels False) on the small fixed inputs of tests/kmeans_ref.py, for the
tests that pin the restatement and the device path without scikit-learn at run time.

    python scripts/gen_kmeans_golden.py

Per data set X.<name> (fp16, fed to scikit-learn as fp32); per case of kmeans_ref.CASES the explicit centres if
any, the arguments as JSON (with the data set's name), and cluster_centers_, n_steps_, inertia_.  Needs scikit-learn (written with the version the file records)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kmeans_ref as KR     # noqa: E402


def sklearn_fit(X, kw):
    from sklearn.cluster import MiniBatchKMeans
    kw = dict(kw)
    km = MiniBatchKMeans(n_clusters=kw.pop("n_clusters"), init=kw.pop("init"), random_state=kw.pop("seed"), tol=0.0,
                         reassignment_ratio=0.0, compute_labels=False, verbose=0, **kw)
    return km.fit(np.asarray(X, np.float32))


def main():
    import sklearn
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in KR.CASES:
        X, kw = KR.case_inputs(name)
        km = sklearn_fit(X, kw)
        out["X." + KR.CASES[name]["data"]] = X
        if not isinstance(kw["init"], str):
            out[f"{name}.init"] = kw["init"]
        out[f"{name}.args"] = np.array(json.dumps(dict({k: v for k, v in kw.items() if k != "init"}, data=KR.CASES[name]["data"])))
        out[f"{name}.cluster_centers_"] = km.cluster_centers_.astype(np.float32)
        out[f"{name}.n_steps_"] = np.array(km.n_steps_)
        out[f"{name}.inertia_"] = np.array(km.inertia_, np.float64)
        print(f"{name}: n_steps_ {km.n_steps_}, inertia_ {km.inertia_:.6f}")
    path = os.path.join(ROOT, "tests", "golden", "kmeans_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

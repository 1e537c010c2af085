"""Unit codebook training: the k-means model whose centroids units.py quantises HuBERT features with, fitted on
the device -- fairseq's examples/textless_nlp/gslm/speech2unit/clustering/cluster_kmeans.py, the step before
the reference pipeline's scripts/preprocess/3_cluster.sh.  The semantics are scikit-learn's
MiniBatchKMeans.fit as that script configures it (init k-means++, max_iter 150, batch_size 10000, tol 0,
max_no_improvement 100, n_init 20, reassignment_ratio 0, compute_labels False).

All randomness comes from one numpy.random.RandomState(seed) on the host, with fit's calls in fit's order:
randint(0, n, init_size) for the validation set; per init randint(0, n, init_size) when init_size < n,
choice(n_sub, p=uniform) for the first centre, one uniform(size=2 + int(log K)) per further centre; per step
randint(0, n, batch_size).  None of the draws depends on the data, so the host draws ahead and the device
never waits for it.  Everything else runs on csrc/kmeans.hip and units.hip's kmeans_assign: k-means++ and the
validation inertias of all inits without a host read (one read then picks the best init), and the mini-batch
steps with scikit-learn's EWA-inertia stopping rule kept on the device: once it is met the remaining queued
steps do nothing, and the host looks at the state once per POLL steps.  The result does not depend on POLL.

The data are fp16 rows; centres and sums are fp32, counts int64, inertias double.  No float atomics: two fits
with one seed give the same bits."""
import os
import random
import time

import numpy as np
import torch

from . import kernels as K
from . import units as U
from .encoders import wave_batches

POLL = 32           # mini-batch steps queued between two reads of the device state
ST_STEPS, ST_EWA, ST_EWA_MIN, ST_NO_IMPROVEMENT, ST_DONE = range(5)     # csrc/kmeans.hip's state


class NonFiniteCentres(RuntimeError):
    """A centre or a row's best score left fp16's range or is not finite: no codebook is returned."""


def _dev_idx(idx, device):
    return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(device)


class UnitKMeans:
    """scikit-learn's MiniBatchKMeans (the subset fairseq's cluster_kmeans.py uses) on HIP kernels.

    fit(X) takes fp16 [N, d] on the device, d a multiple of 8, and sets cluster_centers_ (fp32 numpy [K, d]),
    n_steps_, n_iter_, inertia_ (the EWA inertia times N: compute_labels is off) and ewa_inertia_."""

    def __init__(self, n_clusters, init="k-means++", max_iter=150, batch_size=10000, tol=0.0, max_no_improvement=100,
                 n_init=20, reassignment_ratio=0.0, seed=0):
        if reassignment_ratio != 0:
            raise NotImplementedError("reassignment_ratio must be 0 (fairseq's setting): random reassignment of "
                                      "low-count centres is not implemented")
        if tol != 0:
            raise NotImplementedError("tol must be 0 (fairseq's setting): stopping on the centres' movement is not implemented")
        if isinstance(init, str):
            if init != "k-means++":
                raise NotImplementedError(f"init '{init}': only 'k-means++' or an array of centres")
        else:
            init = np.ascontiguousarray(init, dtype=np.float32)
            if init.ndim != 2 or init.shape[0] != n_clusters:
                raise ValueError(f"init of shape {init.shape} for {n_clusters} clusters")
        if n_clusters < 1 or max_iter < 1 or batch_size < 1 or n_init < 1:
            raise ValueError("n_clusters, max_iter, batch_size and n_init must be >= 1")
        if max_no_improvement is not None and max_no_improvement < 0:
            raise ValueError("max_no_improvement must be >= 0 or None")
        if 2 + int(np.log(n_clusters)) > K.KMEANS_PP_MAX_TRIALS:
            raise NotImplementedError(f"{n_clusters} clusters need more than {K.KMEANS_PP_MAX_TRIALS} k-means++ trials")
        self.n_clusters, self.init, self.max_iter, self.batch_size = int(n_clusters), init, int(max_iter), int(batch_size)
        self.max_no_improvement, self.n_init, self.seed = max_no_improvement, int(n_init), seed

    # ------------------------------------------------------------------------------------------ fit

    def _check(self, X):
        if not (torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float16 and X.dim() == 2 and X.is_contiguous()):
            raise ValueError("fp16 [N, d] contiguous rows on the device expected")
        n, d = X.shape
        if d % 8 or d < 8:
            raise ValueError(f"the feature width {d} must be a multiple of 8 (kmeans_assign)")
        if n < self.n_clusters:
            raise ValueError(f"n_samples={n} should be >= n_clusters={self.n_clusters}")
        if n >= 2 ** 31:
            raise ValueError(f"{n} rows exceed the int32 row indices of the kernels")
        return n, d

    def _init_centres(self, X, norms, rs, init_size):
        """-> fp32 [K, d] on the device: the init whose inertia on the validation rows is lowest."""
        n, d = X.shape
        Kc, dev = self.n_clusters, X.device
        Xv, nv = K.kmeans_gather(X, _dev_idx(rs.randint(0, n, init_size), dev), norms)
        explicit = not isinstance(self.init, str)
        cands, inertias = [], []
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        for _ in range(1 if explicit else self.n_init):
            sub = rs.randint(0, n, init_size) if init_size < n else None      # drawn for explicit centres too, as fit does
            if explicit:
                if self.init.shape[1] != d:
                    raise ValueError(f"init of width {self.init.shape[1]} for features of width {d}")
                C = torch.from_numpy(self.init).to(dev)
            else:
                Xs = X if sub is None else K.kmeans_gather(X, _dev_idx(sub, dev))
                w = np.ones(Xs.shape[0], np.float32)
                first = int(rs.choice(Xs.shape[0], p=w / w.sum()))
                T = 2 + int(np.log(Kc))
                u = np.stack([rs.uniform(size=T) for _ in range(Kc - 1)]) if Kc > 1 else np.zeros((0, T))
                chosen = K.kmeans_pp(Xs, Kc, first, torch.from_numpy(u).to(dev))
                C = K.kmeans_gather(Xs, chosen, wide=True)
            images = K.kmeans_images(Kc, d, dev)
            K.kmeans_update(C, images, bad)
            inertia, b = K.kmeans_train_assign(Xv, nv, *images)[2:]
            bad |= b
            cands.append(C)
            inertias.append(inertia)
        inertias = torch.cat(inertias).cpu().numpy()          # the one read of the initialisation
        if int(bad) or not np.isfinite(inertias).all():
            raise NonFiniteCentres("non-finite features or initial centres")
        self.init_inertias_ = inertias
        return cands[int(np.argmin(inertias))]                # the first of equal ones, as fit's strict <

    def fit(self, X, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("sample weights are not implemented")
        n, d = self._check(X)
        Kc = self.n_clusters
        rs = np.random.RandomState(self.seed)
        bs = min(self.batch_size, n)
        init_size = 3 * bs
        if init_size < Kc:
            init_size = 3 * Kc
        init_size = min(init_size, n)
        n_steps = self.max_iter * n // bs
        norms = K.kmeans_row_norms(X)
        C = self._init_centres(X, norms, rs, init_size).clone()
        step = K.KMeansStep(X, norms, C, bs, min(bs * 2.0 / (n + 1), 1.0), self.max_no_improvement)
        done = 0
        while done < n_steps:
            m = min(POLL, n_steps - done)
            idx = _dev_idx(np.stack([rs.randint(0, n, bs) for _ in range(m)]), X.device)
            for j in range(m):
                step(idx[j])
            done += m
            if self.max_no_improvement is not None and float(step.state[ST_DONE]) != 0.0:
                break
        state = step.state.cpu().numpy()                      # also the end of the queue
        if int(step.bad):
            raise NonFiniteCentres("a centre or a row's best score is not finite or left fp16's range")
        self.cluster_centers_ = C.cpu().numpy()
        self.counts_ = step.counts.cpu().numpy()
        self.n_steps_ = int(state[ST_STEPS])
        self.n_iter_ = int(np.ceil(self.n_steps_ * bs / n))
        self.ewa_inertia_ = float(state[ST_EWA]) if self.n_steps_ > 1 else float("nan")
        self.inertia_ = self.ewa_inertia_ * n
        self._images = step.images
        return self

    def predict(self, X):
        """int64 numpy [N]: the nearest fitted centre of fp16 rows X [N, d] on the device (kmeans_assign)."""
        n, d = self._check_predict(X)
        if not hasattr(self, "_images"):
            self._images = K.kmeans_pack(torch.from_numpy(self.cluster_centers_).to(X.device))
        code, _, _, bad = K.kmeans_assign(X, *self._images)
        if int(bad[0]):
            raise U.NonFiniteFeatures("predict: non-finite features")
        return code[0].cpu().numpy().astype(np.int64)

    def _check_predict(self, X):
        if not hasattr(self, "cluster_centers_"):
            raise RuntimeError("predict before fit")
        if not (torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float16 and X.dim() == 2 and X.is_contiguous()
                and X.shape[1] == self.cluster_centers_.shape[1]):
            raise ValueError(f"fp16 [N, {self.cluster_centers_.shape[1]}] contiguous rows on the device expected")
        return X.shape


# ---------------------------------------------------------------------------------------------- features

def sample_features(model, manifest_path, sample_pct=1.0, seed=0, extension=".wav", batch_size=8):
    """fp16 [frames, d] on the device: the valid frames of HubertUnits.features_batch over a sampled share of
    the manifest's files (random.Random(seed).sample of ceil(sample_pct * files), in the sampled order; files
    not ending in `extension` are left out first).  Non-finite features raise units.NonFiniteFeatures naming
    the file."""
    if not 0.0 < sample_pct <= 1.0:
        raise ValueError(f"sample_pct must be in (0, 1], got {sample_pct}")
    root, files = U.read_manifest(manifest_path)
    if extension:
        files = [f for f in files if f.endswith(extension)]
    if not files:
        raise ValueError(f"{manifest_path}: no files ending in '{extension}'")
    if sample_pct < 1.0:
        files = random.Random(seed).sample(files, int(np.ceil(sample_pct * len(files))))
    out = []
    for names, waves in wave_batches(root, files, batch_size, model.sampling_rate, model.min_samples):
        Fb, lens, _ = model.features_batch(waves)
        bad = K.nonfinite_rows(Fb).tolist() if Fb.shape[1] * Fb.shape[2] % 8 == 0 else None
        for b, (f, T) in enumerate(zip(names, lens)):
            rows = Fb[b, :T]
            # the rows past an utterance's length mean nothing: a flagged batch row is looked at again without them
            if (bad is None or bad[b]) and not bool(torch.isfinite(rows).all()):
                raise U.NonFiniteFeatures(f"{os.path.join(root, f)} ({T} frames): non-finite features (the fp16 "
                                          "activations overflowed); no codebook is trained")
            out.append(rows)
    return torch.cat(out).contiguous()


# ---------------------------------------------------------------------------------------------- files

def save_centroids(path, km):
    """The fitted codebook.  *.npy: cluster_centers_ (fp32 [K, d]).  Any other suffix: a joblib pickle of a
    scikit-learn MiniBatchKMeans that carries the fitted attributes, so that joblib.load(path).predict works
    and units.load_centroids (and fairseq's quantize_with_kmeans.py) read it."""
    C = np.ascontiguousarray(km.cluster_centers_, dtype=np.float32)
    if path.endswith(".npy"):
        np.save(path, C)
        return
    try:
        import joblib
        from sklearn.cluster import MiniBatchKMeans
    except ImportError:
        raise ImportError(f"{path}: a joblib-pickled scikit-learn model needs the 'joblib' and 'scikit-learn' packages; "
                          "name the file *.npy to save the centroids alone") from None
    sk = MiniBatchKMeans(n_clusters=C.shape[0], init="k-means++" if isinstance(km.init, str) else km.init,
                         max_iter=km.max_iter, batch_size=km.batch_size, tol=0.0, max_no_improvement=km.max_no_improvement,
                         n_init=km.n_init, reassignment_ratio=0.0, compute_labels=False,
                         random_state=km.seed if isinstance(km.seed, (int, np.integer)) else None)
    sk.cluster_centers_ = C
    sk._n_features_out = C.shape[0]
    sk.n_features_in_ = C.shape[1]
    sk._n_threads = 1
    sk.n_steps_, sk.n_iter_, sk.inertia_ = km.n_steps_, km.n_iter_, km.inertia_
    sk._counts = np.asarray(km.counts_, dtype=np.float32)
    joblib.dump(sk, path)


def learn_kmeans(feats, n_clusters, **kw):
    """UnitKMeans(n_clusters, **kw).fit(feats) -> (the model, wall seconds of the fit, queue drained)."""
    km = UnitKMeans(n_clusters, **kw)
    torch.cuda.synchronize(feats.device)
    t0 = time.perf_counter()
    km.fit(feats)
    torch.cuda.synchronize(feats.device)
    return km, time.perf_counter() - t0

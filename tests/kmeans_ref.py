"""Numpy restatement of scikit-learn's MiniBatchKMeans.fit as fairseq's cluster_kmeans.py configures it
(tol 0, reassignment_ratio 0, compute_labels False, no sample weights), for the codebook-training tests.
Nothing here imports the product package or scikit-learn; tests/test_kmeans.py pins it against the library by
the golden of scripts/gen_kmeans_golden.py (tests/golden/kmeans_small.npz) and, where scikit-learn is
importable, against a live fit.

All randomness comes from one numpy.random.RandomState(seed) with fit's calls in fit's order:
randint(0, n, init_size) for the validation set; per init randint(0, n, init_size) when init_size < n (also
with explicit centres, which then ignore it), choice(n_sub, p=uniform) for the first centre and one
uniform(size=2 + int(log K)) per further centre; per step randint(0, n, batch_size).

dtype float64 is the reference.  dtype float32 does what scikit-learn does in fp32 on fp32 input: distances
|x|^2 - 2 x . c + |c|^2 in fp32, centres and counts in fp32, and the update as its Cython loop orders it
(centre * count, the rows added one by one, times 1 / new count); sums that scikit-learn keeps in double
(the cumulative sum of k-means++) stay double.  Its distance from the float64 run is the floor an allowance
is TOL_FACTOR times."""
import functools
import math

import numpy as np

TOL_FACTOR = 3


def sqdist(A, B, dtype=np.float64):
    """[len(A), len(B)] squared distances |a|^2 - 2 a . b + |b|^2 in dtype, clamped at 0."""
    A, B = np.asarray(A, dtype), np.asarray(B, dtype)
    D = (A * A).sum(1, dtype=dtype)[:, None] - dtype(2) * (A @ B.T) + (B * B).sum(1, dtype=dtype)[None]
    return np.maximum(D, dtype(0))


def sizes(n, K, batch_size, max_iter):
    """(batch, init_size, n_steps) of a fit."""
    bs = min(batch_size, n)
    isz = 3 * bs
    if isz < K:
        isz = 3 * K
    return bs, min(isz, n), max_iter * n // bs


def trials(K):
    return 2 + int(math.log(K))


def pp_draws(rs, n_sub, K):
    """The draws of _kmeans_plusplus, which do not depend on the data: (first row, uniforms [K - 1, trials])."""
    w = np.ones(n_sub, np.float32)
    first = int(rs.choice(n_sub, p=w / w.sum()))
    u = np.stack([rs.uniform(size=trials(K)) for _ in range(K - 1)]) if K > 1 else np.zeros((0, trials(K)))
    return first, u


def plusplus(Xs, K, first, u, dtype=np.float64):
    """Rows of Xs that k-means++ takes, given its draws."""
    Xs = np.asarray(Xs, dtype)
    n = Xs.shape[0]
    chosen = [first]
    closest = sqdist(Xs[[first]], Xs, dtype)[0]
    pot = closest.sum(dtype=dtype)
    for c in range(1, K):
        cand = np.searchsorted(np.cumsum(closest, dtype=np.float64), u[c - 1] * pot)
        np.clip(cand, None, n - 1, out=cand)
        D = np.minimum(closest[None], sqdist(Xs[cand], Xs, dtype))
        pots = D.sum(1, dtype=dtype)
        b = int(np.argmin(pots))                              # the lowest trial on a tie
        pot, closest = pots[b], D[b]
        chosen.append(int(cand[b]))
    return np.array(chosen)


def labels_inertia(Xb, C, dtype=np.float64):
    """(argmin, the lowest index on ties; the sum of the rows' distances, in double)."""
    D = sqdist(Xb, C, dtype)
    lab = D.argmin(1)
    return lab, float(D[np.arange(len(lab)), lab].sum(dtype=np.float64))


def update(C, counts, Xb, lab, dtype=np.float64):
    """One mini-batch update, in place: a centre that received m rows becomes (old * count + sum x) / (count + m)."""
    for c in np.unique(lab):
        rows = Xb[lab == c]
        m = len(rows)
        if dtype == np.float64:
            C[c] = (C[c] * counts[c] + rows.sum(0)) / (counts[c] + m)
        else:                                                 # fp32, in the order of scikit-learn's loop
            acc = np.cumsum(np.vstack([(C[c] * counts[c])[None], rows]), axis=0, dtype=dtype)[-1]
            C[c] = acc * (dtype(1) / (counts[c] + dtype(m)))
        counts[c] += m


def fit(X, n_clusters, init="k-means++", max_iter=150, batch_size=10000, max_no_improvement=100, n_init=20, seed=0,
        dtype=np.float64, reassignment_ratio=0.0, tol=0.0):
    """-> dict: cluster_centers_, n_steps_, n_iter_, inertia_, and what the tests look into: inits (per init its
    subset rows or None, first, u, chosen, validation inertia), best_init, decisions (per comparison of the
    stopping rule: (ewa, the minimum it was compared with)), batch_inertia (per step)."""
    if reassignment_ratio != 0 or tol != 0:
        raise NotImplementedError("reassignment_ratio and tol must be 0")
    X = np.asarray(X, dtype)
    n, d = X.shape
    K = n_clusters
    rs = np.random.RandomState(seed)
    bs, isz, n_steps = sizes(n, K, batch_size, max_iter)
    explicit = not isinstance(init, str)
    valid = rs.randint(0, n, isz)
    inits = []
    for _ in range(1 if explicit else n_init):
        sub = rs.randint(0, n, isz) if isz < n else None
        if explicit:
            rec = dict(sub=sub, centers=np.array(init, dtype))
        else:
            Xs = X if sub is None else X[sub]
            first, u = pp_draws(rs, Xs.shape[0], K)
            chosen = plusplus(Xs, K, first, u, dtype)
            rec = dict(sub=sub, first=first, u=u, chosen=chosen, centers=Xs[chosen].copy())
        rec["inertia"] = labels_inertia(X[valid], rec["centers"], dtype)[1]
        inits.append(rec)
    best = int(np.argmin([r["inertia"] for r in inits]))      # the first of equal ones, as fit's strict <
    C = inits[best]["centers"].copy()
    counts = np.zeros(K, dtype)
    alpha = min(bs * 2.0 / (n + 1), 1)
    ewa = ewa_min = None
    no_improvement = 0
    decisions, batch_inertia = [], []
    for i in range(n_steps):
        Xb = X[rs.randint(0, n, bs)]
        lab, inertia = labels_inertia(Xb, C, dtype)
        update(C, counts, Xb, lab, dtype)
        batch_inertia.append(inertia)
        if i == 0:
            continue
        b = inertia / bs
        ewa = b if ewa is None else ewa * (1 - alpha) + b * alpha
        if ewa_min is not None:
            decisions.append((ewa, ewa_min))
        if ewa_min is None or ewa < ewa_min:
            no_improvement, ewa_min = 0, ewa
        else:
            no_improvement += 1
        if max_no_improvement is not None and no_improvement >= max_no_improvement:
            break
    return dict(cluster_centers_=C, n_steps_=i + 1, n_iter_=int(np.ceil((i + 1) * bs / n)), inertia_=ewa * n, inits=inits,
                best_init=best, decisions=decisions, batch_inertia=batch_inertia, valid=valid)


def blobs(n, K, d, seed, scale=15.0, noise=1.0):
    """fp16 rows around K well-separated centres (uniform in [-scale, scale]^d), and the fp32 centres."""
    g = np.random.RandomState(seed)
    cen = g.uniform(-scale, scale, size=(K, d)).astype(np.float32)
    X = cen[g.randint(0, K, n)] + noise * g.standard_normal((n, d)).astype(np.float32)
    return X.astype(np.float16), cen


# the golden's cases (scripts/gen_kmeans_golden.py): data set, then MiniBatchKMeans' arguments
DATA = {"a": dict(n=3000, K=12, d=16, seed=0), "b": dict(n=200, K=5, d=16, seed=1)}
_A = dict(data="a", n_clusters=12, batch_size=256, max_iter=4)
CASES = {
    "explicit_100": dict(_A, init="rows", n_init=1, max_no_improvement=100, seed=3),
    "explicit_5": dict(_A, init="rows", n_init=1, max_no_improvement=5, seed=3),
    "pp_100": dict(_A, init="k-means++", n_init=3, max_no_improvement=100, seed=4),
    "pp_5": dict(_A, init="k-means++", n_init=3, max_no_improvement=5, seed=4),
    "pp_small": dict(data="b", n_clusters=5, batch_size=100, max_iter=6, init="k-means++", n_init=4,
                     max_no_improvement=100, seed=5),          # n 200 below init_size 300: no seeding subset
    "pp_none": dict(_A, init="k-means++", n_init=2, max_no_improvement=None, seed=6),
}
EARLY = ("explicit_5", "pp_5")


def case_inputs(name):
    """(X fp16, keyword arguments of fit) of a golden case; explicit centres are rows of X drawn with the
    case's seed."""
    c = dict(CASES[name])
    X = blobs(**DATA[c.pop("data")])[0]
    if c["init"] == "rows":
        rows = np.random.RandomState(100 + c["seed"]).choice(len(X), c["n_clusters"], replace=False)
        c["init"] = X[rows].astype(np.float32)
    return X, c


@functools.lru_cache(maxsize=None)
def reference(name, fp32=False):
    """fit's result for a golden case, computed once per process; treat it as read-only."""
    X, kw = case_inputs(name)
    return fit(X, dtype=np.float32 if fp32 else np.float64, **kw)


def floor(name):
    """The fp32 variant's distance from the float64 restatement (max-abs over the centres)."""
    return float(np.abs(reference(name, True)["cluster_centers_"].astype(np.float64) - reference(name)["cluster_centers_"]).max())

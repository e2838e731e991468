"""float64 numpy reference for the k-means tests (never imported by ``sapr_amd``) and the shared test recipe.

Recipe: group g is the frames of word g of ``synth_feature_set(VOCAB, 6, D, seed=21, tmin=1, tmax=110)`` concatenated
(182-484 frames: one or two tiles with a partial last tile; the duplicated "silence" frames are wanted); restart r of
group g starts from the rows ``default_rng(1000 * g + r).choice(n_g, K, replace=False)``, r = 0..2.

Lloyd follows scikit-learn's rules (threshold ``tol * mean(var(X, axis=0))``, new centre = mean of the cluster, stop when
the summed squared centre shift is <= threshold, inertia from one more assignment at the final centres) with ONE
deviation: an empty cluster keeps its previous centre.  Like scikit-learn, :func:`lloyd` works on the data minus its column
mean and adds the mean back to the centres (c0 sits near -300: coordinates near zero would otherwise carry the rounding
of sums near -300 n, which an element-wise comparison against scikit-learn at rtol 1e-12 sees).

:func:`seed_centres` and :func:`kmeans_seeded` restate the seeding of ``kmeans(init=None, seeds=...)`` for one rank from
its documented rules (kmeans.py's docstring): ``default_rng(seed)``, a sorted uniform subsample of
``min(n, 256 K)`` rows shared by the restarts, plain k-means++ on it.
"""
from __future__ import annotations

import functools

import numpy as np

from tests._synth import VOCAB, synth_feature_set

SHAPES = [(13, 10), (39, 18), (26, 5), (5, 1), (13, 3)]   # (D, K)
R = 3


@functools.lru_cache(maxsize=None)
def recipe_groups(D):
    """tuple of float32 [n_g, D] arrays, one per word."""
    by_word, _ = synth_feature_set(VOCAB, 6, D, seed=21, tmin=1, tmax=110)
    out = tuple(np.ascontiguousarray(np.concatenate([f.T for f in by_word[w]], axis=0)) for w in VOCAB)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def recipe_lengths(D):
    """tuple over the words of the utterance lengths behind :func:`recipe_groups` (hmmlearn's ``lengths``)."""
    by_word, _ = synth_feature_set(VOCAB, 6, D, seed=21, tmin=1, tmax=110)
    return tuple(tuple(f.shape[1] for f in by_word[w]) for w in VOCAB)


@functools.lru_cache(maxsize=None)
def recipe_init(D, K):
    """start centres [G, R, K, D] float64."""
    groups = recipe_groups(D)
    out = np.empty((len(groups), R, K, D))
    for g, X in enumerate(groups):
        for r in range(R):
            out[g, r] = X[np.random.default_rng(1000 * g + r).choice(X.shape[0], K, replace=False)]
    out.setflags(write=False)
    return out


def distances(X, c):
    """[n, K] float64: sum_d (x_d - c_kd)^2, the difference squared directly."""
    X = np.asarray(X, dtype=np.float64)
    return ((X[:, None, :] - np.asarray(c, dtype=np.float64)[None, :, :]) ** 2).sum(axis=2)


def step(X, c):
    """One Lloyd step -> (labels[n], stats[K, 2D+1] = {count, sum_x[D], sqdev[D]}, dist[n, K])."""
    X = np.asarray(X, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    K, D = c.shape
    dist = distances(X, c)
    labels = np.argmin(dist, axis=1) if X.shape[0] else np.zeros(0, np.int64)
    stats = np.zeros((K, 2 * D + 1))
    for k in range(K):
        Xk = X[labels == k]
        stats[k, 0] = Xk.shape[0]
        if Xk.shape[0]:
            stats[k, 1:1 + D] = Xk.sum(axis=0)
            stats[k, 1 + D:] = ((Xk - c[k]) ** 2).sum(axis=0)
    return labels, stats, dist


def relative_gaps(dist):
    """Per frame (d2 - d1) / d2 of its two nearest distances (0 where d2 == 0); [] for K == 1."""
    if dist.shape[1] < 2 or dist.shape[0] == 0:
        return np.zeros(0)
    two = np.partition(dist, 1, axis=1)[:, :2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)


def zero_gaps_come_from_identical_centres(dist, c):
    """Every frame whose two nearest distances are EQUAL must owe that to bit-identical centre rows."""
    if dist.shape[1] < 2:
        return True
    order = np.argsort(dist, axis=1, kind="stable")[:, :2]
    n = np.arange(dist.shape[0])
    tie = dist[n, order[:, 0]] == dist[n, order[:, 1]]
    return all(np.array_equal(c[a], c[b]) for a, b in order[tie])


def lloyd(X, c0, tol=1e-4, max_iter=300):
    """-> dict(centers, inertia, n_iter, emptied (a cluster was empty in some step), min_gap (smallest non-zero
    relative gap over all steps), shifts (every summed squared centre shift), threshold)."""
    X = np.asarray(X, dtype=np.float64)
    thr = tol * np.mean(np.var(X, axis=0))
    mu = X.mean(axis=0)
    X = X - mu
    c = np.array(c0, dtype=np.float64) - mu
    emptied, min_gap, shifts, n_iter = False, np.inf, [], 0
    for it in range(max_iter):
        _, st, dist = step(X, c)
        gaps = relative_gaps(dist)
        if (gaps > 0).any():
            min_gap = min(min_gap, gaps[gaps > 0].min())
        cnt = st[:, 0:1]
        emptied |= bool((cnt == 0).any())
        with np.errstate(divide="ignore", invalid="ignore"):
            new = np.where(cnt > 0, st[:, 1:1 + X.shape[1]] / cnt, c)
        shift = float(((new - c) ** 2).sum())
        shifts.append(shift)
        c = new
        n_iter = it + 1
        if shift <= thr:
            break
    _, st, _ = step(X, c)
    emptied |= bool((st[:, 0] == 0).any())
    return dict(centers=c + mu, inertia=float(st[:, 1 + X.shape[1]:].sum()), n_iter=n_iter, emptied=emptied,
                min_gap=min_gap, shifts=shifts, threshold=thr)


@functools.lru_cache(maxsize=None)
def recipe_lloyd(D, K):
    """The reference Lloyd run of every (group, restart) problem of one shape: list over g of list over r."""
    groups, init = recipe_groups(D), recipe_init(D, K)
    return tuple(tuple(lloyd(X, init[g, r]) for r in range(R)) for g, X in enumerate(groups))


# ---- kmeans(init=None, seeds=...): the seeding of ONE rank, restated from kmeans.py's docstring and DESIGN.md §8 ------
SUBSAMPLE_PER_CLUSTER = 256


def kmeans_pp(X, K, rng):
    """Plain k-means++ -> indices of K rows of ``X[n, D]``: the first uniform (``rng.integers``), each further one
    ``rng.choice`` in proportion to the squared distance to the nearest row chosen so far; when that total is zero (or
    not finite) uniform among the rows not chosen yet."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    idx = [int(rng.integers(n))]
    near = ((X - X[idx[0]]) ** 2).sum(axis=1)
    for _ in range(1, K):
        total = near.sum()
        if np.isfinite(total) and total > 0:
            i = int(rng.choice(n, p=near / total))
        else:
            free = np.setdiff1d(np.arange(n), idx)
            i = int(free[rng.integers(free.size)])
        idx.append(i)
        near = np.minimum(near, ((X - X[i]) ** 2).sum(axis=1))
    return np.array(idx, dtype=np.int64)


def seed_centres(X, K, n_init, seed):
    """-> (centres[n_init, K, D] float64, pick[m]): ``default_rng(seed)`` first draws the group's subsample — the sorted
    ``choice(n, m, replace=False)`` with ``m = min(n, 256 K)``, every row when ``m == n`` (no draw) — which all restarts
    share, then restart after restart one :func:`kmeans_pp` on it from the same stream."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    rng = np.random.default_rng(int(seed))
    m = min(n, SUBSAMPLE_PER_CLUSTER * K)
    pick = np.sort(rng.choice(n, m, replace=False)) if m < n else np.arange(n)
    sub = X[pick]
    return np.stack([sub[kmeans_pp(sub, K, rng)] for _ in range(n_init)]), pick


def best_restart(runs):
    """-> (index of the lowest inertia (first lowest), relative margin to the runner-up (inf for one run), indices of
    the runs within 1e-9 of the best)."""
    ri = np.array([run["inertia"] for run in runs])
    order = np.argsort(ri, kind="stable")
    if len(ri) < 2:
        return int(order[0]), np.inf, [int(order[0])]
    second = ri[order[1]]
    margin = (second - ri[order[0]]) / second if second > 0 else 0.0
    tied = [int(r) for r in range(len(ri)) if ri[r] - ri[order[0]] <= 1e-9 * ri[order[0]]]
    return int(order[0]), float(margin), tied


def kmeans_seeded(X, K, n_init, seed, tol=1e-4, max_iter=300):
    """``kmeans(init=None, seeds=[seed])`` for one group -> dict(runs (one :func:`lloyd` per restart), best, margin,
    tied, init, pick)."""
    init, pick = seed_centres(X, K, n_init, seed)
    runs = [lloyd(X, init[r], tol=tol, max_iter=max_iter) for r in range(n_init)]
    best, margin, tied = best_restart(runs)
    return dict(runs=runs, best=best, margin=margin, tied=tied, init=init, pick=pick)

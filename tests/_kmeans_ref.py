"""float64 numpy reference for the k-means tests (never imported by ``sapr_amd``) and the shared test recipe.

Recipe: group g is the frames of word g of ``synth_feature_set(VOCAB, 6, D, seed=21, tmin=1, tmax=110)`` concatenated
(182-484 frames: one or two tiles with a partial last tile; the duplicated "silence" frames are wanted); restart r of
group g starts from the rows ``default_rng(1000 * g + r).choice(n_g, K, replace=False)``, r = 0..2.

Lloyd follows scikit-learn's rules (threshold ``tol * mean(var(X, axis=0))``, new centre = mean of the cluster, stop when
the summed squared centre shift is <= threshold, inertia from one more assignment at the final centres) with ONE
deviation: an empty cluster keeps its previous centre.  Like scikit-learn, :func:`lloyd` works on the data minus its column
mean and adds the mean back to the centres (c0 sits near -300: coordinates near zero would otherwise carry the rounding
of sums near -300 n, which an element-wise comparison against scikit-learn at rtol 1e-12 sees).
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

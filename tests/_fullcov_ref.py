"""numpy float64 restatement of the Gaussian HMM with "full", "tied", "spherical" and "diag" covariances that
``sapr_amd.hmmlearn_hmm.GaussianHMM`` runs on the device (the definition the GPU tests compare against; hmmlearn's
``GaussianHMM``, restated from knowledge of hmmlearn 0.3.x — its source is not available where this is built).

S states, D features: ``startprob[S]``, ``transmat[S, S]`` (any pattern of zeros), ``means[S, D]``, ``covars[S, D, D]``
(the E-step always sees full matrices; a tied, spherical or diagonal model expands to them).

    logb[t,s]  = -(D log 2 pi + log|Sigma_s| + (x_t - mu_s)^T Sigma_s^-1 (x_t - mu_s)) / 2     (Cholesky, triangular solve)
    gamma_t(s) = softmax_s(fwd + bwd)        obs[s] = sum_t gamma_t(s) x_t        oo[s] = sum_t gamma_t(s) x_t x_t^T
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

from tests._gmmhmm_ref import _log, forward_backward

COVARIANCE_TYPES = ("diag", "spherical", "tied", "full")


def log_density(X, means, covars):
    """logb[T, S] of the frames X[T, D] under N(means[s], covars[s])."""
    X = np.asarray(X, dtype=np.float64)
    T, D = X.shape
    out = np.empty((T, means.shape[0]))
    for s, (mu, cv) in enumerate(zip(means, covars)):
        L = np.linalg.cholesky(cv)
        y = solve_triangular(L, (X - mu).T, lower=True)
        out[:, s] = -0.5 * (D * np.log(2 * np.pi) + 2.0 * np.log(np.diag(L)).sum() + (y ** 2).sum(axis=0))
    return out


def expand(covars, covariance_type, S, D):
    """``_covars_`` of a type -> [S, D, D]."""
    covars = np.asarray(covars, dtype=np.float64)
    if covariance_type == "full":
        return covars
    if covariance_type == "tied":
        return np.tile(covars, (S, 1, 1))
    if covariance_type == "diag":
        return np.array([np.diag(c) for c in covars])
    return np.array([np.eye(D) * c for c in covars])


def estep_utt(X, startprob, transmat, means, covars, acc=np.float64):
    """One utterance -> dict(loglik, gamma[T, S], start, trans, post, obs, oo, obs2).  ``acc``: the type the sums over
    the frames are accumulated in (np.longdouble gives the measure of the float64 sums' own rounding).  No frames:
    loglik -inf and zero statistics."""
    S, D = means.shape
    X32 = np.asarray(X, dtype=np.float32)
    T = X32.shape[0]
    z = {"loglik": -np.inf, "gamma": np.zeros((0, S)), "start": np.zeros(S), "trans": np.zeros((S, S)),
         "post": np.zeros(S), "obs": np.zeros((S, D)), "oo": np.zeros((S, D, D)), "obs2": np.zeros((S, D))}
    if T == 0:
        return z
    X64 = X32.astype(np.float64)
    logb = log_density(X64, means, covars)
    loglik, fwd, bwd = forward_backward(startprob, transmat, logb)
    lg = fwd + bwd
    with np.errstate(invalid="ignore", under="ignore"):
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        gamma = e / e.sum(axis=1, keepdims=True)
        lA = _log(transmat)
        trans = np.zeros((S, S))
        for t in range(1, T):
            trans += np.exp(fwd[t - 1][:, None] + lA + (logb[t] + bwd[t])[None, :] - loglik)
    ga, xa = gamma.astype(acc), X64.astype(acc)
    z.update(loglik=loglik, gamma=gamma, start=gamma[0].copy(), trans=trans, post=gamma.sum(axis=0),
             obs=np.einsum("ts,td->sd", ga, xa), oo=np.einsum("ts,ta,tb->sab", ga, xa, xa),
             obs2=np.einsum("ts,td->sd", ga, (X32 ** 2).astype(np.float64).astype(acc)))
    return z


def new_stats(S, D, acc=np.float64):
    return {"nobs": 0.0, "logprob": 0.0, "start": np.zeros(S), "trans": np.zeros((S, S)), "post": np.zeros(S),
            "obs": np.zeros((S, D), dtype=acc), "oo": np.zeros((S, D, D), dtype=acc), "obs2": np.zeros((S, D), dtype=acc)}


def accumulate(stats, u):
    if u["gamma"].shape[0] == 0:
        return
    stats["nobs"] += 1
    stats["logprob"] += u["loglik"]
    for k in ("start", "trans", "post", "obs", "oo", "obs2"):
        stats[k] += u[k]


def estep(utts, startprob, transmat, means, covars, acc=np.float64):
    """Statistics of one model over its utterances (list of [T, D] arrays) and the per-utterance results."""
    S, D = means.shape
    st, res = new_stats(S, D, acc), []
    for X in utts:
        res.append(estep_utt(X, startprob, transmat, means, covars, acc))
        accumulate(st, res[-1])
    return st, res


def viterbi(X, startprob, transmat, means, covars):
    """hmmlearn's viterbi over logb -> (logprob, path int64[T], gap), ties to the first maximum; ``gap`` as in
    ``tests/_gmmhmm_ref.viterbi``: the smallest relative distance between the best and the second-best finite candidate
    of any arg-max taken."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    T = X64.shape[0]
    logb = log_density(X64, means, covars)
    ls, lA = _log(startprob), _log(transmat)
    S = ls.shape[0]
    d = np.empty((T, S))
    d[0] = ls + logb[0]
    for t in range(1, T):
        d[t] = np.max(d[t - 1][:, None] + lA, axis=0) + logb[t]
    gap = np.inf

    def take(v):
        nonlocal gap
        k = int(np.argmax(v))
        fin = np.sort(v[np.isfinite(v)])
        if fin.size >= 2:
            gap = min(gap, (fin[-1] - fin[-2]) / abs(fin[-1]))
        return k
    path = np.empty(T, dtype=np.int64)
    path[T - 1] = take(d[T - 1])
    logprob = float(d[T - 1, path[T - 1]])
    for t in range(T - 2, -1, -1):
        path[t] = take(d[t] + lA[:, path[t + 1]])
    return logprob, path, gap


def m_step(stats, startprob, transmat, means, covars, covariance_type, params="stmc", startprob_prior=1.0,
           transmat_prior=1.0, means_prior=0.0, means_weight=0.0, covars_prior=1e-2, covars_weight=1.0):
    """hmmlearn 0.3.x ``GaussianHMM._do_mstep`` for the four covariance types; ``covars`` in the type's own shape.
    -> (startprob, transmat, means, covars)."""
    S, D = means.shape
    if "s" in params:
        sp = np.maximum(startprob_prior - 1 + stats["start"], 0)
        sp = np.where(startprob == 0, 0, sp)
        tot = sp.sum()
        startprob = sp / (tot if tot != 0 else 1.0)
    if "t" in params:
        tm = np.maximum(transmat_prior - 1 + stats["trans"], 0)
        tm = np.where(transmat == 0, 0, tm)
        rs = tm.sum(axis=1)
        rs[rs == 0] = 1
        transmat = tm / rs[:, None]
    post = stats["post"]
    denom = post[:, None]
    obs = np.asarray(stats["obs"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if "m" in params:
            means = (means_weight * means_prior + obs) / (means_weight + denom)
        if "c" in params:
            meandiff = means - means_prior
            if covariance_type in ("diag", "spherical"):
                obs2 = np.asarray(stats["obs2"], dtype=np.float64)
                c_n = means_weight * meandiff ** 2 + obs2 - 2 * means * obs + means ** 2 * denom
                c_d = max(covars_weight - 1, 0) + denom
                covars = (covars_prior + c_n) / np.maximum(c_d, 1e-5)
                if covariance_type == "spherical":
                    covars = covars.mean(axis=1)
            else:
                oo = np.asarray(stats["oo"], dtype=np.float64)
                c_n = np.empty((S, D, D))
                for s in range(S):
                    om = np.outer(obs[s], means[s])
                    c_n[s] = (means_weight * np.outer(meandiff[s], meandiff[s]) + oo[s] - (om + om.T)
                              + np.outer(means[s], means[s]) * post[s])
                cvweight = max(covars_weight - D, 0)
                if covariance_type == "tied":
                    covars = (covars_prior + c_n.sum(axis=0)) / (cvweight + post.sum())
                else:
                    covars = (covars_prior + c_n) / (cvweight + post[:, None, None])
    return startprob, transmat, means, covars


def em(utts, startprob, transmat, means, covars, covariance_type, n_iter, **hyper):
    """Fixed-parameter EM: ``n_iter`` iterations of E-step, M-step, report (no convergence test); ``covars`` in the
    type's own shape.  -> (parameters, history, covariances [S, D, D] after every iteration)."""
    prm = [np.array(a, dtype=np.float64) for a in (startprob, transmat, means, covars)]
    S, D = prm[2].shape
    hist, cvs = [], []
    for _ in range(n_iter):
        st, _ = estep(utts, prm[0], prm[1], prm[2], expand(prm[3], covariance_type, S, D))
        prm = list(m_step(st, *prm, covariance_type, **hyper))
        hist.append(st["logprob"])
        cvs.append(expand(prm[3], covariance_type, S, D))
    return tuple(prm), hist, cvs

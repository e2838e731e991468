"""numpy float64 restatement of the Gaussian-mixture HMM that ``sapr_amd.gmm_hmm`` runs on the device (the
definition the GPU tests compare against; hmmlearn's ``GMMHMM`` with diagonal covariances, restated from knowledge of
hmmlearn 0.3.x — its source is not available where this is built).

S states, M components per state, D features: ``startprob[S]``, ``transmat[S, S]`` (any pattern of zeros),
``weights[S, M]``, ``means[S, M, D]``, ``covars[S, M, D]``.

    lc[t,s,m] = log w[s,m] - (D log 2 pi + sum_d log var[s,m,d] + sum_d (x[t,d] - mu[s,m,d])^2 / var[s,m,d]) / 2
    logb[t,s] = logsumexp_m lc[t,s,m]                 (log 0 = -inf flows through)
    gamma_t(s) = softmax_s(fwd + bwd)                  r[t,s,m] = gamma_t(s) exp(lc[t,s,m] - logb[t,s])
"""
from __future__ import annotations

import numpy as np


def _log(x):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(x, dtype=np.float64))


def _lse(v, axis):
    """max-shifted logsumexp; the maximum itself where it is infinite (_hmmc.cpp logsumexp)."""
    m = np.max(v, axis=axis, keepdims=True)
    with np.errstate(invalid="ignore", under="ignore", divide="ignore"):
        out = np.log(np.sum(np.exp(v - m), axis=axis, keepdims=True)) + m
    out = np.where(np.isinf(m), m, out)
    return np.squeeze(out, axis=axis)


def log_components(X, weights, means, covars):
    """lc[T, S, M]; the difference is squared directly (c0 sits near -300: the expanded form cancels)."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    diff = X[:, None, None, :] - means[None]
    quad = (diff ** 2 / covars[None]).sum(axis=-1)
    return _log(weights)[None] - 0.5 * (D * np.log(2 * np.pi) + np.log(covars).sum(axis=-1)[None] + quad)


def forward_backward(startprob, transmat, logb):
    ls, lA = _log(startprob), _log(transmat)
    T, S = logb.shape
    fwd = np.empty((T, S))
    bwd = np.zeros((T, S))
    fwd[0] = ls + logb[0]
    for t in range(1, T):
        fwd[t] = _lse(fwd[t - 1][:, None] + lA, axis=0) + logb[t]
    for t in range(T - 2, -1, -1):
        bwd[t] = _lse(lA + (logb[t + 1] + bwd[t + 1])[None, :], axis=1)
    return float(_lse(fwd[T - 1], axis=0)), fwd, bwd


def estep_utt(X, startprob, transmat, weights, means, covars):
    """One utterance -> dict(loglik, gamma[T, S], start, trans, post, post_mix, obs, obs2).  ``X**2`` is evaluated in
    float32, X's own dtype, as numpy squares a float32 feature array, and only then promoted.  No frames: loglik
    -inf and zero statistics."""
    S, M, D = means.shape
    X32 = np.asarray(X, dtype=np.float32)
    T = X32.shape[0]
    z = {"loglik": -np.inf, "gamma": np.zeros((0, S)), "start": np.zeros(S), "trans": np.zeros((S, S)),
         "post": np.zeros(S), "post_mix": np.zeros((S, M)), "obs": np.zeros((S, M, D)), "obs2": np.zeros((S, M, D))}
    if T == 0:
        return z
    X64 = X32.astype(np.float64)
    lc = log_components(X64, weights, means, covars)
    logb = _lse(lc, axis=2)
    loglik, fwd, bwd = forward_backward(startprob, transmat, logb)
    lg = fwd + bwd
    with np.errstate(invalid="ignore", under="ignore"):
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        gamma = e / e.sum(axis=1, keepdims=True)
        lA = _log(transmat)
        trans = np.zeros((S, S))
        for t in range(1, T):
            trans += np.exp(fwd[t - 1][:, None] + lA + (logb[t] + bwd[t])[None, :] - loglik)
        resp = np.where(np.isneginf(lc), 0.0, np.exp(lc - logb[:, :, None]))
        r = gamma[:, :, None] * resp
    z.update(loglik=loglik, gamma=gamma, start=gamma[0].copy(), trans=trans, post=gamma.sum(axis=0),
             post_mix=r.sum(axis=0), obs=np.einsum("tsm,td->smd", r, X64),
             obs2=np.einsum("tsm,td->smd", r, (X32 ** 2).astype(np.float64)))
    return z


def new_stats(S, M, D):
    return {"nobs": 0.0, "logprob": 0.0, "start": np.zeros(S), "trans": np.zeros((S, S)), "post": np.zeros(S),
            "post_mix": np.zeros((S, M)), "obs": np.zeros((S, M, D)), "obs2": np.zeros((S, M, D))}


def accumulate(stats, u):
    """Add one :func:`estep_utt` result; an utterance without frames contributes nothing."""
    if u["gamma"].shape[0] == 0:
        return
    stats["nobs"] += 1
    stats["logprob"] += u["loglik"]
    for k in ("start", "trans", "post", "post_mix", "obs", "obs2"):
        stats[k] += u[k]


def estep(utts, startprob, transmat, weights, means, covars):
    """Statistics of one model over its utterances (list of [T, D] arrays) and the per-utterance results."""
    S, M, D = means.shape
    st, res = new_stats(S, M, D), []
    for X in utts:
        res.append(estep_utt(X, startprob, transmat, weights, means, covars))
        accumulate(st, res[-1])
    return st, res


def viterbi(X, startprob, transmat, weights, means, covars):
    """hmmlearn's viterbi over logb -> (logprob, path int64[T], gap): ties go to the first maximum; ``gap`` is the
    smallest relative distance between the best and the second-best FINITE candidate of any arg-max taken (inf when no
    arg-max had two finite candidates) — a path is only comparable across implementations when it is well above the
    rounding error of the scores."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    T = X64.shape[0]
    logb = _lse(log_components(X64, weights, means, covars), axis=2)
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


def m_step(stats, startprob, transmat, weights, means, covars, params="stmcw", startprob_prior=1.0,
           transmat_prior=1.0, weights_prior=1.0, means_prior=0.0, means_weight=0.0, covars_prior=-1.5,
           covars_weight=0.0, min_covar=1e-3):
    """hmmlearn 0.3.x ``GMMHMM._do_mstep`` (diag), restated, with two deliberate rules on top: a component whose mean
    denominator is exactly 0 keeps its previous mean and covariance; ``covars = max(covars, min_covar)`` after the
    formula.  A state whose weight denominator is exactly 0 keeps its weights.  -> (startprob, transmat, weights, means,
    covars)."""
    S, M = weights.shape
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
    pm = stats["post_mix"]
    new_w, new_m, new_c = weights.copy(), means.copy(), covars.copy()
    wp = np.broadcast_to(np.asarray(weights_prior, dtype=np.float64), (S, M))
    for s in range(S):
        if "w" in params:
            den = stats["post"][s] + (wp[s] - 1).sum()
            if den != 0:
                new_w[s] = (pm[s] + wp[s] - 1) / den
        for m in range(M):
            den = means_weight + pm[s, m]
            if den == 0:
                continue   # the empty-component rule
            if "m" in params:
                new_m[s, m] = (means_weight * means_prior + stats["obs"][s, m]) / den
            if "c" in params:
                mu = new_m[s, m]
                num = (stats["obs2"][s, m] - 2 * mu * stats["obs"][s, m] + mu ** 2 * pm[s, m]
                       + means_weight * (mu - means_prior) ** 2 + 2 * covars_weight)
                with np.errstate(divide="ignore", invalid="ignore"):
                    new_c[s, m] = np.maximum(num / (pm[s, m] + 1 + 2 * (covars_prior + 1)), min_covar)
    return startprob, transmat, new_w, new_m, new_c


def em(utts, startprob, transmat, weights, means, covars, n_iter, **hyper):
    """Fixed-parameter EM: ``n_iter`` iterations of E-step, M-step, report (no convergence test).  -> (parameters,
    history, occupancy) with ``occupancy[it]`` = post_mix of iteration ``it``."""
    prm = tuple(np.array(a, dtype=np.float64) for a in (startprob, transmat, weights, means, covars))
    hist, occ = [], []
    for _ in range(n_iter):
        st, _ = estep(utts, *prm)
        occ.append(st["post_mix"].copy())
        prm = m_step(st, *prm, **hyper)
        hist.append(st["logprob"])
    return prm, hist, occ

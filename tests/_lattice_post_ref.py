"""CPU restatement of the lattice posteriors (plain numpy, float64): THE DEFINITION of what
``sapr_connected_lattice_posteriors`` computes (include/sapr_hip.h) — forward-backward in the sum semiring over the
word lattice of ``tests/_lattice_ref.py``.  The records, ``tau``, ``in`` and ``ac`` are that file's (``records``, with
its skip rules); nothing of it is restated here.

Inputs, per utterance of T frames: the forward tables X, N, B; ``forward_lm_start``, the table the lattice was made
under (it defines ``ac``); the tables ``(lm', lm_start', lm_end')`` of this pass; an acoustic scale kappa > 0; optionally
a mask ``keep[T][W]`` — a record with ``keep == 0`` does not exist for this pass.  With ``a = kappa * ac``, ``lse`` the
log-sum-exp (the maximum taken out, the exponentials added in ascending order of the index) and alpha, Q, beta, H
initialised to -inf::

    forward, t ascending:    for every record (w, t) with start tau:
                                 alpha_t(w) = a + (lm_start'[w] if tau = 0 else Q_{tau-1}(w))
                             then for every w:  Q_t(w) = lse_v (alpha_t(v) + lm'[v][w])
    backward, t descending:  for every v:  beta_t(v) = lse_w (lm'[v][w] + H_{t+1}(w)),  H_T = -inf,
                                 and at t = T - 1 log-added with lm_end'[v]
                             then for every record (w, t), w ascending:
                                 g = a + beta_t(w);   H_tau(w) = logaddexp(H_tau(w), g)

    loglik            = lse_w (alpha_{T-1}(w) + lm_end'[w])        (backward form: lse_w (lm_start'[w] + H_0(w)))
    record_post[t][w] = exp(alpha_t(w) + beta_t(w) - loglik) for a record, 0 elsewhere
    word_post[f][w]   = the sum of record_post[t][w] over the records of w with tau <= f <= t

T = 0 gives ``loglik`` = -inf; a ``loglik`` that is not finite gives exact zeros in both tables.
"""
import numpy as np

from . import _lattice_ref as lref


def lse(v, axis=0):
    """The log-sum-exp along ``axis``: the maximum taken out; an infinite maximum is the result."""
    v = np.asarray(v, dtype=np.float64)
    m = v.max(axis=axis)
    safe = np.where(np.isinf(m), 0.0, m)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = np.log(np.exp(v - np.expand_dims(safe, axis)).sum(axis=axis)) + safe
    return np.where(np.isinf(m), m, r)


def posteriors(X, N, B, forward_lm_start, lm2, lm_start2, lm_end2, kappa=1.0, keep=None):
    """One utterance -> a dict of ``loglik``, ``loglik_backward``, ``record_post[T, W]``, ``word_post[T, W]`` and the
    recursion's tables ``alpha``, ``Q``, ``beta``, ``H`` (each ``[T, W]``)."""
    X = np.asarray(X, dtype=np.float64)
    T, W = X.shape
    lm2 = np.asarray(lm2, dtype=np.float64)
    lm_start2 = np.asarray(lm_start2, dtype=np.float64)
    lm_end2 = np.asarray(lm_end2, dtype=np.float64)
    kappa = np.float64(kappa)
    alpha, Q, beta, H = (np.full((T, W), -np.inf) for _ in range(4))
    rp, wp = np.zeros((T, W)), np.zeros((T, W))
    out = dict(loglik=-np.inf, loglik_backward=-np.inf, record_post=rp, word_post=wp, alpha=alpha, Q=Q, beta=beta, H=H)
    if T == 0:
        return out
    recs = [r for r in lref.records(X, N, B, forward_lm_start) if keep is None or keep[r[0], r[1]]]
    by_end = {}
    for r in recs:
        by_end.setdefault(r[0], []).append(r)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            for _, w, tau, _, ac in by_end.get(t, []):
                alpha[t, w] = kappa * np.float64(ac) + (lm_start2[w] if tau == 0 else Q[tau - 1, w])
            Q[t] = lse(alpha[t][:, None] + lm2, axis=0)
        for t in range(T - 1, -1, -1):
            beta[t] = lse(lm2 + H[t + 1][None, :], axis=1) if t + 1 < T else np.logaddexp(-np.inf, lm_end2)
            for _, w, tau, _, ac in by_end.get(t, []):
                g = kappa * np.float64(ac) + beta[t, w]
                H[tau, w] = np.logaddexp(H[tau, w], g)
        ll = float(lse(alpha[T - 1] + lm_end2))
        out["loglik"], out["loglik_backward"] = ll, float(lse(lm_start2 + H[0]))
        if not np.isfinite(ll):
            return out
        for t, w, tau, _, _ in recs:
            rp[t, w] = np.exp(alpha[t, w] + beta[t, w] - ll)
            wp[tau:t + 1, w] += rp[t, w]
    return out


def batch(tabs, lengths, forward_lm_start, lm2, lm_start2, lm_end2, kappa=1.0, keep=None):
    """A packed batch (``tabs``: the concatenated X, N, B of ``_lattice_ref.batch``) -> ``(per_utt, dict(loglik[N],
    record_post, word_post))`` as the device returns them."""
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    W = tabs["X"].shape[1]
    per = [posteriors(tabs["X"][a:b], tabs["N"][a:b], tabs["B"][a:b], forward_lm_start, lm2, lm_start2, lm_end2, kappa,
                      None if keep is None else keep[a:b]) for a, b in zip(offs[:-1], offs[1:])]
    cat = lambda k: np.concatenate([p[k] for p in per]) if per else np.zeros((0, W))  # noqa: E731
    return per, dict(loglik=np.asarray([p["loglik"] for p in per], np.float64), record_post=cat("record_post"),
                     word_post=cat("word_post"))

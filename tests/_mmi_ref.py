"""CPU restatement of discriminative (MMI) training of the word models over the word loop (plain numpy, float64): THE
DEFINITION of what ``sapr_connected_loop_stats``, ``connected.mmi_estep``, ``connected.mmi_update`` and
``connected.mmi_fit`` compute.  Built on ``tests/_embedded_ref.py`` (the numerator: forward-backward over the
transcript's chain) and ``tests/_loop_fb_ref.py`` (the denominator: forward-backward over the word loop).

With utterance u, its transcript ``w_0 .. w_{K-1}``, the language model ``(lm, lm_start, lm_end)`` and
``logb' = acoustic_scale * logb``::

    lmscore(u)    = lm_start[w_0] + sum_{k>=1} lm[w_{k-1}, w_k] + lm_end[w_{K-1}]
    num_loglik(u) = loglik of _embedded_ref.forward_backward on logb' with pen = 0.0,  + lmscore(u)
    den_loglik(u) = loglik of _loop_fb_ref.forward_backward on logb' under (lm, lm_start, lm_end)
    keep(u)       = both finite
    F             = sum_{keep} (num_loglik(u) - den_loglik(u))

The chain's paths are a subset of the loop's, so every term is <= 0 up to rounding: the log posterior of the
transcript.  The denominator statistics per word w and state s sum over the frames of the kept utterances::

    post[w][s] = sum post_t(w,s)     obs[w][s] = sum post_t(w,s) x_t     obs2[w][s] = sum post_t(w,s) (x_t x_t)_float32

and ``nobs`` = the kept utterances with at least one frame.  The numerator statistics are
``_embedded_ref.estep_batch``'s over the kept utterances alone.  :func:`update` is the extended Baum-Welch step, written
out state by state and feature by feature.
"""
import copy
import math

import numpy as np

from tests import _embedded_ref as eref
from tests import _loop_fb_ref as fref

NEG = -np.inf


def lm_score(words, lm, lm_start, lm_end):
    words = [int(w) for w in words]
    sc = np.float64(lm_start[words[0]])
    for a, b in zip(words[:-1], words[1:]):
        sc = sc + lm[a, b]
    return float(sc + lm_end[words[-1]])


def den_stats(post, feats, lengths, keep=None):
    """``post[total_frames, W, S]`` and the float32 frames ``feats[total_frames, D]`` -> a dict with ``nobs`` (a
    number), ``post[W, S]``, ``obs[W, S, D]``, ``obs2[W, S, D]`` over the utterances with ``keep[u]`` (all of them
    without ``keep``).  A frame of an utterance that is not kept is not looked at, whatever it holds."""
    post = np.asarray(post, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.r_[0, np.cumsum(lengths)]
    keep = np.ones(len(lengths), bool) if keep is None else np.asarray(keep).astype(bool)
    _, W, S = post.shape
    x32 = np.asarray(feats, dtype=np.float32)
    D = x32.shape[1]
    out = {"nobs": 0.0, "post": np.zeros((W, S)), "obs": np.zeros((W, S, D)), "obs2": np.zeros((W, S, D))}
    for u, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        if not keep[u] or b == a:
            continue
        x = x32[a:b].astype(np.float64)
        x2 = (x32[a:b] * x32[a:b]).astype(np.float64)            # (the float32 square, as hmmlearn evaluates X**2)
        g = post[a:b].reshape(b - a, W * S)
        out["nobs"] += 1.0
        out["post"] += g.sum(axis=0).reshape(W, S)
        out["obs"] += (g.T @ x).reshape(W, S, D)
        out["obs2"] += (g.T @ x2).reshape(W, S, D)
    return out


def objective(logb, lengths, transcripts, ls, lt, lx, lm, lm_start, lm_end):
    """A packed ``logb[total_frames, W, S]`` (already scaled) -> a dict with ``num_loglik[N]``, ``den_loglik[N]``,
    ``lmscore[N]``, ``keep[N]``, ``terms[N]`` (num - den where kept, 0.0 elsewhere), ``F`` and the denominator's
    ``post[total_frames, W, S]``."""
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.r_[0, np.cumsum(lengths)]
    N = len(lengths)
    W, S = np.shape(ls)
    num, den, lms = np.full(N, NEG), np.full(N, NEG), np.zeros(N)
    post = np.zeros((int(offs[-1]), W, S))
    for u, (a, b, words) in enumerate(zip(offs[:-1], offs[1:], transcripts)):
        lms[u] = lm_score(words, lm, lm_start, lm_end)
        num[u] = eref.forward_backward(logb[a:b], words, ls, lt, lx, 0.0)["loglik"] + lms[u]
        r = fref.forward_backward(logb[a:b], ls, lt, lx, lm, lm_start, lm_end)
        den[u], post[a:b] = r["loglik"], r["post"]
    keep = np.isfinite(num) & np.isfinite(den)
    terms = np.where(keep, np.where(keep, num, 0.0) - np.where(keep, den, 0.0), 0.0)
    return {"num_loglik": num, "den_loglik": den, "lmscore": lms, "keep": keep, "terms": terms,
            "F": float(terms[keep].sum()), "post": post}


def estep(logb, feats, lengths, transcripts, ls, lt, lx, lm, lm_start, lm_end):
    """:func:`objective` plus ``num`` (``_embedded_ref.estep_batch`` over the kept utterances alone) and ``den``
    (:func:`den_stats` over the kept utterances)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.r_[0, np.cumsum(lengths)]
    out = objective(logb, lengths, transcripts, ls, lt, lx, lm, lm_start, lm_end)
    kept = np.flatnonzero(out["keep"])
    rows = np.concatenate([np.arange(offs[u], offs[u + 1]) for u in kept] + [np.zeros(0, np.int64)]).astype(np.int64)
    x32 = np.asarray(feats, dtype=np.float32)
    out["num"] = eref.estep_batch(np.asarray(logb)[rows], lengths[kept], [transcripts[u] for u in kept], ls, lt, lx,
                                  0.0, feats=x32[rows])
    out["den"] = den_stats(out["post"], x32, lengths, out["keep"])
    return out


def d_min(occ, th1, th2, mu, var):
    """The smallest constant that keeps every variance of one state positive: the larger real root over the features
    of ``var D^2 + (th2 + occ (var + mu^2) - 2 mu th1) D + occ th2 - th1^2`` (none: 0), ``-occ`` and 0."""
    best = max(0.0, -float(occ))
    for d in range(len(mu)):
        a = float(var[d])
        b = float(th2[d] + occ * (var[d] + mu[d] * mu[d]) - 2.0 * mu[d] * th1[d])
        c = float(occ * th2[d] - th1[d] * th1[d])
        disc = b * b - 4.0 * a * c
        if disc >= 0.0:
            best = max(best, (-b + math.sqrt(disc)) / (2.0 * a))
    return best


def update(num, den, means, covars, covariance_type, E=2.0, tau=0.0, min_covar=1e-3, D_s=None):
    """The extended Baum-Welch step of one word model: ``num`` / ``den`` carry ``post[S]``, ``obs[S, D]`` and
    ``obs**2[S, D]`` (``obs2`` is read too); ``covars`` is ``[S, D]`` ("diag") or ``[S]`` ("spherical").  ``D_s``:
    the constants to use in place of ``max(E den.post, 2 D_min)`` (one per state).  Returns ``(means, covars)``."""
    mu_all = np.array(means, dtype=np.float64)
    cv = np.array(covars, dtype=np.float64)
    S, D = mu_all.shape
    sq = lambda st: np.asarray(st["obs**2"] if "obs**2" in st else st["obs2"], dtype=np.float64)  # noqa: E731
    out_mu, out_cv = mu_all.copy(), cv.copy()
    for s in range(S):
        mu = mu_all[s]
        var = np.full(D, cv[s]) if covariance_type == "spherical" else cv[s]
        n_post = float(num["post"][s])
        scale = 1.0 + tau / n_post if (tau != 0.0 and n_post != 0.0) else 1.0
        occ = n_post * scale - float(den["post"][s])
        th1 = np.asarray(num["obs"][s], dtype=np.float64) * scale - np.asarray(den["obs"][s], dtype=np.float64)
        th2 = sq(num)[s] * scale - sq(den)[s]
        Ds = max(E * float(den["post"][s]), 2.0 * d_min(occ, th1, th2, mu, var)) if D_s is None else float(D_s[s])
        if occ + Ds == 0.0:
            continue                                             # an empty state keeps its parameters
        mu_new = (th1 + Ds * mu) / (occ + Ds)
        var_new = np.maximum((th2 + Ds * (var + mu * mu)) / (occ + Ds) - mu_new * mu_new, min_covar)
        out_mu[s] = mu_new
        if covariance_type == "spherical":
            out_cv[s] = var_new.mean()
        else:
            out_cv[s] = var_new
    return out_mu, out_cv


def fit(models, features, transcripts, lm=None, n_iter=4, E=2.0, tau=0.0, acoustic_scale=1.0, exit_states="last",
        word_penalty=0.0):
    """MMI training on the host over copies of ``models`` ("diag" / "spherical" ``GaussianHMM`` objects that share S
    and D); ``lm``: ``(lm, lm_start, lm_end)`` as the word loop runs under it, or ``None`` for ``lm == word_penalty``.
    Returns ``(models, history of F, the last E-step)``; F is evaluated before each update."""
    models = [copy.deepcopy(m) for m in models]
    feats = [np.asarray(f, dtype=np.float32) for f in features]
    lengths = [len(f) for f in feats]
    x = np.concatenate(feats)
    W = len(models)
    if lm is None:
        lm = (np.full((W, W), np.float64(word_penalty)), np.zeros(W), np.zeros(W))
    history, last = [], None
    for _ in range(n_iter):
        ls, lt, lx, means, vars_, gconst = eref.tables(models, exit_states)
        logb = eref.emit_diag(x.astype(np.float64), means, vars_, gconst)
        if acoustic_scale != 1.0:
            logb = acoustic_scale * logb
        last = estep(logb, x, lengths, transcripts, ls, lt, lx, *lm)
        history.append(last["F"])
        for w, m in enumerate(models):
            if last["num"]["nobs"][w] == 0:
                continue
            num = {"post": last["num"]["post_sum"][w], "obs": last["num"]["obs"][w], "obs**2": last["num"]["obs2"][w]}
            den = {"post": last["den"]["post"][w], "obs": last["den"]["obs"][w], "obs**2": last["den"]["obs2"][w]}
            m.means_, m._covars_ = update(num, den, m.means_, m._covars_, m.covariance_type, E, tau,
                                          getattr(m, "min_covar", 1e-3))
    return models, history, last

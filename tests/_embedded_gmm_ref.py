"""CPU restatement of embedded Baum-Welch for Gaussian-mixture word models (plain numpy, float64): THE DEFINITION of
what ``sapr_connected_embed_gmm`` computes (include/sapr_hip.h).  It builds on ``tests/_embedded_ref.py`` — the
recursion, ``gamma``, ``loglik``, ``nobs``, ``start``, ``trans`` and ``post`` are those of ``estep_batch`` — and on
``tests/_gmmhmm_ref.py`` for the component log-terms ``lc = log_components``.  With ``x_t`` the float32 frame widened to
float64 and ``g_t(w,s) = sum_{k: w_k = w} gamma_t(k,s)``, for every word model ``w``::

    r_t(w,s,m)        = g_t(w,s) exp(lc[t,w,s,m] - max_m lc) / sum_m exp(lc - max_m lc)
                        (0 where every component of the state is switched off: max_m lc = -inf)
    post_mix[w][s][m] = sum r      obs[w][s][m] = sum r x_t      obs2[w][s][m] = sum r f64(RN32(x_t x_t))

over the utterances with a finite ``loglik`` and all their frames.  The float32 square is the rule of
``sapr_gmm_estep_diag`` and of hmmlearn's ``X**2`` on float32 features.  An utterance without a path contributes exact
zeros, as in ``sapr_connected_embed``.

``fit_gmm`` is the host EM loop over ``GMMHMM`` objects; it mirrors ``_embedded_ref.fit`` / ``_embedded_full_ref
.fit_full``.
"""
import copy

import numpy as np

from tests import _embedded_ref as eref
from tests import _gmmhmm_ref as gref
from tests._embedded_ref import NEG  # noqa: F401


def responsibilities(x, weights, means, covars):
    """``resp[T, S, M]`` of one word model over the widened frames ``x[T, D]``: the softmax of ``lc`` over the
    components, 0 for a state whose components are all switched off."""
    lc = gref.log_components(x, weights, means, covars)
    mx = lc.max(axis=2, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(lc - mx)
        resp = e / e.sum(axis=2, keepdims=True)
    return np.where(np.isneginf(mx), 0.0, resp)


def _mix_sums(g, x, x2, weights, means, covars):
    """``(post_mix, obs, obs2)`` of one word from its collapsed weights ``g[T, S]``."""
    r = g[:, :, None] * responsibilities(x, weights, means, covars)
    r = np.where(g[:, :, None] == 0.0, 0.0, r)
    return r.sum(axis=0), np.einsum("tsm,td->smd", r, x), np.einsum("tsm,td->smd", r, x2)


def estep_batch_gmm(logb, lengths, transcripts, ls, lt, lx, pen, feats, weights, means, covars, max_words=None):
    """``_embedded_ref.estep_batch`` (without its single-Gaussian ``obs`` / ``obs2``) plus ``post_mix[W, S, M]``,
    ``obs[W, S, M, D]`` and ``obs2[W, S, M, D]``; ``weights[W, S, M]``, ``means[W, S, M, D]``,
    ``covars[W, S, M, D]``."""
    res = eref.estep_batch(logb, lengths, transcripts, ls, lt, lx, pen, None, max_words)
    weights, means, covars = (np.asarray(a, dtype=np.float64) for a in (weights, means, covars))
    W, S, M, D = means.shape
    x32 = np.asarray(feats, dtype=np.float32)
    x, x2 = x32.astype(np.float64), (x32 * x32).astype(np.float64)
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    post_mix, obs, obs2 = np.zeros((W, S, M)), np.zeros((W, S, M, D)), np.zeros((W, S, M, D))
    for u, (a, b, words) in enumerate(zip(offs[:-1], offs[1:], transcripts)):
        if not np.isfinite(res["loglik"][u]):
            continue
        gam = res["post"][a:b]                                    # [T][max_words][S]
        for w in sorted(set(int(v) for v in words)):
            g = np.zeros((b - a, S))
            for k, wk in enumerate(words):                        # (k ascending)
                if wk == w:
                    g += gam[:, k]
            pm, o1, o2 = _mix_sums(g, x[a:b], x2[a:b], weights[w], means[w], covars[w])
            post_mix[w] += pm
            obs[w] += o1
            obs2[w] += o2
    res.update(post_mix=post_mix, obs=obs, obs2=obs2)
    return res


def brute_mix(logb, words, ls, lt, lx, pen, x, weights, means, covars):
    """``(post_mix[W, S, M], obs[W, S, M, D], obs2[W, S, M, D])`` of one utterance from the posteriors of the path
    enumeration (``_embedded_ref.brute``), frame by frame."""
    r = eref.brute(logb, words, ls, lt, lx, pen)
    x32 = np.asarray(x, dtype=np.float32)
    x64, x2 = x32.astype(np.float64), (x32 * x32).astype(np.float64)
    W, S, M, D = np.shape(means)
    post_mix, obs, obs2 = np.zeros((W, S, M)), np.zeros((W, S, M, D)), np.zeros((W, S, M, D))
    if np.isfinite(r["loglik"]):
        for k, w in enumerate(words):
            resp = responsibilities(x64, weights[w], means[w], covars[w])
            for t in range(x64.shape[0]):
                rt = r["gamma"][t, k][:, None] * resp[t]          # [S][M]
                post_mix[w] += rt
                obs[w] += rt[:, :, None] * x64[t]
                obs2[w] += rt[:, :, None] * x2[t]
    return post_mix, obs, obs2


def gmm_tables(models, exit_states="last"):
    """``(log_start, log_trans, log_exit, weights[W, S, M], means[W, S, M, D], covars[W, S, M, D])`` of ``GMMHMM``
    models that share S, M and D: what ``ConnectedNetwork.from_models`` reads through ``GmmPack.from_models``."""
    W = len(models)
    S, M, D = np.asarray(models[0].means_).shape
    ls, lt, lx = np.full((W, S), NEG), np.full((W, S, S), NEG), np.full((W, S), NEG)
    weights, means, covars = np.zeros((W, S, M)), np.zeros((W, S, M, D)), np.ones((W, S, M, D))
    with np.errstate(divide="ignore"):
        for w, m in enumerate(models):
            ls[w] = np.log(np.asarray(m.startprob_, dtype=np.float64))
            lt[w] = np.log(np.asarray(m.transmat_, dtype=np.float64))
            weights[w], means[w], covars[w] = m.weights_, m.means_, m.covars_
    if exit_states == "last":
        lx[:, S - 1] = 0.0
    else:
        lx[:] = 0.0
    return ls, lt, lx, weights, means, covars


def emit_gmm(feats, weights, means, covars):
    """``logb[T, W, S]``: the log-sum-exp of each state's component log-terms."""
    x = np.asarray(feats, dtype=np.float64)
    return np.stack([gref._lse(gref.log_components(x, weights[w], means[w], covars[w]), axis=2)
                     for w in range(weights.shape[0])], axis=1)


def word_stats(r, w):
    """The statistics dict ``_gmmhmm_ref.m_step`` reads, of word ``w`` from :func:`estep_batch_gmm`'s result."""
    return {"nobs": r["nobs"][w], "start": r["start"][w], "trans": r["trans"][w], "post": r["post_sum"][w],
            "post_mix": r["post_mix"][w], "obs": r["obs"][w], "obs2": r["obs2"][w]}


def fit_gmm(models, features, transcripts, n_iter=10, tol=1e-2, exit_states="last", word_penalty=0.0):
    """Embedded Baum-Welch on the host over copies of ``models`` (``GMMHMM`` objects that share S, M and D);
    ``features``: frame-major ``(T, D)`` arrays.  Per iteration: the tables of the current models, the emission,
    :func:`estep_batch_gmm`, ``_gmmhmm_ref.m_step`` per word that occurred with the model's own hyper-parameters, then
    the sum of the log-likelihoods of the utterances with a path goes to one ``ConvergenceMonitor``.  Returns
    ``(models, history)``."""
    from sapr_amd.hmmlearn_hmm import ConvergenceMonitor
    models = [copy.deepcopy(m) for m in models]
    feats = [np.asarray(f, dtype=np.float32) for f in features]
    lengths = [len(f) for f in feats]
    x = np.concatenate(feats)
    monitor = ConvergenceMonitor(tol, n_iter)
    for _ in range(n_iter):
        ls, lt, lx, weights, means, covars = gmm_tables(models, exit_states)
        logb = emit_gmm(x.astype(np.float64), weights, means, covars)
        r = estep_batch_gmm(logb, lengths, transcripts, ls, lt, lx, word_penalty, x, weights, means, covars)
        for w, m in enumerate(models):
            if r["nobs"][w] == 0:
                continue
            m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_ = gref.m_step(
                word_stats(r, w), *(np.asarray(a, dtype=np.float64) for a in
                                    (m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_)),
                params=m.params, startprob_prior=m.startprob_prior, transmat_prior=m.transmat_prior,
                weights_prior=m.weights_prior, means_prior=m.means_prior, means_weight=m.means_weight,
                covars_prior=m.covars_prior, covars_weight=m.covars_weight, min_covar=m.min_covar)
        ll = r["loglik"]
        monitor.report(float(ll[np.isfinite(ll)].sum()))
        if monitor.converged:
            break
    return models, list(monitor.history)

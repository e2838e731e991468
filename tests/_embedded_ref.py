"""CPU restatement of embedded Baum-Welch (plain numpy, float64): THE DEFINITION of what ``sapr_connected_embed``
computes (include/sapr_hip.h).  The conventions are those of ``tests/_align_ref.py``: utterance u has frames
``0..T-1`` and a transcript ``w_0..w_{K-1}``; its network is the left-to-right chain of these K words.  With
``b_t(k,s) = logb[t][w_k][s]`` and ``lse`` the log-sum-exp over the finite terms::

    alpha_0(0,j)  = log_start[w_0][j] + b_0(0,j)             alpha_0(k>0,j) = -inf
    X_{t-1}(k)    = lse_s (alpha_{t-1}(k,s) + log_exit[w_k][s])
    alpha_t(k,j)  = lse( lse_i (alpha_{t-1}(k,i) + log_trans[w_k][i][j]),
                         (X_{t-1}(k-1) + word_penalty) + log_start[w_k][j] ) + b_t(k,j)      (k = 0: no entry term)
    loglik        = X_{T-1}(K-1)

    beta_{T-1}(K-1,s) = log_exit[w_{K-1}][s]                 beta_{T-1}(k<K-1,s) = -inf
    E_t(k)        = word_penalty + lse_j (log_start[w_k][j] + b_t(k,j) + beta_t(k,j))        (k >= 1)
    beta_t(k,i)   = lse( lse_j (log_trans[w_k][i][j] + b_{t+1}(k,j) + beta_{t+1}(k,j)),
                         log_exit[w_k][i] + E_{t+1}(k+1) )                                   (k = K-1: no exit term)
    gamma_t(k,s)  = exp(alpha_t(k,s) + beta_t(k,s) - loglik)

The statistics are kept per word model w and sum over every slot k with ``w_k = w`` of every utterance whose
``loglik`` is finite: ``post``, ``obs``, ``obs**2`` (sums of gamma, gamma x, gamma x^2 in float64 over the float32
features, x^2 being the float32 square as in the isolated-word E-step and in hmmlearn), ``trans`` (the expected
transitions inside a word), ``start`` (gamma_0 of slot 0 plus the expected entries of the later slots) and ``nobs``
(the number of such slots).  An utterance without a path — no frames, no words, more words than frames or than
``max_words``, a word outside the vocabulary, a likelihood that is not finite — contributes exact zeros and its
posterior rows are 0.
"""
import copy

import numpy as np

NEG = -np.inf


def _lse(a, axis):
    return np.logaddexp.reduce(a, axis=axis)


def forward_backward(logb, words, ls, lt, lx, pen=0.0):
    """One utterance: ``logb[T, W, S]`` and its transcript -> a dict with ``loglik``, ``gamma[T, K, S]`` and the
    per-slot ``start[K, S]``, ``trans[K, S, S]`` (zeros, and the likelihood that is not finite, without a path)."""
    logb = np.asarray(logb, dtype=np.float64)
    ls, lt, lx = (np.asarray(a, dtype=np.float64) for a in (ls, lt, lx))
    words = [int(w) for w in words]
    pen = np.float64(pen)
    T, K = logb.shape[0], len(words)
    W, S = ls.shape
    out = {"loglik": NEG, "gamma": np.zeros((T, K, S)), "start": np.zeros((K, S)), "trans": np.zeros((K, S, S))}
    if T == 0 or K == 0 or any(w < 0 or w >= W for w in words):
        return out
    LS, LT, LX = ls[words], lt[words], lx[words]
    B = logb[:, words, :]                                        # [T][K][S]
    with np.errstate(invalid="ignore", over="ignore"):
        alpha = np.full((T, K, S), NEG)
        X = np.full((T, K), NEG)
        alpha[0, 0] = LS[0] + B[0, 0]
        X[0] = _lse(alpha[0] + LX, 1)
        for t in range(1, T):
            within = _lse(alpha[t - 1][:, :, None] + LT, 1)      # [k][j]
            entry = np.full((K, S), NEG)
            entry[1:] = (X[t - 1, :-1, None] + pen) + LS[1:]
            alpha[t] = np.logaddexp(within, entry) + B[t]
            X[t] = _lse(alpha[t] + LX, 1)
        ll = X[T - 1, K - 1]
        out["loglik"] = float(ll)
        if not np.isfinite(ll):
            return out
        beta = np.full((T, K, S), NEG)
        beta[T - 1, K - 1] = LX[K - 1]
        for t in range(T - 2, -1, -1):
            c = B[t + 1] + beta[t + 1]
            E = np.full(K + 1, NEG)
            E[1:K] = pen + _lse(LS[1:] + c[1:], 1)
            beta[t] = np.logaddexp(_lse(LT + c[:, None, :], 2), LX + E[1:, None])
        out["gamma"] = np.exp(alpha + beta - ll)
        c = B[1:] + beta[1:]                                     # [T-1][K][S]
        out["trans"] = np.exp(alpha[:-1, :, :, None] + LT[None] + c[:, :, None, :] - ll).sum(axis=0)
        start = np.zeros((K, S))
        start[0] = out["gamma"][0, 0]
        start[1:] += np.exp((X[:-1, :-1, None] + pen) + LS[None, 1:] + c[:, 1:] - ll).sum(axis=0)
        out["start"] = start
    return out


def estep_batch(logb, lengths, transcripts, ls, lt, lx, pen=0.0, feats=None, max_words=None):
    """A packed batch ``logb[total_frames, W, S]`` (and ``feats[total_frames, D]``): a dict with ``loglik[N]``,
    ``post[total_frames, max_words, S]`` and the per-word ``nobs[W]``, ``start[W, S]``, ``trans[W, S, S]``,
    ``post_sum[W, S]``, ``obs[W, S, D]``, ``obs2[W, S, D]``.  ``max_words``: transcripts longer than this have no path
    (what a call sized for fewer words answers); by default the longest transcript."""
    ls = np.asarray(ls, dtype=np.float64)
    W, S = ls.shape
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.r_[0, np.cumsum(lengths)]
    if max_words is None:
        max_words = max([len(t) for t in transcripts] + [1])
    D = 0 if feats is None else int(np.shape(feats)[1])
    x32 = np.zeros((int(offs[-1]), 0), np.float32) if feats is None else np.asarray(feats, dtype=np.float32)
    x, x2 = x32.astype(np.float64), (x32 * x32).astype(np.float64)   # (the float32 square, as hmmlearn evaluates X**2)
    res = {"loglik": np.full(len(lengths), NEG), "post": np.zeros((int(offs[-1]), max_words, S)),
           "nobs": np.zeros(W), "start": np.zeros((W, S)), "trans": np.zeros((W, S, S)), "post_sum": np.zeros((W, S)),
           "obs": np.zeros((W, S, D)), "obs2": np.zeros((W, S, D))}
    for u, (a, b, words) in enumerate(zip(offs[:-1], offs[1:], transcripts)):
        if len(words) > max_words:
            continue
        r = forward_backward(logb[a:b], words, ls, lt, lx, pen)
        res["loglik"][u] = r["loglik"]
        if not np.isfinite(r["loglik"]):
            continue
        g = r["gamma"]
        res["post"][a:b, :len(words)] = g
        for k, w in enumerate(words):
            res["nobs"][w] += 1
            res["start"][w] += r["start"][k]
            res["trans"][w] += r["trans"][k]
            res["post_sum"][w] += g[:, k].sum(axis=0)
            res["obs"][w] += g[:, k].T @ x[a:b]
            res["obs2"][w] += g[:, k].T @ x2[a:b]
    return res


def brute(logb, words, ls, lt, lx, pen=0.0):
    """``loglik``, ``gamma``, ``start`` and ``trans`` of one utterance by enumerating EVERY path of the chain (tiny
    cases only): each complete path adds its probability to what it passes through."""
    logb = np.asarray(logb, dtype=np.float64)
    words = [int(w) for w in words]
    T, K, S = logb.shape[0], len(words), ls.shape[1]
    paths = []                                                   # (log score, [(k, s)] * T)

    def walk(t, k, s, acc, trail):
        if acc == NEG:
            return
        w = words[k]
        if t == T - 1:
            if k == K - 1 and lx[w, s] > NEG:
                paths.append((acc + lx[w, s], trail))
            return
        for s2 in range(S):
            walk(t + 1, k, s2, (acc + lt[w, s, s2]) + logb[t + 1, w, s2], trail + [(k, s2)])
            if k + 1 < K:
                w2 = words[k + 1]
                walk(t + 1, k + 1, s2, (((acc + lx[w, s]) + pen) + ls[w2, s2]) + logb[t + 1, w2, s2],
                     trail + [(k + 1, s2)])

    if T and K:
        for s in range(S):
            walk(0, 0, s, ls[words[0], s] + logb[0, words[0], s], [(0, s)])
    out = {"loglik": NEG, "gamma": np.zeros((T, K, S)), "start": np.zeros((K, S)), "trans": np.zeros((K, S, S))}
    if not paths:
        return out
    scores = np.array([p[0] for p in paths])
    ll = scores.max() + np.log(np.exp(scores - scores.max()).sum())
    out["loglik"] = float(ll)
    for sc, trail in paths:
        p = np.exp(sc - ll)
        for t, (k, s) in enumerate(trail):
            out["gamma"][t, k, s] += p
            if t == 0 or trail[t - 1][0] != k:
                out["start"][k, s] += p
            else:
                out["trans"][k, trail[t - 1][1], s] += p
    return out


# ---- the EM loop on the host -------------------------------------------------------------------------------------
_TINY = np.finfo(float).tiny


def tables(models, exit_states="last"):
    """``(log_start, log_trans, log_exit, means, vars, gconst)`` of "diag" / "spherical" models that share S and D:
    what ``ConnectedNetwork.from_models`` reads."""
    W = len(models)
    S, D = np.asarray(models[0].means_).shape
    ls, lt, lx = np.full((W, S), NEG), np.full((W, S, S), NEG), np.full((W, S), NEG)
    means, vars_, gconst = np.zeros((W, S, D)), np.ones((W, S, D)), np.zeros((W, S))
    with np.errstate(divide="ignore"):
        for w, m in enumerate(models):
            cv = np.asarray(m._covars_, dtype=np.float64)
            cv = np.broadcast_to(cv[:, None], (S, D)) if cv.ndim == 1 else cv
            ls[w] = np.log(np.asarray(m.startprob_, dtype=np.float64))
            lt[w] = np.log(np.asarray(m.transmat_, dtype=np.float64))
            means[w] = m.means_
            vars_[w] = np.maximum(cv, _TINY)
            gconst[w] = D * np.log(2 * np.pi) + np.log(vars_[w]).sum(axis=-1)
    if exit_states == "last":
        lx[:, S - 1] = 0.0
    else:
        lx[:] = 0.0
    return ls, lt, lx, means, vars_, gconst


def emit_diag(feats, means, vars_, gconst):
    x = np.asarray(feats, dtype=np.float64)[:, None, None, :]
    return -0.5 * (gconst[None] + ((x - means[None]) ** 2 / vars_[None]).sum(axis=-1))


def fit(models, features, transcripts, n_iter=10, tol=1e-2, exit_states="last", word_penalty=0.0):
    """Embedded Baum-Welch on the host over copies of ``models`` ("diag" / "spherical" ``GaussianHMM`` objects that
    share S and D); ``features``: frame-major ``(T, D)`` arrays.  Per iteration: the tables of the current models, the
    emission, :func:`estep_batch`, ``hmmlearn_hmm.m_step_typed`` per word that occurred, then the sum of the
    log-likelihoods of the utterances with a path goes to one ``ConvergenceMonitor``.  Returns ``(models, history)``."""
    from sapr_amd.hmmlearn_hmm import ConvergenceMonitor, m_step_typed
    models = [copy.deepcopy(m) for m in models]
    feats = [np.asarray(f, dtype=np.float32) for f in features]
    lengths = [len(f) for f in feats]
    x = np.concatenate(feats)
    monitor = ConvergenceMonitor(tol, n_iter)
    for _ in range(n_iter):
        ls, lt, lx, means, vars_, gconst = tables(models, exit_states)
        logb = emit_diag(x.astype(np.float64), means, vars_, gconst)
        r = estep_batch(logb, lengths, transcripts, ls, lt, lx, word_penalty, feats=x)
        for w, m in enumerate(models):
            if r["nobs"][w] == 0:
                continue
            st = {"nobs": r["nobs"][w], "start": r["start"][w], "trans": r["trans"][w], "post": r["post_sum"][w],
                  "obs": r["obs"][w], "obs**2": r["obs2"][w]}
            m.startprob_, m.transmat_, m.means_, m._covars_ = m_step_typed(
                st, m.covariance_type, m.startprob_, m.transmat_, m.params, m.startprob_prior, m.transmat_prior,
                m.means_prior, m.means_weight, m.covars_prior, m.covars_weight, np.asarray(m.means_, dtype=np.float64),
                np.asarray(m._covars_, dtype=np.float64))
        ll = r["loglik"]
        monitor.report(float(ll[np.isfinite(ll)].sum()))
        if monitor.converged:
            break
    return models, list(monitor.history)

"""CPU restatement of forward-backward over the word loop under a word-pair language model (plain numpy, float64,
``np.logaddexp``): THE DEFINITION of what ``sapr_connected_posteriors`` computes (include/sapr_hip.h).  The conventions
are those of ``tests/_bigram_ref.py``, of which this is the soft counterpart: the sum over every word string the
language model allows where that one takes the maximum.

With ``b_t(w,s) = logb[t][w][s]`` and ``lse`` the log-sum-exp::

    alpha_0(w,j)  = (lm_start[w] + log_start[w][j]) + b_0(w,j)
    X_t(v)        = lse_s (alpha_t(v,s) + log_exit[v][s])
    N_t(w)        = lse_v (X_t(v) + lm[v][w])
    alpha_t(w,j)  = lse( lse_i (alpha_{t-1}(w,i) + log_trans[w][i][j]),  N_{t-1}(w) + log_start[w][j] ) + b_t(w,j)
    loglik        = lse_v (X_{T-1}(v) + lm_end[v])

    beta_{T-1}(v,s) = log_exit[v][s] + lm_end[v]
    E_t(w)        = lse_j (log_start[w][j] + b_t(w,j) + beta_t(w,j))
    F_t(v)        = lse_w (lm[v][w] + E_t(w))
    beta_t(v,i)   = lse( lse_j (log_trans[v][i][j] + b_{t+1}(v,j) + beta_{t+1}(v,j)),  log_exit[v][i] + F_{t+1}(v) )

    post_t(w,s)    = exp(alpha_t(w,s) + beta_t(w,s) - loglik)
    word_post_t(w) = sum_s post_t(w,s)                       s ascending
    entry_post_0(w) = word_post_0(w)
    entry_post_t(w) = exp(N_{t-1}(w) + E_t(w) - loglik)      t >= 1: "a word w begins at frame t"

A step inside a word and a step that leaves the word and enters the same word again (``lm[w][w]``) are different
paths; both count.  An utterance without frames has the likelihood -inf; where the likelihood is not finite (-inf: no
path; NaN: a NaN was met) the posterior rows are exact zeros.  :func:`brute` enumerates every (word, state,
boundary-flag) sequence of a tiny case and is what the recursions are checked against.
"""
import itertools

import numpy as np

NEG = -np.inf


def _lse(a, axis):
    return np.logaddexp.reduce(a, axis=axis)


def forward_backward(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end):
    """One utterance: ``logb[T, W, S]`` -> a dict with ``loglik``, ``post[T, W, S]``, ``word_post[T, W]``,
    ``entry_post[T, W]`` (and the lattices ``alpha``, ``beta``, ``N``)."""
    logb = np.asarray(logb, dtype=np.float64)
    ls, lt, lx = (np.asarray(a, dtype=np.float64) for a in (log_start, log_trans, log_exit))
    lm, lm0, lm1 = (np.asarray(a, dtype=np.float64) for a in (lm, lm_start, lm_end))
    W, S = ls.shape
    if lm.shape != (W, W) or lm0.shape != (W,) or lm1.shape != (W,):
        raise ValueError("lm must be [W, W], lm_start and lm_end [W]")
    T = logb.shape[0]
    out = {"loglik": NEG, "post": np.zeros((T, W, S)), "word_post": np.zeros((T, W)), "entry_post": np.zeros((T, W)),
           "alpha": np.full((T, W, S), NEG), "beta": np.full((T, W, S), NEG), "N": np.full((T, W), NEG)}
    if T == 0:
        return out
    alpha, beta, N = out["alpha"], out["beta"], out["N"]
    X = np.full((T, W), NEG)
    E = np.full((T, W), NEG)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            if t == 0:
                alpha[0] = (lm0[:, None] + ls) + logb[0]
            else:
                within = _lse(alpha[t - 1][:, :, None] + lt, 1)            # [w][j]
                alpha[t] = np.logaddexp(within, N[t - 1][:, None] + ls) + logb[t]
            X[t] = _lse(alpha[t] + lx, 1)
            N[t] = _lse(X[t][:, None] + lm, 0)                             # over the predecessor words v
        ll = _lse(X[T - 1] + lm1, 0)
        out["loglik"] = float(ll)
        if not np.isfinite(ll):
            return out
        beta[T - 1] = lx + lm1[:, None]
        for t in range(T - 2, -1, -1):
            c = logb[t + 1] + beta[t + 1]
            E[t + 1] = _lse(ls + c, 1)
            F = _lse(lm + E[t + 1][None, :], 1)                            # over the successor words w
            beta[t] = np.logaddexp(_lse(lt + c[:, None, :], 2), lx + F[:, None])
        post = np.exp(alpha + beta - ll)
        word_post = np.zeros((T, W))
        for s in range(S):                                                 # s ascending
            word_post += post[:, :, s]
        entry = np.zeros((T, W))
        entry[0] = word_post[0]
        entry[1:] = np.exp(N[:-1] + E[1:] - ll)
    out["post"], out["word_post"], out["entry_post"] = post, word_post, entry
    return out


def posteriors_batch(logb, lengths, log_start, log_trans, log_exit, lm, lm_start, lm_end):
    """A packed batch ``logb[total_frames, W, S]``: ``(loglik[N], word_post[total, W], entry_post[total, W],
    post[total, W, S])``."""
    logb = np.asarray(logb, dtype=np.float64)
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    W, S = np.shape(log_start)
    ll = np.full(len(lengths), NEG)
    wp = np.zeros((int(offs[-1]), W))
    ep = np.zeros((int(offs[-1]), W))
    post = np.zeros((int(offs[-1]), W, S))
    for u, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        r = forward_backward(logb[a:b], log_start, log_trans, log_exit, lm, lm_start, lm_end)
        ll[u], wp[a:b], ep[a:b], post[a:b] = r["loglik"], r["word_post"], r["entry_post"], r["post"]
    return ll, wp, ep, post


def brute(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end):
    """Every path of a tiny case by enumeration: a path is a (word, state) per frame and, from frame 1 on, a flag
    "a word begins here" — a step inside a word and a step out of the word and into the same word again are two
    paths.  Returns ``(loglik, post[T, W, S], entry_post[T, W])`` from the paths' own totals."""
    logb = np.asarray(logb, dtype=np.float64)
    ls, lt, lx = (np.asarray(a, dtype=np.float64) for a in (log_start, log_trans, log_exit))
    lm, lm0, lm1 = (np.asarray(a, dtype=np.float64) for a in (lm, lm_start, lm_end))
    T = logb.shape[0]
    W, S = ls.shape
    cells = list(itertools.product(range(W), range(S)))
    totals, paths = [], []
    for seq in itertools.product(cells, repeat=T):
        for flags in itertools.product((0, 1), repeat=T - 1):
            w, s = seq[0]
            acc = lm0[w] + ls[w, s] + logb[0, w, s]
            for t in range(1, T):
                (v, i), (w, s) = seq[t - 1], seq[t]
                if flags[t - 1]:
                    acc = acc + lx[v, i] + lm[v, w] + ls[w, s]
                elif v == w:
                    acc = acc + lt[w, i, s]
                else:
                    acc = NEG
                acc = acc + logb[t, w, s]
                if acc == NEG:
                    break
            else:
                w, s = seq[T - 1]
                acc = acc + lx[w, s] + lm1[w]
            if acc > NEG:
                totals.append(acc)
                paths.append((seq, (1,) + flags))
    post = np.zeros((T, W, S))
    entry = np.zeros((T, W))
    if not totals:
        return NEG, post, entry
    totals = np.asarray(totals)
    m = totals.max()
    ll = float(m + np.log(np.exp(totals - m).sum()))
    for p, (seq, flags) in zip(np.exp(totals - ll), paths):
        for t, ((w, s), f) in enumerate(zip(seq, flags)):
            post[t, w, s] += p
            if f:
                entry[t, w] += p
    return ll, post, entry

"""Forward-backward of a diagonal-Gaussian HMM in np.longdouble (x87 80-bit: eps 1.08e-19), written from the textbook
definitions (Rabiner 1989, section III) as the reference of tests/test_fb_regimes_*.py.

    log b_t(s)   = -1/2 (D log 2 pi + sum_d log var[s,d] + sum_d (x[t,d] - mu[s,d])^2 / var[s,d])
    alpha_0      = log pi + log b_0;   alpha_t(j) = logsumexp_i(alpha_{t-1}(i) + log a_ij) + log b_t(j)
    beta_{T-1}   = 0;                  beta_t(i)  = logsumexp_j(log a_ij + log b_{t+1}(j) + beta_{t+1}(j))
    log P(x)     = logsumexp_s alpha_{T-1}(s)
    gamma_t      = softmax_s(alpha_t + beta_t)
    xi_t(i, j)   = softmax_{ij}(alpha_t(i) + log a_ij + log b_{t+1}(j) + beta_{t+1}(j))

gamma_t and xi_t are normalised per frame (both sum to one by definition) and not by subtracting log P(x): at
|log P(x)| = 1e9 the rounding of that subtraction alone would cost nine of the nineteen digits.  logsumexp returns its
maximum when that is infinite (or NaN), so an unreachable state stays at -inf and its posterior is exp(-inf) = 0 exactly.

Per utterance: ``start`` = gamma_0, ``trans`` = sum_t xi_t (zero for a one-frame sequence), ``post`` = sum_t gamma_t,
``obs`` = gamma^T X, ``obs2`` = gamma^T (X * X rounded to float32 first: hmmlearn squares the float32 array before the
product promotes it, oracle/hmmlearn_oracle.accumulate).

Results are cached per case (functools.lru_cache on the case object, which tests/_fb_regimes.py caches in turn) and
read-only."""
import functools

import numpy as np

from oracle import hmmlearn_oracle as ho

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))


def _log(x):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(x, dtype=LD))


def log_density(X, mu, cv):
    """(T, D) features, (S, D) means and variances -> (T, S) longdouble."""
    X, mu, cv = np.asarray(X, dtype=LD), np.asarray(mu, dtype=LD), np.asarray(cv, dtype=LD)
    with np.errstate(over="ignore", invalid="ignore"):
        quad = ((X[:, None, :] - mu[None]) ** 2 / cv[None]).sum(axis=-1)
    return LD(-0.5) * (mu.shape[1] * np.log(2 * PI) + np.log(cv).sum(axis=-1)[None] + quad)


def logsumexp(v, axis=-1):
    """max + log sum exp(v - max); the maximum itself where it is infinite (or NaN)."""
    v = np.asarray(v, dtype=LD)
    m = np.max(v, axis=axis, keepdims=True)
    safe = np.where(np.isfinite(m), m, LD(0))
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        r = np.log(np.sum(np.exp(v - safe), axis=axis, keepdims=True)) + safe
    return np.squeeze(np.where(np.isfinite(m), r, m), axis=axis)


def forward(sp, A, logB):
    ls, lA = _log(sp), _log(A)
    fwd = np.empty(logB.shape, dtype=LD)
    with np.errstate(invalid="ignore"):
        fwd[0] = ls + logB[0]
        for t in range(1, logB.shape[0]):
            fwd[t] = logsumexp(fwd[t - 1][:, None] + lA, axis=0) + logB[t]
    return logsumexp(fwd[-1]), fwd


def backward(A, logB):
    lA = _log(A)
    bwd = np.zeros(logB.shape, dtype=LD)
    with np.errstate(invalid="ignore"):
        for t in range(logB.shape[0] - 2, -1, -1):
            bwd[t] = logsumexp(lA + (logB[t + 1] + bwd[t + 1])[None, :], axis=1)
    return bwd


def _softmax(lg, axes):
    m = np.max(lg, axis=axes, keepdims=True)
    with np.errstate(invalid="ignore", under="ignore"):
        e = np.exp(lg - m)          # an infinite or NaN maximum gives NaN rows: nothing is repaired
        return e / e.sum(axis=axes, keepdims=True)


def bidiag_gaps(sp, A, fwd):
    """|a - b| of the two candidates alpha_{t-1}(j) + log a_jj and alpha_{t-1}(j-1) + log a_{j-1,j} of every forward
    step of a bidiagonal model, wherever both are finite."""
    lA = _log(A)
    S = lA.shape[0]
    idx = np.arange(1, S)
    with np.errstate(invalid="ignore"):
        a = fwd[:-1, 1:] + lA[idx, idx][None]
        b = fwd[:-1, :-1] + lA[idx - 1, idx][None]
    both = np.isfinite(a) & np.isfinite(b)
    return np.abs(a[both] - b[both])


def utterance(X, sp, A, mu, cv):
    """Every reference quantity of one (utterance, model) pair, longdouble."""
    logB = log_density(X, mu, cv)
    ll, fwd = forward(sp, A, logB)
    bwd = backward(A, logB)
    with np.errstate(invalid="ignore"):
        post = _softmax(fwd + bwd, 1)
    S = logB.shape[1]
    if X.shape[0] > 1:
        with np.errstate(invalid="ignore"):
            lx = fwd[:-1, :, None] + _log(A)[None] + (logB[1:] + bwd[1:])[:, None, :]
        trans = _softmax(lx, (1, 2)).sum(axis=0)
    else:
        trans = np.zeros((S, S), dtype=LD)
    X32 = np.asarray(X, dtype=np.float32)
    return {"ll": ll, "fwd": fwd, "gamma": post, "start": post[0], "trans": trans, "post": post.sum(axis=0),
            "obs": post.T @ X32.astype(LD), "obs2": post.T @ (X32 * X32).astype(LD)}


def loglik(X, sp, A, mu, cv):
    return forward(sp, A, log_density(X, mu, cv))[0]


STAT_KEYS = ("start", "trans", "post", "obs", "obs2")


class Result:
    """ll[N] (own model), scores[N, W], gamma[total_frames, S], path, per-word statistics, gaps; see reference()."""


def _freeze(r):
    for v in vars(r).values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return r


def _finish(r, case, per_utt):
    r.ll = np.asarray([p["ll"] for p in per_utt])
    r.gamma = np.concatenate([p["gamma"] for p in per_utt], axis=0)
    r.offs = np.r_[0, np.cumsum([X.shape[0] for X in case.utts])]
    with np.errstate(invalid="ignore"):
        r.path = np.argmax(r.gamma, axis=1)
        top = np.sort(r.gamma, axis=1)
        r.top_gap = top[:, -1] - top[:, -2]
        r.top = top[:, -1]
    r.stats = []
    for w in range(case.W):
        mine = [p for u, p in enumerate(per_utt) if case.utt_model[u] == w]
        S, D = case.mu.shape[1:]
        zero = {"start": (S,), "trans": (S, S), "post": (S,), "obs": (S, D), "obs2": (S, D)}
        st = {k: sum((p[k] for p in mine), np.zeros(zero[k], dtype=r.ll.dtype)) for k in STAT_KEYS}
        st["logprob"] = sum((p["ll"] for p in mine), r.ll.dtype.type(0))
        st["nobs"] = len(mine)
        r.stats.append(st)
    return _freeze(r)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The longdouble reference of a case of tests/_fb_regimes.py: every utterance under its own model (all
    quantities) and under every other model (log-likelihood only)."""
    r = Result()
    per_utt, gaps = [], []
    r.scores = np.empty((len(case.utts), case.W), dtype=LD)
    for u, X in enumerate(case.utts):
        w = case.utt_model[u]
        p = utterance(X, case.sp[w], case.A[w], case.mu[w], case.cv[w])
        fwd = p.pop("fwd")
        if case.bidiag:
            gaps.append(bidiag_gaps(case.sp[w], case.A[w], fwd))
        per_utt.append(p)
        for v in range(case.W):
            r.scores[u, v] = p["ll"] if v == w else loglik(X, case.sp[v], case.A[v], case.mu[v], case.cv[v])
    r.gaps = np.concatenate(gaps) if gaps else np.zeros(0, dtype=LD)
    return _finish(r, case, per_utt)


@functools.lru_cache(maxsize=None)
def float64_oracle(case):
    """The same quantities from oracle/hmmlearn_oracle.py (float64 numpy restatement of hmmlearn): what the existing
    GPU tests compare the kernels with.  Its deviation from reference() is E_ref."""
    r = Result()
    per_utt = []
    r.scores = np.empty((len(case.utts), case.W))
    for u, X in enumerate(case.utts):
        w = case.utt_model[u]
        sp, A, mu, cv = case.sp[w], case.A[w], case.mu[w], case.cv[w]
        logB = ho.log_density_diag(X, mu, cv)
        lp, fwd = ho.forward_log(sp, A, logB)
        bwd = ho.backward_log(sp, A, logB)
        post = ho.posteriors(fwd, bwd)
        st = ho.new_stats(*mu.shape)
        st["start"] += post[0]
        if X.shape[0] > 1:
            with np.errstate(under="ignore"):
                st["trans"] += np.exp(ho.log_xi_sum(fwd, A, bwd, logB))
        st["post"] += post.sum(axis=0)
        st["obs"] += post.T @ X
        st["obs2"] += post.T @ (X ** 2)
        per_utt.append({"ll": lp, "gamma": post, **{k: st[k] for k in STAT_KEYS}})
        for v in range(case.W):
            r.scores[u, v] = lp if v == w else ho.forward_log(
                case.sp[v], case.A[v], ho.log_density_diag(X, case.mu[v], case.cv[v]))[0]
    return _finish(r, case, per_utt)


def rel_err(x, ref):
    """max |x - ref| / |ref|: the measure of the rtol 1e-11 pin on log-likelihoods."""
    x, ref = np.asarray(x, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(x - ref) / np.abs(ref))) if ref.size else 0.0


def scaled_err(x, ref):
    """max |x - ref| / (1 + |ref|): at most 1e-9 exactly when assert_allclose(rtol=1e-9, atol=1e-9) passes."""
    x, ref = np.asarray(x, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(x - ref) / (1 + np.abs(ref)))) if ref.size else 0.0


@functools.lru_cache(maxsize=None)
def e_ref(case):
    """Deviation of the float64 oracle from the longdouble reference on the case's inputs, per compared quantity."""
    ref, o64 = reference(case), float64_oracle(case)
    e = {"ll": rel_err(o64.scores, ref.scores), "gamma": scaled_err(o64.gamma, ref.gamma),
         "logprob": max(rel_err(o64.stats[w]["logprob"], ref.stats[w]["logprob"]) for w in range(case.W)
                        if ref.stats[w]["nobs"])}
    for k in STAT_KEYS:
        e[k] = max(scaled_err(o64.stats[w][k], ref.stats[w][k]) for w in range(case.W))
    return e

"""Sampled connected-word cases for the mixture and the full-covariance emission families, with their numpy
references: the generators follow ``tests/_connected_ref.sample_case`` (left-to-right words, utterances of 1-5 words,
every state held for 1-4 frames, float32 features), the recursion is ``tests/_connected_ref`` (the definition), the
emissions are ``tests/_gmmhmm_ref.log_components`` + ``_lse`` and ``tests/_fullcov_ref.log_density``.

* mixtures: component means = state mean N(0, 20^2) + N(0, 8^2), variances U(4, 36), weights Dirichlet(5); a frame is
  drawn from a component chosen by the weights;
* full: Sigma = A A^T (20 / D) + 4 I with A standard normal; odd words are tied (one matrix for all their states);
  ``kinds`` names other covariance types per word ("diag": a diagonal matrix with entries U(4, 36), "spherical": one
  variance per state).

Variances and eigenvalues are >= 4, so every log-density term is negative and nothing cancels.  The committed case
lists are below; ``tests/test_connected_families_cpu.py`` checks the margins that let the GPU tests demand equal
paths.  References are computed once per (case, penalty) and shared (``functools.lru_cache``): do not write into them.
"""
import functools

import numpy as np

from tests import _connected_ref as ref
from tests import _fullcov_ref as fref
from tests import _gmmhmm_ref as gref


def _topology(rng, W, S):
    stay = rng.uniform(0.3, 0.7, (W, S))
    transmat = np.zeros((W, S, S))
    for s in range(S):
        if s + 1 < S:
            transmat[:, s, s], transmat[:, s, s + 1] = stay[:, s], 1.0 - stay[:, s]
        else:
            transmat[:, s, s] = 1.0
    startprob = np.zeros((W, S))
    startprob[:, 0] = 1.0
    with np.errstate(divide="ignore"):
        log_start, log_trans = np.log(startprob), np.log(transmat)
    return dict(startprob=startprob, transmat=transmat, log_start=log_start, log_trans=log_trans)


def log_exit(W, S, exit_states="last"):
    lx = np.full((W, S), -np.inf)
    if exit_states == "last":
        lx[:, S - 1] = 0.0
    else:
        lx[:] = 0.0
    return lx


def _utterances(rng, W, S, n_utts, draw):
    utts, truth = [], []
    for _ in range(n_utts):
        words = rng.integers(0, W, int(rng.integers(1, 6))).tolist()
        rows = []
        for w in words:
            for s in range(S):
                rows.append(draw(w, s, int(rng.integers(1, 5))))
        utts.append(np.concatenate(rows).astype(np.float32))
        truth.append(words)
    return utts, truth


@functools.lru_cache(maxsize=None)
def gmm_case(seed, W, S, M, D, n_utts):
    """``(model, utterances, truth)``: ``model`` holds startprob[W,S], transmat[W,S,S], weights[W,S,M],
    means[W,S,M,D], covars[W,S,M,D] and log_start / log_trans / log_exit ("last")."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, 20.0, (W, S, 1, D)) + rng.normal(0.0, 8.0, (W, S, M, D))
    covars = rng.uniform(4.0, 36.0, (W, S, M, D))
    weights = rng.dirichlet(np.full(M, 5.0), (W, S))
    model = dict(_topology(rng, W, S), weights=weights, means=means, covars=covars, log_exit=log_exit(W, S))

    def draw(w, s, n):
        m = rng.choice(M, size=n, p=weights[w, s])
        return rng.normal(means[w, s, m], np.sqrt(covars[w, s, m]))

    utts, truth = _utterances(rng, W, S, n_utts, draw)
    return model, utts, truth


@functools.lru_cache(maxsize=None)
def full_case(seed, W, S, D, n_utts, kinds=None):
    """``(model, utterances, truth)``: ``model`` holds startprob, transmat, means[W,S,D], covars[W,S,D,D], ``kinds``
    (the covariance type of every word) and log_start / log_trans / log_exit ("last")."""
    rng = np.random.default_rng(seed)
    kinds = tuple("tied" if w % 2 else "full" for w in range(W)) if kinds is None else tuple(kinds)
    means = rng.normal(0.0, 20.0, (W, S, D))
    covars = np.empty((W, S, D, D))
    for w in range(W):
        for s in range(S):
            if kinds[w] in ("full", "tied"):
                A = rng.normal(size=(D, D))
                covars[w, s] = A @ A.T * (20.0 / D) + 4.0 * np.eye(D)
            elif kinds[w] == "diag":
                covars[w, s] = np.diag(rng.uniform(4.0, 36.0, D))
            else:
                covars[w, s] = np.eye(D) * rng.uniform(4.0, 36.0)
        if kinds[w] == "tied":
            covars[w] = covars[w, 0]
    chol = np.linalg.cholesky(covars)
    model = dict(_topology(rng, W, S), means=means, covars=covars, kinds=kinds, log_exit=log_exit(W, S))

    def draw(w, s, n):
        return means[w, s] + rng.normal(size=(n, D)) @ chol[w, s].T

    utts, truth = _utterances(rng, W, S, n_utts, draw)
    return model, utts, truth


# the committed cases: (seed, W, S, M, D, utterances) and (seed, W, S, D, utterances); every SP, MP and DP instantiation
GMM_CASES = [(201, 3, 4, 2, 5, 16), (202, 11, 10, 2, 13, 12), (203, 5, 7, 3, 26, 12), (204, 6, 18, 8, 39, 6),
             (205, 4, 5, 1, 13, 12)]
FULL_CASES = [(211, 3, 4, 5, 16), (212, 11, 10, 13, 12), (213, 5, 7, 26, 12), (214, 6, 18, 39, 6)]
# Decoder.decode_connected (also run with a word penalty of -30): GMMHMM pickles; diag + spherical + tied + full
GMM_DECODER_CASE = (206, 4, 5, 2, 13, 10)
FULL_DECODER_CASE = (215, 4, 5, 13, 10)
FULL_DECODER_KINDS = ("diag", "spherical", "tied", "full")
# emission parity only: the smallest shapes
GMM_TINY = (207, 2, 1, 4, 1, 4)
FULL_TINY = (216, 2, 1, 1, 4)


def case(family, spec):
    """``(model, utterances, truth)`` of a committed case of either family."""
    if family == "gmm":
        return gmm_case(*spec)
    return full_case(*spec, kinds=FULL_DECODER_KINDS if spec == FULL_DECODER_CASE else None)


def emission(family, model, x):
    """The numpy reference ``logb[T, W, S]`` of frames ``x[T, D]``."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    W = model["means"].shape[0]
    if family == "gmm":
        rows = [gref._lse(gref.log_components(x, model["weights"][w], model["means"][w], model["covars"][w]), axis=-1)
                for w in range(W)]
    else:
        rows = [fref.log_density(x, model["means"][w], model["covars"][w]) for w in range(W)]
    return np.stack(rows, axis=1)


@functools.lru_cache(maxsize=None)
def case_logb(family, spec):
    """``(logb[total_frames, W, S], lengths)`` of a committed case's utterances."""
    model, utts, _ = case(family, spec)
    return emission(family, model, np.concatenate(utts)), tuple(len(x) for x in utts)


@functools.lru_cache(maxsize=None)
def reference(family, spec, pen=0.0, exit_states="last", order=None):
    """``_connected_ref.viterbi_batch`` of a committed case: ``(score, n_words, path_word, path_state, path_entry)``.
    ``order``: the words of the network in another order (a tuple of the case's word indices)."""
    model, _, _ = case(family, spec)
    logb, lengths = case_logb(family, spec)
    W, S = model["log_start"].shape
    idx = list(range(W)) if order is None else list(order)
    return ref.viterbi_batch(logb[:, idx], lengths, model["log_start"][idx], model["log_trans"][idx],
                             log_exit(W, S, exit_states), pen)


def models_of(family, model):
    """The case's words as fitted model objects: ``GMMHMM`` or ``GaussianHMM`` (of the word's covariance type)."""
    W, S = model["log_start"].shape
    out = []
    for w in range(W):
        if family == "gmm":
            from sapr_amd.gmm_hmm import GMMHMM
            m = GMMHMM(n_components=S, n_mix=model["weights"].shape[2])
            m.weights_, m.means_, m.covars_ = model["weights"][w], model["means"][w], model["covars"][w]
        else:
            from sapr_amd.hmmlearn_hmm import GaussianHMM
            kind = model["kinds"][w]
            m = GaussianHMM(n_components=S, covariance_type=kind)
            cv = model["covars"][w]
            m.means_ = model["means"][w]
            m._covars_ = {"full": lambda: cv.copy(), "tied": lambda: cv[0].copy(),
                          "diag": lambda: np.array([np.diag(c) for c in cv]),
                          "spherical": lambda: np.array([c[0, 0] for c in cv])}[kind]()
        m.startprob_, m.transmat_ = model["startprob"][w], model["transmat"][w]
        out.append(m)
    return out

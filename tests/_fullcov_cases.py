"""Seeded cases shared by the full-covariance tests: multi-modal synthetic words (every word's utterances are drawn
from TWO prototype sets), fixed model parameters from a time-slice initialisation of the means and the start covariance
``0.25 cov(all frames) + I`` (real off-diagonals), and the numpy reference results (tests/_fullcov_ref.py), computed
once per case and never modified.

The utterance counts are the smallest at which a full covariance per state stays well conditioned through three EM
iterations (clearly more than D frames per state); tests/test_fullcov_cpu.py asserts the conditions from the reference
alone."""
from __future__ import annotations

import functools

import numpy as np

from tests import _fullcov_ref as ref
from tests._synth import VOCAB, synth_utterance, word_prototypes

# name -> (D, S, transmat, words, utterances per word, tmin, tmax (exclusive), extra lengths appended to word 0, seed)
CASES = {
    "d13_s10_bidiag": (13, 10, "bidiag", 3, 14, 40, 90, (), 0),        # DP 13 / SP 10 unpadded; 1 Gram tile
    "d5_s3_dense": (5, 3, "dense", 3, 6, 12, 40, (1, 0), 0),           # padding in D and S; a 1-frame and a 0-frame utterance
    "d14_s5_dense": (14, 5, "dense", 1, 12, 12, 40, (), 0),            # smallest DP 26: one real row in the second tile
    "d26_s6_dense": (26, 6, "dense", 1, 24, 20, 50, (), 0),            # DP 26 full
    "d27_s11_bidiag": (27, 11, "bidiag", 1, 40, 30, 60, (), 0),        # smallest DP 39 / SP 18
    "d39_s18_bidiag": (39, 18, "bidiag", 1, 64, 40, 90, (), 0),        # largest instantiation; 6 Gram tiles
    "d5_s3_tiles": (5, 3, "dense", 1, 300, 12, 13, (), 0),             # two tiles and a part
}
EM_ITERS = 3


def time_slice_params(utts, S, topology, rng):
    """State s takes its mean from the s-th of S equal time slices of the word's utterances; every state starts from
    ``0.25 cov(all frames) + I``."""
    D = utts[0].shape[1]
    long = [x for x in utts if x.shape[0] >= S]
    means = np.empty((S, D))
    for s in range(S):
        fr = np.concatenate([x[x.shape[0] * s // S: x.shape[0] * (s + 1) // S] for x in long], axis=0)
        means[s] = fr.astype(np.float64).mean(axis=0)
    allf = np.concatenate(utts, axis=0).astype(np.float64)
    cv = 0.25 * np.cov(allf.T) + np.eye(D)
    cv = (cv + cv.T) / 2
    covars = np.tile(cv, (S, 1, 1))
    if topology == "bidiag":
        sp = np.zeros(S)
        sp[0] = 1.0
        A = np.zeros((S, S))
        stay = rng.uniform(0.7, 0.9, S)
        for i in range(S - 1):
            A[i, i], A[i, i + 1] = stay[i], 1 - stay[i]
        A[S - 1, S - 1] = 1.0
    else:
        sp = rng.dirichlet(np.full(S, 2.0))
        A = rng.dirichlet(np.full(S, 2.0), size=S)
    return sp, A, means, covars


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: D, S, utts (per word: list of [T, D] float32), params (per word: startprob, transmat, means, covars[S, D,
    D]), feats [N, D] float32 packed word after word, lengths, utt_model."""
    D, S, topo, n_words, n_per, tmin, tmax, extra, seed = CASES[name]
    rng = np.random.default_rng(2000 + seed)
    words = VOCAB[:n_words]
    protos = [word_prototypes(words, D, seed=seed + 11), word_prototypes(words, D, seed=seed + 77)]
    utts, params = [], []
    for w, word in enumerate(words):
        lst = []
        for _ in range(n_per):
            T = int(rng.integers(tmin, tmax))
            lst.append(np.ascontiguousarray(synth_utterance(rng, protos[int(rng.integers(2))][word], T).T))
        params.append(time_slice_params(lst, S, topo, rng))
        if w == 0:
            for T in extra:
                lst.append(np.ascontiguousarray(synth_utterance(rng, protos[0][word], max(T, 1)).T)[:T])
        utts.append(lst)
    flat = [x for lst in utts for x in lst]
    return {"D": D, "S": S, "utts": utts, "params": params, "feats": np.concatenate(flat, axis=0),
            "lengths": np.array([x.shape[0] for x in flat], dtype=np.int64),
            "utt_model": np.concatenate([np.full(len(lst), w) for w, lst in enumerate(utts)])}


@functools.lru_cache(maxsize=None)
def reference_estep(name):
    """(per-word statistics, per-utterance results in batch order) of tests/_fullcov_ref.py."""
    c = case(name)
    stats, res = [], []
    for utts, prm in zip(c["utts"], c["params"]):
        st, r = ref.estep(utts, *prm)
        stats.append(st)
        res += r
    return stats, res


@functools.lru_cache(maxsize=None)
def reference_viterbi(name):
    """Per utterance (logprob, path, gap); an utterance without frames: (-inf, empty, inf)."""
    c = case(name)
    out = []
    for utts, prm in zip(c["utts"], c["params"]):
        for x in utts:
            out.append(ref.viterbi(x, *prm) if x.shape[0] else (-np.inf, np.zeros(0, np.int64), np.inf))
    return out


def start_covars(prm, covariance_type):
    """The case's start covariance (S equal matrices) in the shape of the type's ``_covars_``."""
    cv = prm[3]
    if covariance_type == "full":
        return cv
    if covariance_type == "tied":
        return cv[0]
    if covariance_type == "diag":
        return np.array([np.diag(c) for c in cv])
    return np.array([np.diag(c).mean() for c in cv])


@functools.lru_cache(maxsize=None)
def reference_em(name, covariance_type, n_iter=EM_ITERS):
    """Per word (parameters, history, covariances after every iteration) of the fixed-parameter EM loop with hmmlearn's
    default priors."""
    c = case(name)
    return [ref.em(utts, prm[0], prm[1], prm[2], start_covars(prm, covariance_type), covariance_type, n_iter)
            for utts, prm in zip(c["utts"], c["params"])]

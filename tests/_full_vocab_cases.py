"""Seeded cases shared by the tests of the full-covariance vocabulary scoring (csrc/full_vocab.hip): the recipe of
tests/_fullcov_cases.case (multi-modal synthetic words, time-slice means, the start covariance ``0.25 cov(all frames) +
I`` with real off-diagonals) with several words per case, and the numpy reference (tests/_fullcov_ref.py looped over
the words), computed once per case and never modified.

The sizes are the smallest that run the padded instantiation named beside them; tests/test_full_vocab_cpu.py asserts
from the reference alone that no word and no path arg-max is close enough to a tie for the tolerance to flip it."""
from __future__ import annotations

import functools

import numpy as np

from tests import _fullcov_ref as ref
from tests._fullcov_cases import time_slice_params
from tests._synth import VOCAB, synth_utterance, word_prototypes

# name -> (D, S, transmat, words, utterances per word, tmin, tmax (exclusive), extra lengths appended to word 0, seed)
CASES = {
    "d13_s10_bidiag": (13, 10, "bidiag", 3, 8, 40, 90, (), 0),       # SP 10 / DP 13 unpadded; -inf transitions skipped
    "d5_s3_dense": (5, 3, "dense", 3, 6, 12, 40, (1, 0), 0),         # padding in S and D; a 1-frame and a 0-frame utterance
    "d14_s5_dense": (14, 5, "dense", 3, 6, 12, 40, (), 0),           # smallest DP 26
    "d26_s6_dense": (26, 6, "dense", 3, 6, 20, 50, (), 0),           # DP 26 full
    "d27_s11_bidiag": (27, 11, "bidiag", 3, 6, 30, 60, (), 0),       # smallest DP 39 / SP 18
    "d39_s18_bidiag": (39, 18, "bidiag", 3, 6, 40, 90, (), 0),       # largest instantiation
    "d13_s4_dense_300": (13, 4, "dense", 2, 150, 12, 14, (), 0),     # 300 utterances: two tiles, the second partial
    # the (SP, DP) pairs the cases above leave out: with them every full_vocab_kernel instantiation is run
    "d13_s11_bidiag": (13, 11, "bidiag", 3, 6, 30, 60, (), 0),       # SP 18 / DP 13
    "d14_s4_dense": (14, 4, "dense", 3, 6, 12, 40, (), 0),           # SP 4 / DP 26
    "d26_s11_bidiag": (26, 11, "bidiag", 3, 6, 30, 60, (), 0),       # SP 18 / DP 26
    "d27_s4_dense": (27, 4, "dense", 3, 6, 12, 40, (), 0),           # SP 4 / DP 39
    "d27_s10_bidiag": (27, 10, "bidiag", 3, 6, 30, 60, (), 0),       # SP 10 / DP 39
}
MODES = ("forward", "viterbi")


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: D, S, utts (per word: list of [T, D] float32), params (per word: startprob, transmat, means, covars[S, D,
    D]), feats [N, D] float32 packed word after word, lengths, flat (the utterances in batch order)."""
    D, S, topo, n_words, n_per, tmin, tmax, extra, seed = CASES[name]
    rng = np.random.default_rng(3000 + seed)
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
            "lengths": np.array([x.shape[0] for x in flat], dtype=np.int64), "flat": flat}


def ref_pair(x, prm, mode):
    """The reference's score of one utterance [T, D] float32 under one model ``(startprob, transmat, means,
    covars[S, D, D])``; no frames: -inf."""
    if x.shape[0] == 0:
        return -np.inf
    if mode == "viterbi":
        return ref.viterbi(x, *prm)[0]
    sp, A, mu, cv = prm
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    return ref.forward_backward(sp, A, ref.log_density(x64, mu, cv))[0]


def first_strict_max(scores):
    """decoder.py:42-47 on the rows of a score matrix: from -inf, first strict maximum in model order; -1 if none."""
    out = np.full(scores.shape[0], -1, dtype=np.int64)
    for u, row in enumerate(scores):
        best = -np.inf
        for w, sc in enumerate(row):
            if sc > best:
                best, out[u] = sc, w
    return out


def ref_scores(utts, params):
    """{mode: (score[N, W], best_word[N])} of the reference, looped over the words."""
    out = {}
    for mode in MODES:
        sc = np.array([[ref_pair(x, prm, mode) for prm in params] for x in utts], dtype=np.float64).reshape(
            len(utts), len(params))
        out[mode] = (sc, first_strict_max(sc))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return ref_scores(c["flat"], c["params"])


def two_state(prm):
    """A model cut to its first two states, start and transitions renormalised."""
    sp, A, mu, cv = prm
    return (sp[:2] / sp[:2].sum(), A[:2, :2] / A[:2, :2].sum(axis=1, keepdims=True), mu[:2], cv[:2])


# the two derived vocabularies over the utterances of d5_s3_dense; the seed is the first at which the conditions of
# tests/test_full_vocab_cpu.py hold (0 for both)
@functools.lru_cache(maxsize=None)
def mixed_size():
    """d5_s3_dense with model 1 cut to two states -> (params, reference)."""
    c = case("d5_s3_dense")
    params = [c["params"][0], two_state(c["params"][1]), c["params"][2]]
    return params, ref_scores(c["flat"], params)


MIXED_TYPES = ("full", "tied", "diag")


def typed_covars(prm, covariance_type):
    """The ``_covars_`` of a model of ``covariance_type`` made from a case's [S, D, D] start covariance: the matrices
    themselves, the first of them, or their diagonals."""
    cv = prm[3]
    if covariance_type == "full":
        return cv
    if covariance_type == "tied":
        return cv[0]
    return np.array([np.diag(c) for c in cv])


@functools.lru_cache(maxsize=None)
def mixed_type():
    """d5_s3_dense as {full, tied (= cv[0]), diag (= the diagonals)} -> (params with [S, D, D] covariances through
    ref.expand, reference)."""
    c = case("d5_s3_dense")
    S, D = c["S"], c["D"]
    params = [(p[0], p[1], p[2], ref.expand(typed_covars(p, ct), ct, S, D))
              for p, ct in zip(c["params"], MIXED_TYPES)]
    return params, ref_scores(c["flat"], params)


def winner_path_gap(utts, params, best_word):
    """Smallest relative arg-max gap (ref.viterbi's) on the Viterbi path of each utterance's winner."""
    gap = np.inf
    for x, w in zip(utts, best_word):
        if w >= 0 and x.shape[0]:
            gap = min(gap, ref.viterbi(x, *params[w])[2])
    return gap


def top_two_gap(scores):
    """Smallest distance between the best and the second-best score over the rows with finite scores."""
    rows = scores[np.all(np.isfinite(scores), axis=1)]
    s = np.sort(rows, axis=1)
    return float((s[:, -1] - s[:, -2]).min())

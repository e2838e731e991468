"""Seeded cases shared by the GMMHMM GPU tests: multi-modal synthetic words (every word's utterances are drawn from
TWO prototype sets), fixed model parameters from a time-slice initialisation, and the numpy reference results
(tests/_gmmhmm_ref.py), computed once per case and never modified."""
from __future__ import annotations

import functools

import numpy as np

from tests import _gmmhmm_ref as ref
from tests._synth import VOCAB, synth_utterance, word_prototypes

# name -> (D, S, M, transmat, utterances per word, tmin, tmax (exclusive), extra lengths appended to word 0, seed).
# The seeds were picked on the CPU so that the REFERENCE alone meets the tests' conditions on their inputs: every
# Viterbi arg-max gap above 1e-9, and at most one component in ten whose occupancy falls below 1e-6 within three EM
# iterations (none with these seeds).
CASES = {
    "d13_s10_m2_bidiag": (13, 10, 2, "bidiag", 14, 40, 90, (), 0),
    "d5_s3_m3_dense": (5, 3, 3, "dense", 6, 12, 40, (1, 0), 0),       # + an utterance of one frame and one of none
    "d39_s18_m2_bidiag": (39, 18, 2, "bidiag", 12, 40, 90, (), 2),
    "d13_s4_m8_dense": (13, 4, 8, "dense", 16, 40, 90, (), 0),
    "d26_s6_m1_dense": (26, 6, 1, "dense", 6, 12, 40, (), 0),
    "d5_s3_m3_tiles": (5, 3, 3, "dense", 0, 12, 13, (), 0),           # one word, 300 utterances: two tiles and a part
}
N_WORDS = 3


def time_slice_params(utts, S, M, topology, rng):
    """State s takes its M means from the s-th of S equal time slices of the word's utterances (component m from the
    utterances u = m mod M); the word's global variance everywhere; Dirichlet weights."""
    D = utts[0].shape[1]
    long = [x for x in utts if x.shape[0] >= S]
    means = np.empty((S, M, D))
    for s in range(S):
        for m in range(M):
            own = [x for i, x in enumerate(long) if i % M == m] or long
            fr = np.concatenate([x[x.shape[0] * s // S: x.shape[0] * (s + 1) // S] for x in own], axis=0)
            means[s, m] = fr.astype(np.float64).mean(axis=0)
    allf = np.concatenate(utts, axis=0).astype(np.float64)
    covars = np.tile(allf.var(axis=0) * 0.25 + 1.0, (S, M, 1))
    weights = rng.dirichlet(np.full(M, 5.0), size=S)
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
    return sp, A, weights, means, covars


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    """dict: D, S, M, utts (per word: list of [T, D] float32), params (per word), feats [N, D] float32 packed word
    after word, lengths, utt_model."""
    D, S, M, topo, n_per, tmin, tmax, extra, case_seed = CASES[name]
    seed = case_seed if seed is None else seed
    rng = np.random.default_rng(1000 + seed)
    if n_per == 0:
        words, n_per_word = VOCAB[:1], [300]
    else:
        words, n_per_word = VOCAB[:N_WORDS], [n_per] * N_WORDS
    protos = [word_prototypes(words, D, seed=seed + 11), word_prototypes(words, D, seed=seed + 77)]
    utts, params = [], []
    for w, word in enumerate(words):
        lst = []
        for _ in range(n_per_word[w]):
            T = int(rng.integers(tmin, tmax))
            lst.append(np.ascontiguousarray(synth_utterance(rng, protos[int(rng.integers(2))][word], T).T))
        params.append(time_slice_params(lst, S, M, topo, rng))
        if w == 0:
            for T in extra:
                lst.append(np.ascontiguousarray(synth_utterance(rng, protos[0][word], max(T, 1)).T)[:T])
        utts.append(lst)
    flat = [x for lst in utts for x in lst]
    return {"D": D, "S": S, "M": M, "utts": utts, "params": params,
            "feats": np.concatenate(flat, axis=0), "lengths": np.array([x.shape[0] for x in flat], dtype=np.int64),
            "utt_model": np.concatenate([np.full(len(lst), w) for w, lst in enumerate(utts)])}


@functools.lru_cache(maxsize=None)
def reference_estep(name):
    """(per-word statistics, per-utterance results in batch order) of tests/_gmmhmm_ref.py."""
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


@functools.lru_cache(maxsize=None)
def reference_em(name, n_iter=3):
    """Per word (parameters, history, occupancy per iteration) of the fixed-parameter EM loop."""
    c = case(name)
    return [ref.em(utts, *prm, n_iter=n_iter) for utts, prm in zip(c["utts"], c["params"])]

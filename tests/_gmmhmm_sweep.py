"""Seeded cases that run every padded instantiation of the GMMHMM kernels (csrc/gmm_hmm.hip, csrc/gmm_vocab.hip) and
the branches only some shapes reach, with the numpy reference results (tests/_gmmhmm_ref.py), computed once per case
and never modified.  Shared by tests/test_gmmhmm_shapes_cpu.py (the conditions on the inputs, from the reference alone)
and tests/test_gmmhmm_shapes_gpu.py.

A case is a dict like tests/_gmmhmm_cases.case's: D, S, M, utts (per word: list of [T, D] float32, possibly empty),
params (per word), feats [N, D] float32 in batch order, lengths, utt_model.  The batch order is word after word unless
the case carries its own ``order`` (the ragged batch is fed shuffled).

    sweep-NNN        72 cases: (S, M, D) = (SP, MP, DP) for the 36 triples ("tight"), then the smallest size every
                     padded width serves ("loose"); two words of five utterances, word 0 with utterances of 1, 2 and 0
                     frames after its own
    ragged-*         one word whose running frame counts land on and off the 64- and 256-frame boundaries, an
                     utterance of 1024 frames, a word with one frame and a word without utterances
    tiles            nine tiles of one model behind a one-tile model
    zero_weight ...  degenerate but valid models
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import _gmmhmm_ref as ref
from tests._gmmhmm_cases import time_slice_params
from tests._synth import VOCAB, synth_utterance, word_prototypes

MODES = ("forward", "viterbi")
SPS, MPS, DPS = (4, 10, 18), (1, 2, 4, 8), (13, 26, 39)
TIGHT = list(itertools.product(SPS, MPS, DPS))
LOOSE = list(itertools.product((1, 5, 11), (1, 2, 3, 5), (1, 14, 27)))
SHAPES = TIGHT + LOOSE
SWEEP = [f"sweep-{k:03d}" for k in range(len(SHAPES))]
EXTRA = (1, 2, 0)           # word 0 of every sweep-like case carries utterances of these lengths after its own
# One seed per case: its index in the list, except where that seed missed a condition that
# tests/test_gmmhmm_shapes_cpu.py sets on the inputs (the REFERENCE alone decides: case 23, (10, 8, 39) dense, left
# 56 % of one model's components below an occupancy of 1e-6, the cap is one in two).
SWEEP_SEED = {23: 323}

RAGGED_LENGTHS = (1024, 256, 192, 128, 65, 64, 63, 2, 1, 0)
RAGGED = {"ragged-s10m2d13": (10, 2, 13, "bidiag", 0), "ragged-s4m8d39": (4, 8, 39, "dense", 1)}
TILES_N = (40, 2100)        # utterances of word 0 (one tile) and of word 1 (nine tiles: 2049..2304)
# name -> (S, M, D, topology, seed) of the data and parameters the model is made from: a sweep case's (its index is
# the seed) wherever the sweep has the shape
DEGENERATE_FROM = {"zero_weight": (5, 3, 14, "dense", SHAPES.index((5, 3, 14))),
                   "unreachable": (5, 3, 14, "dense", SHAPES.index((5, 3, 14))),
                   "skips": (11, 2, 13, "bidiag", 900),          # left to right; the rows are replaced
                   "absorbing": (4, 8, 13, "dense", SHAPES.index((4, 8, 13))),
                   "outlier": (4, 4, 13, "bidiag", SHAPES.index((4, 4, 13)))}
DEGENERATE = list(DEGENERATE_FROM)
OUTLIER_SHIFT = 1000.0
OUTLIER_AT = (0, 2, 4)      # (word, utterance, frame) of the shifted frame


def sweep_topology(k):
    return "bidiag" if k % 2 == 0 else "dense"


def _utt(rng, proto, T):
    return np.ascontiguousarray(synth_utterance(rng, proto, max(T, 1)).T)[:T]


def _finish(S, M, D, utts, params, order=None):
    """The batch of a case: the utterances word after word, or in ``order`` (indices into that list)."""
    flat = [x for lst in utts for x in lst]
    model = np.concatenate([np.full(len(lst), w, dtype=np.int64) for w, lst in enumerate(utts)])
    order = np.arange(len(flat)) if order is None else np.asarray(order)
    flat = [flat[i] for i in order]
    return {"D": D, "S": S, "M": M, "utts": utts, "params": params, "order": order,
            "feats": np.concatenate(flat, axis=0) if flat else np.zeros((0, D), np.float32),
            "lengths": np.array([x.shape[0] for x in flat], dtype=np.int64), "utt_model": model[order]}


def _two_words(S, M, D, topo, k):
    """The sweep's data at one shape: two words, five utterances each with T in [max(S, 6), max(S, 6) + 12), every
    utterance drawn from one of two prototype sets, parameters from time_slice_params; one seed ``k`` per case."""
    rng = np.random.default_rng(5000 + k)
    words = VOCAB[:2]
    protos = [word_prototypes(words, D, seed=k + 11), word_prototypes(words, D, seed=k + 77)]
    tmin = max(S, 6)
    utts, params = [], []
    for w, word in enumerate(words):
        lst = [_utt(rng, protos[int(rng.integers(2))][word], int(rng.integers(tmin, tmin + 12))) for _ in range(5)]
        params.append(time_slice_params(lst, S, M, topo, rng))
        if w == 0:
            lst += [_utt(rng, protos[0][word], T) for T in EXTRA]
        utts.append(lst)
    return utts, params


def _renorm(a):
    a = np.asarray(a, dtype=np.float64)
    return a / a.sum(axis=-1, keepdims=True)


def _ragged(name):
    S, M, D, topo, seed = RAGGED[name]
    rng = np.random.default_rng(7000 + seed)
    words = VOCAB[:3]
    protos = [word_prototypes(words, D, seed=seed + 311), word_prototypes(words, D, seed=seed + 377)]
    own = [_utt(rng, protos[int(rng.integers(2))][words[0]], T) for T in RAGGED_LENGTHS]
    params = [time_slice_params([x for x in own if x.shape[0] >= 22], S, M, topo, rng)]
    for word in words[1:]:   # the other words' models come from utterances of their own that are not in the batch
        aux = [_utt(rng, protos[int(rng.integers(2))][word], int(rng.integers(22, 34))) for _ in range(5)]
        params.append(time_slice_params(aux, S, M, topo, rng))
    utts = [own, [_utt(rng, protos[0][words[1]], 1)], []]
    return _finish(S, M, D, utts, params, order=rng.permutation(len(own) + 1))


def _tiles():
    S, M, D = 3, 3, 5
    rng = np.random.default_rng(7100)
    words = VOCAB[:2]
    protos = [word_prototypes(words, D, seed=411), word_prototypes(words, D, seed=477)]
    utts, params = [], []
    for word, n in zip(words, TILES_N):
        lst = [_utt(rng, protos[int(rng.integers(2))][word], int(rng.integers(3, 8))) for _ in range(n)]
        params.append(time_slice_params(lst, S, M, "dense", rng))
        utts.append(lst)
    return _finish(S, M, D, utts, params)


def _skip_rows(S):
    A = np.zeros((S, S))
    for i in range(S):
        for j, p in zip(range(i, min(i + 3, S)), (0.7, 0.2, 0.1)):
            A[i, j] = p
    return _renorm(A)


def _degenerate(name):
    """Both words of a sweep-like case, each model changed in the same way (tests/test_gmmhmm_shapes_gpu.py)."""
    S, M, D, topo, seed = DEGENERATE_FROM[name]
    utts, params = _two_words(S, M, D, topo, seed)
    out = []
    for sp, A, wt, mu, cv in params:
        sp, A, wt = sp.copy(), A.copy(), wt.copy()
        if name == "zero_weight":
            wt[:, 1] = 0.0
            wt = _renorm(wt)
        elif name == "unreachable":
            sp[1] = sp[2] = 0.0
            A[:, 2] = 0.0
            sp, A = _renorm(sp), _renorm(A)
        elif name == "skips":
            A = _skip_rows(S)
        elif name == "absorbing":
            A[3] = 0.0
            A[3, 3] = 1.0
        out.append((sp, A, wt, mu, cv))
    if name == "outlier":
        w, u, t = OUTLIER_AT
        utts[w][u] = utts[w][u].copy()
        utts[w][u][t] += np.float32(OUTLIER_SHIFT)
    return _finish(S, M, D, utts, out)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in SWEEP:
        k = SWEEP.index(name)
        S, M, D = SHAPES[k]
        return _finish(S, M, D, *_two_words(S, M, D, sweep_topology(k), SWEEP_SEED.get(k, k)))
    if name in RAGGED:
        return _ragged(name)
    if name == "tiles":
        return _tiles()
    return _degenerate(name)


def word_utts(c):
    """Per batch position: (word, index within the word's list)."""
    pos = [(w, i) for w, lst in enumerate(c["utts"]) for i in range(len(lst))]
    return [pos[i] for i in c["order"]]


def batch_utts(c):
    return [c["utts"][w][i] for w, i in word_utts(c)]


# ---- the reference ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_estep(name):
    """(per-word statistics, per-utterance results in batch order) of tests/_gmmhmm_ref.py."""
    c = case(name)
    stats, by_word = [], []
    for utts, prm in zip(c["utts"], c["params"]):
        st, r = ref.estep(utts, *prm)
        stats.append(st)
        by_word.append(r)
    return stats, [by_word[w][i] for w, i in word_utts(c)]


@functools.lru_cache(maxsize=None)
def reference_viterbi(name):
    """Per utterance in batch order (logprob, path, gap); an utterance without frames: (-inf, empty, inf)."""
    c = case(name)
    return [ref.viterbi(x, *c["params"][w]) if x.shape[0] else (-np.inf, np.zeros(0, np.int64), np.inf)
            for x, w in zip(batch_utts(c), c["utt_model"])]


def ref_pair(x, prm, mode):
    """The reference's score of one utterance under one model: ``forward_backward(...)[0]`` over the log emissions or
    ``viterbi(...)[0]``; no frames: -inf."""
    if x.shape[0] == 0:
        return -np.inf
    if mode == "viterbi":
        return ref.viterbi(x, *prm)[0]
    sp, A, wt, mu, cv = prm
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    return ref.forward_backward(sp, A, ref._lse(ref.log_components(x64, wt, mu, cv), axis=2))[0]


def first_strict_max(scores):
    """The decoder's rule on the rows of a score matrix: from -inf, first strict maximum in model order; -1 if none."""
    out = np.full(scores.shape[0], -1, dtype=np.int64)
    for u, row in enumerate(scores):
        best = -np.inf
        for w, sc in enumerate(row):
            if sc > best:
                best, out[u] = sc, w
    return out


@functools.lru_cache(maxsize=None)
def reference_scores(name):
    """{mode: (score[N, W], best_word[N])}: every utterance of the batch under every model of the case."""
    c = case(name)
    out = {}
    for mode in MODES:
        sc = np.array([[ref_pair(x, prm, mode) for prm in c["params"]] for x in batch_utts(c)], dtype=np.float64)
        out[mode] = (sc, first_strict_max(sc))
    return out


def word_gap(scores):
    """Smallest distance between the two best word scores over the utterances with frames."""
    fin = scores[np.all(np.isfinite(scores), axis=1)]
    if fin.shape[1] < 2 or fin.shape[0] == 0:
        return np.inf
    top = np.sort(fin, axis=1)
    return float((top[:, -1] - top[:, -2]).min())

"""The cases behind tests/test_mmi_cpu.py and tests/test_mmi_gpu.py, seeded: the sweep of
``sapr_connected_loop_stats`` over its shapes, the chain-grammar identity and the confusable vocabulary.  The CPU
tests check from the reference alone that each case holds what the GPU tests rely on."""
import functools

import numpy as np

from tests import _loop_fb_ref as fref
from tests._synth import synth_utterance, word_prototypes

NEG = -np.inf

# (W, S, D): less than one row tile and 3 columns; 27 columns; 29 columns; 16 row tiles, the last part-filled, 79 columns
SWEEP = ((3, 3, 1), (5, 10, 13), (11, 10, 14), (14, 18, 39))
# the utterance lengths of every sweep case, in batch order: 442 frames, two spans of 256 — the boundary lies inside
# the 300-frame utterance
SWEEP_LENGTHS = (65, 0, 3, 64, 300, 1, 5, 4)
SWEEP_MASKED = 3     # the 64-frame utterance, in the middle of the batch: keep = 0
SWEEP_ZERO = 6       # the 5-frame utterance: no path, its rows of post are exact zeros


@functools.lru_cache(maxsize=None)
def sweep_case(W, S, D):
    """``(tables (ls, lt, lx), n_states, post[total, W, S], feats[total, D] float32, keep[N], loglik[N])``: the
    posteriors are ``_loop_fb_ref``'s on a random ``logb`` under the free word loop (every state may exit, so that a
    one-frame utterance has a path).  Word 1 has fewer states than S; its states behind them emit -inf."""
    rng = np.random.default_rng(1000 * W + 10 * S + D)
    n_states = [S] * W
    n_states[1] = max(1, S - 3)
    ls, lt, lx = np.full((W, S), NEG), np.full((W, S, S), NEG), np.full((W, S), NEG)
    for w, k in enumerate(n_states):
        ls[w, 0] = 0.0
        for i in range(k):
            stay = rng.uniform(0.5, 0.9)
            lt[w, i, i] = np.log(stay) if i + 1 < k else 0.0
            if i + 1 < k:
                lt[w, i, i + 1] = np.log(1.0 - stay)
        lx[w, :k] = 0.0
    total = int(sum(SWEEP_LENGTHS))
    logb = rng.normal(-20.0, 3.0, (total, W, S))
    for w, k in enumerate(n_states):
        logb[:, w, k:] = NEG
    offs = np.r_[0, np.cumsum(SWEEP_LENGTHS)]
    logb[offs[SWEEP_ZERO]:offs[SWEEP_ZERO + 1]] = NEG
    lm, lm_start, lm_end = np.zeros((W, W)), np.zeros(W), np.zeros(W)
    loglik, _, _, post = fref.posteriors_batch(logb, SWEEP_LENGTHS, ls, lt, lx, lm, lm_start, lm_end)
    feats = rng.normal(0.0, 20.0, (total, D)).astype(np.float32)
    feats[:, 0] -= 300.0
    keep = np.ones(len(SWEEP_LENGTHS), bool)
    keep[SWEEP_MASKED] = False
    for a in (post, feats, loglik, keep):
        a.setflags(write=False)
    return (ls, lt, lx), tuple(n_states), post, feats, keep, loglik


# ---- the two training cases ----------------------------------------------------------------------------------------
NAMES = ["ba", "pa", "left", "right"]    # "ba" and "pa" are the confusable pair
S_FIT, D_FIT = 3, 4


def _models(protos, rng, shared):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    models = []
    for w, name in enumerate(NAMES):
        m = GaussianHMM(n_components=S_FIT, covariance_type="spherical" if w == 3 else "diag")
        m.startprob_ = np.array([1.0, 0.0, 0.0])
        m.transmat_ = np.array([[0.7, 0.3, 0.0], [0.0, 0.7, 0.3], [0.0, 0.0, 1.0]])
        mu = protos[name] + rng.normal(0.0, 2.0, (S_FIT, D_FIT))
        mu[:, 0] -= 300.0
        m.means_ = mu
        m._covars_ = np.full(S_FIT, 40.0) if w == 3 else np.full((S_FIT, D_FIT), 40.0)
        models.append(m)
    if shared:                                                   # the pair shares its Gaussians: the mean of the two
        both = 0.5 * (models[0].means_ + models[1].means_)
        models[0].means_, models[1].means_ = both.copy(), both.copy()
    return models


def _utterance(rng, protos, words):
    return np.concatenate([synth_utterance(rng, protos[NAMES[w]], int(rng.integers(6, 11))).T
                           for w in words]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def confusable_case():
    """``(models, utterances, transcripts, (lm, lm_start, lm_end))``: "ba" and "pa" are spoken a little differently
    but their models share one set of Gaussians, so only the grammar tells them apart — "ba" follows "left" and "pa"
    follows "right" three times out of four, and the add-one bigram of the transcripts says so.  16 recordings of 4
    words; one more has too few frames for its three words and one has no frames: ``keep`` drops both."""
    from sapr_amd.connected import WordBigram
    rng = np.random.default_rng(2024)
    protos = word_prototypes(NAMES, D_FIT, n_seg=S_FIT, seed=11)
    protos["pa"] = protos["ba"] + rng.normal(0.0, 6.0, (S_FIT, D_FIT))
    utts, truth = [], []
    for n in range(16):
        first = int(rng.integers(2, 4))
        second = int(rng.integers(2, 4))
        pick = lambda lead, k: (lead - 2) if (n + k) % 4 else (3 - lead)  # noqa: E731
        words = [first, pick(first, 0), second, pick(second, 1)]
        utts.append(_utterance(rng, protos, words))
        truth.append(words)
    utts.append(_utterance(rng, protos, [2])[:4])                # 4 frames for 3 words of 3 states: the loop has a
                                                                 # path (one word), the transcript's chain has none
    truth.append([2, 0, 3])
    utts.append(np.zeros((0, D_FIT), np.float32))                # no frames
    truth.append([3, 1])
    bigram = WordBigram.from_transcripts(truth[:16], len(NAMES))
    return _models(protos, rng, True), utts, truth, (bigram.lm, bigram.lm_start, bigram.lm_end)


CHAIN = (2, 0, 3, 1)                     # the one transcript of the chain-grammar case: distinct words


@functools.lru_cache(maxsize=None)
def chain_case():
    """``(models, utterances, transcripts, (lm, lm_start, lm_end))``: every utterance says ``CHAIN`` and the grammar
    allows only that chain, so the word loop's paths ARE the transcript's: denominator = numerator.  12 recordings, one
    of them with fewer frames than words (dropped by ``keep``)."""
    from sapr_amd.connected import WordBigram
    rng = np.random.default_rng(909)
    protos = word_prototypes(NAMES, D_FIT, n_seg=S_FIT, seed=12)
    utts = [_utterance(rng, protos, CHAIN) for _ in range(11)]
    utts.insert(5, _utterance(rng, protos, [CHAIN[0]])[:3])      # 3 frames for 4 words
    truth = [list(CHAIN)] * 12
    g = WordBigram.from_grammar(len(NAMES), list(zip(CHAIN[:-1], CHAIN[1:])), starts=[CHAIN[0]], ends=[CHAIN[-1]])
    return _models(protos, rng, False), utts, truth, (g.lm, g.lm_start, g.lm_end)

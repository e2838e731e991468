"""The inputs the online-decoding tests share (tests/test_online_cpu.py asserts, from the restatement alone, the
conditions that make them worth running; tests/test_online_gpu.py runs the device on them)."""
import numpy as np

from . import _align_ref as aref
from . import _bigram_ref as bref
from . import _connected_ref as ref


def random_case(W, S, topology, exits, frames, seed=None):
    """``(tabs, lm, logb[frames, W, S])``: ``aref.network`` tables, ``bref.random_lm`` with a dead word, and
    ``logb ~ N(-40, 15)`` (the inputs of tests/test_bigram_gpu.py's recursion test)."""
    rng = np.random.default_rng(100 * W + S + (topology == "dense") + 2 * (exits == "any") if seed is None else seed)
    tabs = aref.network(rng, W, S, topology, exits, False)
    lm = bref.random_lm(rng, W, dead_word=W // 2)
    return tabs, lm, rng.normal(-40.0, 15.0, (frames, W, S))


def e2e_case(k):
    """``_connected_ref.E2E_CASES[k]`` emitted with ``ref.emit_diag`` under the word loop:
    ``(tabs, lm, [logb[T, W, S] per utterance], model, utterances)``."""
    seed, W, S, D, n = ref.E2E_CASES[k]
    model, utts, _ = ref.sample_case(seed, W, S, D, n)
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    logbs = [ref.emit_diag(x, model["means"], model["vars"], model["gconst"]) for x in utts]
    return tabs, bref.word_loop_lm(W, 0.0), logbs, model, utts


def two_longest(logbs):
    return sorted(range(len(logbs)), key=lambda u: -len(logbs[u]))[:2]


def forcing_case():
    """(11, 18) bidiagonal words that end in their last state, random ``logb``, 150 frames: no frame becomes stable,
    so a window of 64 (or 16) frames has to force."""
    return random_case(11, 18, "bidiag", "last", 150)


def fixed_chunks(T, n):
    """Chunk lengths of ``n`` frames (the last one shorter) that sum to T."""
    return [min(n, T - a) for a in range(0, T, n)]


def ragged_chunks(rng, T, max_chunk):
    """Random chunk lengths in 0 .. max_chunk that sum to T."""
    out, left = [], T
    while left:
        n = min(int(rng.integers(0, max_chunk + 1)), left)
        out.append(n)
        left -= n
    return out

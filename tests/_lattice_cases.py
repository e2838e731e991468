"""The cases the lattice tests share (tests/test_lattice_cpu.py guards on the CPU what tests/test_lattice_gpu.py relies
on): the eleven (W, S) shapes and the nine ragged lengths of tests/test_bigram_gpu.py with their random networks, and
the end-to-end case of ``_bigram_ref`` decoded under the free loop and rescored under its grammar."""
import functools

import numpy as np

from . import _align_ref as aref
from . import _bigram_ref as bref
from . import _connected_ref as ref
from . import _lattice_ref as lref

# RL = 1; RL = 2 (word 6 straddles lanes 63 / 64); RL = 4, R = 252 twice; R = 250; R = 256 and the largest lm; padded;
# (RL, SP) = (1, 18), (2, 4), (2, 18): with the rest, all nine instantiations
SHAPES = [(3, 4), (11, 10), (11, 18), (14, 18), (25, 10), (64, 4), (5, 7), (2, 1), (3, 12), (17, 3), (4, 11)]
LENGTHS = [3, 40, 1, 65, 0, 17, 2, 64, 33]          # 9 utterances: not a multiple of the 4 a workgroup serves
TOPOLOGIES = ("bidiag", "dense")
EXITS = ("last", "any")
MARGIN = 1e-6   # every record off the best path lies further below it than this, on every random case


def seed_of(W, S, topology, exits):
    return 7000 + 100 * W + S + (topology == "dense") + 2 * (exits == "any")


def random_case(W, S, topology, exits):
    """``(ls, lt, lx, lm, lm2, logb, dead)``: a random network, ``lm`` dense random with about a third of the pairs
    forbidden and one unreachable word ``dead``, a second random table ``lm2`` without a dead word, random ``logb``
    over ``LENGTHS``."""
    rng = np.random.default_rng(seed_of(W, S, topology, exits))
    ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
    dead = W // 2
    lm = bref.random_lm(rng, W, dead_word=dead)
    lm2 = bref.random_lm(rng, W)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    return ls, lt, lx, lm, lm2, logb, dead


@functools.lru_cache(maxsize=None)
def reference(W, S, topology, exits):
    """The definition on :func:`random_case`, computed once: ``(per_utt, tables, per_utt2, tables2)`` under ``lm`` and
    with the backward pass under ``lm2``.  Nobody writes to what this returns."""
    ls, lt, lx, lm, lm2, logb, _ = random_case(W, S, topology, exits)
    per, tabs = lref.batch(logb, LENGTHS, ls, lt, lx, *lm)
    per2, tabs2 = lref.batch(logb, LENGTHS, ls, lt, lx, *lm, lm2=lm2)
    return per, tabs, per2, tabs2


def off_path_margin(lat):
    """The largest margin of a record that is not on the walked best path (-inf without one)."""
    m = lat["margin"].copy()
    pw, pe = lat["path_word"], lat["path_entry"]
    T = len(pw)
    for t in range(T):
        if pw[t] >= 0 and (t == T - 1 or pe[t + 1]):
            m[t, pw[t]] = -np.inf
    return float(m.max()) if m.size else -np.inf


# ---- the end-to-end case: _bigram_ref's committed case, free loop -> lattice -> grammar ------------------------------
E2E_NAMES = ("zero", "one", "two", "three")
# the decoder loads the words in directory order, so any order can occur; only the tie between words 2 and 3 depends on
# it: the case's own order (2 before 3), the names' alphabetical order and one more (3 before 2)
E2E_ORDERS = ((0, 1, 2, 3), (1, 3, 2, 0), (3, 0, 1, 2))


@functools.lru_cache(maxsize=None)
def e2e(order=E2E_ORDERS[0]):
    """``_bigram_ref.E2E_CASE`` from the definition alone (CPU emission) with the vocabulary in ``order`` (position ->
    the case's word; words 2 and 3 tie exactly under the free loop, and the lowest POSITION wins a tie): per utterance
    the truth, the free loop's words, the grammar decode's words and score, the lattice's rescored root and words — all
    as positions —, ``eps_u``, and ``reach``: the rescored root equals the grammar decode's score within ``eps_u``."""
    seed, W, S, D, n = bref.E2E_CASE
    model, utts, truth, _ = bref.sample_bigram_case(seed, W, S, D, n, bigram=bref.e2e_bigram(), shared=bref.E2E_SHARED)
    order = list(order)
    pos = {c: order.index(c) for c in range(W)}
    tabs = tuple(model[k][order] for k in ("log_start", "log_trans", "log_exit"))
    gram = bref.grammar_lm(W, [(pos[a], pos[b]) for a, b in bref.E2E_PAIRS], starts=[pos[a] for a in bref.E2E_STARTS])
    loop = bref.word_loop_lm(W, 0.0)
    words = lambda r: [w for w, _, _ in bref.segments(r[0], r[1])]  # noqa: E731
    rows = []
    for x, t in zip(utts, truth):
        logb = ref.emit_diag(x, model["means"][order], model["vars"][order], model["gconst"][order])
        free = bref.viterbi(logb, *tabs, *loop)
        want = bref.viterbi(logb, *tabs, *gram)
        lat = lref.lattice(logb, *tabs, *loop, lm2=gram)
        rows.append(dict(truth=[pos[w] for w in t], free_words=words((free[2], free[4])),
                         grammar_words=words((want[2], want[4])), grammar_score=want[0], root=lat["root"],
                         words=words((lat["path_word"], lat["path_entry"])), eps=lat["eps"],
                         reach=abs(lat["root"] - want[0]) <= lat["eps"]))
    return rows

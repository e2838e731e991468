"""CPU: the restatement of the connected-word N-best list (tests/_nbest_ref.py) against an enumeration of every path,
against the bigram loop, level building and forced alignment, and the C ABI of ``sapr_connected_nbest`` /
``sapr_connected_nbest_capacity`` as far as it can be checked without a device (symbols, the capacity function, the
refusals before any launch)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _bigram_ref as bref
from tests import _connected_ref as ref
from tests import _levels_ref as lref
from tests import _nbest_ref as nref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(x):
    return np.float64(x).tobytes()


# ---- the definition against an enumeration of every path ----------------------------------------------------
def test_reference_equals_the_enumeration_of_every_path():
    """W in {2, 3}, S = 2, T = 0 .. 6, dense random tables with forbidden pairs, starts, exits and transitions, n in
    {1, 2, 3, 4, 8}: where the enumerated top n + 1 string scores are pairwise distinct — a condition read from the
    enumeration alone — the list is the enumeration's first n, scores bit for bit and codes."""
    rng = np.random.default_rng(5)
    cases = distinct = strings = 0
    for case in range(60):
        W, S, T = 2 + case % 2, 2, (case // 2) % 7
        ls = np.log(rng.uniform(0.05, 1.0, (W, S)))
        lt = np.log(rng.uniform(0.05, 1.0, (W, S, S)))
        lx = np.log(rng.uniform(0.05, 1.0, (W, S)))
        ls[rng.random((W, S)) < 0.25] = NEG
        lt[rng.random((W, S, S)) < 0.25] = NEG
        lx[rng.random((W, S)) < 0.25] = NEG
        lm, lm0, lm1 = bref.random_lm(rng, W, forbidden=0.3)
        logb = rng.normal(-5.0, 3.0, (T, W, S))
        every = nref.enumerate_strings(logb, ls, lt, lx, lm, lm0, lm1)
        assert len({c for _, c in every}) == len(every)
        for n in (1, 2, 3, 4, 8):
            cases += 1
            top = [s for s, _ in every[:n + 1]]
            if len(set(top)) != len(top):
                continue
            distinct += 1
            score, code, n_found, overflow = nref.nbest(logb, ls, lt, lx, lm, lm0, lm1, n)
            want = every[:n]
            assert n_found == len(want) and overflow == 0, (case, n)
            assert score[:n_found].tobytes() == np.array([s for s, _ in want], np.float64).tobytes(), (case, n)
            assert code[:n_found].tolist() == [c for _, c in want], (case, n)
            assert (score[n_found:] == NEG).all() and (code[n_found:] == 0).all()
            assert [w for _, w in nref.strings(score, code, W)] == [nref.decode(c, W) for _, c in want]
            strings += n_found
    assert cases == 300 and distinct >= 150 and strings >= 300


def test_codes_and_capacity():
    assert [nref.cap(W) for W in (1, 2, 11, 25, 64)] == [64, 40, 17, 13, 10]
    for W in (1, 2, 11, 64):
        assert (W + 1) ** nref.cap(W) <= 2 ** 64 < (W + 1) ** (nref.cap(W) + 1)
    assert nref.encode([8, 4, 4], 11) == 9 * 144 + 5 * 12 + 5 and nref.decode(9 * 144 + 5 * 12 + 5, 11) == [8, 4, 4]
    assert nref.decode(0, 11) == [] and nref.decode(nref.encode([0] * 17, 11), 11) == [0] * 17
    assert nref.encode([63] * 10, 64) < 2 ** 64
    # merge_n is a function of the values: any order of the candidates gives the same list
    rng = np.random.default_rng(1)
    s = np.r_[rng.normal(0, 1, 9).round(1), NEG, np.nan]
    c = np.r_[rng.integers(1, 5, 9), 3, 2].astype(np.uint64)
    want = nref.merge_n(s, c, 3)
    for _ in range(5):
        p = rng.permutation(s.size)
        got = nref.merge_n(s[p], c[p], 3)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    assert len(set(want[1].tolist())) == 3 and (np.diff(want[0]) <= 0).all()


# ---- the committed device case and the identities, reference side ---------------------------------------------
N_DEVICE = 10   # the utterances of the case whose lists the GPU test requires to be full


@functools.lru_cache(maxsize=None)
def _case():
    seed, W, S, D, n = ref.E2E_CASES[0]
    model, utts, truth = ref.sample_case(seed, W, S, D, n)
    logb = [ref.emit_diag(x, model["means"], model["vars"], model["gconst"]) for x in utts[:N_DEVICE]]
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    lms = bref.word_loop_lm(W, -7.25)
    return W, tabs, lms, logb, [nref.nbest(b, *tabs, *lms, 8) for b in logb]


def test_the_device_case_has_full_lists_without_equal_neighbours():
    """``_connected_ref.E2E_CASES[0]`` under ``word_loop_lm(W, -7.25)`` at n = 8: the first ten utterances."""
    assert ref.E2E_CASES[0] == (101, 11, 10, 13, 24)
    W, _, _, logb, lists = _case()
    assert len(logb) == N_DEVICE and max(len(b) for b in logb) <= 131
    for score, code, n_found, overflow in lists:
        assert n_found == 8 and overflow == 0
        assert (np.diff(score) < 0).all() and len(set(code.tolist())) == 8
    assert min(float(-np.diff(s).max()) for s, _, _, _ in lists) > 0.1


def test_rank_one_is_the_bigram_loop():
    W, tabs, lms, logb, lists = _case()
    for b, (score, code, _, _) in zip(logb, lists):
        want = bref.viterbi(b, *tabs, *lms)
        assert _bytes(score[0]) == _bytes(want[0])
        assert nref.decode(code[0], W) == [w for w, _, _ in bref.segments(want[2], want[4])]
        one = nref.nbest(b, *tabs, *lms, 1)
        assert _bytes(one[0][0]) == _bytes(score[0]) and one[1][0] == code[0] and one[2] == 1


def test_levels_identity():
    """Every entry of k <= 8 words is at most level building's ``level_score[k-1]``, and the first of each k has its
    bytes."""
    W, tabs, lms, logb, lists = _case()
    firsts = 0
    for b, (score, code, n_found, _) in zip(logb, lists):
        level, _ = lref.levels(b, *tabs, *lms, 8)
        seen = set()
        for r in range(n_found):
            k = len(nref.decode(code[r], W))
            if k > 8:
                continue
            assert score[r] <= level[k - 1]
            if k not in seen:
                seen.add(k)
                firsts += 1
                assert _bytes(score[r]) == _bytes(level[k - 1])
    assert firsts >= 2 * N_DEVICE


def test_alignment_identity():
    """Forced alignment of an entry's string plus the string's language-model score is the entry's score within
    rtol 1e-12: T <= 131 frames give at most 4 T additions, each within 2^-53 of a partial sum no larger in magnitude
    than the score — about 6e-14 — so 1e-12 leaves margin without hiding a wrong term."""
    W, tabs, lms, logb, lists = _case()
    lm, lm0, lm1 = lms
    for b, (score, code, n_found, _) in zip(logb, lists):
        for r in range(n_found):
            words = nref.decode(code[r], W)
            acoustic = aref.align(b, words, *tabs, 0.0)[0]
            lmscore = lm0[words[0]] + sum(lm[a, c] for a, c in zip(words[:-1], words[1:])) + lm1[words[-1]]
            np.testing.assert_allclose(acoustic + lmscore, score[r], rtol=1e-12, atol=0.0)


# ---- ties and overflow ----------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_lower_code():
    *args, _ = bref.tie_case()
    score, code, n_found, overflow = nref.nbest(*args, 4)
    assert nref.strings(score, code, 3) == [(0.0, [0, 2]), (0.0, [1, 2])]
    assert n_found == 2 and overflow == 0 and score[2:].tolist() == [NEG, NEG] and code[2:].tolist() == [0, 0]


def test_overflow_is_flagged_and_the_strings_have_the_capacity():
    """W = 2, S = 1, T = 45, a state that is expensive to hold: the best strings want a word per frame, a code holds
    ``cap(2) = 40``."""
    W, S, T = 2, 1, 45
    logb = np.random.default_rng(45).normal(-5.0, 1.0, (T, W, S))
    tabs = (np.zeros((W, S)), np.full((W, S, S), -3.0), np.zeros((W, S)))
    score, code, n_found, overflow = nref.nbest(logb, *tabs, *bref.word_loop_lm(W, 0.0), 4)
    assert overflow == 1 and n_found == 4
    assert [len(w) for _, w in nref.strings(score, code, W)] == [40] * 4
    assert nref.nbest(logb[:40], *tabs, *bref.word_loop_lm(W, 0.0), 4)[3] == 0
    assert nref.nbest(logb[:0], *tabs, *bref.word_loop_lm(W, 0.0), 4)[2:] == (0, 0)


# ---- the C ABI, without a device ----------------------------------------------------------------------------------
NAMES = ("sapr_connected_nbest", "sapr_connected_nbest_capacity")


def test_symbols_are_declared_bound_and_exported():
    from sapr_amd import _lib
    with open(os.path.join(ROOT, "include", "sapr_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "tests/_nbest_ref.py" in header
    assert "N_t(w)      = merge_n{ (h + lm[v][w], code * B + (w+1)) : v, h in X_t(v), code < B^(cap-1) }" in header
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    import sapr_amd
    from sapr_amd import connected
    for name in ("NBestResult", "connected_nbest", "nbest_capacity"):
        assert getattr(sapr_amd, name) is getattr(connected, name)
    with open(os.path.join(ROOT, "sapr_amd", "build.py"), encoding="utf-8") as fh:
        assert '"connected_nbest.hip"' in fh.read()


def _run(lib, n_utts=1, total=10, W=2, S=4, n_best=3, lm=1, lm_start=1, lm_end=1, score=0, code=0):
    """``sapr_connected_nbest`` with every pointer NULL except the ones switched on (a host address the checks never
    dereference)."""
    dummy = (C.c_double * 1)()
    p = lambda on: C.cast(dummy, C.c_void_p) if on else None  # noqa: E731
    return lib.sapr_connected_nbest(None, None, n_utts, total, None, None, None, p(lm), p(lm_start), p(lm_end), W, S,
                                    n_best, p(score), p(code), None, None, None)


def test_capacity_and_refusals_before_any_launch():
    from sapr_amd import _lib
    from sapr_amd.connected import nbest_capacity
    lib = _lib.load()
    k = C.c_int32(0)
    for W in (1, 2, 11, 25, 64):
        assert lib.sapr_connected_nbest_capacity(W, C.byref(k)) == 0 and k.value == nref.cap(W) == nbest_capacity(W)
    assert [nbest_capacity(W) for W in (1, 2, 11, 25, 64)] == [64, 40, 17, 13, 10]
    assert lib.sapr_connected_nbest_capacity(0, C.byref(k)) == -1
    assert lib.sapr_connected_nbest_capacity(11, None) == -1
    # unsupported: S = 19, W * SP = 260, n_best outside 1 .. 8
    assert _run(lib, W=2, S=19) == -2
    assert _run(lib, W=26, S=10) == -2
    assert b"W * SP" in lib.sapr_last_error()
    assert _run(lib, W=65, S=4) == -2
    for n in (0, 9, -1):
        assert _run(lib, n_best=n) == -2
        assert b"n_best in 1..8" in lib.sapr_last_error()
    # bad sizes
    for kw in (dict(n_utts=-1), dict(total=-1), dict(W=0), dict(S=-3)):
        assert _run(lib, **kw) == -1
        assert b"bad sizes" in lib.sapr_last_error()
    # a NULL language model, each of the three — also where there is nothing to do
    for kw in (dict(lm=0), dict(lm_start=0), dict(lm_end=0)):
        assert _run(lib, **kw) == -1
        assert b"NULL language model" in lib.sapr_last_error()
        assert _run(lib, n_utts=0, total=0, **kw) == -1
    # the other required pointers, score and code among them
    for kw in (dict(), dict(score=1), dict(code=1), dict(score=1, code=1)):
        assert _run(lib, **kw) == -1
        assert b"NULL pointer" in lib.sapr_last_error()
    # nothing to do
    assert _run(lib, n_utts=0, total=0) == 0
    assert _run(lib, n_utts=0, total=0, W=64, S=4, n_best=8) == 0


# ---- interface refusals ---------------------------------------------------------------------------------------
def test_python_argument_refusals_come_before_a_device_is_asked_for():
    from sapr_amd.connected import ConnectedNetwork, ConnectedResult, connected_decode, connected_nbest
    W, S = 3, 4
    z = np.zeros((W, S))
    net = ConnectedNetwork(z, np.zeros((W, S, S)), z)
    x = [np.zeros((5, 2), np.float32)] * 2
    for bad in (0, 9, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"n_best must be an int inside 1\.\.8"):
            connected_nbest(np.zeros((5, W, S)), [5], net, bad)
        with pytest.raises(ValueError, match=r"n_best must be an int inside 1\.\.8"):
            connected_decode(x, net, n_best=bad)
    assert ConnectedResult(*[None] * 5, offsets=None).nbest is None


def test_decoder_refuses_alternatives_outside_the_range(tmp_path):
    import pickle
    from sapr_amd.decoder import Decoder
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    d = tmp_path / "trained_models" / "hmmlearn"
    d.mkdir(parents=True)
    for word in ("yes", "no"):
        m = GaussianHMM(n_components=2, covariance_type="diag")
        m.startprob_, m.transmat_ = np.r_[1.0, 0.0], np.array([[0.5, 0.5], [0.0, 1.0]])
        m.means_, m._covars_ = np.zeros((2, 3)), np.ones((2, 3))
        with open(d / f"{word}_hmmlearn_15.pkl", "wb") as f:
            pickle.dump(m, f)
    dec = Decoder(models_dir=str(tmp_path / "trained_models"), implementation="hmmlearn")
    for bad in (0, 9):
        with pytest.raises(ValueError, match=r"n_best must be an int inside 1\.\.8"):
            dec.decode_connected([np.zeros((3, 6), np.float32)], alternatives=bad)

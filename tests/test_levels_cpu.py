"""CPU: the restatement of connected-word decoding with a known or bounded word count (tests/_levels_ref.py) against
an enumeration of every path, against the bigram loop and the forced alignment it generalises, and the C ABI of
``sapr_connected_levels`` / ``sapr_connected_levels_backtrace`` as far as it can be checked without a device (symbols,
the size function, the refusals before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _bigram_ref as bref
from tests import _connected_ref as ref
from tests import _levels_ref as lref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(x):
    return np.float64(x).tobytes()


def _case_logb(case):
    seed, W, S, D, n = case
    model, utts, truth = ref.sample_case(seed, W, S, D, n)
    logb = [ref.emit_diag(x, model["means"], model["vars"], model["gconst"]) for x in utts]
    return model, logb, truth


# ---- the definition against an enumeration of every path ----------------------------------------------------
def test_reference_equals_the_enumeration_of_every_path():
    """W = 2, S = 2, T = 0 .. 5, L = 5, dense random tables with forbidden pairs, starts, exits and transitions: the
    recursion's ``level_score`` is the best enumerated path of exactly k words bit for bit, and the path the
    back-trace returns has k words and, summed in the recursion's order, that score."""
    W, S, L = 2, 2, 5
    rng = np.random.default_rng(5)
    checked = finite = 0
    for case in range(24):
        T = case % 6
        ls = np.log(rng.uniform(0.05, 1.0, (W, S)))
        lt = np.log(rng.uniform(0.05, 1.0, (W, S, S)))
        lx = np.log(rng.uniform(0.05, 1.0, (W, S)))
        ls[rng.random((W, S)) < 0.25] = NEG
        lt[rng.random((W, S, S)) < 0.25] = NEG
        lx[rng.random((W, S)) < 0.25] = NEG
        lm, lm0, lm1 = bref.random_lm(rng, W, forbidden=0.3)
        logb = rng.normal(-5.0, 3.0, (T, W, S))
        score, lattice = lref.levels(logb, ls, lt, lx, lm, lm0, lm1, L)
        want = lref.enumerate_best(logb, ls, lt, lx, lm, lm0, lm1, L)
        assert score.tobytes() == want.tobytes(), case
        for k in range(1, L + 1):
            sc, n, pw, ps, pe = lref.backtrace(T, score, lattice, k, k)
            checked += 1
            if not np.isfinite(score[k - 1]):
                assert sc == NEG and n == 0 and (pw == -1).all() and (ps == -1).all() and not pe.any()
                continue
            finite += 1
            assert _bytes(sc) == _bytes(score[k - 1]) and n == k and int(pe.sum()) == k and pe[0] == 1
            acc = (lm0[pw[0]] + ls[pw[0], ps[0]]) + logb[0, pw[0], ps[0]]
            for t in range(1, T):
                if pe[t]:
                    acc = ((acc + lx[pw[t - 1], ps[t - 1]]) + lm[pw[t - 1], pw[t]]) + ls[pw[t], ps[t]]
                else:
                    assert pw[t] == pw[t - 1]
                    acc = acc + lt[pw[t], ps[t - 1], ps[t]]
                acc = acc + logb[t, pw[t], ps[t]]
            assert _bytes((acc + lx[pw[-1], ps[-1]]) + lm1[pw[-1]]) == _bytes(sc), (case, k)
        assert (score[T:] == NEG).all()                 # more words than frames
    assert checked == 120 and finite >= 30


# ---- the three identities ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, -7.25])
def test_loop_identity(p):
    """Where the bigram loop decodes n <= L words, ``level_score[n-1]`` has its score's bytes and no level scores
    higher; without an exact tie between counts the selection over 1 .. L returns its outputs.  For an utterance of
    T <= L frames the best level has the loop's score unconditionally."""
    L = 8
    qualified = short = 0
    for case in (ref.E2E_CASES[0], ref.E2E_CASES[3]):
        model, logb, _ = _case_logb(case)
        W = model["log_start"].shape[0]
        tabs = (model["log_start"], model["log_trans"], model["log_exit"])
        lms = bref.word_loop_lm(W, p)
        for u, b in enumerate(logb[:12]):
            for cut in (b, b[:L - (u % 5)]):
                want = bref.viterbi(cut, *tabs, *lms)
                score, got = lref.decode(cut, *tabs, *lms, L)
                if len(cut) <= L:
                    short += 1
                    assert _bytes(score.max()) == _bytes(want[0]), (u, len(cut))
                if not 1 <= want[1] <= L:
                    continue
                qualified += 1
                assert _bytes(score[want[1] - 1]) == _bytes(want[0]) and not (score > want[0]).any(), u
                if (score == want[0]).sum() == 1:
                    assert got[0] == want[0] and got[1] == want[1]
                    for a, c in zip(got[2:], want[2:]):
                        assert np.array_equal(a, c), u
    assert qualified >= 12 and short >= 24


def test_one_level_is_the_loop_with_every_pair_forbidden():
    model, logb, _ = _case_logb(ref.E2E_CASES[3])
    W = model["log_start"].shape[0]
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    rng = np.random.default_rng(3)
    lm, lm0, lm1 = bref.random_lm(rng, W)
    for b in logb[:8]:
        score, got = lref.decode(b, *tabs, lm, lm0, lm1, 1)
        want = bref.viterbi(b, *tabs, np.full((W, W), NEG), lm0, lm1)
        assert _bytes(score[0]) == _bytes(want[0])
        assert got[1] == want[1]
        for a, c in zip(got[2:], want[2:]):
            assert np.array_equal(a, c)


@pytest.mark.parametrize("p", [0.0, -3.5])
def test_chain_identity(p):
    model, logb, _ = _case_logb(ref.E2E_CASES[0])
    W = model["log_start"].shape[0]
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    long = max(logb, key=len)
    assert len(long) >= 40
    for n, (b, words) in enumerate([(long, [4]), (long, [7, 2]), (long, [9, 0, 3, 6]), (long[:25], [9, 0, 3, 6])]):
        want, pw, ps, pe, _ = aref.align(b, words, *tabs, p)
        K = len(words)
        score, got = lref.decode(b, *tabs, *bref.chain_lm(W, words, p), 5)
        assert _bytes(score[K - 1]) == _bytes(want), n
        assert (np.delete(score, K - 1) == NEG).all(), n
        assert np.array_equal(got[2], pw) and np.array_equal(got[3], ps) and np.array_equal(got[4], pe), n
        assert got[1] == (K if np.isfinite(want) else 0)
        assert np.isfinite(want) == (n < 3)             # 25 frames cannot hold 4 words of 10 states


# ---- ties ---------------------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_lowest_index_and_the_fewest_words():
    *args, L, level_score, expected = lref.tie_case()
    score, lattice = lref.levels(*args, L)
    assert score.tolist() == level_score.tolist()
    T = args[0].shape[0]
    for k, want in expected.items():
        got = lref.backtrace(T, score, lattice, k, k) if k is not None else lref.backtrace(T, score, lattice)
        assert got[0] == want[0] and got[1] == want[1], k
        for a, b in zip(got[2:], want[2:]):
            assert a.tolist() == b.tolist(), k
    assert lref.select(score) == 2 and lref.select(score, 3, 5) == 3 and lref.select(score, 4, 3) == 0
    assert lref.select(score, -2, 2) == 2 and lref.select(score, 9, 12) == 5 and lref.select(score, 1, 1) == 1
    assert lref.backtrace(T, score, lattice, 4, 3)[:2] == (NEG, 0)
    # the bigram case itself, as the issue states it
    *targs, texp = bref.tie_case()
    score, got = lref.decode(*targs, 4, 2, 2)
    assert score.tolist() == [NEG, 0.0, NEG, NEG]
    assert got[0] == texp[0] and got[1] == texp[1]
    for a, b in zip(got[2:], texp[2:]):
        assert a.tolist() == b.tolist()


# ---- the committed device case ----------------------------------------------------------------------------------
def test_the_device_case_has_utterances_on_both_sides_of_three_words():
    """``_connected_ref.E2E_CASES[0]`` under the word-loop language model at p = 0.0: with L = 3 the bound bites on
    at least 8 utterances and the loop identity still has at least 8 to check."""
    seed, W, S, D, n = ref.E2E_CASES[0]
    assert (seed, W, S, D, n) == (101, 11, 10, 13, 24)
    model, logb, truth = _case_logb(ref.E2E_CASES[0])
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    counts = [bref.viterbi(b, *tabs, *bref.word_loop_lm(W, 0.0))[1] for b in logb]
    assert sum(c > 3 for c in counts) >= 8 and sum(1 <= c <= 3 for c in counts) >= 8
    assert counts == [len(t) for t in truth]


def test_the_decoder_case_holds_the_spoken_strings_and_one_word_more():
    """``_connected_ref.E2E_CASES[3]`` (the end-to-end test through ``Decoder.decode_connected``): the level of the
    spoken count decodes the spoken string, and every utterance can hold one word more, at a lower score."""
    seed, W, S, D, n = ref.E2E_CASES[3]
    model, logb, truth = _case_logb(ref.E2E_CASES[3])
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    for b, t in zip(logb, truth):
        k = len(t)
        score, got = lref.decode(b, *tabs, *bref.word_loop_lm(W, 0.0), 8, k, k)
        assert [w for w, _, _ in lref.segments(got[2], got[4])] == t and got[1] == k
        assert np.isfinite(score[k]) and score[k] < score[k - 1] == score.max()


# ---- the C ABI, without a device ----------------------------------------------------------------------------------
NAMES = ("sapr_connected_levels_workspace_bytes", "sapr_connected_levels", "sapr_connected_levels_backtrace")


def test_symbols_are_declared_bound_and_exported():
    from sapr_amd import _lib
    with open(os.path.join(ROOT, "include", "sapr_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "tests/_levels_ref.py" in header
    assert "N_t(l,w)       = max_v (X_t(l-1,v) + lm[v][w])   for l >= 1" in header
    assert "a16(total_frames * L * R) + 2 * a16(total_frames * L * W) + a16(4 * n_utts * L)" in header
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    import sapr_amd
    from sapr_amd import connected
    for name in ("LevelResult", "connected_levels", "levels_workspace_bytes"):
        assert getattr(sapr_amd, name) is getattr(connected, name)
    with open(os.path.join(ROOT, "sapr_amd", "build.py"), encoding="utf-8") as fh:
        assert '"connected_levels.hip"' in fh.read()


def _run(lib, n_utts=1, total=10, W=2, S=4, L=3, lm=1, lm_start=1, lm_end=1, ws=None, ws_bytes=0):
    """``sapr_connected_levels`` with every pointer NULL except the three language-model tables (a host address the
    checks never dereference) and the workspace."""
    dummy = (C.c_double * 1)()
    p = lambda on: C.cast(dummy, C.c_void_p) if on else None  # noqa: E731
    return lib.sapr_connected_levels(None, None, n_utts, total, None, None, None, p(lm), p(lm_start), p(lm_end), W, S,
                                     L, ws, ws_bytes, None, None)


def _walk(lib, n_utts=1, total=10, W=2, S=4, L=3, ws=None, ws_bytes=0):
    return lib.sapr_connected_levels_backtrace(None, n_utts, total, W, S, L, ws, ws_bytes, None, None, None, None,
                                               None, None, None, None, None)


def test_size_function_and_refusals_before_any_launch():
    from sapr_amd import _lib
    from sapr_amd.connected import levels_workspace_bytes
    lib = _lib.load()
    n = C.c_size_t(0)
    size = lib.sapr_connected_levels_workspace_bytes
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    # (total_frames, n_utts, W, S, L) = (1000, 7, 11, 10, 8): R = 110
    assert size(1000, 7, 11, 10, 8, C.byref(n)) == 0
    assert n.value == a16(1000 * 8 * 110) + 2 * a16(1000 * 8 * 11) + a16(4 * 7 * 8) == 880000 + 2 * 88000 + 224
    assert levels_workspace_bytes(1000, 7, 11, 10, 8) == n.value
    assert size(0, 0, 1, 1, 1, C.byref(n)) == 0 and n.value == 0
    assert size(3, 1, 5, 7, 3, C.byref(n)) == 0                                          # SP = 10
    assert n.value == a16(3 * 3 * 50) + 2 * a16(3 * 3 * 5) + 16
    # one level costs what the bigram's workspace costs
    m = C.c_size_t(0)
    assert size(1000, 7, 11, 10, 1, C.byref(n)) == 0
    assert lib.sapr_connected_bigram_workspace_bytes(1000, 7, 11, 10, C.byref(m)) == 0 and n.value == m.value
    # unsupported: S = 19, W * SP = 260, L = 0 and 9 — from the size function and both entry points
    assert size(10, 1, 2, 19, 3, C.byref(n)) == -2
    assert size(10, 1, 26, 10, 3, C.byref(n)) == -2
    assert b"W * SP" in lib.sapr_last_error()
    assert size(10, 1, 65, 4, 3, C.byref(n)) == -2
    assert size(10, 1, 64, 4, 8, C.byref(n)) == 0
    for L in (0, 9, -1):
        assert size(10, 1, 2, 4, L, C.byref(n)) == -2
        assert b"L in 1..8" in lib.sapr_last_error()
        assert _run(lib, L=L) == -2 and _walk(lib, L=L) == -2
    assert _run(lib, W=2, S=19) == -2 and _walk(lib, W=2, S=19) == -2
    assert _run(lib, W=26, S=10) == -2 and _walk(lib, W=26, S=10) == -2
    # bad sizes
    assert size(-1, 1, 2, 4, 3, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert size(10, -1, 2, 4, 3, C.byref(n)) == -1
    assert size(10, 1, 0, 4, 3, C.byref(n)) == -1
    assert size(10, 1, 2, 0, 3, C.byref(n)) == -1
    assert size(10, 1, 2, 4, 3, None) == -1
    for kw in (dict(n_utts=-1), dict(total=-1), dict(W=0), dict(S=-3)):
        for call in (_run, _walk):
            assert call(lib, **kw) == -1
            assert b"bad sizes" in lib.sapr_last_error()
    # a NULL language model, each of the three
    for kw in (dict(lm=0), dict(lm_start=0), dict(lm_end=0)):
        assert _run(lib, **kw) == -1
        assert b"NULL language model" in lib.sapr_last_error()
        assert _run(lib, n_utts=0, total=0, **kw) == -1
    # a workspace one byte short (host memory: never touched before the refusal)
    assert size(10, 1, 2, 4, 3, C.byref(n)) == 0
    buf = (C.c_uint8 * n.value)()
    for call in (_run, _walk):
        assert call(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value - 1) == -1
        assert b"workspace too small" in lib.sapr_last_error()
        # a full workspace passes on to the next check: the other required pointers
        assert call(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value) == -1
        assert b"NULL pointer" in lib.sapr_last_error()
        # nothing to do
        assert call(lib, n_utts=0, total=0) == 0


# ---- interface refusals ---------------------------------------------------------------------------------------
def test_python_argument_refusals_come_before_a_device_is_asked_for():
    from sapr_amd.connected import ConnectedNetwork, ConnectedResult, connected_decode, connected_levels
    W, S = 3, 4
    z = np.zeros((W, S))
    net = ConnectedNetwork(z, np.zeros((W, S, S)), z)
    x = [np.zeros((5, 2), np.float32)] * 2
    with pytest.raises(ValueError, match=r"max_words must be inside 1\.\.8"):
        connected_decode(x, net, max_words=9)
    with pytest.raises(ValueError, match=r"max_words must be inside 1\.\.8"):
        connected_decode(x, net, n_words=9)                  # n_words alone implies max_words
    with pytest.raises(ValueError, match=r"max_words must be inside 1\.\.8"):
        connected_decode(x, net, max_words=0)
    with pytest.raises(ValueError, match=r"n_words must be inside 1\.\.max_words = 1\.\.3 .*at most 8.*got 4"):
        connected_decode(x, net, n_words=4, max_words=3)
    with pytest.raises(ValueError, match=r"n_words must be inside 1\.\.max_words = 1\.\.3 .*got 0\.\.2"):
        connected_decode(x, net, n_words=[0, 2], max_words=3)
    with pytest.raises(ValueError, match="3 word counts for 2 utterances"):
        connected_decode(x, net, n_words=[1, 2, 3])
    with pytest.raises(ValueError, match="n_words must be an int"):
        connected_decode(x, net, n_words=2.5)
    with pytest.raises(ValueError, match=r"max_words must be inside 1\.\.8"):
        connected_levels(np.zeros((5, W, S)), [5], net, 9)
    assert ConnectedResult(*[None] * 5, offsets=None).level_score is None


def test_decoder_refusals(tmp_path):
    import pickle
    from sapr_amd.decoder import Decoder
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    d = tmp_path / "trained_models" / "custom"
    d.mkdir(parents=True)
    with open(d / "zero_custom_15.pkl", "wb") as f:
        pickle.dump({"placeholder": "custom"}, f)
    with pytest.raises(ValueError, match="implementation='custom'"):
        Decoder(models_dir=str(tmp_path / "trained_models"), implementation="custom").decode_connected(
            [np.zeros((13, 4), np.float32)], n_words=2)
    d = tmp_path / "h" / "trained_models" / "hmmlearn"
    d.mkdir(parents=True)
    for word in ("yes", "no"):
        m = GaussianHMM(n_components=2, covariance_type="diag")
        m.startprob_, m.transmat_ = np.r_[1.0, 0.0], np.array([[0.5, 0.5], [0.0, 1.0]])
        m.means_, m._covars_ = np.zeros((2, 3)), np.ones((2, 3))
        with open(d / f"{word}_hmmlearn_15.pkl", "wb") as f:
            pickle.dump(m, f)
    dec = Decoder(models_dir=str(tmp_path / "h" / "trained_models"), implementation="hmmlearn")
    x = [np.zeros((3, 6), np.float32)]
    with pytest.raises(ValueError, match=r"max_words must be inside 1\.\.8"):
        dec.decode_connected(x, max_words=12)
    with pytest.raises(ValueError, match=r"n_words must be inside 1\.\.max_words = 1\.\.2"):
        dec.decode_connected(x, n_words=3, max_words=2)
    with pytest.raises(ValueError, match="2 word counts for 1 utterances"):
        dec.decode_connected(x, n_words=[1, 2])

"""CPU: the restatement of forward-backward over the word loop (tests/_loop_fb_ref.py) against the enumeration of every
path, against the embedded forward-backward it generalises (the chain identity) and against the isolated-word forward
likelihoods (the isolated identity); the C ABI of ``sapr_connected_posteriors`` as far as it can be checked without a
device (symbols, the size function, the refusals before any launch); and ``ConnectedResult`` without posteriors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _bigram_ref as bref
from tests import _embedded_ref as eref
from tests import _loop_fb_ref as lref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(seed, W, S, T, forbid=(), dead=None):
    rng = np.random.default_rng(seed)
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    lx = np.log(rng.uniform(0.05, 1.0, (W, S)))
    lm, lm0, lm1 = bref.random_lm(rng, W, forbidden=0.0, dead_word=dead)
    for v, w in forbid:
        lm[v, w] = NEG
    return rng.normal(-4.0, 2.0, (T, W, S)), ls, lt, lx, lm, lm0, lm1


# ---- the recursions against the enumeration of every path ------------------------------------------
@pytest.mark.parametrize("W,S,T,forbid,dead", [(2, 2, 4, (), None), (3, 2, 3, ((0, 2),), 1)])
def test_reference_equals_enumeration(W, S, T, forbid, dead):
    args = _tiny(31 + W, W, S, T, forbid, dead)
    got = lref.forward_backward(*args)
    ll, post, entry = lref.brute(*args)
    assert np.isfinite(ll)
    assert abs(got["loglik"] - ll) <= 1e-13 * abs(ll)
    np.testing.assert_allclose(got["post"], post, rtol=0, atol=1e-13)
    np.testing.assert_allclose(got["entry_post"], entry, rtol=0, atol=1e-13)
    np.testing.assert_allclose(got["word_post"], post.sum(axis=2), rtol=0, atol=1e-13)
    np.testing.assert_allclose(got["word_post"].sum(axis=1), 1.0, rtol=0, atol=1e-13)
    if dead is not None:
        assert (got["post"][:, dead] == 0.0).all() and (got["entry_post"][:, dead] == 0.0).all()
    # the same word again through lm[w][w] is a path of its own: forbidding it changes the likelihood
    lm = args[4].copy()
    lm[0, 0] = NEG
    assert lref.forward_backward(*args[:4], lm, *args[5:])["loglik"] < got["loglik"]


def test_entry_posterior_of_frame_zero_is_the_word_posterior():
    args = _tiny(5, 3, 3, 6)
    got = lref.forward_backward(*args)
    assert np.array_equal(got["entry_post"][0], got["word_post"][0])
    # a word begins somewhere: the expected number of words is at least one
    assert got["entry_post"].sum() >= 1.0 - 1e-12


def test_no_frames_and_no_path_give_zero_rows():
    logb, ls, lt, lx, lm, lm0, lm1 = _tiny(9, 2, 3, 4)
    empty = lref.forward_backward(logb[:0], ls, lt, lx, lm, lm0, lm1)
    assert empty["loglik"] == NEG and empty["post"].shape == (0, 2, 3)
    none = lref.forward_backward(logb, ls, lt, lx, lm, np.full(2, NEG), lm1)
    assert none["loglik"] == NEG and not none["post"].any() and not none["word_post"].any()
    bad = logb.copy()
    bad[2] = np.nan
    nan = lref.forward_backward(bad, ls, lt, lx, lm, lm0, lm1)
    assert np.isnan(nan["loglik"]) and not nan["post"].any() and not nan["entry_post"].any()


# ---- the two identities ---------------------------------------------------------------------------
@pytest.mark.parametrize("words,p", [([1], 0.0), ([2, 0], -1.5), ([3, 1, 0], -1.5)])
def test_chain_identity(words, p):
    """The chain language model of a transcript of distinct words: the embedded forward-backward's loglik and gamma,
    chain position k at word words[k]; every other word carries nothing."""
    W, S = 4, 3
    rng = np.random.default_rng(77)
    ls, lt, lx = aref.network(rng, W, S, "bidiag", "last", False)
    for T in (2, 7, 12):
        logb = rng.normal(-6.0, 3.0, (T, W, S))
        want = eref.forward_backward(logb, words, ls, lt, lx, p)
        got = lref.forward_backward(logb, ls, lt, lx, *bref.chain_lm(W, words, p))
        if not np.isfinite(want["loglik"]):
            assert got["loglik"] == want["loglik"] and not got["post"].any()
            continue
        assert abs(got["loglik"] - want["loglik"]) <= 1e-13 * abs(want["loglik"])
        gamma = np.zeros((T, W, S))
        gamma[:, words] = want["gamma"]
        np.testing.assert_allclose(got["post"], gamma, rtol=0, atol=1e-12)


def _isolated_forward(logb, ls, lt):
    """log P(frames | one word model), ended in any state: ``[W]``."""
    alpha = ls + logb[0]
    for t in range(1, logb.shape[0]):
        alpha = np.logaddexp.reduce(alpha[:, :, None] + lt, axis=1) + logb[t]
    return np.logaddexp.reduce(alpha, axis=1)


def test_isolated_identity():
    """Every pair forbidden, free starts and ends, log_exit == 0: the word loop is W isolated words, its likelihood
    the log-sum of their forward likelihoods and the word posterior, at every frame, their softmax."""
    W, S, T = 5, 4, 9
    rng = np.random.default_rng(3)
    ls, lt, _ = aref.network(rng, W, S, "dense", "any", False)
    logb = rng.normal(-6.0, 3.0, (T, W, S))
    got = lref.forward_backward(logb, ls, lt, np.zeros((W, S)), np.full((W, W), NEG), np.zeros(W), np.zeros(W))
    fwd = _isolated_forward(logb, ls, lt)
    ll = np.logaddexp.reduce(fwd)
    assert abs(got["loglik"] - ll) <= 1e-13 * abs(ll)
    np.testing.assert_allclose(got["word_post"], np.tile(np.exp(fwd - ll), (T, 1)), rtol=0, atol=1e-12)
    assert not got["entry_post"][1:].any()


def test_soft_bound_on_the_best_path():
    """The sum over all paths is at least the best path: loglik >= the bigram Viterbi score."""
    W, S = 4, 3
    rng = np.random.default_rng(19)
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    lm = bref.random_lm(rng, W, dead_word=2)
    logb = rng.normal(-40.0, 15.0, (20, W, S))
    score = bref.viterbi(logb, ls, lt, lx, *lm)[0]
    ll = lref.forward_backward(logb, ls, lt, lx, *lm)["loglik"]
    assert np.isfinite(score) and ll >= score


# ---- the C ABI, without a device ----------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from sapr_amd import _lib
    with open(os.path.join(ROOT, "include", "sapr_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "tests/_loop_fb_ref.py" in header and "N_t(w)        = lse_v (X_t(v) + lm[v][w])" in header
    assert "entry_post_t(w) = exp(N_{t-1}(w) + E_t(w) - loglik)" in header
    lib = _lib.load()
    for name in ("sapr_connected_posteriors", "sapr_connected_posteriors_workspace_bytes"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert lib.sapr_abi_version() == 2


def _call(lib, n_utts=1, total=10, W=2, S=4, lm=1, lm_start=1, lm_end=1, ws=None, ws_bytes=0):
    """``sapr_connected_posteriors`` with every pointer NULL except the three language-model tables (a host address
    the checks never dereference) and the workspace."""
    dummy = (C.c_double * 1)()
    p = lambda on: C.cast(dummy, C.c_void_p) if on else None  # noqa: E731
    return lib.sapr_connected_posteriors(None, None, n_utts, total, None, None, None, p(lm), p(lm_start), p(lm_end), W,
                                         S, ws, ws_bytes, None, None, None, None, None)


def test_size_function_and_refusals_before_any_launch():
    from sapr_amd import _lib
    from sapr_amd.connected import posteriors_workspace_bytes
    lib = _lib.load()
    n = C.c_size_t(0)
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    # (total_frames, n_utts, W, S) = (1001, 7, 11, 10): R = 110; 8 (R + W) bytes per frame
    assert lib.sapr_connected_posteriors_workspace_bytes(1001, 7, 11, 10, C.byref(n)) == 0
    assert n.value == a16(8 * 1001 * 110) + a16(8 * 1001 * 11)
    assert posteriors_workspace_bytes(1001, 7, 11, 10) == n.value
    assert lib.sapr_connected_posteriors_workspace_bytes(0, 0, 1, 1, C.byref(n)) == 0 and n.value == 0
    assert lib.sapr_connected_posteriors_workspace_bytes(3, 1, 5, 7, C.byref(n)) == 0        # SP = 10
    assert n.value == a16(8 * 150) + a16(8 * 15)
    # unsupported: S = 19, W * SP = 260 — from the size function and the entry point
    assert lib.sapr_connected_posteriors_workspace_bytes(10, 1, 2, 19, C.byref(n)) == -2
    assert lib.sapr_connected_posteriors_workspace_bytes(10, 1, 26, 10, C.byref(n)) == -2
    assert b"W * SP" in lib.sapr_last_error()
    assert lib.sapr_connected_posteriors_workspace_bytes(10, 1, 65, 4, C.byref(n)) == -2
    assert lib.sapr_connected_posteriors_workspace_bytes(10, 1, 64, 4, C.byref(n)) == 0
    assert _call(lib, W=2, S=19) == -2
    assert _call(lib, W=26, S=10) == -2
    # bad sizes
    assert lib.sapr_connected_posteriors_workspace_bytes(-1, 1, 2, 4, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_posteriors_workspace_bytes(10, 1, 2, 4, None) == -1
    for kw in (dict(n_utts=-1), dict(total=-1), dict(W=0), dict(S=-3)):
        assert _call(lib, **kw) == -1
        assert b"bad sizes" in lib.sapr_last_error()
    # a NULL language model, each of the three
    for kw in (dict(lm=0), dict(lm_start=0), dict(lm_end=0)):
        assert _call(lib, **kw) == -1
        assert b"NULL language model" in lib.sapr_last_error()
        assert _call(lib, n_utts=0, total=0, **kw) == -1
    # a workspace one byte short (host memory: never touched before the refusal)
    assert lib.sapr_connected_posteriors_workspace_bytes(10, 1, 2, 4, C.byref(n)) == 0
    buf = (C.c_uint8 * n.value)()
    assert _call(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value - 1) == -1
    assert b"workspace too small" in lib.sapr_last_error()
    # a full workspace passes on to the next check: the other required pointers
    assert _call(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value) == -1
    assert b"NULL pointer" in lib.sapr_last_error()
    # nothing to do
    assert _call(lib, n_utts=0, total=0) == 0


# ---- the host side ------------------------------------------------------------------------------------
def test_result_without_posteriors_behaves_as_before():
    import sapr_amd
    from sapr_amd.connected import ConnectedPosteriors, ConnectedResult
    res = ConnectedResult(np.array([-3.0, NEG]), np.array([2, 0], np.int32), np.array([1, 1, 0, -1], np.int32),
                          np.array([0, 1, 0, -1], np.int32), np.array([1, 0, 1, 0], np.uint8),
                          offsets=np.array([0, 3, 4]))
    assert res.posteriors is None
    assert res.segments(0) == [(1, 0, 2), (0, 2, 3)] and res.words(0) == [1, 0] and res.segments(1) == []
    assert sapr_amd.ConnectedPosteriors is ConnectedPosteriors
    assert sapr_amd.connected_posteriors is sapr_amd.connected.connected_posteriors
    # the confidences of a result: the mean word posterior over each segment; score - loglik per utterance
    wp = np.array([[0.1, 0.9], [0.3, 0.7], [0.6, 0.4], [0.0, 0.0]])
    post = ConnectedPosteriors(np.array([-2.5, NEG]), wp, wp.copy(), None, np.array([0, 3, 4]))
    assert post.segment_confidence(res, 0) == [pytest.approx(0.8), pytest.approx(0.6)]
    assert post.segment_confidence(res, 1) == []
    lp = post.path_log_posterior(res)
    assert lp[0] == -0.5 and np.isnan(lp[1])


def test_a_network_without_a_bigram_runs_under_its_penalty():
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    z = np.zeros((3, 4))
    lm, lm0, lm1 = ConnectedNetwork(z, np.zeros((3, 4, 4)), z, word_penalty=-2.5).loop_lm()
    assert np.array_equal(lm, np.full((3, 3), -2.5)) and not lm0.any() and not lm1.any()
    bg = WordBigram(*bref.random_lm(np.random.default_rng(1), 3))
    got = ConnectedNetwork(z, np.zeros((3, 4, 4)), z, bigram=bg).loop_lm()
    assert got[0] is bg.lm and got[1] is bg.lm_start and got[2] is bg.lm_end

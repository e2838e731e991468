"""CPU: the connected-word reference (tests/_connected_ref.py) against a brute-force enumeration of every path, the
size and layout functions of the C ABI, and the margin condition that lets the end-to-end GPU test
(tests/test_connected_gpu.py) demand equal paths for every utterance."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import _connected_ref as ref

NEG = -np.inf


def _brute(logb, ls, lt, lx, pen):
    """Every (word, state, entry) path by depth-first enumeration: the best total and the set of totals' maximum."""
    T, W, S = logb.shape
    best = [NEG]

    def walk(t, w, s, acc):
        if acc == NEG:
            return
        if t == T - 1:
            best[0] = max(best[0], acc + lx[w, s])
            return
        for w2, s2 in itertools.product(range(W), range(S)):
            if w2 == w:
                walk(t + 1, w2, s2, (acc + lt[w, s, s2]) + logb[t + 1, w2, s2])
            walk(t + 1, w2, s2, (((acc + lx[w, s]) + pen) + ls[w2, s2]) + logb[t + 1, w2, s2])

    for w, s in itertools.product(range(W), range(S)):
        walk(0, w, s, ls[w, s] + logb[0, w, s])
    return best[0]


def _path_score(logb, ls, lt, lx, pen, pw, ps, pe):
    acc = ls[pw[0], ps[0]] + logb[0, pw[0], ps[0]]
    for t in range(1, len(pw)):
        if pe[t]:
            acc = ((acc + lx[pw[t - 1], ps[t - 1]]) + pen) + ls[pw[t], ps[t]]
        else:
            assert pw[t] == pw[t - 1]
            acc = acc + lt[pw[t], ps[t - 1], ps[t]]
        acc = acc + logb[t, pw[t], ps[t]]
    return acc + lx[pw[-1], ps[-1]]


def _dyadic(rng, shape, p_inf):
    """Multiples of 1/4 in [-4, 0] (every sum of a path is exact in float64, whatever its order) with -inf sprinkled."""
    a = -rng.integers(0, 17, shape) / 4.0
    return np.where(rng.random(shape) < p_inf, NEG, a)


@pytest.mark.parametrize("W,S", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_reference_equals_brute_force(W, S, T):
    for seed in range(3 if T < 5 else 2):
        rng = np.random.default_rng(1000 * T + 100 * W + 10 * S + seed)
        p_inf = (0.0, 0.25, 0.5)[seed]
        ls, lt, lx = _dyadic(rng, (W, S), p_inf), _dyadic(rng, (W, S, S), p_inf), _dyadic(rng, (W, S), p_inf)
        logb = _dyadic(rng, (T, W, S), p_inf / 2)
        pen = float(rng.integers(-8, 5)) / 4.0
        score, n_words, pw, ps, pe = ref.viterbi(logb, ls, lt, lx, pen)
        assert score == _brute(logb, ls, lt, lx, pen)
        if np.isfinite(score):
            assert pe[0] == 1 and n_words == int(pe.sum())
            assert _path_score(logb, ls, lt, lx, pen, pw, ps, pe) == score   # the reference path attains the optimum
            assert [w for w, _, _ in ref.segments(pw, pe)] == [int(pw[a]) for a in np.flatnonzero(pe)]
        else:
            assert n_words == 0 and (pw == -1).all() and (ps == -1).all() and not pe.any()


def test_reference_ties_and_empty():
    # (2, 1) with penalty 0 and zero scores everywhere: "stay" and "re-enter" tie exactly, stay wins; word 0 wins E
    z = np.zeros((2, 1))
    score, n_words, pw, ps, pe = ref.viterbi(np.zeros((4, 2, 1)), z, np.zeros((2, 1, 1)), z, 0.0)
    assert score == 0.0 and n_words == 1 and pw.tolist() == [0] * 4 and pe.tolist() == [1, 0, 0, 0]
    score, n_words, pw, ps, pe = ref.viterbi(np.zeros((0, 2, 1)), z, np.zeros((2, 1, 1)), z, 0.0)
    assert score == NEG and n_words == 0 and pw.size == 0


def test_layout_and_size_functions():
    from sapr_amd import _lib
    lib = _lib.load()
    sp, dp, r = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    for (W, S, D), want in {(3, 4, 5): (4, 13, 12), (5, 7, 26): (10, 26, 50), (11, 10, 13): (10, 13, 110),
                            (11, 18, 39): (18, 39, 198), (14, 18, 14): (18, 26, 252), (64, 4, 27): (4, 39, 256),
                            (2, 1, 1): (4, 13, 8), (25, 5, 13): (10, 13, 250)}.items():
        assert lib.sapr_connected_layout(W, S, D, C.byref(sp), C.byref(dp), C.byref(r)) == 0
        assert (sp.value, dp.value, r.value) == want
    assert lib.sapr_connected_layout(3, 4, 5, None, None, None) == 0
    n = C.c_size_t(0)
    assert lib.sapr_connected_workspace_bytes(1000, 7, 11, 10, C.byref(n)) == 0
    assert n.value == 1000 * 110 + 4 * 1000                      # back-pointer bytes (a multiple of 16) + exit indices
    assert lib.sapr_connected_workspace_bytes(3, 1, 5, 7, C.byref(n)) == 0
    assert n.value == 160 + 12                                   # 3 * 50 = 150 bytes rounded up to 16
    assert lib.sapr_connected_workspace_bytes(0, 0, 2, 1, C.byref(n)) == 0 and n.value == 0
    # unsupported shapes: W * SP = 260, S = 19, D = 40 — from the size function too
    assert lib.sapr_connected_layout(26, 10, 13, C.byref(sp), C.byref(dp), C.byref(r)) == -2
    assert b"W * SP" in lib.sapr_last_error()
    assert lib.sapr_connected_layout(2, 19, 13, C.byref(sp), C.byref(dp), C.byref(r)) == -2
    assert lib.sapr_connected_layout(2, 4, 40, C.byref(sp), C.byref(dp), C.byref(r)) == -2
    assert lib.sapr_connected_workspace_bytes(10, 1, 26, 10, C.byref(n)) == -2
    assert lib.sapr_connected_workspace_bytes(10, 1, 2, 19, C.byref(n)) == -2
    assert lib.sapr_connected_emit_diag(None, 10, 40, None, 2, 4, None, None) == -2
    assert lib.sapr_connected_viterbi(None, None, 1, 10, None, None, None, 0.0, 65, 4, None, 0, None, None, None,
                                      None, None, None) == -2
    # bad sizes
    assert lib.sapr_connected_layout(0, 4, 13, C.byref(sp), C.byref(dp), C.byref(r)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_workspace_bytes(-1, 1, 2, 4, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_workspace_bytes(10, 1, 2, 4, None) == -1
    assert lib.sapr_connected_emit_diag(None, -1, 13, None, 2, 4, None, None) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    # NULL required pointers and a workspace that is too small, before any launch; nothing to do returns 0
    assert lib.sapr_connected_emit_diag(None, 10, 13, None, 2, 4, None, None) == -1
    assert lib.sapr_connected_emit_diag(None, 0, 13, None, 2, 4, None, None) == 0
    assert lib.sapr_connected_viterbi(None, None, 1, 10, None, None, None, 0.0, 2, 4, None, 0, None, None, None,
                                      None, None, None) == -1
    assert b"workspace too small" in lib.sapr_last_error()
    assert lib.sapr_connected_viterbi(None, None, 1, 0, None, None, None, 0.0, 2, 4, None, 0, None, None, None, None,
                                      None, None) == -1
    assert b"NULL" in lib.sapr_last_error()
    assert lib.sapr_connected_viterbi(None, None, 0, 0, None, None, None, 0.0, 2, 4, None, 0, None, None, None, None,
                                      None, None) == 0


def test_network_from_models_pads_and_sets_exits():
    from sapr_amd.connected import ConnectedNetwork, emit_operands
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    rng = np.random.default_rng(0)
    models = []
    for k, ct in ((3, "diag"), (5, "spherical")):
        m = GaussianHMM(n_components=k, covariance_type=ct)
        m.startprob_ = np.r_[1.0, np.zeros(k - 1)]
        m.transmat_ = np.eye(k) * 0.5 + np.eye(k, k=1) * 0.5
        m.transmat_[-1, -1] = 1.0
        m.means_ = rng.normal(size=(k, 6))
        m._covars_ = rng.uniform(1, 2, (k, 6) if ct == "diag" else (k,))
        models.append(m)
    net = ConnectedNetwork.from_models(models, exit_states="last", word_penalty=-2.0)
    assert (net.W, net.S, net.SP, net.DP, net.R, net.D) == (2, 5, 10, 13, 20, 6) and net.n_states == [3, 5]
    assert net.word_penalty == -2.0
    assert np.array_equal(np.isfinite(net.log_exit), np.array([[0, 0, 1, 0, 0], [0, 0, 0, 0, 1]], bool))
    assert np.all(net.log_start[0, 3:] == NEG) and np.all(net.log_trans[0, 3:] == NEG)
    assert np.all(net.log_trans[0, :, 3:] == NEG)
    assert np.allclose(net.vars[1], np.broadcast_to(models[1]._covars_[:, None], (5, 6)))
    want = 6 * np.log(2 * np.pi) + np.log(models[0]._covars_).sum(axis=1)
    assert np.array_equal(net.gconst[0, :3], want)
    any_net = ConnectedNetwork.from_models(models, exit_states="any")
    assert np.isfinite(any_net.log_exit).sum() == 8
    ops = emit_operands(net.means, net.vars, net.gconst, net.n_states)
    assert ops.shape == (20, 27) and np.all(ops[3:10, 0] == np.inf) and np.all(ops[:, 1 + 6:14] == 0)
    assert np.array_equal(ops[11, 14:20], 1.0 / net.vars[1, 1])
    full = GaussianHMM(n_components=2, covariance_type="full")
    with pytest.raises(ValueError, match="covariance_type"):
        ConnectedNetwork.from_models([full])


@pytest.mark.parametrize("case", ref.E2E_CASES + [ref.DECODER_CASE])
def test_margins_of_the_end_to_end_cases(case):
    """Along every optimal path of the committed cases each decision is an exact tie or is won by at least 1e-6: the
    device's emission differs from numpy's by rounding only (1e-13 relative), so it must take the same path."""
    seed, W, S, D, n = case
    model, utts, truth = ref.sample_case(seed, W, S, D, n, spherical=case == ref.DECODER_CASE)
    smallest, hits = np.inf, 0
    # (Decoder.decode_connected is also run with a word penalty)
    for pen in ((0.0, -30.0) if case == ref.DECODER_CASE else (0.0,)):
        for x, words in zip(utts, truth):
            logb = ref.emit_diag(x, model["means"], model["vars"], model["gconst"])
            m = np.asarray(ref.margins(logb, model["log_start"], model["log_trans"], model["log_exit"], pen))
            assert m.size, "a sampled concatenation must have a finite score"
            assert np.all((m == 0.0) | (m >= 1e-6)), m[(m != 0) & (m < 1e-6)]
            smallest = min(smallest, m[m > 0].min())
            got = ref.viterbi(logb, model["log_start"], model["log_trans"], model["log_exit"], pen)
            hits += pen == 0.0 and [w for w, _, _ in ref.segments(got[2], got[4])] == words
    print(f"case {case}: smallest margin {smallest:.3g}, {hits}/{n} word strings recovered")
    assert hits >= n // 2   # (the generator makes recognisable utterances: the test is not about trivia)

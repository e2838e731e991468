"""CPU: the forced-alignment restatement (tests/_align_ref.py) against an exhaustive enumeration of every path and
against the word-loop restatement, the conditions that keep the GPU tests (tests/test_align_gpu.py) from passing on
trivia, the size function of the C ABI and the refusals of the Python layer."""
import ctypes as C

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _connected_ref as ref

NEG = -np.inf


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_restatement_equals_exhaustive_enumeration(K):
    """W = 2, S = 2, T = 6, integer tables (every path sum is exact), penalty -1."""
    W, S, T = 2, 2, 6
    finite = 0
    for seed in range(6):
        rng = np.random.default_rng(100 * K + seed)
        p_inf = (0.0, 0.2, 0.4)[seed % 3]

        def table(shape):
            return np.where(rng.random(shape) < p_inf, NEG, -rng.integers(0, 5, shape).astype(np.float64))

        ls, lt, lx = table((W, S)), table((W, S, S)), table((W, S))
        logb = -rng.integers(0, 6, (T, W, S)).astype(np.float64)
        words = rng.integers(0, W, K).tolist()
        score, pw, ps, pe, start = aref.align(logb, words, ls, lt, lx, -1.0)
        assert score == aref.brute(logb, words, ls, lt, lx, -1.0)
        if np.isfinite(score):
            finite += 1
            segs = aref.segments(words, start, T)
            assert [w for w, _, _ in segs] == words and segs[0][1] == 0 and segs[-1][2] == T
            assert all(a < b for _, a, b in segs) and all(x[2] == y[1] for x, y in zip(segs, segs[1:]))
            assert np.flatnonzero(pe).tolist() == start.tolist()
            for (w, a, b) in segs:
                assert (pw[a:b] == w).all()
            # the path attains the optimum, with the additions in the definition's order
            acc = ls[pw[0], ps[0]] + logb[0, pw[0], ps[0]]
            for t in range(1, T):
                if pe[t]:
                    acc = ((acc + lx[pw[t - 1], ps[t - 1]]) + -1.0) + ls[pw[t], ps[t]]
                else:
                    acc = acc + lt[pw[t], ps[t - 1], ps[t]]
                acc = acc + logb[t, pw[t], ps[t]]
            assert acc + lx[pw[-1], ps[-1]] == score
        else:
            assert (pw == -1).all() and (ps == -1).all() and not pe.any() and (start == -1).all()
            assert aref.segments(words, start, T) == []
    assert finite >= 2


def test_restatement_without_a_path():
    z = np.zeros((2, 1))
    lt = np.zeros((2, 1, 1))
    for logb, words in ((np.zeros((0, 2, 1)), [0]), (np.zeros((3, 2, 1)), []), (np.zeros((2, 2, 1)), [0, 1, 0])):
        score, pw, ps, pe, start = aref.align(logb, words, z, lt, z, 0.0)
        assert score == NEG and (pw == -1).all() and (ps == -1).all() and not pe.any() and (start == -1).all()
    # K = T: every word gets exactly one frame; the same word may follow itself
    score, pw, ps, pe, start = aref.align(np.zeros((3, 2, 1)), [1, 1, 0], z, lt, z, -2.0)
    assert score == -4.0 and pw.tolist() == [1, 1, 0] and pe.tolist() == [1, 1, 1] and start.tolist() == [0, 1, 2]
    got = aref.align_batch(np.zeros((3, 2, 1)), [3], [[1, 1, 0]], z, lt, z, -2.0, max_words=2)
    assert got[0].tolist() == [NEG] and (got[1] == -1).all() and (got[4] == -1).all()


@pytest.mark.parametrize("case", ref.E2E_CASES + [ref.DECODER_CASE])
def test_aligning_to_the_decoded_string_reproduces_the_word_loop(case):
    """Float addition is monotone, so a Viterbi maximum is the maximum of the chained path values: aligned to the
    string the free word loop decoded, the score is the word loop's bit for bit, and — no decision along these optimal
    paths is an exact tie — so are the path rows.  This is what the GPU consistency test relies on."""
    seed, W, S, D, n = case
    model, utts, _ = ref.sample_case(seed, W, S, D, n, spherical=case == ref.DECODER_CASE)
    tables = (model["log_start"], model["log_trans"], model["log_exit"])
    for pen in (0.0, -7.5):
        for x in utts:
            logb = ref.emit_diag(x, model["means"], model["vars"], model["gconst"])
            score, n_words, pw, ps, pe = ref.viterbi(logb, *tables, pen)
            assert np.isfinite(score)
            assert 0.0 not in ref.margins(logb, *tables, pen)
            words = [w for w, _, _ in ref.segments(pw, pe)]
            got = aref.align(logb, words, *tables, pen)
            assert got[0] == score
            assert np.array_equal(got[1], pw) and np.array_equal(got[2], ps) and np.array_equal(got[3], pe)
            assert got[4].tolist() == np.flatnonzero(pe).tolist()


@pytest.mark.parametrize("W,S,max_words", aref.RECURSION_SHAPES)
def test_recursion_cases_have_paths(W, S, max_words):
    """The generator of the GPU recursion test against its condition: in every case the restatement alone gives a
    finite score for at least 6 of the 10 utterances (the three deliberately pathless ones and, with exits only in the
    last state, a short one are the rest), so that test cannot pass by comparing -inf with -inf."""
    lengths = aref.RECURSION_LENGTHS
    for topology in aref.TOPOLOGIES:
        for exits in aref.EXITS:
            for integer in (False, True):
                ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, topology, exits, integer)
                assert [len(t) for t in transcripts] == [
                    T + 1 if T in (1, 2) else min(max_words, max(1, T // (S + 1))) for T in lengths]
                assert max(len(t) for t in transcripts) * (4 if S <= 4 else 10 if S <= 10 else 18) <= 256
                score = aref.align_batch(logb, lengths, transcripts, ls, lt, lx, 0.0, max_words)[0]
                assert int(np.isfinite(score).sum()) >= 6, (topology, exits, integer, score)
                for u in (lengths.index(0), lengths.index(1), lengths.index(2)):
                    assert score[u] == NEG


def test_size_function():
    from sapr_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(0)
    assert lib.sapr_connected_align_workspace_bytes(1000, 7, 5, 10, C.byref(n)) == 0
    assert n.value == 1000 * 50 + 5008          # back-pointers (a multiple of 16) + 5000 exit states rounded up to 16
    assert lib.sapr_connected_align_workspace_bytes(3, 1, 3, 7, C.byref(n)) == 0
    assert n.value == 96 + 16                   # 3 * 30 = 90 and 3 * 3 = 9 bytes, each rounded up to 16
    assert lib.sapr_connected_align_workspace_bytes(0, 0, 1, 1, C.byref(n)) == 0 and n.value == 0
    assert lib.sapr_connected_align_workspace_bytes(10, 1, 64, 4, C.byref(n)) == 0
    # unsupported: max_words * SP = 260, S = 19 — before anything else is looked at
    assert lib.sapr_connected_align_workspace_bytes(10, 1, 26, 10, C.byref(n)) == -2
    assert b"max_words * SP" in lib.sapr_last_error()
    assert lib.sapr_connected_align_workspace_bytes(10, 1, 65, 4, C.byref(n)) == -2
    assert lib.sapr_connected_align_workspace_bytes(10, 1, 2, 19, C.byref(n)) == -2
    none = [None] * 5
    assert lib.sapr_connected_align(None, None, 1, 10, None, None, 26, 26, None, None, None, 0.0, 2, 10, None, 0,
                                    *none, None) == -2
    assert lib.sapr_connected_align(None, None, 1, 10, None, None, 2, 2, None, None, None, 0.0, 26, 10, None, 0,
                                    *none, None) == -2
    # bad sizes, a short workspace and NULL required pointers, before any launch; nothing to do returns 0
    assert lib.sapr_connected_align_workspace_bytes(-1, 1, 2, 4, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_align_workspace_bytes(10, 1, 0, 4, C.byref(n)) == -1
    assert lib.sapr_connected_align_workspace_bytes(10, 1, 2, 4, None) == -1
    assert lib.sapr_connected_align(None, None, 1, 10, None, None, -1, 2, None, None, None, 0.0, 2, 4, None, 0,
                                    *none, None) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_align(None, None, 1, 10, None, None, 2, 2, None, None, None, 0.0, 2, 4, None, 0,
                                    *none, None) == -1
    assert b"workspace too small" in lib.sapr_last_error()
    assert lib.sapr_connected_align(None, None, 1, 0, None, None, 0, 2, None, None, None, 0.0, 2, 4, None, 0,
                                    *none, None) == -1
    assert b"NULL" in lib.sapr_last_error()
    assert lib.sapr_connected_align(None, None, 0, 0, None, None, 0, 2, None, None, None, 0.0, 2, 4, None, 0,
                                    *none, None) == 0


def test_python_layer_refuses_bad_transcripts():
    from sapr_amd.connected import ConnectedNetwork, align_viterbi, connected_align
    W, S = 3, 7                                  # SP = 10: at most 25 words
    z = np.zeros((W, S))
    net = ConnectedNetwork(z, np.zeros((W, S, S)), z)
    logb = np.zeros((8, W, S))
    for call in (lambda tr: align_viterbi(logb, [5, 3], tr, net),
                 lambda tr: connected_align([np.zeros((5, 2), np.float32), np.zeros((3, 2), np.float32)], tr, net)):
        with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
            call([[0]])
        with pytest.raises(ValueError, match="utterance 1 is empty"):
            call([[0], []])
        with pytest.raises(ValueError, match="outside the vocabulary"):
            call([[0, 3], [1]])
        with pytest.raises(ValueError, match="outside the vocabulary"):
            call([[0], [-1]])
        with pytest.raises(ValueError, match=r"K \* SP = 260 exceeds the limit of 256"):
            call([[0] * 26, [1]])


def test_align_result_segments_and_word_examples():
    from sapr_amd.connected import AlignResult
    res = AlignResult(score=np.array([-3.0, NEG]), path_word=np.array([2, 2, 0, 0, 0, -1, -1], np.int32),
                      path_state=np.array([0, 1, 0, 0, 1, -1, -1], np.int32),
                      path_entry=np.array([1, 0, 1, 0, 0, 0, 0], np.uint8),
                      word_start=np.array([0, 2, -1, -1, -1], np.int32), word_offsets=np.array([0, 2, 5]),
                      offsets=np.array([0, 5, 7]), words=np.array([2, 0, 1, 1, 1], np.int32))
    assert res.segments(0) == [(2, 0, 2), (0, 2, 5)] and res.segments(1) == []
    feats = [np.arange(10.0).reshape(5, 2), np.zeros((2, 2))]
    ex = res.word_examples(feats)
    assert sorted(ex) == [0, 2] and np.array_equal(ex[2][0], feats[0][:2]) and np.array_equal(ex[0][0], feats[0][2:])
    with pytest.raises(ValueError, match="feature arrays"):
        res.word_examples(feats[:1])
    with pytest.raises(ValueError, match="frames"):
        res.word_examples([feats[1], feats[1]])

"""CPU: the restatement of connected-word decoding under a word bigram (tests/_bigram_ref.py) against the word loop
and the forced alignment it generalises, the host-side ``WordBigram``, and the C ABI of ``sapr_connected_bigram`` as
far as it can be checked without a device (symbols, the size function, the refusals before any launch)."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _bigram_ref as bref
from tests import _connected_ref as ref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_CASES = [ref.E2E_CASES[0], ref.E2E_CASES[1], ref.E2E_CASES[3]]


def _case_logb(case):
    seed, W, S, D, n = case
    model, utts, _ = ref.sample_case(seed, W, S, D, n)
    logb = [ref.emit_diag(x, model["means"], model["vars"], model["gconst"]) for x in utts]
    return model, logb


# ---- the two identities ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOOP_CASES)
def test_word_loop_identity(case):
    """lm == p, lm_start == lm_end == 0: p = 0.0 gives every output of the word loop; p = -7.25 its score bit for bit
    (rounding is monotone) and a path whose own total is that score."""
    model, logb = _case_logb(case)
    W = model["log_start"].shape[0]
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    for u, b in enumerate(logb):
        want = ref.viterbi(b, *tabs, 0.0)
        got = bref.viterbi(b, *tabs, *bref.word_loop_lm(W, 0.0))
        assert got[0] == want[0] and got[1] == want[1], u
        for a, c in zip(got[2:], want[2:]):
            assert np.array_equal(a, c), u
        want = ref.viterbi(b, *tabs, -7.25)
        got = bref.viterbi(b, *tabs, *bref.word_loop_lm(W, -7.25))
        assert np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes(), u
        assert np.isfinite(got[0]) and got[1] >= 1 and got[3][-1] == model["log_start"].shape[1] - 1


def _chain_cases():
    """(logb, words) on the (11, 10) case: transcripts of 1, 2 and 4 distinct words over an utterance long enough, and
    a 4-word transcript over one that is too short."""
    model, logb = _case_logb(ref.E2E_CASES[0])
    long = max(logb, key=len)
    assert len(long) >= 40
    return model, [(long, [4]), (long, [7, 2]), (long, [9, 0, 3, 6]), (long[:25], [9, 0, 3, 6])]


@pytest.mark.parametrize("p", [0.0, -3.5])
def test_chain_identity(p):
    model, cases = _chain_cases()
    W, S = model["log_start"].shape
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    for n, (b, words) in enumerate(cases):
        score, pw, ps, pe, _ = aref.align(b, words, *tabs, p)
        got = bref.viterbi(b, *tabs, *bref.chain_lm(W, words, p))
        assert np.float64(got[0]).tobytes() == np.float64(score).tobytes(), n
        assert np.array_equal(got[2], pw) and np.array_equal(got[3], ps) and np.array_equal(got[4], pe), n
        if n == 3:      # 25 frames cannot hold 4 words of 10 states
            assert got[0] == NEG and got[1] == 0 and (got[2] == -1).all() and (got[3] == -1).all() and not got[4].any()
        else:
            assert np.isfinite(got[0]) and got[1] == len(words)
            assert [w for w, _, _ in bref.segments(got[2], got[4])] == words


# ---- grammar ----------------------------------------------------------------------------------------
def test_forbidden_pairs_never_appear_and_a_closed_start_scores_minus_infinity():
    model, logb = _case_logb(ref.E2E_CASES[3])          # (3, 4)
    W = model["log_start"].shape[0]
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    allowed = [(0, 1), (1, 2), (2, 0), (1, 1)]
    lm, lm0, lm1 = bref.grammar_lm(W, allowed)
    seen = set()
    for b in logb:
        score, n_words, pw, ps, pe = bref.viterbi(b, *tabs, lm, lm0, lm1)
        words = [w for w, _, _ in bref.segments(pw, pe)]
        assert len(words) == n_words
        for pair in zip(words[:-1], words[1:]):
            assert pair in allowed
            seen.add(pair)
        free = [w for w, _, _ in ref.segments(*ref.viterbi(b, *tabs, 0.0)[2::2])]
        if all(pair in allowed for pair in zip(free[:-1], free[1:])):
            assert words == free                         # the grammar changes nothing where it forbids nothing
    assert seen                                          # (some utterance has more than one word)
    for b in logb[:3]:
        got = bref.viterbi(b, *tabs, lm, np.full(W, NEG), lm1)
        assert got[0] == NEG and got[1] == 0 and (got[2] == -1).all() and not got[4].any()
    got = bref.viterbi(logb[0][:0], *tabs, lm, lm0, lm1)
    assert got[0] == NEG and got[1] == 0 and got[2].size == 0


def test_exact_ties_go_to_the_lowest_index():
    *args, expected = bref.tie_case()
    got = bref.viterbi(*args)
    assert got[0] == expected[0] and got[1] == expected[1]
    for a, b in zip(got[2:], expected[2:]):
        assert a.tolist() == b.tolist()
    # the lattice shows the three ties the case was built for
    _, _, _, _, _, (deltas, back, xarg, warg, final) = bref.viterbi(*args, want_lattice=True)
    lx, lm = args[3], args[4]
    x0 = deltas[0] + lx
    assert x0[0, 0] + lm[0, 2] == x0[1, 0] + lm[1, 2] and warg[0, 2] == 0          # two predecessor words
    x3 = deltas[3] + lx
    assert x3[2, 0] == x3[2, 1] and xarg[3, 2] == 0 and final == 2                  # two exit states
    x1 = deltas[1] + lx
    n1 = x1[warg[1, 2], xarg[1, warg[1, 2]]] + lm[warg[1, 2], 2]
    assert deltas[1, 2, 0] + args[2][2, 0, 0] == n1 + args[1][2, 0] and back[2, 2, 0] == 0   # within == entry: within


def test_the_end_to_end_case_needs_its_grammar():
    """The committed seed: under the grammar the restatement returns the sampled strings; the word loop cannot (words
    2 and 3 share their Gaussians) and differs on an utterance that holds one of them."""
    seed, W, S, D, n = bref.E2E_CASE
    model, utts, truth, _ = bref.sample_bigram_case(seed, W, S, D, n, bigram=bref.e2e_bigram(),
                                                    shared=bref.E2E_SHARED)
    assert any(3 in t for t in truth) and any(2 in t for t in truth)
    for t in truth:
        assert t[0] in bref.E2E_STARTS and all(pair in bref.E2E_PAIRS for pair in zip(t[:-1], t[1:]))
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    lm = bref.grammar_lm(W, bref.E2E_PAIRS, bref.E2E_STARTS)
    differs = 0
    for x, t in zip(utts, truth):
        b = ref.emit_diag(x, model["means"], model["vars"], model["gconst"])
        _, _, pw, _, pe = bref.viterbi(b, *tabs, *lm)
        assert [w for w, _, _ in bref.segments(pw, pe)] == t
        _, _, pw, _, pe = ref.viterbi(b, *tabs, 0.0)
        free = [w for w, _, _ in ref.segments(pw, pe)]
        differs += free != t and (2 in t or 3 in t)
    assert differs >= 1


# ---- WordBigram -------------------------------------------------------------------------------------
def test_from_transcripts_against_a_hand_count():
    from sapr_amd.connected import WordBigram
    corpus = [[0, 1, 2], [0, 1], [1, 1, 2], [2], [0, 2, 1, 0]]
    W, k = 3, 1.0
    # pairs (v, w) and ends by hand:  0: ->1 x2, ->2 x1, end x1 | 1: ->2 x2, ->1 x1, ->0 x1, end x1 | 2: ->1 x1, end x3
    pair = np.array([[0, 2, 1], [1, 1, 2], [0, 1, 0]], float)
    end = np.array([1.0, 1.0, 3.0])
    first = np.array([3.0, 1.0, 1.0])
    bg = WordBigram.from_transcripts(corpus, W, add_k=k)
    tot = pair.sum(axis=1) + end + k * (W + 1)
    assert np.allclose(bg.lm, np.log((pair + k) / tot[:, None]), rtol=1e-15, atol=0)
    assert np.allclose(bg.lm_end, np.log((end + k) / tot), rtol=1e-15, atol=0)
    assert np.allclose(bg.lm_start, np.log((first + k) / (first.sum() + k * W)), rtol=1e-15, atol=0)
    assert np.allclose(np.exp(bg.lm).sum(axis=1) + np.exp(bg.lm_end), 1.0, rtol=1e-14)
    assert np.isclose(np.exp(bg.lm_start).sum(), 1.0, rtol=1e-14)
    raw = WordBigram.from_transcripts(corpus, W, add_k=0.0)          # unsmoothed: an unseen pair is forbidden
    assert raw.lm[0, 0] == NEG and raw.lm[2, 0] == NEG and raw.lm[2, 2] == NEG and np.isfinite(raw.lm[0, 1])
    assert np.allclose(np.exp(raw.lm).sum(axis=1) + np.exp(raw.lm_end), 1.0, rtol=1e-14)
    never = WordBigram.from_transcripts([[0, 0]], 2, add_k=0.0)      # word 1 never occurs: -inf, not NaN
    assert (never.lm[1] == NEG).all() and never.lm_end[1] == NEG and never.lm_start[1] == NEG
    with pytest.raises(ValueError, match="outside the vocabulary"):
        WordBigram.from_transcripts([[0, 3]], 3)
    with pytest.raises(ValueError, match="add_k"):
        WordBigram.from_transcripts(corpus, 3, add_k=-1.0)


def test_from_grammar_scaled_and_shapes():
    from sapr_amd.connected import WordBigram
    g = WordBigram.from_grammar(3, [(0, 1), (1, 2), (2, 2)], starts=[0], ends=[2])
    want = bref.grammar_lm(3, [(0, 1), (1, 2), (2, 2)], [0], [2])
    for a, b in zip((g.lm, g.lm_start, g.lm_end), want):
        assert np.array_equal(a, b)
    free = WordBigram.from_grammar(2, [(0, 1)])
    assert free.lm_start.tolist() == [0.0, 0.0] and free.lm_end.tolist() == [0.0, 0.0]
    with pytest.raises(ValueError, match="outside the vocabulary"):
        WordBigram.from_grammar(3, [(0, 3)])
    with np.errstate(divide="ignore"):
        bg = WordBigram(np.log([[0.5, 0.25], [0.125, 0.0]]), np.log([1.0, 0.0]), np.log([0.25, 0.5]))
    s = bg.scaled(2.0, -3.0)
    assert np.array_equal(s.lm, 2.0 * bg.lm + -3.0) and s.lm[1, 1] == NEG
    assert np.array_equal(s.lm_start, 2.0 * bg.lm_start) and np.array_equal(s.lm_end, 2.0 * bg.lm_end)
    z = bg.scaled(0.0, -1.5)                             # 0 * -inf stays forbidden
    assert z.lm.tolist() == [[-1.5, -1.5], [-1.5, NEG]] and z.lm_start.tolist() == [0.0, NEG]
    assert z.lm_end.tolist() == [0.0, 0.0] and not np.isnan(z.lm).any()
    same = bg.scaled(1.0)
    assert np.array_equal(same.lm, bg.lm) and same.lm is not bg.lm
    with pytest.raises(ValueError, match="scale must be >= 0"):
        bg.scaled(-0.5)
    with pytest.raises(ValueError, match="scale must be >= 0"):
        bg.scaled(float("nan"))
    for lm, a, b in ((np.zeros((2, 3)), np.zeros(2), np.zeros(2)), (np.zeros(4), np.zeros(2), np.zeros(2)),
                     (np.zeros((2, 2)), np.zeros(3), np.zeros(2)), (np.zeros((2, 2)), np.zeros(2), np.zeros((2, 1))),
                     (np.zeros((0, 0)), np.zeros(0), np.zeros(0))):
        with pytest.raises(ValueError, match="must be"):
            WordBigram(lm, a, b)
    import sapr_amd
    assert sapr_amd.WordBigram is WordBigram


# ---- the C ABI, without a device ----------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from sapr_amd import _lib
    with open(os.path.join(ROOT, "include", "sapr_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "tests/_bigram_ref.py" in header and "N_{t-1}(w)    = max_v (X_{t-1}(v) + lm[v][w])" in header
    lib = _lib.load()
    for name in ("sapr_connected_bigram", "sapr_connected_bigram_workspace_bytes"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    arg = re.sub(r"/\*.*?\*/", "", re.search(r"int\s+sapr_connected_bigram\s*\(([^;]*)\)", header).group(1), flags=re.S)
    arg = "".join(arg.split())
    assert "constdouble*log_exit,constdouble*lm,constdouble*lm_start,constdouble*lm_end,int32_tW,int32_tS," in arg
    assert "word_penalty" not in arg


def _call(lib, n_utts=1, total=10, W=2, S=4, lm=1, lm_start=1, lm_end=1, ws=None, ws_bytes=0):
    """``sapr_connected_bigram`` with every pointer NULL except the three language-model tables (a host address the
    checks never dereference) and the workspace."""
    dummy = (C.c_double * 1)()
    p = lambda on: C.cast(dummy, C.c_void_p) if on else None  # noqa: E731
    return lib.sapr_connected_bigram(None, None, n_utts, total, None, None, None, p(lm), p(lm_start), p(lm_end), W, S,
                                     ws, ws_bytes, None, None, None, None, None, None)


def test_size_function_and_refusals_before_any_launch():
    from sapr_amd import _lib
    from sapr_amd.connected import bigram_workspace_bytes
    lib = _lib.load()
    n = C.c_size_t(0)
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    # (total_frames, n_utts, W, S) = (1000, 7, 11, 10): R = 110
    assert lib.sapr_connected_bigram_workspace_bytes(1000, 7, 11, 10, C.byref(n)) == 0
    assert n.value == a16(1000 * 110) + 2 * a16(1000 * 11) + a16(4 * 7) == 110000 + 2 * 11008 + 32
    assert bigram_workspace_bytes(1000, 7, 11, 10) == n.value
    assert lib.sapr_connected_bigram_workspace_bytes(0, 0, 1, 1, C.byref(n)) == 0 and n.value == 0
    assert lib.sapr_connected_bigram_workspace_bytes(3, 1, 5, 7, C.byref(n)) == 0        # SP = 10
    assert n.value == a16(150) + 2 * a16(15) + 16
    # unsupported: S = 19, W * SP = 260 — from the size function and the entry point
    assert lib.sapr_connected_bigram_workspace_bytes(10, 1, 2, 19, C.byref(n)) == -2
    assert lib.sapr_connected_bigram_workspace_bytes(10, 1, 26, 10, C.byref(n)) == -2
    assert b"W * SP" in lib.sapr_last_error()
    assert lib.sapr_connected_bigram_workspace_bytes(10, 1, 65, 4, C.byref(n)) == -2
    assert lib.sapr_connected_bigram_workspace_bytes(10, 1, 64, 4, C.byref(n)) == 0
    assert _call(lib, W=2, S=19) == -2
    assert _call(lib, W=26, S=10) == -2
    # bad sizes
    assert lib.sapr_connected_bigram_workspace_bytes(-1, 1, 2, 4, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_bigram_workspace_bytes(10, -1, 2, 4, C.byref(n)) == -1
    assert lib.sapr_connected_bigram_workspace_bytes(10, 1, 0, 4, C.byref(n)) == -1
    assert lib.sapr_connected_bigram_workspace_bytes(10, 1, 2, 0, C.byref(n)) == -1
    assert lib.sapr_connected_bigram_workspace_bytes(10, 1, 2, 4, None) == -1
    for kw in (dict(n_utts=-1), dict(total=-1), dict(W=0), dict(S=-3)):
        assert _call(lib, **kw) == -1
        assert b"bad sizes" in lib.sapr_last_error()
    # a NULL language model, each of the three
    for kw in (dict(lm=0), dict(lm_start=0), dict(lm_end=0)):
        assert _call(lib, **kw) == -1
        assert b"NULL language model" in lib.sapr_last_error()
        assert _call(lib, n_utts=0, total=0, **kw) == -1
    # a workspace one byte short (host memory: never touched before the refusal)
    assert lib.sapr_connected_bigram_workspace_bytes(10, 1, 2, 4, C.byref(n)) == 0
    buf = (C.c_uint8 * n.value)()
    assert _call(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value - 1) == -1
    assert b"workspace too small" in lib.sapr_last_error()
    # a full workspace passes on to the next check: the other required pointers
    assert _call(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value) == -1
    assert b"NULL pointer" in lib.sapr_last_error()
    # nothing to do
    assert _call(lib, n_utts=0, total=0) == 0


# ---- interface refusals -----------------------------------------------------------------------------
def test_network_refuses_a_bigram_with_a_penalty_or_of_another_size():
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    W, S = 3, 4
    z = np.zeros((W, S))
    bg = WordBigram.from_grammar(W, [(0, 1)])
    net = ConnectedNetwork(z, np.zeros((W, S, S)), z, bigram=bg)
    assert net.bigram is bg and net.word_penalty == 0.0
    assert ConnectedNetwork(z, np.zeros((W, S, S)), z, word_penalty=-2.0).bigram is None
    with pytest.raises(ValueError, match=r"WordBigram\.scaled.*word_penalty must be 0\.0, got -2\.0"):
        ConnectedNetwork(z, np.zeros((W, S, S)), z, word_penalty=-2.0, bigram=bg)
    with pytest.raises(ValueError, match="over 2 words, the network over 3"):
        ConnectedNetwork(z, np.zeros((W, S, S)), z, bigram=WordBigram.from_grammar(2, []))
    with pytest.raises(ValueError, match="must be a WordBigram"):
        ConnectedNetwork(z, np.zeros((W, S, S)), z, bigram=np.zeros((W, W)))


def _pickle_models(tmp_path, impl, models, names, n_iter=15):
    d = tmp_path / "trained_models" / impl
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_{impl}_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


def test_decoder_refusals(tmp_path):
    """A "custom" decoder refuses ``decode_connected`` with a bigram as it does without; a transcript bigram that
    names an unknown word is refused by name, before a device is asked for."""
    from sapr_amd.connected import WordBigram
    from sapr_amd.decoder import Decoder
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    other = _pickle_models(tmp_path / "c", "custom", [{"placeholder": "custom"}], ["zero"])
    with pytest.raises(ValueError, match="implementation='custom'"):
        Decoder(models_dir=other, implementation="custom").decode_connected(
            [np.zeros((13, 4), np.float32)], bigram=WordBigram.from_grammar(1, [(0, 0)]))
    models = []
    for _ in range(2):
        m = GaussianHMM(n_components=2, covariance_type="diag")
        m.startprob_, m.transmat_ = np.r_[1.0, 0.0], np.array([[0.5, 0.5], [0.0, 1.0]])
        m.means_, m._covars_ = np.zeros((2, 3)), np.ones((2, 3))
        models.append(m)
    dec = Decoder(models_dir=_pickle_models(tmp_path / "h", "hmmlearn", models, ["yes", "no"]),
                  implementation="hmmlearn")
    x = [np.zeros((3, 6), np.float32)]
    with pytest.raises(ValueError, match=r"transcript 1 of the bigram names 'maybe'.*not in the vocabulary"):
        dec.decode_connected(x, bigram=[["yes", "no"], ["no", "maybe"]])
    with pytest.raises(ValueError, match="over 3 words, the vocabulary has 2"):
        dec.decode_connected(x, bigram=WordBigram.from_grammar(3, []))
    bg = dec._word_bigram([["yes", "no"], ["no"]])
    assert bg.W == 2 and np.allclose(np.exp(bg.lm).sum(axis=1) + np.exp(bg.lm_end), 1.0)

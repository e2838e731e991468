"""CPU: the restatement of the chain units with optional transcript slots (tests/_optional_ref.py) against the
enumeration of every path, against the restatements without flags (all-zero flags, and the explicit expansions an
optional transcript stands for), the conditions that keep the GPU tests (tests/test_optional_gpu.py) from passing on
trivia, the new symbols of the C ABI and the refusals of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _connected_family_cases as cases
from tests import _connected_ref as cref
from tests import _embedded_ref as eref
from tests import _optional_ref as oref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sapr_connected_align_opt_workspace_bytes": 5, "sapr_connected_align_opt": 23, "sapr_connected_embed_opt": 23,
       "sapr_connected_embed_full_opt": 23, "sapr_connected_embed_gmm_opt": 25}


def test_definition_equals_the_enumeration_of_every_path():
    """The alignment score with ``==`` (the additions along a path are the recursion's), ``loglik``, gamma, ``start``
    and ``trans`` to 1e-12."""
    finite = stepped = taken = 0
    for seed in range(150):
        ls, lt, lx, logb, words, opt, pen = oref.tiny_case(seed)
        score, pw, ps, pe, start = oref.align(logb, words, opt, ls, lt, lx, pen)
        want = oref.brute(logb, words, opt, ls, lt, lx, pen)
        assert score == want["best"], seed
        fb = oref.forward_backward(logb, words, opt, ls, lt, lx, pen)
        if not np.isfinite(want["loglik"]):
            assert fb["loglik"] == NEG and score == NEG and not fb["gamma"].any()
            continue
        assert abs(fb["loglik"] - want["loglik"]) <= 1e-12
        for key in ("gamma", "start", "trans"):
            np.testing.assert_allclose(fb[key], want[key], rtol=0, atol=1e-12, err_msg=f"{key} {seed}")
        np.testing.assert_allclose(fb["gamma"].sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-12)
        facts = oref.path_facts(words, opt, start, len(logb), score)
        finite, stepped, taken = finite + facts[0], stepped + facts[1], taken + facts[2]
        segs = oref.segments(words, start, len(logb))
        assert segs[0][1] == 0 and segs[-1][2] == len(logb) and all(a < b for _, a, b in segs)
        assert np.flatnonzero(pe).tolist() == [a for _, a, _ in segs]
    assert finite >= 100 and stepped >= 30 and taken >= 30, (finite, stepped, taken)


def test_all_zero_flags_are_the_restatements_without_flags():
    for seed in range(60):
        ls, lt, lx, logb, words, _, pen = oref.tiny_case(seed)
        zero = [0] * len(words)
        got, want = oref.align(logb, words, zero, ls, lt, lx, pen), aref.align(logb, words, ls, lt, lx, pen)
        assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
        fb, eb = oref.forward_backward(logb, words, zero, ls, lt, lx, pen), eref.forward_backward(logb, words, ls, lt,
                                                                                                 lx, pen)
        assert fb["loglik"] == eb["loglik"]
        for key in ("gamma", "start", "trans"):
            assert np.array_equal(fb[key], eb[key]), key
    W, S, max_words = 5, 7, 25
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, "skip", "any", False)
    zero = [[0] * len(t) for t in transcripts]
    for a, b in zip(oref.align_batch(logb, aref.RECURSION_LENGTHS, transcripts, zero, ls, lt, lx, -2.0),
                    aref.align_batch(logb, aref.RECURSION_LENGTHS, transcripts, ls, lt, lx, -2.0)):
        assert np.array_equal(a, b)


def _expansion_rows(exp, K, T):
    """The outputs of ``_align_ref.align`` over one expansion, with ``word_start`` spread over the K slots."""
    keep, (score, pw, ps, pe, start) = exp
    full = np.full(K, -1, np.int32)
    full[keep] = start
    return score, pw, ps, pe, full


def test_alignment_is_the_best_explicit_expansion():
    """Per utterance the best of ``_align_ref.align`` over every explicit transcript the optional one stands for:
    ``==`` on the score, and equal rows where the best expansion is unique."""
    rng = np.random.default_rng(5)
    unique = 0
    for case in range(120):
        W, S = 4, 3
        K, T = int(rng.integers(2, 7)), int(rng.integers(6, 30))
        ls, lt, lx = aref.network(rng, W, S, aref.TOPOLOGIES[case % 3], aref.EXITS[case % 2], False)
        logb = rng.normal(-10.0, 4.0, (T, W, S))
        words = rng.integers(0, W, K).tolist()
        opt = oref.silence_flags(K) if case % 2 else oref.random_flags(rng, K)
        pen = float(rng.choice([0.0, -2.0, 1.0]))
        got = oref.align(logb, words, opt, ls, lt, lx, pen)
        exps = [(keep, aref.align(logb, sub, ls, lt, lx, pen)) for keep, sub in oref.expansions(words, opt)]
        best = max(e[1][0] for e in exps)
        assert got[0] == best
        winners = [e for e in exps if e[1][0] == best]
        if np.isfinite(best) and len(winners) == 1:
            unique += 1
            for a, b in zip(got[1:], _expansion_rows(winners[0], K, T)[1:]):
                assert np.array_equal(a, b), case
    assert unique >= 80


def test_likelihood_and_posteriors_are_the_sums_over_the_expansions():
    rng = np.random.default_rng(6)
    finite = 0
    for case in range(60):
        W, S = 4, 3
        K, T = int(rng.integers(2, 6)), int(rng.integers(5, 16))
        ls, lt, lx = aref.network(rng, W, S, aref.TOPOLOGIES[case % 3], aref.EXITS[case % 2], False)
        logb = rng.normal(-6.0, 3.0, (T, W, S))
        words = rng.integers(0, W, K).tolist()
        opt = oref.silence_flags(K) if case % 2 else oref.random_flags(rng, K)
        pen = float(rng.choice([0.0, -2.0, 1.0]))
        fb = oref.forward_backward(logb, words, opt, ls, lt, lx, pen)
        parts = [(keep, eref.forward_backward(logb, sub, ls, lt, lx, pen)) for keep, sub in oref.expansions(words, opt)]
        lls = np.array([p["loglik"] for _, p in parts])
        if not np.isfinite(lls).any():
            assert fb["loglik"] == NEG
            continue
        finite += 1
        ll = np.logaddexp.reduce(lls)
        assert abs(fb["loglik"] - ll) <= 1e-12 * max(1.0, abs(ll))
        gamma, start = np.zeros((T, K, S)), np.zeros((K, S))
        for keep, p in parts:
            if np.isfinite(p["loglik"]):
                gamma[:, keep] += np.exp(p["loglik"] - ll) * p["gamma"]
                start[keep] += np.exp(p["loglik"] - ll) * p["start"]
        np.testing.assert_allclose(fb["gamma"], gamma, rtol=0, atol=1e-12)
        np.testing.assert_allclose(fb["start"], start, rtol=0, atol=1e-12)
    assert finite >= 40


# ---- the conditions of the GPU recursion cases ------------------------------------------------------------------
_INSTANCES = {}


def _instantiation(S, max_words):
    SP = 4 if S <= 4 else (10 if S <= 10 else 18)
    return (1 if max_words * SP <= 64 else (2 if max_words * SP <= 128 else 4)), SP


@pytest.mark.parametrize("exits", aref.EXITS)
@pytest.mark.parametrize("topology", aref.TOPOLOGIES)
@pytest.mark.parametrize("W,S,max_words", aref.RECURSION_SHAPES)
def test_recursion_cases_exercise_the_optional_slots(W, S, max_words, topology, exits):
    """Caps, not measurements: every run of the case has at least 6 utterances with a path; over its runs (real and
    integer tables, the three penalties) at least one path steps over a slot and at least one takes an optional one.
    The counts of paths that start in slot 1 and end in slot K - 2 are kept for the per-instantiation test below."""
    lengths = aref.RECURSION_LENGTHS
    total = np.zeros(5, int)
    for integer in (False, True):
        ls, lt, lx, logb, transcripts, optional = oref.optional_case(W, S, max_words, topology, exits, integer)
        assert all(oref.flags_ok(o, len(t)) for o, t in zip(optional, transcripts))
        woffs = np.r_[0, np.cumsum([len(t) for t in transcripts])]
        for pen in oref.PENALTIES:
            score, _, _, _, start = oref.align_batch(logb, lengths, transcripts, optional, ls, lt, lx, pen)
            facts = np.array([oref.path_facts(transcripts[u], optional[u], start[woffs[u]:woffs[u + 1]], lengths[u],
                                              score[u]) for u in range(len(lengths))]).sum(axis=0)
            assert facts[0] >= 6, (integer, pen, facts)
            total += facts
    assert total[1] >= 1 and total[2] >= 1, total
    key = _instantiation(S, max_words)
    _INSTANCES[key] = _INSTANCES.get(key, np.zeros(5, int)) + total


def test_every_instantiation_sees_both_ends_of_the_chain_move():
    """Over the cases of each of the nine (RL, SP) instantiations together: a path that starts in slot 1 and one that
    ends in slot K - 2 (runs after the parametrised test above, whose counts it reads; alone, it computes them)."""
    if len(_INSTANCES) < 9:
        for W, S, max_words in aref.RECURSION_SHAPES:
            for topology in aref.TOPOLOGIES:
                for exits in aref.EXITS:
                    test_recursion_cases_exercise_the_optional_slots(W, S, max_words, topology, exits)
    assert sorted(_INSTANCES) == sorted((rl, sp) for rl in (1, 2, 4) for sp in (4, 10, 18))
    for key, total in _INSTANCES.items():
        assert total[3] >= 1 and total[4] >= 1, (key, total)


# ---- recordings with pauses nobody wrote down --------------------------------------------------------------------
def pause_family_case(family):
    if family == "diag":
        seed, W, S, D, n = cref.DECODER_CASE
        model, utts, truth = cref.sample_case(seed, W, S, D, n, spherical=True)
    else:
        model, utts, truth = cases.case(family, cases.GMM_DECODER_CASE if family == "gmm" else cases.FULL_DECODER_CASE)
    W, S = model["log_start"].shape
    model.setdefault("log_exit", cases.log_exit(W, S))
    return model, utts, truth


@pytest.mark.parametrize("family", ["diag", "gmm", "full"])
def test_the_definition_takes_exactly_the_inserted_pauses(family):
    from sapr_amd.connected import with_optional
    model, utts, truth = pause_family_case(family)
    recs, inserted, masks = oref.pause_case(family, model, utts, truth)
    transcripts, optional = with_optional(truth, oref.PAUSE_WORD)
    assert sum(len(g) for g in inserted) >= 8 and any(0 in g for g in inserted)
    assert any(len(t) in g for g, t in zip(inserted, truth)) and any(set(g) - {0, len(t)} for g, t in zip(inserted, truth))
    assert any(not g for g in inserted) or any(len(g) < len(t) + 1 for g, t in zip(inserted, truth))
    for pen in (0.0, -30.0):
        for u, x in enumerate(recs):
            slots, flags, want = oref.pause_slots(truth[u], inserted[u])
            assert slots == transcripts[u] and flags == optional[u]
            logb = oref._emission(family, model, x)
            score, pw, _, _, start = oref.align(logb, slots, flags, model["log_start"], model["log_trans"],
                                                model["log_exit"], pen)
            assert np.isfinite(score)
            assert [k for k in range(len(slots)) if flags[k] and start[k] >= 0] == want, (u, pen)
            assert (pw[masks[u]] == oref.PAUSE_WORD).all()


# ---- the Python layer ------------------------------------------------------------------------------------------
def _net(W=3, S=4):
    from sapr_amd.connected import ConnectedNetwork
    ls, lt, lx = aref.network(np.random.default_rng(0), W, S, "bidiag", "last", False)
    return ConnectedNetwork(ls, lt, lx)


def test_refusals_of_the_python_layer():
    from sapr_amd.connected import align_viterbi, embedded_forward_backward
    net = _net()
    logb = np.zeros((12, 3, 4))
    for fn in (align_viterbi, embedded_forward_backward):
        with pytest.raises(ValueError, match="1 optional-flag sequences for 2 transcripts"):
            fn(logb, [6, 6], [[0, 1], [2]], net, optional=[[0, 1]])
        with pytest.raises(ValueError, match="utterance 1 has 2 optional flags for 1 transcript slots"):
            fn(logb, [6, 6], [[0, 1], [2]], net, optional=[[0, 1], [0, 0]])
        with pytest.raises(ValueError, match="optional flags of utterance 0 must be 0 or 1"):
            fn(logb, [6, 6], [[0, 1], [2]], net, optional=[[0, 7], [0]])
        with pytest.raises(ValueError, match="utterance 0 has two neighbouring optional slots"):
            fn(logb, [6, 6], [[0, 1, 2], [2]], net, optional=[[0, 1, 1], [0]])
        with pytest.raises(ValueError, match="every slot of utterance 1 is optional"):
            fn(logb, [6, 6], [[0, 1, 2], [2]], net, optional=[[1, 0, 1], [1]])
        # the K * SP limit counts the optional slots: 33 words and their 34 silences are 67 slots of SP = 4
        with pytest.raises(ValueError, match="has 67 words: K \\* SP = 268 exceeds the limit of 256"):
            fn(logb, [12], [[2, 0] * 33 + [2]], net, optional=[[1, 0] * 33 + [1]])


def test_with_optional():
    from sapr_amd.connected import with_optional
    t, o = with_optional([[0, 2], [1], [2, 1, 0], [1, 1], []], 1)
    assert t == [[1, 0, 1, 2, 1], [1], [1, 2, 1, 0, 1], [1, 1], []]
    assert o == [[1, 0, 1, 0, 1], [0], [1, 0, 0, 0, 1], [0, 0], []]
    for words, flags in zip(t[:4], o[:4]):
        assert oref.flags_ok(flags, len(words))
    for words, (slots, flags) in zip([[0, 2], [2, 1, 0]], zip(t[0::2], o[0::2])):
        assert oref.pause_slots(words, [], 1)[:2] == (slots, flags)


def test_segments_and_word_examples_with_stepped_over_slots():
    from sapr_amd.connected import AlignResult
    # u0: first slot stepped over; u1: last slot stepped over; u2: one in the middle; u3: no path; u4: no flags given
    res = AlignResult(score=np.array([-3.0, -2.0, -1.0, NEG]), path_word=np.zeros(16, np.int32),
                      path_state=np.zeros(16, np.int32), path_entry=np.zeros(16, np.uint8),
                      word_start=np.array([-1, 0, 2, 0, 3, -1, 0, -1, 1, -1, -1], np.int32),
                      word_offsets=np.array([0, 3, 6, 9, 11]), offsets=np.array([0, 5, 9, 13, 16]),
                      words=np.array([1, 0, 1, 1, 2, 1, 0, 1, 2, 1, 0], np.int32),
                      optional=np.array([1, 0, 1, 1, 0, 1, 0, 1, 0, 1, 0], np.uint8))
    assert res.segments(0) == [(0, 0, 2), (1, 2, 5)]
    assert res.segments(1) == [(1, 0, 3), (2, 3, 4)]
    assert res.segments(2) == [(0, 0, 1), (2, 1, 4)]
    assert res.segments(3) == []
    feats = [np.arange(2.0 * n).reshape(n, 2) for n in (5, 4, 4, 3)]
    ex = res.word_examples(feats)
    assert sorted(ex) == [0, 1, 2] and [len(v) for _, v in sorted(ex.items())] == [2, 2, 2]
    assert np.array_equal(ex[1][0], feats[0][2:5]) and np.array_equal(ex[1][1], feats[1][0:3])
    assert np.array_equal(ex[2][1], feats[2][1:4])
    # a finite score with every word_start at -1 (rows the caller did not ask for) is no path either
    blank = AlignResult(score=np.array([-1.0]), path_word=np.zeros(2, np.int32), path_state=np.zeros(2, np.int32),
                        path_entry=np.zeros(2, np.uint8), word_start=np.array([-1, -1], np.int32),
                        word_offsets=np.array([0, 2]), offsets=np.array([0, 2]), words=np.array([0, 1], np.int32),
                        optional=np.array([0, 1], np.uint8))
    assert blank.segments(0) == []
    # without flags: what it returned before, the field defaults to None
    plain = AlignResult(score=np.array([-3.0]), path_word=np.zeros(5, np.int32), path_state=np.zeros(5, np.int32),
                        path_entry=np.zeros(5, np.uint8), word_start=np.array([0, 2], np.int32),
                        word_offsets=np.array([0, 2]), offsets=np.array([0, 5]), words=np.array([2, 0], np.int32))
    assert plain.optional is None and plain.segments(0) == [(2, 0, 2), (0, 2, 5)]
    assert list(AlignResult.__dataclass_fields__)[-1] == "optional"


def test_new_symbols_are_declared_bound_and_exported():
    import sapr_amd
    from sapr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sapr_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, arity in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    # the arguments of the entry point without _opt in their order, with `optional` behind word_offsets
    for name, at in (("sapr_connected_align", 6), ("sapr_connected_embed", 8), ("sapr_connected_embed_full", 8),
                     ("sapr_connected_embed_gmm", 10)):
        sig, base = _lib.SIGNATURES[name + "_opt"][1], _lib.SIGNATURES[name][1]
        assert sig[:at] == base[:at] and sig[at] == C.c_void_p and sig[at + 1:] == base[at:], name
        m = re.search(r"\b" + name + r"_opt\s*\(([^)]*)\)", txt)
        assert "optional" in m.group(1).split(",")[at]
    assert _lib.SIGNATURES["sapr_connected_align_opt_workspace_bytes"] == \
        _lib.SIGNATURES["sapr_connected_align_workspace_bytes"]
    for name in ("with_optional", "align_opt_workspace_bytes"):
        assert getattr(sapr_amd, name) is getattr(sapr_amd.connected, name)


def test_size_function():
    from sapr_amd import _lib
    lib = _lib.load()
    old, new = C.c_size_t(0), C.c_size_t(0)
    for total, n, mw, S in ((0, 0, 1, 1), (727, 10, 5, 10), (727, 17, 14, 18), (5050000, 10000, 11, 10), (100, 1, 64, 4)):
        assert lib.sapr_connected_align_workspace_bytes(total, n, mw, S, C.byref(old)) == 0
        assert lib.sapr_connected_align_opt_workspace_bytes(total, n, mw, S, C.byref(new)) == 0
        assert new.value == old.value + (n + 15) // 16 * 16, (total, n, mw, S)
    assert lib.sapr_connected_align_opt_workspace_bytes(10, 1, 65, 4, C.byref(new)) == -2
    assert lib.sapr_connected_align_opt_workspace_bytes(10, 1, 0, 4, C.byref(new)) == -1
    assert lib.sapr_connected_align_opt_workspace_bytes(10, 1, 5, 4, None) == -1


def test_decoder_refuses_an_unknown_silence_word(tmp_path):
    import pickle
    from sapr_amd.decoder import Decoder
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    d = tmp_path / "trained_models" / "hmmlearn"
    d.mkdir(parents=True)
    for word in ("zero", "one"):
        m = GaussianHMM(n_components=2, covariance_type="diag")
        m.startprob_, m.transmat_ = np.array([1.0, 0.0]), np.array([[0.5, 0.5], [0.0, 1.0]])
        m.means_, m._covars_ = np.zeros((2, 3)), np.ones((2, 3))
        with open(d / f"{word}_hmmlearn_15.pkl", "wb") as f:
            pickle.dump(m, f)
    dec = Decoder(models_dir=str(tmp_path / "trained_models"), implementation="hmmlearn", n_iter=15)
    x = [np.zeros((3, 6), np.float32)]
    with pytest.raises(ValueError, match="optional_silence names 'sil', which is not in the vocabulary"):
        dec.align(x, [["zero"]], optional_silence="sil")
    with pytest.raises(ValueError, match="optional_silence names 'sil', which is not in the vocabulary"):
        dec.train_embedded(x, [["zero"]], optional_silence="sil")

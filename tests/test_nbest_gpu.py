"""GPU: the connected-word N-best list (csrc/connected_nbest.hip) through the Python layer against the CPU restatement
tests/_nbest_ref.py, which is the definition, and against the kernels around it (``sapr_connected_bigram``,
``sapr_connected_levels``, ``sapr_connected_align``).  The recursion is float64 adds and compares and 64-bit integer
arithmetic only, so every comparison is ``np.array_equal`` / ``tobytes()``; the end-to-end tests feed the device's own
emitted ``logb`` to the restatement for the same reason."""
import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _bigram_ref as bref
from tests import _connected_family_cases as cases
from tests import _connected_ref as ref
from tests import _nbest_ref as nref
from tests.test_levels_gpu import LENGTHS, SHAPES, _models, _pickle_models

pytestmark = pytest.mark.gpu

NEG = -np.inf
# n_best per shape: NB = 2 serves 1 and 2, NB = 4 serves 3 and 4, NB = 8 serves 5 .. 8.  With (RL, SP) of the shapes —
# (3, 4) and (2, 1): (1, 4); (17, 3): (2, 4); (64, 4): (4, 4); (5, 7): (1, 10); (11, 10): (2, 10); (25, 10): (4, 10);
# (3, 12): (1, 18); (4, 11): (2, 18); (11, 18) and (14, 18): (4, 18) — every (RL, SP, NB) runs, and 1, 3 and 5 are
# depths below their NB
DEPTHS = {(3, 4): (1, 4, 8), (2, 1): (2, 3, 5), (17, 3): (2, 3, 8), (64, 4): (2, 3, 5), (5, 7): (2, 4, 8),
          (11, 10): (1, 2, 3, 5, 8), (25, 10): (2, 4, 8), (3, 12): (1, 4, 8), (4, 11): (2, 4, 5),
          (11, 18): (2, 4, 8), (14, 18): (1, 3, 5)}


def test_the_depths_cover_every_instantiation():
    seen = set()
    for (W, S), depths in DEPTHS.items():
        SP = 4 if S <= 4 else 10 if S <= 10 else 18
        RL = 1 if W * SP <= 64 else 2 if W * SP <= 128 else 4
        seen |= {(RL, SP, 2 if n <= 2 else 4 if n <= 4 else 8) for n in depths}
    assert seen == {(RL, SP, NB) for RL in (1, 2, 4) for SP in (4, 10, 18) for NB in (2, 4, 8)}
    assert set(DEPTHS) == set(SHAPES)


def _net(ls, lt, lx, lm):
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    return ConnectedNetwork(ls, lt, lx, bigram=WordBigram(*lm))


def _assert_equal(got, want, what):
    score, code, n_found, overflow = want
    assert got.score.tobytes() == score.tobytes(), what
    assert np.array_equal(got.code, code), what
    assert np.array_equal(got.n_found, n_found), what
    assert np.array_equal(got.overflow, overflow.astype(bool)), what


@pytest.mark.parametrize("topology", ["bidiag", "dense"])
@pytest.mark.parametrize("W,S", SHAPES)
def test_recursion_equals_restatement(W, S, topology):
    """Random ``logb``; ``lm`` dense random with about a third of the pairs forbidden and one unreachable word."""
    from sapr_amd.connected import connected_nbest
    exits = "any" if topology == "dense" else "last"
    rng = np.random.default_rng(100 * W + S + (topology == "dense"))
    ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
    dead = W // 2
    lm = bref.random_lm(rng, W, dead_word=dead)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    net = _net(ls, lt, lx, lm)
    for n in DEPTHS[(W, S)]:
        got = connected_nbest(logb, LENGTHS, net, n)
        assert got.score.shape == got.code.shape == (len(LENGTHS), n) and got.code.dtype == np.uint64
        want = nref.nbest_batch(logb, LENGTHS, ls, lt, lx, *lm, n)
        _assert_equal(got, want, (W, S, topology, n))
        assert got.n_found[LENGTHS.index(0)] == 0 and not got.overflow[LENGTHS.index(0)]
        for u in range(len(LENGTHS)):
            rows = got.strings(u)
            assert len(rows) == got.n_found[u]
            assert all(dead not in words for _, words in rows) or W == 1
            assert [w for _, w in rows] == [nref.decode(c, W) for c in want[1][u][:len(rows)]]
    if exits == "any" and W > 2:        # (the restatement's own values: the longer utterances fill their lists)
        assert (want[2] == n).sum() >= 4


def test_overflow_on_the_device():
    """W = 2, S = 1, T = 45 with a state that is expensive to hold: the best strings want a word per frame, a code
    holds ``cap(2) = 40``."""
    from sapr_amd.connected import connected_nbest, nbest_capacity
    W, S, T, n = 2, 1, 45, 4
    rng = np.random.default_rng(45)
    ls, lt, lx = np.zeros((W, S)), np.full((W, S, S), -3.0), np.zeros((W, S))
    lm = bref.word_loop_lm(W, 0.0)
    logb = rng.normal(-5.0, 1.0, (T + 30, W, S))
    got = connected_nbest(logb, [T, 30], _net(ls, lt, lx, lm), n)
    want = nref.nbest_batch(logb, [T, 30], ls, lt, lx, *lm, n)
    _assert_equal(got, want, "overflow")
    assert got.overflow.tolist() == [True, False] and nbest_capacity(W) == 40
    assert [len(w) for _, w in got.strings(0)] == [40] * n and [len(w) for _, w in got.strings(1)] == [30] * n
    assert got.align(0).score.shape == (2,)                 # SP = 4: 64 words fit the alignment


def test_the_alignment_limit_applies_to_align_alone():
    """S = 5 runs at SP = 10: a string of 30 words is found, and only its alignment (25 words) is refused."""
    from sapr_amd.connected import connected_nbest
    W, S, T = 2, 5, 30
    lm = bref.word_loop_lm(W, 0.0)
    net = _net(np.zeros((W, S)), np.full((W, S, S), -3.0), np.zeros((W, S)), lm)
    logb = np.random.default_rng(30).normal(-5.0, 1.0, (T, W, S))
    got = connected_nbest(logb, [T], net, 2)
    assert [len(w) for _, w in got.strings(0)] == [T, T] and not got.overflow[0]
    with pytest.raises(ValueError, match=r"max_words \* SP <= 256 chain positions \(25 words at SP = 10\)"):
        got.align(0)
    with pytest.raises(ValueError, match="rank 2 is outside 0..1"):
        got.align(2)


@pytest.fixture(scope="module")
def emitted():
    """The (11, 10) case's utterances emitted once on the device: ``(model, net, logb_device, logb_host, lengths)``."""
    import torch
    from sapr_amd.connected import ConnectedNetwork, emit_diag
    seed, W, S, D, n = ref.E2E_CASES[0]
    model, utts, _ = ref.sample_case(seed, W, S, D, n)
    net = ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, None, model["means"],
                           model["vars"], model["gconst"])
    logb = emit_diag(torch.from_numpy(np.concatenate(utts)).cuda(), net)
    host = logb.cpu().numpy().reshape(-1, W, net.SP)[:, :, :S].copy()
    return model, net, logb, host, [len(x) for x in utts]


def test_identities_on_the_device(emitted):
    """On the emitted (11, 10) case under the word-loop language model: rank 1 is ``sapr_connected_bigram``'s result;
    n_best = 1 is column 0 of n_best = 8; the first entry of every word count has level building's score and no entry
    beats its count's level; a forced alignment of rank r plus its language-model score is the entry's score."""
    from sapr_amd.connected import _lm_scores, connected_levels, connected_nbest, connected_viterbi
    model, _, logb, host, lengths = emitted
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    W = tabs[0].shape[0]
    N = len(lengths)
    for p in (0.0, -7.25):
        net = _net(*tabs, bref.word_loop_lm(W, p))
        loop = connected_viterbi(logb, lengths, net)
        got = connected_nbest(logb, lengths, net, 8)
        one = connected_nbest(logb, lengths, net, 1)
        assert got.score[:, 0].tobytes() == loop.score.tobytes(), p
        assert one.score.tobytes() == got.score[:, :1].tobytes() and np.array_equal(one.code, got.code[:, :1])
        assert np.array_equal(one.n_found, np.minimum(got.n_found, 1))
        clear = got.score[:, 0] > got.score[:, 1]
        assert clear.sum() >= N // 2
        for u in np.flatnonzero(clear):
            assert got.words(u, 0) == loop.words(u), (p, u)
        # scores non-increasing, codes distinct per row
        assert (np.diff(got.score, axis=1) <= 0).all()
        for u in range(N):
            live = got.code[u, :got.n_found[u]]
            assert len(set(live.tolist())) == live.size and (live != 0).all()
            assert (got.code[u, got.n_found[u]:] == 0).all() and (got.score[u, got.n_found[u]:] == NEG).all()
        # the levels identity
        level = connected_levels(logb, lengths, net, 8).level_score
        firsts = 0
        for u in range(N):
            seen = set()
            for r in range(got.n_found[u]):
                k = len(got.words(u, r))
                if k > 8:
                    continue
                assert got.score[u, r] <= level[u, k - 1]
                if k not in seen:
                    seen.add(k)
                    firsts += 1
                    assert got.score[u, r].tobytes() == level[u, k - 1].tobytes(), (p, u, r)
        assert firsts >= N
        # the alignment identity (rtol 1e-12: at most 4 T <= 524 additions of relative error 2^-53 each, ~6e-14)
        for r in (0, 3, 7):
            al = got.align(r)
            assert np.array_equal(al.utterances, np.flatnonzero(got.n_found > r)) and al.utterances.size >= N // 2
            strings = [got.words(u, r) for u in al.utterances]
            total = al.score + _lm_scores(strings, net)
            np.testing.assert_allclose(total, got.score[al.utterances, r], rtol=1e-12, atol=0.0)
            for k, u in enumerate(al.utterances):
                assert [w for w, _, _ in al.segments(k)] == strings[k]
        if p == -7.25:      # the committed device case (tests/test_nbest_cpu.py): full lists, no two equal neighbours
            assert (got.n_found[:10] == 8).all() and (np.diff(got.score[:10], axis=1) < 0).all()
    # the restatement over the logb the device emitted, ten utterances
    want = nref.nbest_batch(host[:sum(lengths[:10])], lengths[:10], *tabs, *bref.word_loop_lm(W, -7.25), 8)
    sub = connected_nbest(host[:sum(lengths[:10])], lengths[:10], _net(*tabs, bref.word_loop_lm(W, -7.25)), 8)
    _assert_equal(sub, want, "e2e")


def test_utterances_are_isolated_and_runs_repeat():
    from sapr_amd.connected import connected_nbest
    W, S, n = 11, 10, 5
    rng = np.random.default_rng(17)
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    net = _net(ls, lt, lx, bref.random_lm(rng, W, dead_word=3))
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    offs = np.r_[0, np.cumsum(LENGTHS)]
    a, b = connected_nbest(logb, LENGTHS, net, n), connected_nbest(logb, LENGTHS, net, n)
    assert a.score.tobytes() == b.score.tobytes() and a.code.tobytes() == b.code.tobytes()
    for u in (1, 3, 8):
        one = connected_nbest(logb[offs[u]:offs[u + 1]], [LENGTHS[u]], net, n)
        assert one.score.tobytes() == a.score[u:u + 1].tobytes() and np.array_equal(one.code, a.code[u:u + 1])
    # a NaN frame in utterance 3 (65 frames): it has no string left, every other utterance keeps its bytes
    bad = logb.copy()
    bad[offs[3] + 20] = np.nan
    c = connected_nbest(bad, LENGTHS, net, n)
    others = np.arange(len(LENGTHS)) != 3
    assert c.score[others].tobytes() == a.score[others].tobytes() and np.array_equal(c.code[others], a.code[others])
    assert c.n_found[3] == 0 and (c.score[3] == NEG).all() and (c.code[3] == 0).all()
    _assert_equal(c, nref.nbest_batch(bad, LENGTHS, ls, lt, lx, *net.loop_lm(), n), "nan")


def test_exact_ties_go_to_the_lower_code():
    from sapr_amd.connected import connected_nbest
    logb, ls, lt, lx, lm, lm0, lm1, _ = bref.tie_case()
    got = connected_nbest(np.concatenate([logb, logb]), [4, 4], _net(ls, lt, lx, (lm, lm0, lm1)), 4)
    assert got.strings(0) == got.strings(1) == [(0.0, [0, 2]), (0.0, [1, 2])]
    assert got.n_found.tolist() == [2, 2]


@pytest.mark.parametrize("family,spec", [("gmm", cases.GMM_CASES[0]), ("full", cases.FULL_CASES[0])])
def test_other_families_through_connected_decode(family, spec):
    """``connected_decode(n_best=4)`` over a mixture and a full-covariance vocabulary: the list is the restatement's
    over the ``logb`` the device emitted, and its head is the decoded result."""
    import torch
    from sapr_amd import connected
    from sapr_amd.connected import ConnectedNetwork, connected_decode
    model, utts, _ = cases.case(family, spec)
    net = ConnectedNetwork.from_models(cases.models_of(family, model), word_penalty=-2.5)
    assert net.family == family
    res = connected_decode(utts, net, n_best=4)
    W, S = net.W, net.S
    emit = {"gmm": connected.emit_gmm, "full": connected.emit_full}[family]
    logb = emit(torch.from_numpy(np.concatenate(utts)).cuda(), net).cpu().numpy().reshape(-1, W, net.SP)[:, :, :S]
    lengths = [len(x) for x in utts]
    want = nref.nbest_batch(logb, lengths, net.log_start, net.log_trans, net.log_exit, *net.loop_lm(), 4)
    _assert_equal(res.nbest, want, family)
    assert res.nbest.score[:, 0].tobytes() == res.score.tobytes()
    assert (res.nbest.n_found >= 2).all()
    assert connected_decode(utts, net).nbest is None


def test_decoder_lists_alternatives(tmp_path):
    from sapr_amd.decoder import Decoder
    seed, W, S, D, n = ref.E2E_CASES[3]
    model, utts, truth = ref.sample_case(seed, W, S, D, n)
    names = ["zero", "one", "two"]
    root = _pickle_models(tmp_path, "hmmlearn", _models("diag", model), names)
    dec = Decoder(models_dir=root, implementation="hmmlearn", n_iter=15)
    feats = [x.T for x in utts]
    plain = dec.decode_connected(feats)
    rows = dec.decode_connected(feats, alternatives=3)
    assert "alternatives" not in plain[0]
    for row, base, x in zip(rows, plain, utts):
        alts = row["alternatives"]
        assert row["alternatives_complete"] is True and 1 <= len(alts) <= 3
        assert alts[0]["words"] == row["words"] == base["words"]
        assert np.float64(alts[0]["log_likelihood"]).tobytes() == np.float64(row["log_likelihood"]).tobytes()
        assert np.float64(row["log_likelihood"]).tobytes() == np.float64(base["log_likelihood"]).tobytes()
        lls = [a["log_likelihood"] for a in alts]
        assert lls == sorted(lls, reverse=True) and len({tuple(a["words"]) for a in alts}) == len(alts)
        for a in alts:
            assert [w for w, _, _ in a["segments"]] == a["words"]
            assert a["segments"][0][1] == 0 and a["segments"][-1][2] == len(x)
    assert sum(len(row["alternatives"]) == 3 for row in rows) >= len(rows) // 2

"""GPU: connected-word decoding with a known or bounded word count (csrc/connected_levels.hip) through the Python
layer against the CPU restatement tests/_levels_ref.py, which is the definition, and against the kernels it
generalises (``sapr_connected_bigram``, ``sapr_connected_align``).  The recursion is float64 adds and compares only, so
every comparison is ``np.array_equal`` / ``tobytes()``; the end-to-end test feeds the device's own emitted ``logb`` to
the restatement for the same reason."""
import pickle

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _bigram_ref as bref
from tests import _connected_ref as ref
from tests import _levels_ref as lref

pytestmark = pytest.mark.gpu

NEG = -np.inf
FIELDS = ("score", "n_words", "path_word", "path_state", "path_entry")
# (tests/test_bigram_gpu.py) RL = 1; RL = 2 (word 6 straddles lanes 63 / 64); RL = 4, R = 252 twice; R = 250; R = 256
# and the largest lm; padded
SHAPES = [(3, 4), (11, 10), (11, 18), (14, 18), (25, 10), (64, 4), (5, 7), (2, 1),
          (3, 12), (17, 3), (4, 11)]                # (RL, SP) = (1, 18), (2, 4), (2, 18): with the rest, all nine
LENGTHS = [3, 40, 1, 65, 0, 17, 2, 64, 33]          # 9 utterances: not a multiple of the 4 a workgroup serves
MORE_LEVELS = {(11, 10): (1, 2, 3, 5), (11, 18): (1, 2, 3, 5)}  # every LT instantiation, and an L below its LT


def _net(ls, lt, lx, lm):
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    return ConnectedNetwork(ls, lt, lx, bigram=WordBigram(*lm))


def _assert_equal(res, want, what):
    for f, w in zip(FIELDS, want):
        assert np.array_equal(getattr(res, f), w), (what, f)


@pytest.mark.parametrize("topology", ["bidiag", "dense"])
@pytest.mark.parametrize("W,S", SHAPES)
def test_recursion_equals_restatement(W, S, topology):
    """Random ``logb``; ``lm`` dense random with about a third of the pairs forbidden and one unreachable word.  The
    restatement is run once at L = 8: a level reads no level above it, so its first L levels are the run at L."""
    from sapr_amd.connected import connected_levels
    exits = "any" if topology == "dense" else "last"
    rng = np.random.default_rng(100 * W + S + (topology == "dense"))
    ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
    dead = W // 2
    lm = bref.random_lm(rng, W, dead_word=dead)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    net = _net(ls, lt, lx, lm)
    want = lref.Batch(logb, LENGTHS, ls, lt, lx, *lm, 8)
    n = len(LENGTHS)
    for L in (8,) + MORE_LEVELS.get((W, S), ()):
        got = connected_levels(logb, LENGTHS, net, L)
        assert got.level_score.shape == (n, L)
        assert got.level_score.tobytes() == np.ascontiguousarray(want.level_score[:, :L]).tobytes(), L
        assert (got.level_score[LENGTHS.index(0)] == NEG).all()
        sub = lref.Batch.__new__(lref.Batch)            # the restatement at L: the first L levels
        sub.L, sub.offs, sub.lattices, sub.level_score = L, want.offs, want.lattices, want.level_score[:, :L]
        for k in range(1, L + 1):
            res = got.select(k)
            _assert_equal(res, sub.select(k, k), (W, S, topology, L, k))
            assert not (res.path_word == dead).any() or W == 1
        _assert_equal(got.select(), sub.select(), (W, S, topology, L, "default"))
        # one range per utterance: inside, clamped from below and from above, single counts and an empty range
        lo = np.array([1, 2, 1, 3, 1, -4, 2, 9, 5], np.int32)
        hi = np.array([8, 3, 1, 12, 2, 2, 1, 11, 6], np.int32)
        _assert_equal(got.select((lo, hi)), sub.select(lo, hi), (W, S, topology, L, "ranges"))
        _assert_equal(got.select((2, hi)), sub.select(2, hi), (W, S, topology, L, "lo and ranges"))
    if exits == "any" and W > 2:    # (the restatement's own values: every count has utterances that can hold it)
        assert np.isfinite(want.level_score).sum(axis=0).min() >= 4


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


def test_loop_identity_on_the_device(emitted):
    """Against ``sapr_connected_bigram`` on the same ``logb``: where it decodes n <= L words, ``level_score[n-1]`` has
    its score's bytes and no level scores higher; at L = 8 the default selection is its five outputs; at L = 3 the
    utterances it decodes longer come back with exactly 3 words at a strictly lower score."""
    from sapr_amd.connected import ConnectedNetwork, connected_levels, connected_viterbi
    model, _, logb, host, lengths = emitted
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    W = tabs[0].shape[0]
    u = np.arange(len(lengths))
    for p in (0.0, -7.25):
        net = _net(*tabs, bref.word_loop_lm(W, p))
        loop = connected_viterbi(logb, lengths, net)
        assert np.isfinite(loop.score).all() and loop.n_words.max() <= 8
        # a network without a bigram runs under its word_penalty: the same bytes
        plain = connected_levels(logb, lengths, ConnectedNetwork(*tabs, word_penalty=p), 8)
        for L in (8, 3):
            got = connected_levels(logb, lengths, net, L)
            fits = loop.n_words <= L
            assert got.level_score[u[fits], loop.n_words[fits] - 1].tobytes() == loop.score[fits].tobytes(), (p, L)
            assert not (got.level_score > loop.score[:, None]).any()
            res = got.select()
            if L == 8:
                assert fits.all() and got.level_score.tobytes() == plain.level_score.tobytes()
                for f in FIELDS:
                    assert np.array_equal(getattr(res, f), getattr(loop, f)), (p, f)
            else:
                assert (~fits).sum() >= 8 and fits.sum() >= 8
                assert (res.n_words[~fits] == 3).all() and (res.score[~fits] < loop.score[~fits]).all()
                assert np.array_equal(res.n_words[fits], loop.n_words[fits])
                assert res.score[fits].tobytes() == loop.score[fits].tobytes()
                for a in np.flatnonzero(~fits):
                    assert len(res.segments(a)) == 3
            _assert_equal(res, lref.Batch(host, lengths, *tabs, *bref.word_loop_lm(W, p), L).select(), (p, L))


def test_chain_identity_on_the_device(emitted):
    from sapr_amd.connected import ConnectedNetwork, align_viterbi, connected_levels
    model, _, logb, host, lengths = emitted
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    W = tabs[0].shape[0]
    for words, p in (([4], 0.0), ([7, 2], -3.5), ([9, 0, 3, 6], -3.5)):
        K = len(words)
        al = align_viterbi(logb, lengths, [words] * len(lengths), ConnectedNetwork(*tabs, word_penalty=p))
        got = connected_levels(logb, lengths, _net(*tabs, bref.chain_lm(W, words, p)), 5)
        assert got.level_score[:, K - 1].tobytes() == al.score.tobytes(), words
        assert (np.delete(got.level_score, K - 1, axis=1) == NEG).all(), words
        for res in (got.select(K), got.select()):
            assert res.score.tobytes() == al.score.tobytes()
            for f in ("path_word", "path_state", "path_entry"):
                assert np.array_equal(getattr(res, f), getattr(al, f)), (words, f)
            finite = np.isfinite(res.score)
            assert (res.n_words[finite] == K).all() and (res.n_words[~finite] == 0).all()
        if K == 4:              # utterances of fewer than 40 frames cannot hold 4 words of 10 states
            assert finite.any() and (~finite).any()


def test_one_level_is_the_bigram_with_every_pair_forbidden(emitted):
    from sapr_amd.connected import connected_levels, connected_viterbi
    model, _, logb, _, lengths = emitted
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    W = tabs[0].shape[0]
    lm, lm0, lm1 = bref.random_lm(np.random.default_rng(9), W)
    one = connected_viterbi(logb, lengths, _net(*tabs, (np.full((W, W), NEG), lm0, lm1)))
    got = connected_levels(logb, lengths, _net(*tabs, (lm, lm0, lm1)), 1)
    assert got.level_score[:, 0].tobytes() == one.score.tobytes()
    res = got.select()
    for f in FIELDS:
        assert np.array_equal(getattr(res, f), getattr(one, f)), f
    assert np.isfinite(one.score).any()


def test_exact_ties_go_to_the_lowest_index_and_the_fewest_words():
    from sapr_amd.connected import connected_levels
    logb, ls, lt, lx, lm, lm0, lm1, L, level_score, expected = lref.tie_case()
    got = connected_levels(np.concatenate([logb, logb]), [4, 4], _net(ls, lt, lx, (lm, lm0, lm1)), L)
    assert got.level_score.tolist() == [level_score.tolist()] * 2
    for k, want in expected.items():
        res = got.select(k)
        assert res.score.tolist() == [want[0]] * 2 and res.n_words.tolist() == [want[1]] * 2, k
        assert res.path_word.tolist() == want[2].tolist() * 2, k
        assert res.path_state.tolist() == want[3].tolist() * 2, k
        assert res.path_entry.tolist() == want[4].tolist() * 2, k
    assert got.select((3, 5)).n_words.tolist() == [3, 3]
    assert got.select((np.array([1, 4], np.int32), np.array([5, 3], np.int32))).n_words.tolist() == [2, 0]
    assert [k for k, _, _, _ in got.strings(1)] == [2, 3, 4]


def test_utterances_are_isolated_and_runs_repeat():
    from sapr_amd.connected import connected_levels
    W, S, L = 11, 10, 5
    rng = np.random.default_rng(17)
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    lm = bref.random_lm(rng, W, dead_word=3)
    net = _net(ls, lt, lx, lm)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    offs = np.r_[0, np.cumsum(LENGTHS)]
    a, b = connected_levels(logb, LENGTHS, net, L), connected_levels(logb, LENGTHS, net, L)
    assert a.level_score.tobytes() == b.level_score.tobytes()
    ra, rb = a.select(), b.select()
    for f in FIELDS:
        assert getattr(ra, f).tobytes() == getattr(rb, f).tobytes(), f
    for u in (1, 3, 8):
        lo, hi = offs[u], offs[u + 1]
        one = connected_levels(logb[lo:hi], [LENGTHS[u]], net, L)
        assert one.level_score.tobytes() == a.level_score[u:u + 1].tobytes()
        r1 = one.select()
        assert r1.score.tobytes() == ra.score[u:u + 1].tobytes() and r1.n_words[0] == ra.n_words[u]
        for f in FIELDS[2:]:
            assert np.array_equal(getattr(r1, f), getattr(ra, f)[lo:hi]), (u, f)
    # a NaN frame in utterance 3 (65 frames): every other utterance keeps its bytes
    bad = logb.copy()
    bad[offs[3] + 20] = np.nan
    c = connected_levels(bad, LENGTHS, net, L)
    others = np.arange(len(LENGTHS)) != 3
    assert c.level_score[others].tobytes() == a.level_score[others].tobytes()
    keep = np.ones(len(logb), bool)
    keep[offs[3]:offs[4]] = False
    for k in (None, 2, 5):
        rc, rk = c.select(k), a.select(k)
        assert rc.score[others].tobytes() == rk.score[others].tobytes()
        assert np.array_equal(rc.n_words[others], rk.n_words[others])
        for f in FIELDS[2:]:
            assert getattr(rc, f)[keep].tobytes() == getattr(rk, f)[keep].tobytes(), (k, f)
        pw, ps = rc.path_word[offs[3]:offs[4]], rc.path_state[offs[3]:offs[4]]
        assert pw.min() >= -1 and pw.max() <= W - 1 and ps.min() >= -1 and ps.max() <= S - 1


# ---- end to end: Decoder.decode_connected(n_words=..., max_words=..., nbest=...) over the three families --------
def _pickle_models(tmp_path, impl, models, names, n_iter=15):
    d = tmp_path / "trained_models" / impl
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_{impl}_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


def _models(family, model):
    """The case's words as fitted models: "diag" ``GaussianHMM``; the same with word 0 as a "full" model (diagonal
    matrices); ``GMMHMM`` with two equal components per state."""
    from sapr_amd.gmm_hmm import GMMHMM
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    W, S = model["log_start"].shape
    out = []
    for w in range(W):
        if family == "gmm":
            m = GMMHMM(n_components=S, n_mix=2)
            m.weights_ = np.full((S, 2), 0.5)
            m.means_ = np.repeat(model["means"][w][:, None, :], 2, axis=1)
            m.covars_ = np.repeat(model["vars"][w][:, None, :], 2, axis=1)
        elif family == "full" and w == 0:
            m = GaussianHMM(n_components=S, covariance_type="full")
            m.means_ = model["means"][w]
            m._covars_ = np.array([np.diag(v) for v in model["vars"][w]])
        else:
            m = GaussianHMM(n_components=S, covariance_type="diag")
            m.means_, m._covars_ = model["means"][w], model["vars"][w]
        m.startprob_, m.transmat_ = model["startprob"][w], model["transmat"][w]
        out.append(m)
    return out


@pytest.mark.parametrize("family,impl", [("diag", "hmmlearn"), ("full", "hmmlearn"), ("gmm", "gmmhmm")])
def test_decoder_decodes_with_a_known_count_and_lists_the_strings(tmp_path, family, impl):
    """The (3, 4) case: with the spoken count ``Decoder.decode_connected`` returns the spoken strings; one word more
    costs score; the N-best list is sorted and led by the default result; every number is the restatement's over the
    ``logb`` the device emitted."""
    import torch
    from sapr_amd import connected
    from sapr_amd.connected import ConnectedNetwork
    from sapr_amd.decoder import Decoder
    seed, W, S, D, n = ref.E2E_CASES[3]
    model, utts, truth = ref.sample_case(seed, W, S, D, n)
    names = ["zero", "one", "two"]
    root = _pickle_models(tmp_path, impl, _models(family, model), names)
    dec = Decoder(models_dir=root, implementation=impl, n_iter=15)
    feats = [x.T for x in utts]
    counts = [len(t) for t in truth]
    want_words = [[names[w] for w in t] for t in truth]
    free = dec.decode_connected(feats)
    assert "level_log_likelihoods" not in free[0] and "strings" not in free[0]
    known = dec.decode_connected(feats, n_words=counts)
    assert [row["words"] for row in known] == want_words            # the end-to-end claim
    L = max(counts)
    assert all(len(row["level_log_likelihoods"]) == L for row in known)
    for row, f, k in zip(known, free, counts):
        assert row["log_likelihood"] == f["log_likelihood"] == row["level_log_likelihoods"][k - 1]
        assert row["segments"] == f["segments"] and np.array_equal(row["state_sequence"], f["state_sequence"])
    # one word more than spoken, under the bound of 8
    more = dec.decode_connected(feats, n_words=[k + 1 for k in counts], max_words=8)
    longer = 0
    for row, f, k in zip(more, free, counts):
        if np.isfinite(row["log_likelihood"]):
            longer += 1
            assert len(row["words"]) == len(row["segments"]) == k + 1
            assert row["log_likelihood"] < f["log_likelihood"]
            assert row["log_likelihood"] == row["level_log_likelihoods"][k]
        else:
            assert row["words"] == [] and row["level_log_likelihoods"][k] == NEG
    assert longer >= len(counts) // 2
    # the N-best list, beside the confidences on the same emission
    best = dec.decode_connected(feats, max_words=6, nbest=True, confidence=True)
    for row, f, m in zip(best, free, more):
        lls = [s["log_likelihood"] for s in row["strings"]]
        assert lls == sorted(lls, reverse=True) and len(lls) == int(np.isfinite(row["level_log_likelihoods"]).sum())
        assert sorted(len(s["words"]) for s in row["strings"]) == [
            k + 1 for k, v in enumerate(row["level_log_likelihoods"]) if np.isfinite(v)]
        top = row["strings"][0]
        assert (top["words"], top["log_likelihood"], top["segments"]) == (row["words"], row["log_likelihood"],
                                                                          row["segments"])
        assert row["words"] == f["words"] and row["log_likelihood"] == f["log_likelihood"]
        assert row["level_log_likelihoods"] == m["level_log_likelihoods"][:6]
        assert len(row["confidence"]) == len(row["segments"]) and np.isfinite(row["total_log_likelihood"])
    # exactly the restatement over the logb the device emitted
    net = ConnectedNetwork.from_models([dec.models[w] for w in dec.vocab], names=dec.vocab, implementation=impl)
    assert net.family == family
    emit = {"diag": connected.emit_diag, "gmm": connected.emit_gmm, "full": connected.emit_full}[family]
    logb = emit(torch.from_numpy(np.concatenate(utts)).cuda(), net).cpu().numpy().reshape(-1, W, net.SP)[:, :, :S]
    lengths = [len(x) for x in utts]
    batch = lref.Batch(logb, lengths, net.log_start, net.log_trans, net.log_exit, *net.loop_lm(), 8)
    score, n_words, pw, ps, pe = batch.select([k + 1 for k in counts], [k + 1 for k in counts])
    offs = np.r_[0, np.cumsum(lengths)]
    for u, row in enumerate(more):
        lo, hi = offs[u], offs[u + 1]
        assert row["level_log_likelihoods"] == batch.level_score[u].tolist()
        assert row["log_likelihood"] == score[u]
        segs = bref.segments(pw[lo:hi], pe[lo:hi]) if n_words[u] else []
        assert row["segments"] == [(dec.vocab[w], a, b) for w, a, b in segs]
        assert np.array_equal(row["state_sequence"], ps[lo:hi])

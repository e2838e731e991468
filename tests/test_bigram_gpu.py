"""GPU: connected-word decoding under a word bigram or grammar (csrc/connected_bigram.hip) through the Python layer
against the CPU restatement tests/_bigram_ref.py, which is the definition.  The recursion is float64 adds and compares
only, so every comparison to the restatement is ``np.array_equal``; the end-to-end test feeds the device's own emitted
``logb`` to the restatement for the same reason."""
import pickle

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _bigram_ref as bref
from tests import _connected_ref as ref

pytestmark = pytest.mark.gpu

NEG = -np.inf
FIELDS = ("score", "n_words", "path_word", "path_state", "path_entry")
# RL = 1; RL = 2 (word 6 straddles lanes 63 / 64); RL = 4, R = 252 twice; R = 250; R = 256 and the largest lm; padded
SHAPES = [(3, 4), (11, 10), (11, 18), (14, 18), (25, 10), (64, 4), (5, 7), (2, 1),
          (3, 12), (17, 3), (4, 11)]                # (RL, SP) = (1, 18), (2, 4), (2, 18): with the rest, all nine
LENGTHS = [3, 40, 1, 65, 0, 17, 2, 64, 33]          # 9 utterances: not a multiple of the 4 a workgroup serves


def _net(ls, lt, lx, lm):
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    return ConnectedNetwork(ls, lt, lx, bigram=WordBigram(*lm))


def _assert_equal(res, want, what):
    for f, w in zip(FIELDS, want):
        assert np.array_equal(getattr(res, f), w), (what, f)


@pytest.mark.parametrize("exits", ["last", "any"])
@pytest.mark.parametrize("topology", ["bidiag", "dense"])
@pytest.mark.parametrize("W,S", SHAPES)
def test_recursion_equals_restatement(W, S, topology, exits):
    """Random ``logb``; ``lm`` dense random with about a third of the pairs forbidden and one unreachable word (an
    all -inf column and -inf in ``lm_start``)."""
    from sapr_amd.connected import connected_viterbi
    rng = np.random.default_rng(100 * W + S + (topology == "dense") + 2 * (exits == "any"))
    ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
    dead = W // 2
    lm = bref.random_lm(rng, W, dead_word=dead)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    res = connected_viterbi(logb, LENGTHS, _net(ls, lt, lx, lm))
    want = bref.viterbi_batch(logb, LENGTHS, ls, lt, lx, *lm)
    _assert_equal(res, want, (W, S, topology, exits))
    assert res.score[LENGTHS.index(0)] == NEG and res.n_words[LENGTHS.index(0)] == 0
    assert not (res.path_word == dead).any() or W == 1
    if exits == "any" and W > 2:
        assert np.isfinite(res.score[np.asarray(LENGTHS) > 0]).all()


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


def test_word_loop_identity_on_the_device(emitted):
    from sapr_amd.connected import ConnectedNetwork, connected_viterbi
    model, _, logb, host, lengths = emitted
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    W = tabs[0].shape[0]
    for p in (0.0, -7.25):
        loop = connected_viterbi(logb, lengths, ConnectedNetwork(*tabs, word_penalty=p))
        got = connected_viterbi(logb, lengths, _net(*tabs, bref.word_loop_lm(W, p)))
        assert got.score.tobytes() == loop.score.tobytes(), p
        assert np.isfinite(got.score).all()
        if p == 0.0:
            for f in FIELDS:
                assert np.array_equal(getattr(got, f), getattr(loop, f)), f
        _assert_equal(got, bref.viterbi_batch(host, lengths, *tabs, *bref.word_loop_lm(W, p)), p)


def test_chain_identity_on_the_device(emitted):
    from sapr_amd.connected import ConnectedNetwork, align_viterbi, connected_viterbi
    model, _, logb, host, lengths = emitted
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    W = tabs[0].shape[0]
    for words, p in (([4], 0.0), ([7, 2], -3.5), ([9, 0, 3, 6], -3.5)):
        al = align_viterbi(logb, lengths, [words] * len(lengths), ConnectedNetwork(*tabs, word_penalty=p))
        got = connected_viterbi(logb, lengths, _net(*tabs, bref.chain_lm(W, words, p)))
        assert got.score.tobytes() == al.score.tobytes(), words
        for f in ("path_word", "path_state", "path_entry"):
            assert np.array_equal(getattr(got, f), getattr(al, f)), (words, f)
        finite = np.isfinite(got.score)
        assert (got.n_words[finite] == len(words)).all() and (got.n_words[~finite] == 0).all()
        if len(words) == 4:     # utterances of fewer than 40 frames cannot hold 4 words of 10 states
            assert finite.any() and (~finite).any()


def test_exact_ties_go_to_the_lowest_index():
    from sapr_amd.connected import connected_viterbi
    logb, ls, lt, lx, lm, lm0, lm1, expected = bref.tie_case()
    res = connected_viterbi(np.concatenate([logb, logb]), [4, 4], _net(ls, lt, lx, (lm, lm0, lm1)))
    assert res.score.tolist() == [expected[0]] * 2 and res.n_words.tolist() == [expected[1]] * 2
    assert res.path_word.tolist() == expected[2].tolist() * 2
    assert res.path_state.tolist() == expected[3].tolist() * 2
    assert res.path_entry.tolist() == expected[4].tolist() * 2


def test_utterances_are_isolated_and_runs_repeat():
    from sapr_amd.connected import connected_viterbi
    W, S = 11, 10
    rng = np.random.default_rng(17)
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    lm = bref.random_lm(rng, W, dead_word=3)
    net = _net(ls, lt, lx, lm)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    offs = np.r_[0, np.cumsum(LENGTHS)]
    a, b = connected_viterbi(logb, LENGTHS, net), connected_viterbi(logb, LENGTHS, net)
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for u in (1, 3, 8):
        lo, hi = offs[u], offs[u + 1]
        one = connected_viterbi(logb[lo:hi], [LENGTHS[u]], net)
        assert one.score.tobytes() == a.score[u:u + 1].tobytes() and one.n_words[0] == a.n_words[u]
        for f in FIELDS[2:]:
            assert np.array_equal(getattr(one, f), getattr(a, f)[lo:hi]), (u, f)
    # a NaN frame in utterance 3 (65 frames): every other utterance keeps its bytes
    bad = logb.copy()
    bad[offs[3] + 20] = np.nan
    c = connected_viterbi(bad, LENGTHS, net)
    keep = np.ones(len(logb), bool)
    keep[offs[3]:offs[4]] = False
    others = np.arange(len(LENGTHS)) != 3
    assert c.score[others].tobytes() == a.score[others].tobytes()
    assert np.array_equal(c.n_words[others], a.n_words[others])
    for f in FIELDS[2:]:
        assert getattr(c, f)[keep].tobytes() == getattr(a, f)[keep].tobytes(), f
    pw, ps = c.path_word[offs[3]:offs[4]], c.path_state[offs[3]:offs[4]]
    assert pw.min() >= -1 and pw.max() <= W - 1 and ps.min() >= -1 and ps.max() <= S - 1


# ---- end to end: Decoder.decode_connected(bigram=...) over the three emission families ---------------
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
def test_decoder_decodes_the_sampled_strings_under_the_grammar(tmp_path, family, impl):
    """Words 2 and 3 share their Gaussians; word 2 occurs only after word 0 and word 3 only after word 1.  Under the
    grammar ``Decoder.decode_connected`` returns the sampled strings; the word loop cannot."""
    import torch
    from sapr_amd import connected
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    from sapr_amd.decoder import Decoder
    seed, W, S, D, n = bref.E2E_CASE
    model, utts, truth, _ = bref.sample_bigram_case(seed, W, S, D, n, bigram=bref.e2e_bigram(),
                                                    shared=bref.E2E_SHARED)
    names = ["zero", "one", "two", "three"]
    root = _pickle_models(tmp_path, impl, _models(family, model), names)
    dec = Decoder(models_dir=root, implementation=impl, n_iter=15)
    pos = {c: dec.vocab.index(names[c]) for c in range(W)}       # load order (glob) is the word order of the network
    bigram = WordBigram.from_grammar(W, [(pos[a], pos[b]) for a, b in bref.E2E_PAIRS],
                                     starts=[pos[a] for a in bref.E2E_STARTS])
    feats = [x.T for x in utts]
    got = dec.decode_connected(feats, bigram=bigram)
    want_words = [[names[w] for w in t] for t in truth]
    assert [row["words"] for row in got] == want_words           # the end-to-end claim
    # exactly the restatement over the logb the device emitted
    net = ConnectedNetwork.from_models([dec.models[w] for w in dec.vocab], names=dec.vocab, implementation=impl,
                                       bigram=bigram)
    assert net.family == family
    emit = {"diag": connected.emit_diag, "gmm": connected.emit_gmm, "full": connected.emit_full}[family]
    logb = emit(torch.from_numpy(np.concatenate(utts)).cuda(), net).cpu().numpy().reshape(-1, W, net.SP)[:, :, :S]
    lengths = [len(x) for x in utts]
    score, n_words, pw, ps, pe = bref.viterbi_batch(logb, lengths, net.log_start, net.log_trans, net.log_exit,
                                                    bigram.lm, bigram.lm_start, bigram.lm_end)
    offs = np.r_[0, np.cumsum(lengths)]
    for u, row in enumerate(got):
        lo, hi = offs[u], offs[u + 1]
        segs = bref.segments(pw[lo:hi], pe[lo:hi])
        assert row["segments"] == [(dec.vocab[w], a, b) for w, a, b in segs]
        assert np.array_equal(row["state_sequence"], ps[lo:hi])
        assert row["log_likelihood"] == score[u]
    # a word penalty goes through WordBigram.scaled: the same call on the scaled bigram
    pen = dec.decode_connected(feats, word_penalty=-30.0, bigram=bigram)
    res = connected.connected_decode(utts, ConnectedNetwork.from_models(
        [dec.models[w] for w in dec.vocab], names=dec.vocab, implementation=impl, bigram=bigram.scaled(1.0, -30.0)))
    assert [row["log_likelihood"] for row in pen] == res.score.tolist()
    # without the grammar the word loop gets an utterance with word 2 or 3 wrong
    free = dec.decode_connected(feats)
    assert any(a["words"] != b["words"] and (2 in t or 3 in t) for a, b, t in zip(got, free, truth))
    if family == "diag":        # a list of transcripts of word names is a bigram too
        soft = dec.decode_connected(feats, bigram=want_words)
        same = connected.connected_decode(utts, ConnectedNetwork.from_models(
            [dec.models[w] for w in dec.vocab], names=dec.vocab, implementation=impl,
            bigram=WordBigram.from_transcripts([[pos[w] for w in t] for t in truth], W)))
        assert [row["log_likelihood"] for row in soft] == same.score.tolist()

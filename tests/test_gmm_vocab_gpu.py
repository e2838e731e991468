"""GPU: scoring over the vocabulary for the Gaussian-mixture HMMs (csrc/gmm_vocab.hip: sapr_gmm_vocab_diag,
gmm_hmm.vocab_scores, Decoder(implementation="gmmhmm")) against the numpy restatement tests/_gmmhmm_ref.py looped over
the words, on the seeded cases of tests/_gmmhmm_cases.py (18-48 utterances of 12-89 frames, 3 words; reference results
computed once per case), and against the per-model entry points bit for bit.

The definition of a score: ``forward_backward(...)[0]`` over ``_lse(log_components(...), axis=2)`` (forward mode) and
``viterbi(...)[0]`` (Viterbi mode) of the restatement.  Tolerance: rtol 1e-11 on scores, the project's pin for forward
and Viterbi scores.  The best word must equal the reference's on EVERY utterance: the reference's top-two word gap over
all utterances with frames, computed on the CPU from the reference alone, is

    case                  forward   Viterbi
    d13_s10_m2_bidiag     250       251
    d5_s3_m3_dense        1.11      0.92
    d39_s18_m2_bidiag     1920      1920
    d13_s4_m8_dense       282       289
    d26_s6_m1_dense       50.5      53.0

and the largest |score| is 2.1e4, so rtol 1e-11 moves a score by less than 2.1e-7 and cannot flip a word.  Columns
against the per-model entry points (GmmBatch.estep / .viterbi with utt_model = w) are compared with np.array_equal: the
kernels share their device functions (csrc/gmm_ops.h) and the build never contracts, so no tolerance applies."""
import functools
import pickle

import numpy as np
import pytest

from tests import _gmmhmm_cases as gc
from tests import _gmmhmm_ref as ref
from tests._synth import VOCAB

pytestmark = pytest.mark.gpu

RTOL = 1e-11
MULTI = ["d13_s10_m2_bidiag", "d5_s3_m3_dense", "d39_s18_m2_bidiag", "d13_s4_m8_dense", "d26_s6_m1_dense"]
MODES = ("forward", "viterbi")


# ---- the reference, looped over the words ---------------------------------------------------------------------------
def _ref_pair(x, prm, mode):
    """The reference's score of one utterance [T, D] float32 under one model; no frames: -inf."""
    if x.shape[0] == 0:
        return -np.inf
    if mode == "viterbi":
        return ref.viterbi(x, *prm)[0]
    sp, A, wt, mu, cv = prm
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    return ref.forward_backward(sp, A, ref._lse(ref.log_components(x64, wt, mu, cv), axis=2))[0]


def _ref_matrix(utts, params, mode):
    return np.array([[_ref_pair(x, prm, mode) for prm in params] for x in utts], dtype=np.float64)


def _first_strict_max(scores):
    """decoder.py:42-47 on the rows of a score matrix: from -inf, first strict maximum in model order; -1 if none."""
    out = np.full(scores.shape[0], -1, dtype=np.int64)
    for u, row in enumerate(scores):
        best = -np.inf
        for w, sc in enumerate(row):
            if sc > best:
                best, out[u] = sc, w
    return out


def _flat(c):
    return [x for lst in c["utts"] for x in lst]


@functools.lru_cache(maxsize=None)
def _reference(name, models_of=None):
    """{mode: (score[N, W], best_word[N])} for the utterances of case ``name`` under the models of ``models_of``."""
    params = gc.case(models_of or name)["params"]
    out = {}
    for mode in MODES:
        sc = _ref_matrix(_flat(gc.case(name)), params, mode)
        out[mode] = (sc, _first_strict_max(sc))
    return out


# ---- the device ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_scores(name):
    """{mode: (score, best_word)} as host arrays: one launch per mode over the case's three models."""
    from sapr_amd import gmm_hmm as gh
    c = gc.case(name)
    pack = gh.GmmPack.from_params(c["params"])
    out = {}
    for mode in MODES:
        vs = gh.vocab_scores(c["feats"], c["lengths"], pack, mode=mode)
        assert vs.word_post is None
        out[mode] = (vs.score.cpu().numpy(), vs.best_word.cpu().numpy())
    return out


def _report(tag, got, want):
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    print(f"{tag}: max relative error vs the reference {err.max():.3e} over {int(fin.sum())} finite scores")


@pytest.mark.parametrize("name", MULTI)
def test_scores_and_best_word_match_the_reference(name):
    import torch
    from sapr_amd import gmm_hmm as gh
    from sapr_amd.trellis import FeatureBatch
    c = gc.case(name)
    N = len(c["lengths"])
    want, got = _reference(name), _gpu_scores(name)
    for mode in MODES:
        rsc, rbw = want[mode]
        sc, bw = got[mode]
        assert sc.shape == (N, 3) and sc.dtype == np.float64 and bw.dtype == np.int32
        _report(f"{name} {mode}", sc, rsc)
        np.testing.assert_allclose(sc, rsc, rtol=RTOL)
        print(f"{name} {mode}: best word differs on {int((bw != rbw).sum())} of {N} utterances")
        np.testing.assert_array_equal(bw, rbw)          # every utterance, none left out
    if name == "d5_s3_m3_dense":     # word 0 carries an utterance of one frame and one of none after its own
        last = len(c["utts"][0]) - 1
        assert c["lengths"][last] == 0 and c["lengths"][last - 1] == 1
        for mode in MODES:
            sc, bw = got[mode]
            assert np.all(sc[last] == -np.inf) and bw[last] == -1
            assert np.all(np.isfinite(sc[last - 1])) and bw[last - 1] == want[mode][1][last - 1] >= 0
    # a trellis.FeatureBatch brings its own order and (D = 5, 26) zero columns that are cut off again: the same bits
    fb = FeatureBatch.from_packed(torch.from_numpy(c["feats"]).cuda(), c["lengths"])
    vs = gh.vocab_scores(fb, None, gh.GmmPack.from_params(c["params"]), mode="forward")
    assert np.array_equal(vs.score.cpu().numpy(), got["forward"][0])
    assert np.array_equal(vs.best_word.cpu().numpy(), got["forward"][1])


@pytest.mark.parametrize("name", MULTI)
def test_columns_carry_the_bits_of_the_per_model_entry_points(name):
    from sapr_amd import gmm_hmm as gh
    c = gc.case(name)
    N = len(c["lengths"])
    pack = gh.pack_models(c["params"])
    got = _gpu_scores(name)
    for w in range(3):
        batch = gh.GmmBatch(c["feats"], c["lengths"], np.full(N, w), 3, c["S"], c["M"])
        loglik = batch.estep(pack, want_stats=False)[0].cpu().numpy()
        logprob = batch.viterbi(pack)[0].cpu().numpy()
        assert np.array_equal(got["forward"][0][:, w], loglik), (name, w, "forward")
        assert np.array_equal(got["viterbi"][0][:, w], logprob), (name, w, "viterbi")


def _launch(feats, offsets, order, n_utts, max_T, pack, mode, want_post=False):
    """sapr_gmm_vocab_diag itself, with the caller's ``order``."""
    import torch
    from sapr_amd import _lib
    dev = feats.device
    score = torch.empty((n_utts, pack.W), dtype=torch.float64, device=dev)
    bw = torch.empty(n_utts, dtype=torch.int32, device=dev)
    post = torch.empty((n_utts, pack.W), dtype=torch.float64, device=dev) if want_post else None
    _lib.check(_lib.load().sapr_gmm_vocab_diag(
        _lib.ptr(feats), _lib.ptr(offsets), _lib.ptr(order), n_utts, int(feats.shape[0]), pack.D, max_T,
        _lib.ptr(pack.device(dev)), pack.W, pack.S, pack.M, mode, _lib.ptr(score), _lib.ptr(bw), _lib.ptr(post),
        _lib.current_stream()), "sapr_gmm_vocab_diag")
    return score, bw, post


def test_tiles_order_and_determinism():
    """300 utterances (two tiles and a part) of d5_s3_m3_tiles under the three models of d5_s3_m3_dense."""
    import torch
    from sapr_amd import _lib, gmm_hmm as gh
    c = gc.case("d5_s3_m3_tiles")
    N = len(c["lengths"])
    assert N == 300
    pack = gh.GmmPack.from_params(gc.case("d5_s3_m3_dense")["params"])
    feats, offsets, order, lengths, max_T = gh.vocab_features(c["feats"], c["lengths"])
    want = _reference("d5_s3_m3_tiles", "d5_s3_m3_dense")
    for mode, code in (("forward", _lib.GMM_VOCAB_FORWARD), ("viterbi", _lib.GMM_VOCAB_VITERBI)):
        a = _launch(feats, offsets, None, N, max_T, pack, code)
        sc, bw = a[0].cpu().numpy(), a[1].cpu().numpy()
        _report(f"tiles {mode}", sc, want[mode][0])
        np.testing.assert_allclose(sc, want[mode][0], rtol=RTOL)
        np.testing.assert_array_equal(bw, _first_strict_max(sc))
        rev = torch.flip(torch.arange(N, dtype=torch.int32, device=feats.device), dims=[0]).contiguous()
        for other in (_launch(feats, offsets, None, N, max_T, pack, code),          # a second launch: the same bits
                      _launch(feats, offsets, order, N, max_T, pack, code),         # the length-sorted order
                      _launch(feats, offsets, rev, N, max_T, pack, code)):          # a reversed one
            assert torch.equal(other[0], a[0]) and torch.equal(other[1], a[1])
        vs = gh.vocab_scores(c["feats"], c["lengths"], pack, mode=mode)
        assert torch.equal(vs.score, a[0]) and torch.equal(vs.best_word, a[1])


def test_ties_and_posteriors():
    """Model 3 is a copy of model 1 (an exact tie: the first one must win), model 4 is model 1 with its means shifted
    by 0.01 (a runner-up with a posterior above zero)."""
    import torch
    from sapr_amd import gmm_hmm as gh
    c = gc.case("d13_s10_m2_bidiag")
    p = c["params"]
    near = (p[1][0], p[1][1], p[1][2], p[1][3] + 0.01, p[1][4])
    pack = gh.GmmPack.from_params([p[0], p[1], p[2], p[1], near])
    fs = gh.vocab_scores(c["feats"], c["lengths"], pack, mode="forward", want_post=True)
    assert fs.score.shape == fs.word_post.shape == (len(c["lengths"]), 5)
    assert torch.equal(fs.score[:, 1], fs.score[:, 3])
    assert not bool((fs.best_word == 3).any()) and bool((fs.best_word == 1).any())
    assert torch.equal(fs.word_post[:, 1], fs.word_post[:, 3])
    ll = fs.score.cpu()
    assert bool(torch.isfinite(ll).all())
    post = fs.word_post.cpu().numpy()
    want = torch.softmax(ll, dim=1).numpy()                # float64 soft-max of the device's own scores
    np.testing.assert_allclose(post, want, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0.0, atol=1e-12)
    # the Viterbi scores tie in the same way; without posteriors the same scores and words
    vs = gh.vocab_scores(c["feats"], c["lengths"], pack, mode="viterbi")
    assert torch.equal(vs.score[:, 1], vs.score[:, 3]) and not bool((vs.best_word == 3).any())
    lean = gh.vocab_scores(c["feats"], c["lengths"], pack, mode="forward")
    assert lean.word_post is None and torch.equal(lean.score, fs.score) and torch.equal(lean.best_word, fs.best_word)
    with pytest.raises(ValueError):
        gh.vocab_scores(c["feats"], c["lengths"], pack, mode="viterbi", want_post=True)


def test_padded_vocabulary():
    """Word 1 of d5_s3_m3_dense as a two-state model (slice and renormalise), packed with the others at S = 3."""
    from sapr_amd import gmm_hmm as gh
    c = gc.case("d5_s3_m3_dense")
    sp, A, wt, mu, cv = c["params"][1]
    two = (sp[:2] / sp[:2].sum(), A[:2, :2] / A[:2, :2].sum(axis=1, keepdims=True), wt[:2], mu[:2], cv[:2])
    pack = gh.GmmPack.from_params([c["params"][0], two, c["params"][2]])
    assert (pack.S, pack.n_states) == (3, [3, 2, 3])
    full = _gpu_scores("d5_s3_m3_dense")
    utts = _flat(c)
    for mode in MODES:
        sc = gh.vocab_scores(c["feats"], c["lengths"], pack, mode=mode).score.cpu().numpy()
        want = np.array([_ref_pair(x, two, mode) for x in utts])
        _report(f"two-state model, {mode}", sc[:, 1], want)
        np.testing.assert_allclose(sc[:, 1], want, rtol=RTOL)
        assert np.array_equal(sc[:, [0, 2]], full[mode][0][:, [0, 2]])       # the neighbours keep their bits


def _model_dir(tmp_path, params, n_iter=15):
    from sapr_amd import GMMHMM
    d = tmp_path / "trained_models" / "gmmhmm"
    d.mkdir(parents=True)
    for word, prm in zip(VOCAB, params):
        S, M = prm[2].shape
        m = GMMHMM(n_components=S, n_mix=M, init_params="")
        m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_ = prm
        with open(d / f"{word}_gmmhmm_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


@pytest.mark.parametrize("name", ["d5_s3_m3_dense", "d13_s10_m2_bidiag"])
def test_decoder_gmmhmm(tmp_path, name):
    from sapr_amd import gmm_hmm as gh
    from sapr_amd.decoder import Decoder
    c = gc.case(name)
    utts = _flat(c)
    flat = [np.ascontiguousarray(x.T) for x in utts]                 # (D, T) arrays, as mfcc_extract stores them
    dec = Decoder(models_dir=_model_dir(tmp_path, c["params"]), implementation="gmmhmm")
    order = [VOCAB.index(w) for w in dec.vocab]                      # load order (glob) decides ties and the word index
    assert sorted(order) == [0, 1, 2]
    params = [c["params"][m] for m in order]
    want = _reference(name)
    rvit, rfwd = want["viterbi"][0][:, order], want["forward"][0][:, order]
    vbw, fbw = _first_strict_max(rvit), _first_strict_max(rfwd)
    pack = dec._vocab_pack()
    launch = {mode: gh.vocab_scores(c["feats"], c["lengths"], pack, mode=mode).score.cpu().numpy() for mode in MODES}

    def check(got, rsc, rbw, mode):
        assert len(got) == len(utts)
        for u, (word, score, states) in enumerate(got):
            w = rbw[u]
            if w < 0:                                                # no frames: no word
                assert utts[u].shape[0] == 0 and (word, score, states) == (None, -np.inf, None)
                continue
            assert word == dec.vocab[w]
            assert abs(score - rsc[u, w]) <= RTOL * abs(rsc[u, w])
            assert score == launch[mode][u, w]                       # the vocabulary launch's score, bit for bit
            _, path, gap = ref.viterbi(utts[u], *params[w])          # the path of the chosen word only
            assert gap > 1e-9
            np.testing.assert_array_equal(states, path)

    got = dec.decode_batch(flat)
    check(got, rvit, vbw, "viterbi")
    fwd = Decoder(models_dir=str(tmp_path / "trained_models"), implementation="gmmhmm", scoring="forward")
    assert fwd.vocab == dec.vocab
    check(fwd.decode_batch(flat), rfwd, fbw, "forward")
    # score_batch / nbest: forward mode with posteriors
    sc = dec.score_batch(flat)
    assert sc.shape == (len(utts), 3) and sc.dtype == np.float64
    np.testing.assert_allclose(sc, rfwd, rtol=RTOL)
    assert np.array_equal(sc, launch["forward"])
    nb = dec.nbest(flat, n=2)
    assert len(nb) == len(utts) and all(len(r) == 2 for r in nb)
    for u, row in enumerate(nb):
        if fbw[u] < 0:
            continue
        assert row[0][0] == dec.vocab[fbw[u]] and row[0][1] == sc[u, fbw[u]] and row[0][1] >= row[1][1]
        assert 0.0 <= row[1][2] <= row[0][2] <= 1.0
    # state posteriors under the decoder's word, and under a named one
    live = [u for u in range(len(utts)) if utts[u].shape[0] > 0]
    post = dec.state_posteriors(flat)
    named = dec.state_posteriors(flat, words=[dec.vocab[1]] * len(utts))
    for u, (p, q) in enumerate(zip(post, named)):
        assert p.shape == q.shape == (utts[u].shape[0], c["S"]) and p.dtype == np.float64
        if utts[u].shape[0]:
            np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=0.0, atol=1e-9)
            np.testing.assert_allclose(q.sum(axis=1), 1.0, rtol=0.0, atol=1e-9)
    for w, word in enumerate(dec.vocab):
        own = [u for u in live if vbw[u] == w]
        for sel, res in ((own, post), (live if w == 1 else [], named)):
            if not sel:
                continue
            pp = dec.models[word].predict_proba(np.concatenate([utts[u] for u in sel], axis=0),
                                                [utts[u].shape[0] for u in sel])
            assert np.array_equal(np.concatenate([res[u] for u in sel], axis=0), pp)
    with pytest.raises(ValueError):
        dec.state_posteriors(flat[:2], words=["who", dec.vocab[0]])
    # the reference's API on one (T, D) view
    word, score, states = dec.decode_sequence(utts[0])
    assert (word, score) == got[0][:2]
    np.testing.assert_array_equal(states, got[0][2])

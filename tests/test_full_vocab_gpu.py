"""GPU: scoring over the vocabulary for the full-covariance HMMs (csrc/full_vocab.hip: sapr_full_vocab,
full_cov.vocab_scores, Decoder(implementation="hmmlearn") over full / tied models) against the numpy restatement
tests/_fullcov_ref.py looped over the words, on the seeded cases of tests/_full_vocab_cases.py (18-300 utterances of
0-89 frames, 2-3 words; reference results computed once per case), and against the per-model entry points bit for bit.

The definition of a score: ``forward_backward(sp, A, log_density(x64, mu, cv))[0]`` (forward mode) and
``viterbi(...)[0]`` (Viterbi mode) of the restatement.  Tolerance: rtol 1e-11 on scores, the project's pin for forward
and Viterbi scores.  The best word must equal the reference's on EVERY utterance: from the reference alone
(tests/test_full_vocab_cpu.py asserts it) the smallest top-two word gap of a case is 2.26 at a largest |score| of
1.5e3, and over all cases the largest |score| is 8.6e4, so rtol 1e-11 moves a score by less than 9e-7 and cannot flip a
word; no arg-max on a winner's Viterbi path is within a relative 1e-9 (smallest: 2.3e-6), so every path is compared
too.  Columns against the per-model entry points (FullCovBatch.estep / .viterbi with utt_model = w) are compared with
np.array_equal: the kernels share their device functions (csrc/fullcov_emit.h, csrc/gmm_ops.h) and the build never
contracts, so no tolerance applies."""
import functools
import pickle

import numpy as np
import pytest

from tests import _full_vocab_cases as vc
from tests import _fullcov_ref as ref
from tests._synth import VOCAB

pytestmark = pytest.mark.gpu

RTOL = 1e-11
MODES = vc.MODES
ALL = list(vc.CASES)


@functools.lru_cache(maxsize=None)
def _gpu_scores(name):
    """{mode: (score, best_word)} as host arrays: one launch per mode over the case's models."""
    from sapr_amd import full_cov
    c = vc.case(name)
    pack = full_cov.FullPack.from_params(c["params"])
    out = {}
    for mode in MODES:
        vs = full_cov.vocab_scores(c["feats"], c["lengths"], pack, mode=mode)
        assert vs.word_post is None
        out[mode] = (vs.score.cpu().numpy(), vs.best_word.cpu().numpy())
    return out


def _report(tag, got, want):
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    print(f"{tag}: max relative error vs the reference {err.max():.3e} over {int(fin.sum())} finite scores")


@pytest.mark.parametrize("name", ALL)
def test_scores_and_best_word_match_the_reference(name):
    c = vc.case(name)
    N, W = len(c["lengths"]), len(c["params"])
    want, got = vc.reference(name), _gpu_scores(name)
    for mode in MODES:
        rsc, rbw = want[mode]
        sc, bw = got[mode]
        assert sc.shape == (N, W) and sc.dtype == np.float64 and bw.dtype == np.int32
        _report(f"{name} {mode}", sc, rsc)
        np.testing.assert_allclose(sc, rsc, rtol=RTOL)
        print(f"{name} {mode}: best word differs on {int((bw != rbw).sum())} of {N} utterances")
        np.testing.assert_array_equal(bw, rbw)          # every utterance, none left out
    if name == "d5_s3_dense":        # word 0 carries an utterance of one frame and one of none after its own
        last = len(c["utts"][0]) - 1
        assert c["lengths"][last] == 0 and c["lengths"][last - 1] == 1
        for mode in MODES:
            sc, bw = got[mode]
            assert np.all(sc[last] == -np.inf) and bw[last] == -1
            assert np.all(np.isfinite(sc[last - 1])) and bw[last - 1] == want[mode][1][last - 1] >= 0
    if name == "d13_s4_dense_300":
        assert N == 300                                  # two tiles, the second partial


@pytest.mark.parametrize("name", ALL)
def test_columns_carry_the_bits_of_the_per_model_entry_points(name):
    from sapr_amd import full_cov
    c = vc.case(name)
    N, W = len(c["lengths"]), len(c["params"])
    pack = full_cov.pack_models(c["params"])
    got = _gpu_scores(name)
    for w in range(W):
        batch = full_cov.FullCovBatch(c["feats"], c["lengths"], np.full(N, w), W, c["S"])
        loglik = batch.estep(pack, want_stats=False)[0].cpu().numpy()
        logprob = batch.viterbi(pack)[0].cpu().numpy()
        assert np.array_equal(got["forward"][0][:, w], loglik), (name, w, "forward")
        assert np.array_equal(got["viterbi"][0][:, w], logprob), (name, w, "viterbi")


def _launch(feats, offsets, order, n_utts, max_T, pack, mode, want_post=False):
    """sapr_full_vocab itself, with the caller's ``order``."""
    import ctypes
    import torch
    from sapr_amd import _lib
    dev = feats.device
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    _lib.check(lib.sapr_full_vocab_workspace_bytes(n_utts, int(feats.shape[0]), pack.W, pack.S, pack.D,
                                                   ctypes.byref(n)), "sapr_full_vocab_workspace_bytes")
    ws = torch.empty(int(n.value), dtype=torch.uint8, device=dev) if n.value else None
    score = torch.empty((n_utts, pack.W), dtype=torch.float64, device=dev)
    bw = torch.empty(n_utts, dtype=torch.int32, device=dev)
    post = torch.empty((n_utts, pack.W), dtype=torch.float64, device=dev) if want_post else None
    if n.value:     # a workspace that is too small is refused before a launch
        assert lib.sapr_full_vocab(
            _lib.ptr(feats), _lib.ptr(offsets), _lib.ptr(order), n_utts, int(feats.shape[0]), pack.D, max_T,
            _lib.ptr(pack.device(dev)), pack.W, pack.S, mode, _lib.ptr(ws), int(n.value) - 1, _lib.ptr(score),
            _lib.ptr(bw), _lib.ptr(post), _lib.current_stream()) == -1
        assert b"workspace too small" in lib.sapr_last_error()
    _lib.check(lib.sapr_full_vocab(
        _lib.ptr(feats), _lib.ptr(offsets), _lib.ptr(order), n_utts, int(feats.shape[0]), pack.D, max_T,
        _lib.ptr(pack.device(dev)), pack.W, pack.S, mode, _lib.ptr(ws), int(n.value), _lib.ptr(score), _lib.ptr(bw),
        _lib.ptr(post), _lib.current_stream()), "sapr_full_vocab")
    return score, bw, post


@pytest.mark.parametrize("name", ["d13_s4_dense_300", "d5_s3_dense", "d14_s5_dense"])
def test_order_feature_batch_and_determinism(name):
    """``order`` = None, the length-sorted order, a reversed one and a trellis.FeatureBatch with padded columns
    (D = 5 and 14 are padded to the single-Gaussian kernels' widths and cut off again) all give the same bits."""
    import torch
    from sapr_amd import _lib, full_cov
    from sapr_amd.gmm_hmm import vocab_features
    from sapr_amd.trellis import FeatureBatch
    c = vc.case(name)
    N = len(c["lengths"])
    pack = full_cov.FullPack.from_params(c["params"])
    feats, offsets, order, lengths, max_T = vocab_features(c["feats"], c["lengths"])
    got = _gpu_scores(name)
    fb = FeatureBatch.from_packed(torch.from_numpy(c["feats"]).cuda(), c["lengths"])
    for mode, code in (("forward", _lib.FULL_VOCAB_FORWARD), ("viterbi", _lib.FULL_VOCAB_VITERBI)):
        a = _launch(feats, offsets, None, N, max_T, pack, code)
        assert np.array_equal(a[0].cpu().numpy(), got[mode][0]) and np.array_equal(a[1].cpu().numpy(), got[mode][1])
        np.testing.assert_array_equal(a[1].cpu().numpy(), vc.first_strict_max(a[0].cpu().numpy()))
        rev = torch.flip(torch.arange(N, dtype=torch.int32, device=feats.device), dims=[0]).contiguous()
        for other in (_launch(feats, offsets, None, N, max_T, pack, code),          # a second launch: the same bits
                      _launch(feats, offsets, order, N, max_T, pack, code),         # the length-sorted order
                      _launch(feats, offsets, rev, N, max_T, pack, code)):          # a reversed one
            assert torch.equal(other[0], a[0]) and torch.equal(other[1], a[1])
        vs = full_cov.vocab_scores(fb, None, pack, mode=mode)
        assert torch.equal(vs.score, a[0]) and torch.equal(vs.best_word, a[1])


def test_unserved_utterances_and_order_entries_outside_the_batch():
    """An utterance longer than max_T is served as empty (-inf); an ``order`` entry outside the batch is never
    followed: its slot writes nothing."""
    import torch
    from sapr_amd import _lib, full_cov
    from sapr_amd.gmm_hmm import vocab_features
    c = vc.case("d5_s3_dense")
    N = len(c["lengths"])
    pack = full_cov.FullPack.from_params(c["params"])
    feats, offsets, order, lengths, max_T = vocab_features(c["feats"], c["lengths"])
    full = _gpu_scores("d5_s3_dense")["forward"][0]
    cut = int(lengths.max()) - 1                          # the longest utterance no longer fits
    sc = _launch(feats, offsets, None, N, cut, pack, _lib.FULL_VOCAB_FORWARD)[0].cpu().numpy()
    long = lengths > cut
    assert long.sum() >= 1 and np.all(np.isneginf(sc[long])) and np.array_equal(sc[~long], full[~long])
    bad = torch.arange(N, dtype=torch.int32, device=feats.device)
    bad[3], bad[5] = N + 7, -2
    score = torch.full((N, pack.W), 7.0, dtype=torch.float64, device=feats.device)
    _lib.check(_lib.load().sapr_full_vocab(
        _lib.ptr(feats), _lib.ptr(offsets), _lib.ptr(bad), N, int(feats.shape[0]), pack.D, max_T,
        _lib.ptr(pack.device(feats.device)), pack.W, pack.S, _lib.FULL_VOCAB_FORWARD, None, 0, _lib.ptr(score), None,
        None, _lib.current_stream()), "sapr_full_vocab")
    sc = score.cpu().numpy()
    keep = np.ones(N, bool)
    keep[[3, 5]] = False
    assert np.all(sc[~keep] == 7.0) and np.array_equal(sc[keep], full[keep])


def test_ties_and_posteriors():
    """Model 3 is a copy of model 1 (an exact tie: the first one must win), model 4 is model 1 with its means shifted
    by 0.01 (a runner-up with a posterior above zero).  word_post against exp(score - logsumexp) of the REFERENCE's
    scores at rtol 1e-9, and against the float64 soft-max of the device's own scores at 1e-12, which isolates the
    epilogue from the scores' own error."""
    import torch
    from sapr_amd import full_cov
    c = vc.case("d5_s3_dense")
    p = c["params"]
    near = (p[1][0], p[1][1], p[1][2] + 0.01, p[1][3])
    params = [p[0], p[1], p[2], p[1], near]
    pack = full_cov.FullPack.from_params(params)
    fs = full_cov.vocab_scores(c["feats"], c["lengths"], pack, mode="forward", want_post=True)
    N = len(c["lengths"])
    assert fs.score.shape == fs.word_post.shape == (N, 5)
    assert torch.equal(fs.score[:, 1], fs.score[:, 3])
    assert not bool((fs.best_word == 3).any()) and bool((fs.best_word == 1).any())
    live = c["lengths"] > 0
    ll, post = fs.score.cpu().numpy(), fs.word_post.cpu().numpy()
    assert np.array_equal(post[:, 1], post[:, 3], equal_nan=True)
    assert np.all(np.isnan(post[~live])) and np.all(np.isneginf(ll[~live]))      # the zero-frame row: NaN
    assert np.all(np.isfinite(ll[live]))
    own = torch.softmax(fs.score.cpu()[torch.from_numpy(live)], dim=1).numpy()   # soft-max of the device's own scores
    np.testing.assert_allclose(post[live], own, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(post[live].sum(axis=1), 1.0, rtol=0.0, atol=1e-12)
    rsc = vc.ref_scores(c["flat"], params)["forward"][0][live]
    m = rsc.max(axis=1, keepdims=True)
    want = np.exp(rsc - (m + np.log(np.exp(rsc - m).sum(axis=1, keepdims=True))))
    nz = want > 0
    print("word_post max relative error vs the reference", np.max(np.abs(post[live][nz] - want[nz]) / want[nz]))
    np.testing.assert_allclose(post[live], want, rtol=1e-9, atol=0.0)
    # the Viterbi scores tie in the same way; without posteriors the same scores and words
    vs = full_cov.vocab_scores(c["feats"], c["lengths"], pack, mode="viterbi")
    assert torch.equal(vs.score[:, 1], vs.score[:, 3]) and not bool((vs.best_word == 3).any())
    lean = full_cov.vocab_scores(c["feats"], c["lengths"], pack, mode="forward")
    assert lean.word_post is None and torch.equal(lean.score, fs.score) and torch.equal(lean.best_word, fs.best_word)
    with pytest.raises(ValueError):
        full_cov.vocab_scores(c["feats"], c["lengths"], pack, mode="viterbi", want_post=True)


@pytest.mark.parametrize("name", ["d5_s3_dense", "d27_s11_bidiag"])
def test_a_nan_frame_poisons_its_own_utterance_only(name):
    from sapr_amd import full_cov
    c = vc.case(name)
    pack = full_cov.FullPack.from_params(c["params"])
    offs = np.r_[0, np.cumsum(c["lengths"])]
    u = 4
    feats = c["feats"].copy()
    feats[offs[u] + c["lengths"][u] // 2, c["D"] - 1] = np.nan
    clean = _gpu_scores(name)
    for mode in MODES:
        vs = full_cov.vocab_scores(feats, c["lengths"], pack, mode=mode, want_post=mode == "forward")
        sc, bw = vs.score.cpu().numpy(), vs.best_word.cpu().numpy()
        assert np.all(np.isnan(sc[u])) and bw[u] == -1
        keep = np.arange(len(c["lengths"])) != u
        assert np.array_equal(sc[keep], clean[mode][0][keep]) and np.array_equal(bw[keep], clean[mode][1][keep])
        if mode == "forward":
            assert np.all(np.isnan(vs.word_post.cpu().numpy()[u]))


def _model(prm, ct):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    m = GaussianHMM(n_components=prm[2].shape[0], covariance_type=ct, init_params="")
    m.startprob_, m.transmat_, m.means_ = (np.array(a) for a in prm[:3])
    m.covars_ = vc.typed_covars(prm, ct)
    return m


def test_mixed_size_vocabulary():
    """Word 1 of d5_s3_dense as a two-state model (slice and renormalise), packed with the others at S = 3."""
    from sapr_amd import full_cov
    c = vc.case("d5_s3_dense")
    params, want = vc.mixed_size()
    pack = full_cov.FullPack.from_params(params)
    assert (pack.S, pack.n_states) == (3, [3, 2, 3])
    whole = _gpu_scores("d5_s3_dense")
    for mode in MODES:
        vs = full_cov.vocab_scores(c["feats"], c["lengths"], pack, mode=mode)
        sc, bw = vs.score.cpu().numpy(), vs.best_word.cpu().numpy()
        _report(f"mixed sizes, {mode}", sc, want[mode][0])
        np.testing.assert_allclose(sc, want[mode][0], rtol=RTOL)
        np.testing.assert_array_equal(bw, want[mode][1])
        assert np.array_equal(sc[:, [0, 2]], whole[mode][0][:, [0, 2]])       # the neighbours keep their bits


def test_mixed_type_vocabulary():
    """d5_s3_dense as {full, tied, diag} GaussianHMM objects: the tied and the diagonal model are packed as matrices."""
    from sapr_amd import full_cov
    c = vc.case("d5_s3_dense")
    params, want = vc.mixed_type()
    models = [_model(p, ct) for p, ct in zip(c["params"], vc.MIXED_TYPES)]
    whole = _gpu_scores("d5_s3_dense")
    for mode in MODES:
        vs = full_cov.vocab_scores(c["feats"], c["lengths"], models, mode=mode)
        sc, bw = vs.score.cpu().numpy(), vs.best_word.cpu().numpy()
        _report(f"mixed types, {mode}", sc, want[mode][0])
        np.testing.assert_allclose(sc, want[mode][0], rtol=RTOL)
        np.testing.assert_array_equal(bw, want[mode][1])
        # the case's start covariance is one matrix for every state: the tied model is the full one, bit for bit
        assert np.array_equal(sc[:, :2], whole[mode][0][:, :2])


def _model_dir(tmp_path, params, types, n_iter=15):
    d = tmp_path / "trained_models" / "hmmlearn"
    d.mkdir(parents=True)
    for word, prm, ct in zip(VOCAB, params, types):
        with open(d / f"{word}_hmmlearn_{n_iter}.pkl", "wb") as f:
            pickle.dump(_model(prm, ct), f)
    return str(tmp_path / "trained_models")


@pytest.mark.parametrize("name, types", [("d5_s3_dense", ("full", "tied", "full")),
                                         ("d13_s10_bidiag", ("full", "full", "full"))])
def test_decoder_over_full_covariance_models(tmp_path, name, types):
    """(The cases' start covariance is one matrix for every state, so a "tied" model is its "full" one and the
    reference of the case serves both.)"""
    from sapr_amd import full_cov
    from sapr_amd.decoder import Decoder
    c = vc.case(name)
    utts = c["flat"]
    flat = [np.ascontiguousarray(x.T) for x in utts]                 # (D, T) arrays, as mfcc_extract stores them
    dec = Decoder(models_dir=_model_dir(tmp_path, c["params"], types), implementation="hmmlearn")
    order = [VOCAB.index(w) for w in dec.vocab]                      # load order (glob) decides ties and the word index
    assert sorted(order) == [0, 1, 2] and dec._is_full()
    params = [c["params"][m] for m in order]
    want = vc.reference(name)
    rvit, rfwd = want["viterbi"][0][:, order], want["forward"][0][:, order]
    vbw, fbw = vc.first_strict_max(rvit), vc.first_strict_max(rfwd)
    pack = dec._vocab_pack()
    launch = {mode: full_cov.vocab_scores(c["feats"], c["lengths"], pack, mode=mode).score.cpu().numpy()
              for mode in MODES}
    N = len(utts)

    def check(got, rsc, rbw, mode):
        assert len(got) == N
        dev_path = full_cov.FullCovBatch(c["feats"], c["lengths"], np.maximum(rbw, 0), pack.W, pack.S).viterbi(
            pack)[1].cpu().numpy()
        offs = np.r_[0, np.cumsum(c["lengths"])]
        for u, (word, score, states) in enumerate(got):
            w = rbw[u]
            if w < 0:                                                # no frames: no word
                assert utts[u].shape[0] == 0 and (word, score, states) == (None, -np.inf, None)
                continue
            assert word == dec.vocab[w]
            assert abs(score - rsc[u, w]) <= RTOL * abs(rsc[u, w])
            assert score == launch[mode][u, w]                       # the vocabulary launch's score, bit for bit
            assert np.array_equal(states, dev_path[offs[u]:offs[u + 1]])     # FullCovBatch.viterbi under the winner
            _, path, gap = ref.viterbi(utts[u], *params[w])          # the path of the chosen word only
            assert gap > 1e-9
            np.testing.assert_array_equal(states, path)

    got = dec.decode_batch(flat)
    check(got, rvit, vbw, "viterbi")
    fwd = Decoder(models_dir=str(tmp_path / "trained_models"), implementation="hmmlearn", scoring="forward")
    assert fwd.vocab == dec.vocab
    check(fwd.decode_batch(flat), rfwd, fbw, "forward")
    assert dec._pack is None and fwd._pack is None                   # the single-Gaussian pack was never built
    # score_batch / nbest: forward mode with posteriors
    sc = dec.score_batch(flat)
    assert sc.shape == (N, 3) and sc.dtype == np.float64
    np.testing.assert_allclose(sc, rfwd, rtol=RTOL)
    assert np.array_equal(sc, launch["forward"])
    nb = dec.nbest(flat, n=2)
    assert len(nb) == N and all(len(r) == 2 for r in nb)
    for u, row in enumerate(nb):
        if fbw[u] < 0:
            continue
        assert row[0][0] == dec.vocab[fbw[u]] and row[0][1] == sc[u, fbw[u]] and row[0][1] >= row[1][1]
        assert 0.0 <= row[1][2] <= row[0][2] <= 1.0
        m = rfwd[u].max()
        np.testing.assert_allclose(row[0][2], np.exp(rfwd[u, fbw[u]] - m) / np.exp(rfwd[u] - m).sum(), rtol=1e-9)
    # state posteriors under the decoder's word, and under a named one, against the reference's gamma
    post = dec.state_posteriors(flat)
    named = dec.state_posteriors(flat, words=[dec.vocab[1]] * N)
    for u, (p, q) in enumerate(zip(post, named)):
        assert p.shape == q.shape == (utts[u].shape[0], c["S"]) and p.dtype == np.float64
        if utts[u].shape[0] == 0:
            continue
        for got_u, w in ((p, vbw[u]), (q, 1)):
            gamma = ref.estep_utt(utts[u], *params[w])["gamma"]
            np.testing.assert_allclose(got_u, gamma, rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError):
        dec.state_posteriors(flat[:2], words=["who", dec.vocab[0]])
    # the reference's API on one (T, D) view
    word, score, states = dec.decode_sequence(utts[0])
    assert (word, score) == got[0][:2]
    np.testing.assert_array_equal(states, got[0][2])


def test_decoder_cuts_the_posteriors_to_the_models_own_states(tmp_path):
    from sapr_amd.decoder import Decoder
    c = vc.case("d5_s3_dense")
    params, want = vc.mixed_size()
    dec = Decoder(models_dir=_model_dir(tmp_path, params, ("full", "full", "tied")), implementation="hmmlearn")
    order = [VOCAB.index(w) for w in dec.vocab]
    flat = [np.ascontiguousarray(x.T) for x in c["flat"]]
    two = dec.vocab[order.index(1)]
    named = dec.state_posteriors(flat, words=[two] * len(flat))
    for x, q in zip(c["flat"], named):
        assert q.shape == (x.shape[0], 2)
        if x.shape[0]:
            np.testing.assert_allclose(q, ref.estep_utt(x, *params[1])["gamma"], rtol=1e-9, atol=1e-12)
    got = dec.decode_batch(flat)
    rbw = vc.first_strict_max(want["viterbi"][0][:, order])
    assert [g[0] for g in got] == [dec.vocab[w] if w >= 0 else None for w in rbw]


def test_a_vocabulary_of_diagonal_models_keeps_the_single_gaussian_path(tmp_path):
    from sapr_amd.decoder import Decoder
    from sapr_amd.trellis import DiagModelPack
    c = vc.case("d5_s3_dense")
    dec = Decoder(models_dir=_model_dir(tmp_path, c["params"], ("diag", "diag", "diag")), implementation="hmmlearn")
    assert not dec._is_full()
    got = dec.decode_batch([np.ascontiguousarray(x.T) for x in c["flat"]])
    assert isinstance(dec._pack, DiagModelPack) and dec._vocab is None and len(got) == len(c["flat"])

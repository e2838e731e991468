"""GPU parity of forward scoring over the vocabulary (forward_vocab.hip: sapr_forward_vocab, trellis.forward_scores,
torch.ops.sapr.hmm_forward_scores, Decoder.score_batch / nbest / scoring="forward") against the C oracle's forward
log-likelihoods (oracle/c_oracle.decode_batch(which=1)), the numpy restatement of hmmlearn's forward_log and the
single-model forward kernel.  float64 both sides; the quick emission form and the device exp / log differ from the CPU
evaluation in the last ulps: rtol 1e-11 on log-likelihoods, as the existing forward tests pin them
(test_estep_gpu.test_forward_loglik_matches_oracle, test_estep_statistics_match_oracle).  The posteriors are compared
with the float64 soft-max of the DEVICE's own scores at 1e-12, which isolates the epilogue from those ulps.

The best word must equal the oracle's on EVERY utterance, none left out.  Smallest relative gap between the best and the
second-best DISTINCT score of an utterance, computed on the CPU from the oracle alone for exactly these inputs (all
scores finite, the duplicate model never the oracle's word):
    models seed 3, 330 utterances   (13, 8) 7.2e-6   (39, 16) 1.1e-5   (13, 16) 1.3e-6   (39, 8) 2.5e-6
                                    dense (13, 8) 6.3e-6   dense (39, 16) 3.8e-6
    padded, models seed 5           (26, 5) 5.4e-5   (5, 1) 6.4e-6
    3 080 utterances, seed 3        2.4e-7
— the smallest exceeds twice the 1e-11 tolerance by four orders of magnitude, so an exclusion rule for near-ties would
only hide a failure.  Rows whose runner-up posterior (the duplicate's column left out) exceeds 1e-6 in the oracle: 8 to
47 per shape, thanks to the near-copy model."""
import pickle

import numpy as np
import pytest

from oracle import c_oracle, hmmlearn_oracle as ho
from tests._synth import VOCAB, synth_feature_set, trained_like_models

pytestmark = pytest.mark.gpu

RTOL = 1e-11


def _batch(utts_td):
    import torch
    from sapr_amd.trellis import FeatureBatch
    packed = np.ascontiguousarray(np.concatenate(utts_td, axis=0), dtype=np.float32)
    return FeatureBatch.from_packed(torch.from_numpy(packed).cuda(), np.asarray([u.shape[0] for u in utts_td]))


def _models(ns, D, seed, dense=False):
    """Eleven word models; model 7 is a copy of model 2 (an exact tie: the first one must win) and model 9 is model 2
    with its means shifted by 0.01 (a runner-up with a posterior well above zero)."""
    sp, A, mu, cv = trained_like_models(11, ns, D, seed)
    if dense:
        S = ns + 2
        rng = np.random.default_rng(1)
        A = rng.dirichlet(np.ones(S), (11, S))
        sp = rng.dirichlet(np.ones(S), 11)
    for arr in (sp, A, mu, cv):
        arr[7] = arr[2]
        arr[9] = arr[2]
    mu[9] = mu[2] + 0.01
    return sp, A, mu, cv


def _utterances(D, n_per_word=30, seed=21):
    _, flat = synth_feature_set(VOCAB, n_per_word, D=D, seed=seed, tmin=1, tmax=110)
    utts = [np.ascontiguousarray(f.T) for f in flat]
    feats = np.concatenate(utts, axis=0)
    offs = np.r_[0, np.cumsum([u.shape[0] for u in utts])].astype(np.int64)
    return utts, feats, offs


def _oracle(feats, offs, sp, A, mu, cv):
    sc, bw, _ = c_oracle.decode_batch(feats, offs, sp, A, mu, cv, which=1, sum_order=0)
    return sc, bw


def _check_against_oracle(fs, osc, obw):
    ll = fs.loglik.cpu().numpy()
    assert np.isfinite(osc).all() and np.isfinite(ll).all()
    err = np.abs(ll - osc) / np.abs(osc)
    print(f"max relative error of loglik vs the C oracle: {err.max():.3e}")
    np.testing.assert_allclose(ll, osc, rtol=RTOL)
    bw = fs.best_word.cpu().numpy()
    print(f"best word differs from the oracle's on {int((bw != obw).sum())} of {bw.size} utterances")
    np.testing.assert_array_equal(bw, obw)          # every utterance, none left out
    return ll, bw


SHAPES = [(13, 8, False), (39, 16, False), (13, 16, False), (39, 8, False), (13, 8, True), (39, 16, True)]


@pytest.mark.parametrize("D,ns,dense", SHAPES)
def test_scores_and_best_word_match_the_oracle(D, ns, dense):
    import torch
    from sapr_amd import _lib
    from sapr_amd.trellis import DiagModelPack, forward_loglik, forward_scores
    sp, A, mu, cv = _models(ns, D, seed=3, dense=dense)
    utts, feats, offs = _utterances(D)
    assert len(utts) == 330 and min(u.shape[0] for u in utts) == 1
    batch = _batch(utts)
    pack = DiagModelPack.from_params(sp, A, mu, cv)
    assert pack.topology == (_lib.TOPO_DENSE if dense else _lib.TOPO_BIDIAG) and (pack.D, pack.S) == (D, ns + 2)
    fs = forward_scores(batch, pack)
    osc, obw = _oracle(feats, offs, sp, A, mu, cv)
    ll, bw = _check_against_oracle(fs, osc, obw)
    assert fs.loglik.shape == (330, 11) and fs.best_word.dtype == torch.int32 and fs.word_post.shape == (330, 11)
    # numpy restatement of hmmlearn's forward_log on three (utterance, word) pairs
    for u, w in ((0, 0), (57, 9), (329, 2)):
        lp, _ = ho.forward_log(sp[w], A[w], ho.log_density_diag(utts[u], mu[w], cv[w]))
        assert abs(lp - ll[u, w]) <= RTOL * abs(lp)
    # the single-model forward kernel (exact emission form), every utterance assigned to word w
    for w in range(11):
        one = forward_loglik(batch, pack, np.full(len(utts), w)).cpu().numpy()
        np.testing.assert_allclose(ll[:, w], one, rtol=RTOL)


@pytest.mark.parametrize("D,ns,dense", SHAPES)
def test_ties_and_posteriors(D, ns, dense):
    import torch
    from sapr_amd.trellis import DiagModelPack, forward_scores
    sp, A, mu, cv = _models(ns, D, seed=3, dense=dense)
    utts, feats, offs = _utterances(D)
    fs = forward_scores(_batch(utts), DiagModelPack.from_params(sp, A, mu, cv))
    # equal models: equal bits, and the first of them in model order is the one that can win
    assert torch.equal(fs.loglik[:, 2], fs.loglik[:, 7])
    assert not bool((fs.best_word == 7).any())
    assert torch.equal(fs.word_post[:, 2], fs.word_post[:, 7])
    ll = fs.loglik.cpu()
    post = fs.word_post.cpu().numpy()
    ref = torch.softmax(ll, dim=1).numpy()              # float64 soft-max of the device's own scores
    np.testing.assert_allclose(post, ref, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0.0, atol=1e-12)
    runner_up = np.sort(np.delete(post, 7, axis=1), axis=1)[:, -2]     # (the duplicate's column left out)
    print(f"rows with a runner-up posterior above 1e-6: {int((runner_up > 1e-6).sum())}")
    assert (runner_up > 1e-6).any()
    # without posteriors: the same scores and words
    lean = forward_scores(_batch(utts), DiagModelPack.from_params(sp, A, mu, cv), want_post=False)
    assert lean.word_post is None
    assert torch.equal(lean.loglik, fs.loglik) and torch.equal(lean.best_word, fs.best_word)


@pytest.mark.parametrize("D,ns", [(26, 5), (5, 1)])
def test_padded_models(D, ns):
    """State counts and feature widths between the instantiated ones run padded (trellis.kernel_states /
    kernel_dims): unreachable states add exp(-inf) = 0, zero columns add (0 - 0)^2 / 1 = 0."""
    from sapr_amd.trellis import DiagModelPack, forward_scores
    sp, A, mu, cv = _models(ns, D, seed=5)
    utts, feats, offs = _utterances(D)
    batch = _batch(utts)
    pack = DiagModelPack.from_params(sp, A, mu, cv)
    assert (pack.S_model, pack.D_model) == (ns + 2, D) and pack.S in (10, 18) and pack.D in (13, 39)
    assert (pack.S, pack.D) != (ns + 2, D) and batch.D == pack.D and batch.D_model == D
    fs = forward_scores(batch, pack)
    osc, obw = _oracle(feats, offs, sp, A, mu, cv)           # the oracle on the unpadded arrays
    _check_against_oracle(fs, osc, obw)


def test_tiles_order_determinism_and_lean_pack():
    """3 080 utterances: thirteen 256-utterance tiles, the last one ragged, times eleven words."""
    import torch
    from sapr_amd import _lib
    from sapr_amd.trellis import DiagModelPack, ForwardScores, forward_scores
    D, ns = 13, 8
    sp, A, mu, cv = _models(ns, D, seed=3)
    utts, feats, offs = _utterances(D, n_per_word=280)
    assert len(utts) == 3080
    batch = _batch(utts)
    pack = DiagModelPack.from_params(sp, A, mu, cv)
    a = forward_scores(batch, pack)
    osc, obw = _oracle(feats, offs, sp, A, mu, cv)
    _check_against_oracle(a, osc, obw)
    b = forward_scores(batch, pack)
    for x, y in ((a.loglik, b.loglik), (a.best_word, b.best_word), (a.word_post, b.word_post)):
        assert torch.equal(x, y)                              # two consecutive calls: the same bits

    def run(order, blob):
        N, W = batch.n_utts, pack.W
        ll = torch.empty((N, W), dtype=torch.float64, device="cuda")
        bw = torch.empty(N, dtype=torch.int32, device="cuda")
        post = torch.empty((N, W), dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().sapr_forward_vocab(
            _lib.ptr(batch.feats), _lib.ptr(batch.offsets), _lib.ptr(order), N, batch.D, batch.max_T, _lib.ptr(blob), W,
            pack.S, pack.topology, _lib.ptr(ll), _lib.ptr(bw), _lib.ptr(post), _lib.current_stream()),
            "sapr_forward_vocab")
        return ForwardScores(ll, bw, post)

    for other in (run(None, pack.blob), run(batch.order, pack.blob)):       # with and without the length-sorted order
        assert torch.equal(other.loglik, a.loglik) and torch.equal(other.best_word, a.best_word)
        assert torch.equal(other.word_post, a.word_post)
    lean = DiagModelPack.from_params(sp, A, mu, cv, exact_only=True)        # exact-kernel operands only
    assert lean.flags & _lib.PACK_EXACT_ONLY and not lean.prunable
    c = forward_scores(batch, lean)
    assert torch.equal(c.loglik, a.loglik) and torch.equal(c.best_word, a.best_word)
    assert torch.equal(c.word_post, a.word_post)


def test_torch_op_is_the_same_launch():
    import torch
    import sapr_amd.torch_ops  # noqa: F401  (registers torch.ops.sapr.*)
    from sapr_amd.trellis import DiagModelPack, forward_scores
    D, ns = 13, 8
    sp, A, mu, cv = _models(ns, D, seed=3)
    utts, _, _ = _utterances(D)
    batch = _batch(utts)
    pack = DiagModelPack.from_params(sp, A, mu, cv)
    fs = forward_scores(batch, pack)
    ll, bw, post = torch.ops.sapr.hmm_forward_scores(batch.feats, batch.offsets, batch.order, pack.blob, pack.W, pack.S,
                                                     pack.D, batch.max_T, pack.topology)
    assert torch.equal(ll, fs.loglik) and torch.equal(bw, fs.best_word) and torch.equal(post, fs.word_post)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.sapr.hmm_forward_scores(batch.feats.cpu(), batch.offsets.cpu(), batch.order.cpu(), pack.blob.cpu(),
                                          pack.W, pack.S, pack.D, batch.max_T, pack.topology)   # no CPU implementation


def test_zero_length_utterance_and_unsupported_shape():
    """An utterance without frames follows the C oracle (scores -inf, no word, NaN posteriors as the arithmetic gives
    them); a shape outside the instantiated ones is refused with sapr_forward_diag's message."""
    import torch
    from sapr_amd import _lib
    from sapr_amd.trellis import DiagModelPack, FeatureBatch, forward_scores
    sp, A, mu, cv = _models(8, 13, seed=3)
    utts, _, _ = _utterances(13, n_per_word=1)
    lengths = np.asarray([u.shape[0] for u in utts[:4]] + [0] + [u.shape[0] for u in utts[4:]])
    packed = np.ascontiguousarray(np.concatenate(utts, axis=0), dtype=np.float32)
    batch = FeatureBatch.from_packed(torch.from_numpy(packed).cuda(), lengths)
    pack = DiagModelPack.from_params(sp, A, mu, cv)
    fs = forward_scores(batch, pack)
    ll, bw, post = fs.loglik.cpu().numpy(), fs.best_word.cpu().numpy(), fs.word_post.cpu().numpy()
    assert np.all(ll[4] == -np.inf) and bw[4] == -1 and np.isnan(post[4]).all()
    offs = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    osc, obw = _oracle(packed, offs, sp, A, mu, cv)
    assert np.all(osc[4] == -np.inf) and obw[4] == -1
    keep = np.arange(len(lengths)) != 4
    np.testing.assert_allclose(ll[keep], osc[keep], rtol=RTOL)
    np.testing.assert_array_equal(bw, obw)
    out = torch.empty((batch.n_utts, 11), dtype=torch.float64, device="cuda")
    rc = _lib.load().sapr_forward_vocab(_lib.ptr(batch.feats), _lib.ptr(batch.offsets), None, batch.n_utts, 13, batch.max_T,
                                        _lib.ptr(pack.blob), 11, 12, pack.topology, _lib.ptr(out), None, None,
                                        _lib.current_stream())
    assert rc == -2 and b"{13,39}x{10,18}" in _lib.load().sapr_last_error()


def _model_dir(tmp_path, sp, A, mu, cv, n_iter=15):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    d = tmp_path / "trained_models" / "hmmlearn"
    d.mkdir(parents=True)
    for w, word in enumerate(VOCAB[: sp.shape[0]]):
        m = GaussianHMM(n_components=sp.shape[1], covariance_type="diag")
        m.startprob_, m.transmat_, m.means_, m._covars_ = sp[w], A[w], mu[w], cv[w]
        with open(d / f"{word}_hmmlearn_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


def test_decoder_forward_scoring(tmp_path):
    from sapr_amd.decoder import Decoder
    D, ns = 13, 8
    sp, A, mu, cv = _models(ns, D, seed=3)
    _, flat = synth_feature_set(VOCAB, 30, D=D, seed=21, tmin=1, tmax=110)       # (D, T) arrays, as mfcc_extract stores
    utts = [np.ascontiguousarray(f.T) for f in flat]
    feats = np.concatenate(utts, axis=0)
    offs = np.r_[0, np.cumsum([u.shape[0] for u in utts])].astype(np.int64)
    root = _model_dir(tmp_path, sp, A, mu, cv)
    dec = Decoder(models_dir=root)
    order = [VOCAB.index(w) for w in dec.vocab]                # load order (glob) decides ties and the word index
    osc, obw = _oracle(feats, offs, sp[order], A[order], mu[order], cv[order])
    # score_batch: the [N, W] matrix in load order
    sc = dec.score_batch(flat)
    assert sc.shape == (330, 11) and sc.dtype == np.float64
    np.testing.assert_allclose(sc, osc, rtol=RTOL)
    # nbest: best first, the oracle's best word in front, scores and posteriors of the matrix
    nb = dec.nbest(flat, n=3)
    assert len(nb) == 330 and all(len(r) == 3 for r in nb)
    for u, row in enumerate(nb):
        assert row[0][0] == dec.vocab[obw[u]]
        assert row[0][1] == sc[u, obw[u]] and row[0][1] >= row[1][1] >= row[2][1]
        assert 0.0 <= row[2][2] <= row[1][2] <= row[0][2] <= 1.0
    assert len(dec.nbest(flat[:5], n=50)[0]) == 11             # clipped to the vocabulary
    # scoring="forward": forward winner, its forward score, the Viterbi path of that word
    fwd = Decoder(models_dir=root, scoring="forward")
    assert fwd.vocab == dec.vocab
    got = fwd.decode_batch(flat)
    for u, (word, score, states) in enumerate(got):
        w = obw[u]
        assert word == dec.vocab[w] and score == sc[u, w]
        m = order[w]
        _, rst = ho.decode(flat[u].T, sp[m], A[m], mu[m], cv[m], tie="high")
        np.testing.assert_array_equal(states, rst)
    # the default scoring is the Viterbi decoder, unchanged: words, scores and paths of the oracle, bit for bit
    vsc, vbw, vpath = c_oracle.decode_batch(feats, offs, sp[order], A[order], mu[order], cv[order], tie=1, sum_order=1)
    explicit = Decoder(models_dir=root, scoring="viterbi").decode_batch(flat)
    for u, (word, score, states) in enumerate(dec.decode_batch(flat)):
        assert word == dec.vocab[vbw[u]] and score == vsc[u, vbw[u]]
        np.testing.assert_array_equal(states, vpath[offs[u]:offs[u + 1]])
        assert explicit[u][:2] == (word, score)
        np.testing.assert_array_equal(explicit[u][2], states)
    with pytest.raises(ValueError):
        Decoder(models_dir=root, implementation="custom", scoring="forward")

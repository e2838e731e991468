"""GPU: forward-backward over the word loop (csrc/connected_loop_fb.hip) through the Python layer against the CPU
restatement tests/_loop_fb_ref.py, which is the definition.

Tolerances: the project's pins for the same quantities (tests/test_embedded_gpu.py) — rtol 1e-11 on log-likelihoods,
rtol = atol = 1e-9 on posteriors — always against the numpy restatement.  Where two DEVICE results are compared with
each other (the identities), each is within the pin of the truth, so twice the pin is allowed."""
import pickle

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _bigram_ref as bref
from tests import _connected_ref as ref
from tests import _loop_fb_ref as lref

pytestmark = pytest.mark.gpu

NEG = -np.inf
RTOL_LL = 1e-11
TOL = 1e-9
# RL = 1; RL = 2 (word 6 straddles lanes 63 / 64); RL = 4, R = 252 twice; R = 250; R = 256 and the largest lm; padded
SHAPES = [(3, 4), (11, 10), (11, 18), (14, 18), (25, 10), (64, 4), (5, 7), (2, 1),
          (3, 12), (17, 3), (4, 11)]                # (RL, SP) = (1, 18), (2, 4), (2, 18): with the rest, all nine
LENGTHS = [3, 40, 1, 65, 0, 17, 2, 64, 33]          # 9 utterances: not a multiple of the 4 (3) a workgroup serves
LONG = [LENGTHS.index(T) for T in (33, 40, 64, 65)]
FIELDS = ("loglik", "word_post", "entry_post", "post")


def _net(ls, lt, lx, lm):
    from sapr_amd.connected import ConnectedNetwork, WordBigram
    return ConnectedNetwork(ls, lt, lx, bigram=WordBigram(*lm))


def _states(res, net):
    """``post[total, W, S]`` of a device result (the padded states cut off, after checking that they carry 0.0)."""
    p = res.post.reshape(-1, net.W, net.SP)
    assert not p[:, :, net.S:].any()
    return p[:, :, :net.S]


def _assert_close(res, net, want, what):
    ll, wp, ep, post = want
    finite = np.isfinite(ll)
    assert np.array_equal(res.loglik[~finite], ll[~finite], equal_nan=True), what
    err = np.abs(res.loglik[finite] - ll[finite]) / np.abs(ll[finite])
    print(f"{what}: max relative error of loglik {err.max() if err.size else 0.0:.3e}; max absolute error of word_post "
          f"{np.abs(res.word_post - wp).max():.3e}, entry_post {np.abs(res.entry_post - ep).max():.3e}, post "
          f"{np.abs(_states(res, net) - post).max():.3e}")
    np.testing.assert_allclose(res.loglik[finite], ll[finite], rtol=RTOL_LL, atol=0, err_msg=str(what))
    np.testing.assert_allclose(res.word_post, wp, rtol=TOL, atol=TOL, err_msg=str(what))
    np.testing.assert_allclose(res.entry_post, ep, rtol=TOL, atol=TOL, err_msg=str(what))
    np.testing.assert_allclose(_states(res, net), post, rtol=TOL, atol=TOL, err_msg=str(what))


@pytest.mark.parametrize("exits", ["last", "any"])
@pytest.mark.parametrize("topology", ["bidiag", "dense"])
@pytest.mark.parametrize("W,S", SHAPES)
def test_recursions_equal_restatement(W, S, topology, exits):
    """Random ``logb``; ``lm`` dense random with about a third of the pairs forbidden and one unreachable word.  The
    four long utterances have a path by construction (a single word with finite ``lm_start`` / ``lm_end`` and T >= S),
    so the zero rule cannot hide a broken kernel; the short ones exercise the no-path rule where S > T."""
    from sapr_amd.connected import connected_posteriors, connected_viterbi
    rng = np.random.default_rng(100 * W + S + (topology == "dense") + 2 * (exits == "any"))
    ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
    dead = W // 2
    lm = bref.random_lm(rng, W, dead_word=dead)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    net = _net(ls, lt, lx, lm)
    want = lref.posteriors_batch(logb, LENGTHS, ls, lt, lx, *lm)
    assert np.isfinite(want[0][LONG]).all()
    res = connected_posteriors(logb, LENGTHS, net, want_post=True)
    assert res.word_post.shape == (sum(LENGTHS), W) and res.post.shape == (sum(LENGTHS), net.R)
    _assert_close(res, net, want, (W, S, topology, exits))
    assert res.loglik[LENGTHS.index(0)] == NEG
    # the invariants where the likelihood is finite: the word posteriors of a frame sum to 1; nothing beats the sum
    offs = np.r_[0, np.cumsum(LENGTHS)]
    finite = np.isfinite(res.loglik)
    assert finite[LONG].all()
    rows = np.concatenate([np.arange(offs[u], offs[u + 1]) for u in np.flatnonzero(finite)])
    assert np.abs(res.word_post[rows].sum(axis=1) - 1.0).max() <= 1e-9
    dark = np.concatenate([np.arange(offs[u], offs[u + 1]) for u in np.flatnonzero(~finite)] + [np.zeros(0, int)])
    assert not res.word_post[dark].any() and not res.entry_post[dark].any() and not res.post[dark].any()
    if W > 1:
        assert not res.word_post[:, dead].any()
    best = connected_viterbi(logb, LENGTHS, net).score
    assert np.array_equal(np.isfinite(best), finite)
    assert (res.loglik[finite] >= best[finite] - 1e-11 * np.abs(best[finite])).all()
    # without the state posteriors the other outputs keep their bytes
    lean = connected_posteriors(logb, LENGTHS, net)
    assert lean.post is None
    for f in FIELDS[:3]:
        assert getattr(lean, f).tobytes() == getattr(res, f).tobytes(), f


@pytest.fixture(scope="module")
def emitted():
    """The (11, 10) case's utterances emitted once on the device: ``(model, logb_device, lengths)``."""
    import torch
    from sapr_amd.connected import ConnectedNetwork, emit_diag
    seed, W, S, D, n = ref.E2E_CASES[0]
    model, utts, _ = ref.sample_case(seed, W, S, D, n)
    net = ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, None, model["means"],
                           model["vars"], model["gconst"])
    return model, emit_diag(torch.from_numpy(np.concatenate(utts)).cuda(), net), [len(x) for x in utts]


def test_chain_identity_on_the_device(emitted):
    """The chain language model of a transcript of distinct words gives the embedded forward-backward's loglik and
    gamma, chain position k * SP + s at flat state words[k] * SP + s.  Two device results: twice the pins."""
    from sapr_amd.connected import ConnectedNetwork, connected_posteriors, embedded_forward_backward
    model, logb, lengths = emitted
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    W = tabs[0].shape[0]
    for words, p in (([4], 0.0), ([7, 2], -3.5), ([9, 0, 3, 6], -3.5)):
        emb = embedded_forward_backward(logb, lengths, [words] * len(lengths), ConnectedNetwork(*tabs, word_penalty=p),
                                        want_post=True)
        net = _net(*tabs, bref.chain_lm(W, words, p))
        got = connected_posteriors(logb, lengths, net, want_post=True)
        finite = np.isfinite(emb.loglik)
        assert np.array_equal(got.loglik[~finite], emb.loglik[~finite], equal_nan=True), words
        np.testing.assert_allclose(got.loglik[finite], emb.loglik[finite], rtol=2 * RTOL_LL, atol=0)
        SP = net.SP
        gamma = np.zeros((sum(lengths), W, SP))
        gamma[:, words] = emb.post.reshape(sum(lengths), -1, SP)[:, :len(words)]
        np.testing.assert_allclose(got.post.reshape(-1, W, SP), gamma, rtol=2 * TOL, atol=2 * TOL)
        if len(words) == 4:     # utterances of fewer than 40 frames cannot hold 4 words of 10 states
            assert finite.any() and (~finite).any()


def test_isolated_identity_on_the_device():
    """Every pair forbidden, free starts and ends, log_exit == 0: the log-sum over the words of
    ``trellis.forward_scores``' likelihoods, and its word posteriors at every frame.  Words 2 and 3 share their
    Gaussians, so the posteriors are not all 0 or 1.  Two device results: twice the pins."""
    import torch
    from sapr_amd.connected import ConnectedNetwork, connected_posteriors, emit_diag
    from sapr_amd.trellis import DiagModelPack, FeatureBatch, forward_scores
    seed, W, S, D, n = bref.E2E_CASE
    model, utts, _, _ = bref.sample_bigram_case(seed, W, S, D, n, bigram=bref.e2e_bigram(), shared=bref.E2E_SHARED)
    lengths = [len(x) for x in utts]
    feats = torch.from_numpy(np.concatenate(utts)).cuda()
    fs = forward_scores(FeatureBatch.from_packed(feats, np.asarray(lengths)),
                        DiagModelPack.from_params(model["startprob"], model["transmat"], model["means"], model["vars"]))
    fwd, wpost = fs.loglik.cpu().numpy(), fs.word_post.cpu().numpy()
    from sapr_amd.connected import WordBigram
    net = ConnectedNetwork(model["log_start"], model["log_trans"], np.zeros((W, S)), 0.0, None, model["means"],
                           model["vars"], model["gconst"],
                           bigram=WordBigram(np.full((W, W), NEG), np.zeros(W), np.zeros(W)))
    got = connected_posteriors(emit_diag(feats, net), lengths, net)
    assert np.isfinite(got.loglik).all()
    np.testing.assert_allclose(got.loglik, np.logaddexp.reduce(fwd, axis=1), rtol=2 * RTOL_LL, atol=0)
    np.testing.assert_allclose(got.word_post, np.repeat(wpost, lengths, axis=0), rtol=2 * TOL, atol=2 * TOL)
    assert ((wpost > 0.4) & (wpost < 0.6)).any()
    offs = np.r_[0, np.cumsum(lengths)]
    later = np.ones(sum(lengths), bool)
    later[offs[:-1]] = False
    assert not got.entry_post[later].any()              # no word begins behind frame 0


def test_word_penalty_is_a_constant_bigram(emitted):
    from sapr_amd.connected import ConnectedNetwork, connected_posteriors
    model, logb, lengths = emitted
    tabs = (model["log_start"], model["log_trans"], model["log_exit"])
    W = tabs[0].shape[0]
    for p in (0.0, -7.25):
        a = connected_posteriors(logb, lengths, ConnectedNetwork(*tabs, word_penalty=p), want_post=True)
        b = connected_posteriors(logb, lengths, _net(*tabs, bref.word_loop_lm(W, p)), want_post=True)
        assert np.isfinite(a.loglik).all()
        for f in FIELDS:
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (p, f)


def test_utterances_are_isolated_and_runs_repeat():
    from sapr_amd.connected import connected_posteriors
    W, S = 11, 10
    rng = np.random.default_rng(17)
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    lm = bref.random_lm(rng, W, dead_word=3)
    net = _net(ls, lt, lx, lm)
    logb = rng.normal(-40.0, 15.0, (sum(LENGTHS), W, S))
    offs = np.r_[0, np.cumsum(LENGTHS)]
    a = connected_posteriors(logb, LENGTHS, net, want_post=True)
    b = connected_posteriors(logb, LENGTHS, net, want_post=True)
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for u in (1, 3, 8):
        lo, hi = offs[u], offs[u + 1]
        one = connected_posteriors(logb[lo:hi], [LENGTHS[u]], net, want_post=True)
        assert one.loglik.tobytes() == a.loglik[u:u + 1].tobytes()
        for f in FIELDS[1:]:
            assert getattr(one, f).tobytes() == getattr(a, f)[lo:hi].tobytes(), (u, f)
    # a NaN frame in utterance 3 (65 frames): a NaN likelihood and zero rows there; the others keep their bytes
    bad = logb.copy()
    bad[offs[3] + 20] = np.nan
    c = connected_posteriors(bad, LENGTHS, net, want_post=True)
    assert np.isnan(c.loglik[3])
    keep = np.ones(len(logb), bool)
    keep[offs[3]:offs[4]] = False
    others = np.arange(len(LENGTHS)) != 3
    assert c.loglik[others].tobytes() == a.loglik[others].tobytes()
    for f in FIELDS[1:]:
        assert getattr(c, f)[keep].tobytes() == getattr(a, f)[keep].tobytes(), f
        assert not getattr(c, f)[~keep].any(), f
    assert a.word_post[~keep].any()


# ---- end to end: Decoder.decode_connected(confidence=True) over the three emission families -----------
def _pickle_models(tmp_path, impl, models, names, n_iter=15):
    d = tmp_path / "trained_models" / impl
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_{impl}_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


def _models(family, model):
    """The case's words as fitted models, as tests/test_bigram_gpu.py builds them: "diag" ``GaussianHMM``; the same
    with word 0 as a "full" model (diagonal matrices); ``GMMHMM`` with two equal components per state."""
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
def test_decoder_reports_a_coin_toss_as_a_coin_toss(tmp_path, family, impl):
    """Words 2 and 3 share their Gaussians.  The word loop picks one of them by tie-break and now says so: a segment
    of word 2 or 3 has the confidence 0.5, a segment of word 0 or 1 above 0.99; under the grammar every segment is
    above 0.99.  (The numpy restatement over the "diag" emission gives 0.5 +- 3e-13 and 1 - 1e-12; the "full" and
    "gmm" vocabularies of this case emit the same densities up to rounding, and a relative perturbation of 1e-13 of
    every ``logb`` moves the restatement's 0.5 by 1e-11.)"""
    from sapr_amd.connected import WordBigram
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
    twins = ("two", "three")

    plain = dec.decode_connected(feats)
    loop = dec.decode_connected(feats, confidence=True)
    n_twins = 0
    for a, b in zip(plain, loop):
        assert set(b) == set(a) | {"confidence", "total_log_likelihood", "log_posterior"}
        for key in a:                                            # the existing keys are unchanged
            assert np.array_equal(a[key], b[key]) if key == "state_sequence" else a[key] == b[key], key
        assert len(b["confidence"]) == len(b["segments"]) > 0
        assert b["total_log_likelihood"] >= b["log_likelihood"] - 1e-11 * abs(b["log_likelihood"])
        assert b["log_posterior"] == b["log_likelihood"] - b["total_log_likelihood"]
        for (word, _, _), conf in zip(b["segments"], b["confidence"]):
            print(family, "word loop", word, f"{conf:.15f}")
            if word in twins:
                n_twins += 1
                assert abs(conf - 0.5) <= 1e-6
            else:
                assert conf > 0.99
        if any(word in twins for word in b["words"]):            # a coin toss per twin: the path has at most half
            assert b["log_posterior"] <= np.log(0.5) + 1e-6
    assert n_twins >= 6

    gram = dec.decode_connected(feats, bigram=bigram, confidence=True)
    assert [row["words"] for row in gram] == [[names[w] for w in t] for t in truth]
    for row in gram:
        for (word, _, _), conf in zip(row["segments"], row["confidence"]):
            print(family, "grammar", word, f"{conf:.15f}")
            assert conf > 0.99

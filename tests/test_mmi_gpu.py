"""GPU: the denominator statistics of MMI training (csrc/connected_loop_stats.hip) and the training built on them
(``connected.mmi_estep`` / ``mmi_fit``, ``Decoder.train_discriminative``) against the CPU restatement
tests/_mmi_ref.py.  Tolerances are the pins of tests/test_embedded_gpu.py for the same quantities: rtol = atol = 1e-9
on statistics, rtol 1e-9 on the history of the objective."""
import copy
import pickle

import numpy as np
import pytest

from tests import _connected_family_cases as fam
from tests import _mmi_cases as cases
from tests import _mmi_ref as mref

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-9, atol=1e-9)
# Means and variances after MMI training against the reference's.  The update works on the differences num - den,
# which cancel, so the pin is measured, not derived: the largest relative deviation after three iterations on the
# confusable case, on an MI355X, was 2.91e-12 (test_training_parity_on_the_confusable_case prints it); the pin is ten
# times that (the issue allows nothing looser than 1e-5).
PARAM_RTOL = 2.91e-11


def _network(W, S, D):
    from sapr_amd.connected import ConnectedNetwork
    (ls, lt, lx), n_states, post, feats, keep, loglik = cases.sweep_case(W, S, D)
    return ConnectedNetwork(ls, lt, lx, n_states=n_states), n_states, post, feats, keep, loglik


def _check_rows(rows, want, net, D, what):
    from sapr_amd.trellis import split_stats
    S = net.S
    assert rows.shape == (net.W, 2 + S + S * S + S + 2 * S * D)
    assert np.isfinite(rows).all(), what
    for w in range(net.W):
        st = split_stats(rows[w], S, D)
        assert st["nobs"] == want["nobs"] and st["logprob"] == 0.0, (what, w)
        assert not st["start"].any() and not st["trans"].any(), (what, w)
        for key_ref, key in (("post", "post"), ("obs", "obs"), ("obs2", "obs**2")):
            err = np.max(np.abs(st[key] - want[key_ref][w]) / (1.0 + np.abs(want[key_ref][w])), initial=0.0)
            print(f"{what} word {w} {key_ref}: max scaled difference {err:.3g}")
            np.testing.assert_allclose(st[key], want[key_ref][w], err_msg=f"{what} {key_ref} word {w}", **TOL)
        cut = split_stats(rows[w], S, D, net.n_states[w], D)     # (what EmbeddedStats.split hands to an M-step)
        assert cut["post"].shape == (net.n_states[w],) and cut["obs"].shape == (net.n_states[w], D)


@pytest.mark.parametrize("W,S,D", cases.SWEEP)
def test_loop_stats_equals_reference(W, S, D):
    """Every shape of the sweep; the masked utterance's rows of ``post`` and its frames are NaN on the device (a frame
    that is not kept must not be read), and so are the padded states of every row (they have no place in ``stats``)."""
    from sapr_amd.connected import loop_stats
    net, n_states, post, feats, keep, loglik = _network(W, S, D)
    lengths = cases.SWEEP_LENGTHS
    offs = np.r_[0, np.cumsum(lengths)]
    assert net.R == W * net.SP and (net.SP, net.R) == {3: (4, 12), 5: (10, 50), 11: (10, 110), 14: (18, 252)}[W]
    want = mref.den_stats(post, feats, lengths, keep)
    a, b = offs[cases.SWEEP_MASKED], offs[cases.SWEEP_MASKED + 1]
    wide = np.full((post.shape[0], W, net.SP), np.nan)
    wide[:, :, :S] = post
    wide[a:b] = np.nan
    x = feats.copy()
    x[a:b] = np.nan
    rows = loop_stats(wide, x, lengths, net, keep)
    _check_rows(rows, want, net, D, (W, S, D))
    again = loop_stats(wide, x, lengths, net, keep)
    assert rows.tobytes() == again.tobytes()                     # no atomics: the same bytes from run to run
    # the posteriors of a frame add up to 1: every kept utterance with a path counts its frames
    frames = sum(n for u, n in enumerate(lengths) if keep[u] and np.isfinite(loglik[u]))
    total = sum(float(rows[w][2 + S + S * S:2 + S + S * S + S].sum()) for w in range(W))
    assert total == pytest.approx(frames, rel=1e-9)
    # [total_frames, W, S] is padded by the Python layer; without keep every utterance counts
    every = loop_stats(post.copy(), feats.copy(), lengths, net)
    _check_rows(every, mref.den_stats(post, feats, lengths), net, D, ("all", W, S, D))
    if S != net.SP:
        flat = np.zeros((post.shape[0], W, net.SP))
        flat[:, :, :S] = post
        assert loop_stats(flat.reshape(-1, net.R), feats.copy(), lengths, net).tobytes() == every.tobytes()


def test_loop_stats_without_frames_or_utterances():
    from sapr_amd.connected import loop_stats
    net, _, post, feats, _, _ = _network(3, 3, 1)
    post, feats = post.copy(), feats.copy()
    rows = loop_stats(post[:0], feats[:0], [0, 0], net)
    assert rows.shape == (3, 2 + 3 + 9 + 3 + 6) and not rows.any()
    rows = loop_stats(post[:0], feats[:0], [], net)
    assert not rows.any()
    rows = loop_stats(post[:5], feats[:5], [5], net, keep=[0])   # everything masked
    assert not rows.any()
    with pytest.raises(ValueError, match="keep flags"):
        loop_stats(post[:5], feats[:5], [5], net, keep=[1, 1])


# ---- the chain grammar: the word loop's paths are the transcript's ---------------------------------------------------
def _grammar_of(lm):
    from sapr_amd.connected import WordBigram
    return WordBigram(*lm)


def test_chain_grammar_makes_the_denominator_equal_the_numerator():
    from sapr_amd.connected import ConnectedNetwork, mmi_estep, mmi_fit
    models, utts, truth, lm = cases.chain_case()
    net = ConnectedNetwork.from_models(models, bigram=_grammar_of(lm))
    st = mmi_estep(utts, truth, net)
    assert st.keep.sum() == 11 and not st.keep[5]
    assert (st.lmscore == 0.0).all()
    frames = sum(len(x) for x, k in zip(utts, st.keep) if k)
    print(f"chain grammar: F = {st.objective:.3g} over {frames} frames")
    assert abs(st.objective) <= 1e-9 * frames
    np.testing.assert_allclose(st.num_loglik[st.keep], st.den_loglik[st.keep], rtol=1e-11)
    for w in range(net.W):
        num, den = st.split(w)
        assert den["nobs"] == 11 and num["nobs"] == 11           # every kept utterance says every word once
        assert not den["start"].any() and not den["trans"].any()
        for key in ("post", "obs", "obs**2"):
            err = np.max(np.abs(den[key] - num[key]) / (1.0 + np.abs(num[key])))
            print(f"chain grammar word {w} {key}: max scaled difference {err:.3g}")
            np.testing.assert_allclose(den[key], num[key], err_msg=f"{key} word {w}", **TOL)
    mine = [copy.deepcopy(m) for m in models]
    history = mmi_fit(mine, utts, truth, bigram=_grammar_of(lm), n_iter=1, names=cases.NAMES)
    assert len(history) == 1 and abs(history[0]) <= 1e-9 * frames
    for m, m0 in zip(mine, models):
        for got, was in ((m.means_, m0.means_), (m._covars_, m0._covars_)):
            worst = float(np.max(np.abs(got - was) / np.abs(was)))
            print(f"chain grammar {m.covariance_type}: max relative change {worst:.3g}")
            np.testing.assert_allclose(got, was, rtol=PARAM_RTOL)
        assert np.array_equal(m.startprob_, m0.startprob_) and np.array_equal(m.transmat_, m0.transmat_)


# ---- training parity on the confusable case ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def confusable():
    models, utts, truth, lm = cases.confusable_case()
    ref_models, history, last = mref.fit(models, utts, truth, lm, n_iter=3)
    return models, utts, truth, lm, ref_models, history, last


def test_estep_equals_reference_on_the_confusable_case(confusable):
    from sapr_amd.connected import ConnectedNetwork, mmi_estep
    models, utts, truth, lm, _, _, _ = confusable
    want = mref.fit(models, utts, truth, lm, n_iter=1)[2]
    st = mmi_estep(utts, truth, ConnectedNetwork.from_models(models, bigram=_grammar_of(lm)))
    assert np.array_equal(st.keep, want["keep"]) and not st.keep[16:].any() and st.keep[:16].all()
    np.testing.assert_allclose(st.lmscore, want["lmscore"], rtol=1e-15)
    for got, ref in ((st.num_loglik, want["num_loglik"]), (st.den_loglik, want["den_loglik"])):
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], ref[~fin])
        np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-11)
    assert st.objective == pytest.approx(want["F"], rel=1e-9)
    for w in range(len(models)):
        num, den = st.split(w)
        assert den["nobs"] == want["den"]["nobs"] == 16 and num["nobs"] == want["num"]["nobs"][w]
        for key_ref, key in (("post", "post"), ("obs", "obs"), ("obs2", "obs**2")):
            np.testing.assert_allclose(den[key], want["den"][key_ref][w], err_msg=f"den {key} {w}", **TOL)
        for key_ref, key in (("post_sum", "post"), ("obs", "obs"), ("obs2", "obs**2")):
            np.testing.assert_allclose(num[key], want["num"][key_ref][w], err_msg=f"num {key} {w}", **TOL)
    # the acoustic scale multiplies logb on both sides
    half = mmi_estep(utts, truth, ConnectedNetwork.from_models(models, bigram=_grammar_of(lm)), acoustic_scale=0.5)
    want_half = mref.fit(models, utts, truth, lm, n_iter=1, acoustic_scale=0.5)[2]
    assert half.objective == pytest.approx(want_half["F"], rel=1e-9) and half.objective != st.objective


def test_training_parity_on_the_confusable_case(confusable):
    """Three iterations of ``mmi_fit`` against ``_mmi_ref.fit``.  The history of F is held at rtol 1e-9.  Measured on
    an MI355X: the largest relative deviation of a mean or a variance from the reference after the three iterations
    is 2.91e-12 (printed below; recorded in DESIGN 4.3q); ``PARAM_RTOL`` is ten times it.  On the chain-grammar case
    one iteration moves no parameter by more than 1.82e-12 relative."""
    from sapr_amd.connected import mmi_fit
    models, utts, truth, lm, ref_models, history, _ = confusable
    assert len(history) == 3 and history[0] < history[1] < history[2]
    mine = [copy.deepcopy(m) for m in models]
    got = mmi_fit(mine, utts, truth, bigram=_grammar_of(lm), n_iter=3, names=cases.NAMES)
    print("F history", got, "reference", history)
    np.testing.assert_allclose(got, history, rtol=1e-9)
    worst = 0.0
    for m, r in zip(mine, ref_models):
        for a, b in ((m.means_, r.means_), (m._covars_, r._covars_)):
            worst = max(worst, float(np.max(np.abs(a - b) / np.abs(b))))
    print(f"MMI training parity: largest relative deviation of a mean or variance {worst:.3g}")
    for m, r, m0 in zip(mine, ref_models, models):
        np.testing.assert_allclose(m.means_, r.means_, rtol=PARAM_RTOL)
        np.testing.assert_allclose(m._covars_, r._covars_, rtol=PARAM_RTOL)
        assert not np.array_equal(m.means_, m0.means_)
        assert np.array_equal(m.startprob_, m0.startprob_) and np.array_equal(m.transmat_, m0.transmat_)
    assert mine[3]._covars_.shape == (cases.S_FIT,)
    assert not np.array_equal(mine[0].means_, mine[1].means_)    # the pair no longer shares its Gaussians


def _pickle_models(tmp_path, models, names, sub="trained_models", kind="hmmlearn", n_iter=15):
    d = tmp_path / sub / kind
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_{kind}_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / sub)


def _pair_confidence(rows):
    vals = [c for r in rows for (w, _, _), c in zip(r["segments"], r["confidence"]) if w in ("ba", "pa")]
    assert len(vals) >= 16
    return float(np.mean(vals))


def test_decoder_train_discriminative_raises_the_confidence_of_the_confusable_pair(tmp_path, confusable):
    from sapr_amd.decoder import Decoder
    models, utts, truth, lm, _, history, _ = confusable
    names = cases.NAMES + ["spare"]                              # a word in no transcript
    spare = copy.deepcopy(models[2])
    spare.means_ = spare.means_ + 500.0
    dec = Decoder(models_dir=_pickle_models(tmp_path, models + [spare], names), implementation="hmmlearn", n_iter=15)
    said = [[cases.NAMES[w] for w in t] for t in truth]
    feats = [x.T for x in utts]
    before = _pair_confidence(dec.decode_connected(feats[:16], bigram=said[:16], confidence=True))
    untouched = pickle.dumps(dec.models["spare"])
    got = dec.train_discriminative(feats, said, bigram=said[:16], n_iter=3)
    assert len(got) == 3 and got[0] < got[1] < got[2] <= 1e-9
    after = _pair_confidence(dec.decode_connected(feats[:16], bigram=said[:16], confidence=True))
    print(f"mean confidence of the 'ba' / 'pa' segments: {before:.4f} before, {after:.4f} after; F {got}")
    assert after > before
    assert pickle.dumps(dec.models["spare"]) == untouched        # a word in no transcript keeps its bytes
    # refusals: an unknown word, a transcript the grammar forbids
    with pytest.raises(ValueError, match="'seven'"):
        dec.train_discriminative(feats[:1], [["left", "seven"]])
    from sapr_amd.connected import WordBigram
    order = list(dec.models)
    only = WordBigram.from_grammar(len(order), [(order.index("left"), order.index("ba"))],
                                   starts=[order.index("left")], ends=[order.index("ba")])
    with pytest.raises(ValueError, match="utterance 0"):
        dec.train_discriminative(feats[:1], [["right", "pa"]], bigram=only)


def test_refusals_of_the_families_without_a_denominator_kernel(tmp_path):
    from sapr_amd.connected import mmi_fit
    from sapr_amd.decoder import Decoder
    for family, spec, kind in (("gmm", fam.GMM_CASES[0], "gmmhmm"), ("full", fam.FULL_CASES[0], "hmmlearn")):
        model, utts, truth = fam.case(family, spec)
        models = fam.models_of(family, model)
        with pytest.raises(NotImplementedError, match=repr(family)):
            mmi_fit(models, utts, truth)
        names = [f"w{k}" for k in range(len(models))]
        dec = Decoder(models_dir=_pickle_models(tmp_path, models, names, sub=family, kind=kind), implementation=kind,
                      n_iter=15)
        order = list(dec.models)
        with pytest.raises(NotImplementedError, match=repr(family)):
            dec.train_discriminative([x.T for x in utts], [[order[w] for w in t] for t in truth])
    # an unknown word and a forbidden transcript through mmi_fit itself
    models, utts, truth, lm = cases.chain_case()
    with pytest.raises(ValueError, match="word 9"):
        mmi_fit(copy.deepcopy(models), utts[:1], [[2, 9]], names=cases.NAMES)
    with pytest.raises(ValueError, match="utterance 1"):
        mmi_fit(copy.deepcopy(models), utts[:2], [truth[0], [0, 2, 3, 1]], bigram=_grammar_of(lm))


def test_an_utterance_that_is_dropped_leaves_the_numerator_too():
    """A NaN in the language model at a pair no transcript uses: every transcript scores, every chain has a path, and
    every denominator is NaN — ``keep`` drops all of them, so neither side may carry anything."""
    from sapr_amd.connected import ConnectedNetwork, WordBigram, mmi_estep
    models, utts, truth, lm = cases.chain_case()
    table = lm[0].copy()
    table[1, 2] = np.nan                                         # CHAIN ends with word 1: never followed
    st = mmi_estep(utts, truth, ConnectedNetwork.from_models(models, bigram=WordBigram(table, lm[1], lm[2])))
    assert np.isfinite(st.num_loglik).sum() == 11 and np.isnan(st.den_loglik).all()   # (a NaN in a table: every one)
    assert not st.keep.any() and st.objective == 0.0
    assert not st.den_stats.any() and not st.num.stats.any()
    for w in range(len(models)):
        num, den = st.split(w)
        assert num["nobs"] == 0 and den["nobs"] == 0

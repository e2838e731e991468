"""GPU: connected-word recognition over mixture and full-covariance word models (``sapr_connected_emit_gmm``,
``sapr_connected_emit_full`` in front of ``sapr_connected_viterbi``) against the CPU restatements: the recursion of
tests/_connected_ref.py over the emissions of tests/_gmmhmm_ref.py / tests/_fullcov_ref.py.  The cases and their
shared references are tests/_connected_family_cases.py; tests/test_connected_families_cpu.py guarantees their margins.
"""
import pickle

import numpy as np
import pytest

from tests import _connected_family_cases as cases
from tests import _connected_ref as ref

pytestmark = pytest.mark.gpu

NEG = -np.inf
E2E = [("gmm", c) for c in cases.GMM_CASES] + [("full", c) for c in cases.FULL_CASES]
FIELDS = ("score", "n_words", "path_word", "path_state", "path_entry")


def _network(family, spec, pen=0.0, exit_states="last"):
    from sapr_amd.connected import ConnectedNetwork
    model, utts, truth = cases.case(family, spec)
    net = ConnectedNetwork.from_models(cases.models_of(family, model), exit_states=exit_states, word_penalty=pen)
    assert net.family == family
    return net, model, utts, truth


@pytest.mark.parametrize("family,spec", E2E + [("gmm", cases.GMM_TINY), ("full", cases.FULL_TINY)])
def test_emission_matches_numpy(family, spec):
    """rtol 1e-11, the project's pin for these two families' log scores (test_gmmhmm_gpu.py, test_fullcov_gpu.py);
    padded columns are exactly -inf and nothing is NaN.  Frames: the case's own utterances, repeated up to the
    count."""
    import torch
    from sapr_amd import connected
    net, model, utts, _ = _network(family, spec)
    emit = {"gmm": connected.emit_gmm, "full": connected.emit_full}[family]
    W, S = net.W, net.S
    frames = np.concatenate(utts)
    frames = np.concatenate([frames] * (1000 // len(frames) + 1))[:1000]
    want_all = cases.emission(family, model, frames)
    worst = 0.0
    for total in (1, 255, 257, 1000):
        x = np.ascontiguousarray(frames[:total])
        got = emit(torch.from_numpy(x).cuda(), net).cpu().numpy()
        assert got.shape == (total, net.R)
        got = got.reshape(total, W, net.SP)
        assert not np.isnan(got).any()
        assert np.all(got[:, :, S:] == NEG)                      # padded columns
        want = want_all[:total]
        rel = np.abs(got[:, :, :S] - want) / np.abs(want)
        worst = max(worst, float(rel.max()))
        print(f"{family} emission {spec[1:-1]} x {total} frames: max relative difference {rel.max():.3g}")
        assert rel.max() <= 1e-11
    assert worst <= 1e-11


def test_padded_states_of_shorter_models_emit_minus_infinity():
    """Words with fewer states than the vocabulary's largest: their columns from ``n_states[w]`` on are -inf too."""
    import torch
    from sapr_amd import connected
    for family, spec in (("gmm", cases.GMM_CASES[2]), ("full", cases.FULL_CASES[2])):
        model, utts, _ = cases.case(family, spec)
        models = cases.models_of(family, model)
        short = cases.models_of(family, {k: (v[:, :3] if k in ("means", "covars", "weights") else v)
                                         for k, v in model.items()})[1]
        short.n_components = 3
        short.startprob_ = np.r_[1.0, 0.0, 0.0]
        short.transmat_ = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.0, 0.0, 1.0]])
        if family == "full" and short.covariance_type == "tied":
            short._covars_ = model["covars"][1, 0].copy()
        models[1] = short
        net = connected.ConnectedNetwork.from_models(models)
        assert net.n_states[1] == 3 and net.S == 7
        x = np.ascontiguousarray(utts[0])
        emit = {"gmm": connected.emit_gmm, "full": connected.emit_full}[family]
        got = emit(torch.from_numpy(x).cuda(), net).cpu().numpy().reshape(len(x), net.W, net.SP)
        assert np.all(got[:, 1, 3:] == NEG) and np.isfinite(got[:, 1, :3]).all()
        assert np.isfinite(got[:, 0, :7]).all() and np.all(got[:, :, 7:] == NEG)
        want = cases.emission(family, model, x)
        assert np.allclose(got[:, 1, :3], want[:, 1, :3], rtol=1e-11, atol=0)


@pytest.mark.parametrize("family,spec", E2E)
def test_single_word_anchor_is_bit_exact(family, spec):
    """``word_penalty = -inf`` and ``exit_states="any"``: no second word can be entered, so the score is the maximum
    over the words of the per-model Viterbi score, the word the vocabulary scorer's ``best_word`` and the states that
    word's per-model Viterbi path — with no tolerance: the emission kernels call the per-model kernels' device
    functions in the same order."""
    import torch
    from sapr_amd import _lib
    from sapr_amd.connected import connected_decode
    net, model, utts, _ = _network(family, spec, pen=NEG, exit_states="any")
    res = connected_decode(utts, net)
    feats = torch.from_numpy(np.concatenate(utts)).cuda()
    lengths = np.asarray([len(x) for x in utts], dtype=np.int64)
    vs = net.pack.vocab_scores(feats, lengths, mode="viterbi")
    score, best = (a.copy() for a in _lib.to_host(vs.score, vs.best_word))
    assert np.array_equal(res.score, score.max(axis=1))
    assert (res.n_words == 1).all()
    assert [res.words(u) for u in range(len(utts))] == [[int(w)] for w in best]
    _, path = net.pack.batch(feats, lengths, best.astype(np.int64)).viterbi(net.pack)
    assert np.array_equal(res.path_state, _lib.to_host(path)[0])
    assert np.array_equal(res.path_word, np.repeat(best, lengths))


@pytest.mark.parametrize("family,spec", E2E)
def test_end_to_end_paths_equal_reference(family, spec):
    """Paths and entries of EVERY utterance equal the reference (the CPU test guarantees the margins); score rtol
    1e-11: a score is a sum of negative terms only, so the emissions' bound carries over."""
    from sapr_amd.connected import connected_decode
    net, _, utts, truth = _network(family, spec)
    res = connected_decode(utts, net)
    score, n_words, pw, ps, pe = cases.reference(family, spec)
    rel = np.abs(res.score - score) / np.abs(score)
    print(f"{family} end to end {spec}: max relative score difference {rel.max():.3g}")
    assert np.array_equal(res.path_word, pw) and np.array_equal(res.path_state, ps)
    assert np.array_equal(res.path_entry, pe) and np.array_equal(res.n_words, n_words)
    assert rel.max() <= 1e-11
    assert sum(res.words(u) == truth[u] for u in range(len(utts))) >= len(utts) // 2


@pytest.mark.parametrize("family,spec", [("gmm", cases.GMM_CASES[1]), ("full", cases.FULL_CASES[1])])
def test_decoding_is_deterministic_and_independent_of_the_batch(family, spec):
    from sapr_amd.connected import connected_decode
    net, _, utts, _ = _network(family, spec, pen=-5.0)
    a, b = connected_decode(utts, net), connected_decode(utts, net)
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for u in (0, 7, len(utts) - 1):
        one = connected_decode([utts[u]], net)
        lo, hi = a.offsets[u], a.offsets[u + 1]
        assert one.score.tobytes() == a.score[u:u + 1].tobytes()
        assert np.array_equal(one.path_word, a.path_word[lo:hi]) and np.array_equal(one.path_state, a.path_state[lo:hi])
        assert np.array_equal(one.path_entry, a.path_entry[lo:hi]) and one.n_words[0] == a.n_words[u]


def _pickle_models(tmp_path, impl, models, names, n_iter=15):
    d = tmp_path / "trained_models" / impl
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_{impl}_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / "trained_models")


@pytest.mark.parametrize("family,impl,spec", [("gmm", "gmmhmm", cases.GMM_DECODER_CASE),
                                              ("full", "hmmlearn", cases.FULL_DECODER_CASE)])
def test_decoder_decode_connected(tmp_path, family, impl, spec):
    """Pickled ``GMMHMM`` models under "gmmhmm"; a pickled vocabulary of diag + spherical + tied + full ``GaussianHMM``
    models under "hmmlearn": words, segments, state sequences and scores against the reference at penalties 0, -30."""
    from sapr_amd.decoder import Decoder
    model, utts, truth = cases.case(family, spec)
    names = ["zero", "one", "two", "three"]
    root = _pickle_models(tmp_path, impl, cases.models_of(family, model), names)
    dec = Decoder(models_dir=root, implementation=impl, n_iter=15)
    order = tuple(names.index(w) for w in dec.vocab)             # load order (glob) is the word order of the network
    offs = np.r_[0, np.cumsum([len(x) for x in utts])]
    for pen in (0.0, -30.0):
        got = dec.decode_connected([x.T for x in utts], word_penalty=pen)
        score, n_words, pw, ps, pe = cases.reference(family, spec, pen, "last", order)
        for u, row in enumerate(got):
            lo, hi = offs[u], offs[u + 1]
            segs = ref.segments(pw[lo:hi], pe[lo:hi])
            assert row["words"] == [dec.vocab[w] for w, _, _ in segs]
            assert row["segments"] == [(dec.vocab[w], a, b) for w, a, b in segs]
            assert np.array_equal(row["state_sequence"], ps[lo:hi])
            assert abs(row["log_likelihood"] - score[u]) <= 1e-11 * abs(score[u])
            if pen == 0.0:
                assert row["words"] == [names[w] for w in truth[u]]
    # the isolated-word API of the same decoder still answers (the pack is shared, not consumed)
    assert len(dec.decode_batch([utts[0].T])) == 1


def test_decoder_still_refuses_custom_models(tmp_path):
    from sapr_amd.decoder import Decoder
    other = _pickle_models(tmp_path, "custom", [{"placeholder": "custom"}], ["zero"])
    with pytest.raises(ValueError, match="implementation='custom'"):
        Decoder(models_dir=other, implementation="custom").decode_connected([np.zeros((13, 4), np.float32)])

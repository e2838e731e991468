"""CPU: connected-word recognition over mixture and full-covariance word models — the margin condition that lets the
GPU tests (tests/test_connected_families_gpu.py) demand equal paths, the argument checks of the two emission entry
points, and ``ConnectedNetwork.from_models`` on the host."""
import numpy as np
import pytest

from tests import _connected_family_cases as cases
from tests import _connected_ref as ref

NEG = -np.inf
ALL_CASES = ([("gmm", c) for c in cases.GMM_CASES + [cases.GMM_DECODER_CASE]] +
             [("full", c) for c in cases.FULL_CASES + [cases.FULL_DECODER_CASE]])


@pytest.mark.parametrize("family,spec", ALL_CASES)
def test_margins_of_the_committed_cases(family, spec):
    """Along every optimal path of the committed cases each decision is an exact tie or is won by at least 1e-6: the
    device's emission differs from numpy's by rounding only (1e-11 relative of scores below 1e5), so it must take the
    same path.  At least half the word strings are recovered."""
    model, utts, truth = cases.case(family, spec)
    logb, lengths = cases.case_logb(family, spec)
    offs = np.r_[0, np.cumsum(lengths)]
    decoder = spec in (cases.GMM_DECODER_CASE, cases.FULL_DECODER_CASE)
    smallest, hits = np.inf, 0
    for pen in ((0.0, -30.0) if decoder else (0.0,)):   # (Decoder.decode_connected is also run with a word penalty)
        for u, words in enumerate(truth):
            b = logb[offs[u]:offs[u + 1]]
            m = np.asarray(ref.margins(b, model["log_start"], model["log_trans"], model["log_exit"], pen))
            assert m.size, "a sampled concatenation must have a finite score"
            assert np.all((m == 0.0) | (m >= 1e-6)), m[(m != 0) & (m < 1e-6)]
            smallest = min(smallest, m[m > 0].min())
            got = ref.viterbi(b, model["log_start"], model["log_trans"], model["log_exit"], pen)
            hits += pen == 0.0 and [w for w, _, _ in ref.segments(got[2], got[4])] == words
    print(f"{family} case {spec}: smallest margin {smallest:.3g}, {hits}/{len(truth)} word strings recovered")
    assert hits >= len(truth) // 2


def test_single_word_anchor_holds_in_the_reference():
    """With ``word_penalty = -inf`` and ``exit_states="any"`` no second word can be entered: the reference's score is
    the maximum over the words of the single-word Viterbi score, bit for bit (what the GPU anchor test relies on)."""
    for family, spec in (("gmm", cases.GMM_CASES[0]), ("full", cases.FULL_CASES[0])):
        model, _, _ = cases.case(family, spec)
        logb, lengths = cases.case_logb(family, spec)
        W, S = model["log_start"].shape
        any_exit = cases.log_exit(W, S, "any")
        score, n_words, _, _, _ = cases.reference(family, spec, NEG, "any")
        offs = np.r_[0, np.cumsum(lengths)]
        for u in range(len(lengths)):
            b = logb[offs[u]:offs[u + 1]]
            single = [ref.viterbi(b[:, w:w + 1], model["log_start"][w:w + 1], model["log_trans"][w:w + 1],
                                  any_exit[w:w + 1], NEG)[0] for w in range(W)]
            assert score[u] == max(single) and n_words[u] == 1


def test_argument_checks_of_the_emission_entry_points():
    from sapr_amd import _lib
    lib = _lib.load()
    gmm, full = lib.sapr_connected_emit_gmm, lib.sapr_connected_emit_full
    # bad sizes: total_frames < 0, or a non-positive W / S / M / D
    for args in ((-1, 13, None, 2, 4, 2), (10, 0, None, 2, 4, 2), (10, 13, None, 0, 4, 2), (10, 13, None, 2, 0, 2),
                 (10, 13, None, 2, 4, 0), (10, 13, None, 2, 4, -1)):
        assert gmm(None, *args, None, None) == -1, args
        assert b"bad sizes" in lib.sapr_last_error()
    for args in ((-1, 13, None, 2, 4), (10, 0, None, 2, 4), (10, 13, None, 0, 4), (10, 13, None, 2, 0)):
        assert full(None, *args, None, None) == -1, args
        assert b"bad sizes" in lib.sapr_last_error()
    # unsupported shapes: S = 19, D = 40, M = 9, W * SP = 260 — before any pointer is looked at
    for args, word in (((10, 13, None, 2, 19, 2), b"S="), ((10, 40, None, 2, 4, 2), b"D="),
                       ((10, 13, None, 2, 4, 9), b"M="), ((10, 13, None, 26, 10, 2), b"W * SP")):
        assert gmm(None, *args, None, None) == -2, args
        assert word in lib.sapr_last_error()
    for args in ((10, 13, None, 2, 19), (10, 40, None, 2, 4), (10, 13, None, 26, 10), (0, 13, None, 65, 4)):
        assert full(None, *args, None, None) == -2, args
        assert b"W * SP" in lib.sapr_last_error()
    # nothing to do returns 0 with nothing read; a NULL required pointer is refused before any launch
    assert gmm(None, 0, 13, None, 2, 4, 2, None, None) == 0
    assert full(None, 0, 13, None, 2, 4, None, None) == 0
    assert gmm(None, 10, 13, None, 2, 4, 2, None, None) == -1
    assert b"NULL" in lib.sapr_last_error()
    assert full(None, 10, 13, None, 2, 4, None, None) == -1
    assert b"NULL" in lib.sapr_last_error()


def _gmm_models(rng, shapes, D, n_mix):
    from sapr_amd.gmm_hmm import GMMHMM
    out = []
    for k, M in zip(shapes, n_mix):
        m = GMMHMM(n_components=k, n_mix=M)
        m.startprob_ = np.r_[1.0, np.zeros(k - 1)]
        m.transmat_ = np.eye(k) * 0.5 + np.eye(k, k=1) * 0.5
        m.transmat_[-1, -1] = 1.0
        m.weights_ = rng.dirichlet(np.full(M, 5.0), k)
        m.means_ = rng.normal(size=(k, M, D))
        m.covars_ = rng.uniform(1, 2, (k, M, D))
        out.append(m)
    return out


def test_network_from_gmm_models():
    from sapr_amd.connected import ConnectedNetwork
    from sapr_amd.gmm_hmm import GMMHMM, GmmPack, pack_layout
    rng = np.random.default_rng(1)
    models = _gmm_models(rng, (3, 5), 6, (3, 3))
    net = ConnectedNetwork.from_models(models, exit_states="last", word_penalty=-2.0)
    assert net.family == "gmm" and isinstance(net.pack, GmmPack) and net.pack.M == 3
    assert (net.W, net.S, net.SP, net.DP, net.R, net.D) == (2, 5, 10, 13, 20, 6) and net.n_states == [3, 5]
    assert net.word_penalty == -2.0 and net.means is None
    assert net.pack.data.shape == (2, pack_layout(5, 3, 6)[3])
    assert np.array_equal(np.isfinite(net.log_exit), np.array([[0, 0, 1, 0, 0], [0, 0, 0, 0, 1]], bool))
    assert np.all(net.log_start[0, 3:] == NEG) and np.all(net.log_trans[0, 3:] == NEG)
    assert np.all(net.log_trans[0, :, 3:] == NEG)
    with np.errstate(divide="ignore"):
        assert np.array_equal(net.log_trans[1], np.log(models[1].transmat_))
        assert np.array_equal(net.log_start[0, :3], np.log(models[0].startprob_))
    assert np.isfinite(ConnectedNetwork.from_models(models, exit_states="any").log_exit).sum() == 8
    # models that do not share n_mix: GmmPack.from_models' rule and message
    with pytest.raises(ValueError, match="n_mix"):
        ConnectedNetwork.from_models(_gmm_models(rng, (3, 5), 6, (3, 2)))
    # an unfitted model and an object of another class are refused up front, by index or by name
    with pytest.raises(ValueError, match=r"model 1.*implementation='gmmhmm'.*not fitted"):
        ConnectedNetwork.from_models(models[:1] + [GMMHMM(n_components=3, n_mix=3)])
    with pytest.raises(ValueError, match=r"word 'two'.*dict.*implementation='gmmhmm'"):
        ConnectedNetwork.from_models(models + [{"placeholder": 1}], names=["zero", "one", "two"],
                                     implementation="gmmhmm")


def test_network_from_mixed_covariance_types():
    from sapr_amd.connected import ConnectedNetwork
    from sapr_amd.full_cov import FullPack, pack_layout
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    rng = np.random.default_rng(2)
    D, models = 6, []
    for k, ct in ((3, "diag"), (5, "tied"), (4, "full")):
        m = GaussianHMM(n_components=k, covariance_type=ct)
        m.startprob_ = np.r_[1.0, np.zeros(k - 1)]
        m.transmat_ = np.eye(k) * 0.5 + np.eye(k, k=1) * 0.5
        m.transmat_[-1, -1] = 1.0
        m.means_ = rng.normal(size=(k, D))
        A = rng.normal(size=(k, D, D))
        spd = A @ A.transpose(0, 2, 1) + 4.0 * np.eye(D)
        m._covars_ = {"diag": rng.uniform(1, 2, (k, D)), "tied": spd[0], "full": spd}[ct]
        models.append(m)
    net = ConnectedNetwork.from_models(models, exit_states="last")
    assert net.family == "full" and isinstance(net.pack, FullPack)
    assert (net.W, net.S, net.SP, net.DP, net.R, net.D) == (3, 5, 10, 13, 30, 6) and net.n_states == [3, 5, 4]
    assert net.pack.data.shape == (3, pack_layout(5, 6)[2]) and net.means is None
    want = np.zeros((3, 5), bool)
    want[0, 2] = want[1, 4] = want[2, 3] = True
    assert np.array_equal(np.isfinite(net.log_exit), want)
    assert np.all(net.log_start[2, 4:] == NEG) and np.all(net.log_trans[2, 4:] == NEG)
    assert np.isfinite(ConnectedNetwork.from_models(models, exit_states="any").log_exit).sum() == 12
    # only "diag" / "spherical" models keep the diagonal family
    diag = ConnectedNetwork.from_models(models[:1])
    assert diag.family == "diag" and diag.pack is None and diag.means is not None
    # an unfitted model is refused up front, named by index or by word, with its covariance type
    unfitted = GaussianHMM(n_components=2, covariance_type="tied")
    with pytest.raises(ValueError, match=r"model 3.*covariance_type='tied'.*not fitted"):
        ConnectedNetwork.from_models(models + [unfitted])
    with pytest.raises(ValueError, match=r"word 'b'.*covariance_type='full'.*not fitted"):
        ConnectedNetwork.from_models([models[0], GaussianHMM(n_components=2, covariance_type="full")],
                                     names=["a", "b"], implementation="hmmlearn")
    # a mixture among GaussianHMM models of a decoder's "hmmlearn" vocabulary
    from sapr_amd.gmm_hmm import GMMHMM
    with pytest.raises(ValueError, match="gmmhmm"):
        ConnectedNetwork.from_models(models + [GMMHMM(n_components=2, n_mix=2)], implementation="hmmlearn")


def test_a_network_of_one_family_refuses_the_other_emissions():
    from sapr_amd import connected
    rng = np.random.default_rng(3)
    net = connected.ConnectedNetwork.from_models(_gmm_models(rng, (2, 2), 4, (2, 2)))

    class Feats:   # (the family is checked before the tensor is looked at)
        pass
    for emit in (connected.emit_diag, connected.emit_full):
        with pytest.raises(ValueError, match="gmm"):
            emit(Feats(), net)
    with pytest.raises(ValueError, match="VocabPack"):
        connected.ConnectedNetwork(net.log_start, net.log_trans, net.log_exit, family="gmm")

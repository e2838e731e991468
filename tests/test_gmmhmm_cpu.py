"""GMMHMM without a GPU: the numpy restatement (tests/_gmmhmm_ref.py) against the committed hmmlearn oracle at M = 1,
the mixture identities, the M-step's rules, pickling, and the C ABI's argument checks."""
import ctypes
import pickle

import numpy as np
import pytest

from oracle import hmmlearn_oracle as ho
from tests import _gmmhmm_ref as ref
from tests._synth import synth_batch, trained_like_models


def _case(S=10, D=13, T=60, seed=9, dense=False):
    sp, A, mu, cv = trained_like_models(1, S - 2, D, seed=seed)
    sp, A, mu, cv = sp[0], A[0], mu[0], cv[0]
    if dense:
        rng = np.random.default_rng(seed)
        A = rng.dirichlet(np.full(S, 0.7), size=S)
        sp = rng.dirichlet(np.full(S, 0.7))
    X = synth_batch(1, T=T, D=D, seed=4)[0]
    return X, sp, A, mu, cv


@pytest.mark.parametrize("dense", [False, True])
def test_m1_matches_the_committed_oracle(dense):
    """One component of weight 1 is the single-Gaussian model: loglik, gamma and {start, trans, post, obs, obs2}
    against oracle/hmmlearn_oracle.py's E-step, at the tolerances tests/test_oracle_hmmlearn.py uses for its pins."""
    X, sp, A, mu, cv = _case(dense=dense)
    S, D = mu.shape
    st = ho.new_stats(S, D)
    lp = ho.accumulate(st, X, sp, A, mu, cv)
    logB = ho.log_density_diag(X, mu, cv)
    gamma = ho.posteriors(ho.forward_log(sp, A, logB)[1], ho.backward_log(sp, A, logB))
    u = ref.estep_utt(X, sp, A, np.ones((S, 1)), mu[:, None, :], cv[:, None, :])
    assert u["loglik"] == pytest.approx(lp, rel=1e-12)
    np.testing.assert_allclose(u["gamma"], gamma, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(u["start"], st["start"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(u["post"], st["post"], rtol=1e-10)
    np.testing.assert_allclose(u["trans"], st["trans"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(u["obs"][:, 0], st["obs"], rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(u["obs2"][:, 0], st["obs2"], rtol=1e-10)
    np.testing.assert_allclose(u["post_mix"][:, 0], st["post"], rtol=1e-10)


def test_duplicated_components_reproduce_m1_and_split_the_occupancy():
    X, sp, A, mu, cv = _case(S=6, T=40)
    S, D = mu.shape
    one = ref.estep_utt(X, sp, A, np.ones((S, 1)), mu[:, None, :], cv[:, None, :])
    w2 = np.tile([0.3, 0.7], (S, 1))
    two = ref.estep_utt(X, sp, A, w2, np.repeat(mu[:, None, :], 2, axis=1), np.repeat(cv[:, None, :], 2, axis=1))
    assert two["loglik"] == pytest.approx(one["loglik"], rel=1e-13)
    np.testing.assert_allclose(two["gamma"], one["gamma"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(two["post_mix"], one["post"][:, None] * np.array([0.3, 0.7]), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(two["obs"].sum(axis=1), one["obs"][:, 0], rtol=1e-10, atol=1e-9)
    # a zero weight switches a component off: log 0 = -inf flows through
    off = ref.estep_utt(X, sp, A, np.tile([1.0, 0.0], (S, 1)), np.repeat(mu[:, None, :], 2, axis=1),
                        np.repeat(cv[:, None, :], 2, axis=1))
    assert off["loglik"] == pytest.approx(one["loglik"], rel=1e-13)
    assert np.all(off["post_mix"][:, 1] == 0) and np.all(np.isfinite(off["obs"]))
    # no frames: -inf and nothing to add
    none = ref.estep_utt(np.zeros((0, D), np.float32), sp, A, w2, np.repeat(mu[:, None, :], 2, axis=1),
                         np.repeat(cv[:, None, :], 2, axis=1))
    st = ref.new_stats(S, 2, D)
    ref.accumulate(st, none)
    assert none["loglik"] == -np.inf and st["nobs"] == 0 and not st["post"].any()


def test_viterbi_of_the_restatement_matches_the_oracle_at_m1():
    X, sp, A, mu, cv = _case(dense=True)
    S = mu.shape[0]
    lp, path, gap = ref.viterbi(X, sp, A, np.ones((S, 1)), mu[:, None, :], cv[:, None, :])
    lp_o, path_o = ho.viterbi(sp, A, ho.log_density_diag(X, mu, cv), tie="low")
    assert gap > 1e-9
    assert lp == pytest.approx(lp_o, rel=1e-12) and np.array_equal(path, path_o)


def _stats(S, M, D, rng):
    pm = rng.uniform(0.5, 3.0, (S, M))
    obs = rng.normal(0, 2, (S, M, D)) * pm[:, :, None]
    return {"start": rng.dirichlet(np.ones(S)), "trans": rng.uniform(0, 2, (S, S)), "post": pm.sum(axis=1),
            "post_mix": pm, "obs": obs, "obs2": (obs / pm[:, :, None]) ** 2 * pm[:, :, None] + pm[:, :, None]}


def _both_m_steps(st, prm, **hyper):
    """The restatement's and the product's M-step (the product names the squares 'obs**2')."""
    from sapr_amd.gmm_hmm import gmm_m_step
    a = ref.m_step(st, *prm, **hyper)
    b = gmm_m_step(dict(st, **{"obs**2": st["obs2"]}), *prm, **hyper)
    for x, y in zip(a, b):
        np.testing.assert_allclose(y, x, rtol=1e-13, atol=1e-15)
    return a


def test_m_step_default_priors_give_weights_that_sum_to_one_and_the_ml_estimates():
    rng = np.random.default_rng(3)
    S, M, D = 3, 4, 5
    st = _stats(S, M, D, rng)
    prm = (np.full(S, 1 / S), np.full((S, S), 1 / S), np.full((S, M), 1 / M), np.zeros((S, M, D)), np.ones((S, M, D)))
    sp, tm, w, mu, cv = _both_m_steps(st, prm)
    np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=1e-14)
    np.testing.assert_allclose(w, st["post_mix"] / st["post"][:, None], rtol=1e-14)
    np.testing.assert_allclose(mu, st["obs"] / st["post_mix"][:, :, None], rtol=1e-14)
    np.testing.assert_allclose(cv, st["obs2"] / st["post_mix"][:, :, None] - mu ** 2, rtol=1e-12)   # (= 1 here)
    np.testing.assert_allclose(tm.sum(axis=1), 1.0, rtol=1e-14)


def test_m_step_empty_component_and_variance_floor():
    rng = np.random.default_rng(4)
    S, M, D = 2, 3, 4
    st = _stats(S, M, D, rng)
    st["post_mix"][0, 1] = 0.0                       # an empty component ...
    st["obs"][0, 1] = 0.0
    st["obs2"][0, 1] = 0.0
    st["post"] = st["post_mix"].sum(axis=1)
    st["obs2"][1, 2] = st["obs"][1, 2] ** 2 / st["post_mix"][1, 2]   # ... and one whose variance collapses to 0
    old_mu, old_cv = rng.normal(0, 1, (S, M, D)), rng.uniform(1, 2, (S, M, D))
    prm = (np.full(S, 1 / S), np.full((S, S), 1 / S), np.full((S, M), 1 / M), old_mu, old_cv)
    _, _, w, mu, cv = _both_m_steps(st, prm, min_covar=1e-3)
    assert w[0, 1] == 0.0 and w[0].sum() == pytest.approx(1.0)
    assert np.array_equal(mu[0, 1], old_mu[0, 1]) and np.array_equal(cv[0, 1], old_cv[0, 1])
    assert np.all(cv[1, 2] == 1e-3) and np.all(np.isfinite(mu)) and np.all(cv >= 1e-3)
    # a state nobody visited keeps its weights
    st["post_mix"][0] = 0.0
    st["post"][0] = 0.0
    _, _, w, _, _ = _both_m_steps(st, prm)
    assert np.array_equal(w[0], prm[2][0])


def test_m_step_non_default_priors_hand_computed():
    """One state, two components, one feature, every prior away from its default."""
    st = {"start": np.array([1.0]), "trans": np.array([[3.0]]), "post": np.array([4.0]),
          "post_mix": np.array([[1.0, 3.0]]), "obs": np.array([[[2.0], [9.0]]]), "obs2": np.array([[[5.0], [30.0]]])}
    prm = (np.array([1.0]), np.array([[1.0]]), np.array([[0.5, 0.5]]), np.zeros((1, 2, 1)), np.ones((1, 2, 1)))
    hyper = dict(weights_prior=2.0, means_prior=1.0, means_weight=0.5, covars_prior=0.5, covars_weight=0.25,
                 min_covar=1e-3)
    _, _, w, mu, cv = _both_m_steps(st, prm, **hyper)
    # w = (post_mix + 2 - 1) / (post + 2 * (2 - 1)) = (2, 4) / 6
    np.testing.assert_allclose(w, [[2 / 6, 4 / 6]], rtol=1e-15)
    # mu = (0.5 * 1 + obs) / (0.5 + post_mix) = 2.5 / 1.5, 9.5 / 3.5
    np.testing.assert_allclose(mu[0, :, 0], [2.5 / 1.5, 9.5 / 3.5], rtol=1e-15)
    # c = (obs2 - 2 mu obs + mu^2 post_mix + 0.5 (mu - 1)^2 + 2 * 0.25) / (post_mix + 1 + 2 * 1.5)
    m0, m1 = 2.5 / 1.5, 9.5 / 3.5
    c0 = (5.0 - 2 * m0 * 2.0 + m0 ** 2 * 1.0 + 0.5 * (m0 - 1) ** 2 + 0.5) / (1.0 + 4.0)
    c1 = (30.0 - 2 * m1 * 9.0 + m1 ** 2 * 3.0 + 0.5 * (m1 - 1) ** 2 + 0.5) / (3.0 + 4.0)
    np.testing.assert_allclose(cv[0, :, 0], [c0, c1], rtol=1e-14)


def test_pickle_round_trip_without_a_device():
    from sapr_amd import GMMHMM
    rng = np.random.default_rng(0)
    m = GMMHMM(n_components=3, n_mix=2, init_params="", n_iter=4, random_state=5)
    m.startprob_, m.transmat_ = np.array([1.0, 0, 0]), rng.dirichlet(np.ones(3), size=3)
    m.weights_, m.means_, m.covars_ = np.full((3, 2), 0.5), rng.normal(0, 1, (3, 2, 5)), np.ones((3, 2, 5))
    m.monitor_.report(-12.5)
    m2 = pickle.loads(pickle.dumps(m))
    for k in ("startprob_", "transmat_", "weights_", "means_", "covars_"):
        assert np.array_equal(getattr(m2, k), getattr(m, k))
    assert (m2.n_components, m2.n_mix, m2.n_iter, m2.random_state) == (3, 2, 4, 5)
    assert (m2.covars_prior, m2.covars_weight, m2.params) == (-1.5, 0.0, "stmcw")
    assert list(m2.monitor_.history) == [-12.5]
    m2._check()
    with pytest.raises(NotImplementedError):
        GMMHMM(covariance_type="full")


def test_c_abi_argument_checks_need_no_gpu():
    from sapr_amd import _lib
    lib = _lib.load()
    n, b = ctypes.c_int32(0), ctypes.c_size_t(0)
    assert lib.sapr_gmm_stats_width(10, 2, 13, ctypes.byref(n)) == 0
    assert n.value == 2 + 10 + 100 + 10 + 10 * 2 + 2 * 10 * 2 * 13
    assert lib.sapr_gmm_stats_width(0, 2, 13, ctypes.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_gmm_workspace_bytes(1000, 2, 10, 2, 13, ctypes.byref(b)) == 0
    assert b.value == 8 * (2 * 1000 * 10 + 122 * 257 * 2 + 4 * 2 * 10 * 2 * 27)
    assert lib.sapr_gmm_workspace_bytes(-1, 2, 10, 2, 13, ctypes.byref(b)) == -1
    for S, M, D in ((10, 9, 13), (19, 2, 13), (10, 2, 40)):
        assert lib.sapr_gmm_stats_width(S, M, D, ctypes.byref(n)) == -2
        assert lib.sapr_gmm_workspace_bytes(10, 1, S, M, D, ctypes.byref(b)) == -2
        assert lib.sapr_gmm_estep_diag(None, None, None, None, None, 0, 0, 0, D, 0, None, 1, S, M, None, 0, None, None,
                                       None, None, None) == -2
        assert b"S in 1..18" in lib.sapr_last_error()
        assert lib.sapr_gmm_viterbi_diag(None, None, None, None, 0, 0, 0, D, 0, None, 1, S, M, None, 0, None, None,
                                         None) == -2
    # bad sizes and NULL required pointers: refused before anything is launched; no tiles: nothing to do
    args = (None, None, None, None, None, 0, 0, 0, 13, 0, None, 1, 10, 2, None, 0, None, None, None, None, None)
    assert lib.sapr_gmm_estep_diag(*args) == 0
    assert lib.sapr_gmm_estep_diag(*(args[:11] + (0,) + args[12:])) == -1          # W = 0
    assert lib.sapr_gmm_estep_diag(*(args[:7] + (1,) + args[8:])) == -1            # a tile, but NULL pointers
    assert b"NULL pointer" in lib.sapr_last_error()
    assert lib.sapr_gmm_estep_diag(*(args[:9] + (70000,) + args[10:])) == -1       # max_T beyond the grid
    sp, mp, dp = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.sapr_gmm_pack_layout(6, 3, 5, ctypes.byref(sp), ctypes.byref(mp), ctypes.byref(dp), ctypes.byref(b)) == 0
    assert (sp.value, mp.value, dp.value) == (10, 4, 13)
    assert b.value == 10 + 2 * 100 + 10 * 4 + 10 * 13 * 4 * 2

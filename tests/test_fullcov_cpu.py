"""CPU: the numpy definition of the full / tied / spherical Gaussian HMM (tests/_fullcov_ref.py) against independent
code (scipy, scikit-learn, the product's diag M-step), the conditions the GPU tests put on their inputs, established
from the reference alone, and the host logic of ``GaussianHMM``'s covariance types and of ``sapr_amd.full_cov``."""
import ctypes
import pickle

import numpy as np
import pytest

from tests import _fullcov_cases as fc
from tests import _fullcov_ref as ref

NAMES = list(fc.CASES)
ERR_ARG, ERR_UNSUPPORTED = -1, -2     # include/sapr_hip.h


def _spd(rng, D, scale=4.0):
    A = rng.standard_normal((D, 2 * D))
    return scale * (A @ A.T) / (2 * D) + 0.5 * np.eye(D)


# ------------------------------------------------------------------------------------------
# the reference against independent code
# ------------------------------------------------------------------------------------------
def test_log_density_matches_scipy():
    from scipy.stats import multivariate_normal
    rng = np.random.default_rng(3)
    S, D, T = 4, 9, 50
    mu = rng.normal(0, 5.0, (S, D))
    cv = np.array([_spd(rng, D) for _ in range(S)])
    X = rng.normal(0, 5.0, (T, D))
    got = ref.log_density(X, mu, cv)
    for s in range(S):
        np.testing.assert_allclose(got[:, s], multivariate_normal.logpdf(X, mu[s], cv[s]), rtol=1e-12, atol=0)


@pytest.mark.parametrize("ct", ref.COVARIANCE_TYPES)
def test_m_step_matches_sklearn_gaussian_mixture(ct):
    """With ``covars_prior = covars_weight = 0`` and given posteriors the M-step's means and covariances are those of
    ``sklearn.mixture.GaussianMixture`` (``reg_covar=0``) from the same responsibilities."""
    from sklearn.mixture import GaussianMixture
    rng = np.random.default_rng(11)
    S, D, T = 4, 6, 300
    X = (rng.normal(0, 3.0, (T, D)) @ (np.eye(D) + 0.3 * rng.standard_normal((D, D)))).astype(np.float32).astype(np.float64)
    resp = rng.dirichlet(np.full(S, 0.7), size=T)
    st = {"start": resp[0], "trans": np.ones((S, S)), "post": resp.sum(axis=0), "obs": resp.T @ X,
          "obs2": resp.T @ X ** 2, "oo": np.einsum("ts,ta,tb->sab", resp, X, X)}
    sp, A = np.full(S, 1.0 / S), np.full((S, S), 1.0 / S)
    shape = {"diag": (S, D), "spherical": (S,), "tied": (D, D), "full": (S, D, D)}[ct]
    _, _, mu, cv = ref.m_step(st, sp, A, np.zeros((S, D)), np.zeros(shape), ct, covars_prior=0.0, covars_weight=0.0)
    gm = GaussianMixture(n_components=S, covariance_type=ct, reg_covar=0.0)
    with np.errstate(divide="ignore"):
        gm._m_step(X, np.log(resp))
    assert cv.shape == shape == gm.covariances_.shape
    np.testing.assert_allclose(mu, gm.means_, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(cv, gm.covariances_, rtol=0, atol=1e-9 * np.abs(gm.covariances_).max())


def test_reference_diag_m_step_is_the_products_bit_for_bit():
    from sapr_amd.hmmlearn_hmm import m_step as product_m_step
    c = fc.case("d5_s3_dense")
    sp, A, mu, cv = c["params"][0]
    st, _ = ref.estep(c["utts"][0], sp, A, mu, ref.expand(np.array([np.diag(m) for m in cv]), "diag", 3, 5))
    want = ref.m_step(st, sp, A, mu, np.array([np.diag(m) for m in cv]), "diag")
    pst = {"start": st["start"], "trans": st["trans"], "post": st["post"], "obs": st["obs"], "obs**2": st["obs2"]}
    got = product_m_step(pst, sp, A, means=mu, covars=np.array([np.diag(m) for m in cv]))
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("ct", ref.COVARIANCE_TYPES)
def test_product_m_step_is_the_reference(ct):
    """``hmmlearn_hmm.m_step_typed`` is the same function of the same statistics as the reference, for every type."""
    from sapr_amd.hmmlearn_hmm import m_step_typed
    c = fc.case("d5_s3_dense")
    sp, A, mu, _ = c["params"][0]
    cv0 = fc.start_covars(c["params"][0], ct)
    st, _ = ref.estep(c["utts"][0], sp, A, mu, ref.expand(cv0, ct, 3, 5))
    st["oo"] = (st["oo"] + st["oo"].transpose(0, 2, 1)) / 2     # exactly symmetric, as the device's sums are
    want = ref.m_step(st, sp, A, mu, cv0, ct)
    pst = {"start": st["start"], "trans": st["trans"], "post": st["post"], "obs": st["obs"], "obs**2": st["obs2"],
           "obs*obs.T": st["oo"]}
    got = m_step_typed(pst, ct, sp, A, means=mu, covars=cv0)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    if ct in ("full", "tied"):
        full = ref.expand(got[3], ct, 3, 5)
        assert np.array_equal(full, full.transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU tests, from the reference alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", ["full", "tied"])
@pytest.mark.parametrize("name", NAMES)
def test_cases_stay_well_conditioned(name, ct):
    assert min(g for _, _, g in fc.reference_viterbi(name)) > 1e-9
    for _, hist, cvs in fc.reference_em(name, ct):
        assert len(hist) == fc.EM_ITERS and np.all(np.isfinite(hist))
        for it in cvs:
            for cv in it:
                ev = np.linalg.eigvalsh(cv)
                assert ev[0] > 0 and ev[-1] / ev[0] <= 1e5, (name, ct, ev[0], ev[-1])


# ------------------------------------------------------------------------------------------
# host logic
# ------------------------------------------------------------------------------------------
def test_constructor_accepts_the_four_types_and_refuses_a_fifth():
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    for ct in ("diag", "spherical", "tied", "full"):
        assert GaussianHMM(n_components=3, covariance_type=ct).covariance_type == ct
    with pytest.raises(ValueError, match="covariance_type"):
        GaussianHMM(n_components=3, covariance_type="banded")


def test_covars_setter_and_getter_shapes():
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    rng = np.random.default_rng(0)
    S, D = 3, 4
    full = np.array([_spd(rng, D) for _ in range(S)])
    given = {"diag": rng.uniform(1, 2, (S, D)), "spherical": rng.uniform(1, 2, S), "tied": full[0], "full": full}
    for ct, cv in given.items():
        m = GaussianHMM(n_components=S, covariance_type=ct, init_params="")
        m.startprob_, m.transmat_, m.means_ = np.full(S, 1 / S), np.full((S, S), 1 / S), np.zeros((S, D))
        m.covars_ = cv
        assert m._covars_.shape == cv.shape
        assert m.covars_.shape == (S, D, D)
        np.testing.assert_array_equal(m.covars_, ref.expand(cv, ct, S, D))
        m._check()
        assert m.n_features == D
    bad = {"diag": -given["diag"], "spherical": np.zeros(S), "tied": -full[0], "full": np.stack([full[0], full[1], -full[2]])}
    for ct, cv in bad.items():
        with pytest.raises(ValueError, match=ct):
            GaussianHMM(n_components=S, covariance_type=ct).covars_ = cv
    with pytest.raises(ValueError, match="'full' covars must be symmetric, positive-definite"):
        GaussianHMM(n_components=S, covariance_type="full").covars_ = full + np.triu(np.ones((D, D)), 1)
    with pytest.raises(ValueError, match="shape"):
        GaussianHMM(n_components=S, covariance_type="full").covars_ = full[0]
    m = GaussianHMM(n_components=S, covariance_type="tied", init_params="")
    m.startprob_, m.transmat_, m.means_ = np.full(S, 1 / S), np.full((S, S), 1 / S), np.zeros((S, D))
    m._covars_ = full     # a wrongly shaped array is caught by _check
    with pytest.raises(ValueError, match="shape mismatch"):
        m._check()


@pytest.mark.parametrize("S,D,SP,DP", [(3, 5, 4, 13), (10, 13, 10, 13), (5, 14, 10, 26), (11, 27, 18, 39)])
def test_pack_round_trip(S, D, SP, DP):
    from sapr_amd import full_cov
    rng = np.random.default_rng(S * 100 + D)
    sp = rng.dirichlet(np.full(S, 2.0))
    A = rng.dirichlet(np.full(S, 2.0), size=S)
    A[0, S - 1] = 0.0
    A[0] /= A[0].sum()
    mu = rng.normal(0, 5, (S, D))
    cv = np.array([_spd(rng, D) for _ in range(S)])
    assert full_cov.pack_layout(S, D) == (SP, DP, SP + 2 * SP * SP + SP + SP * DP + SP * DP * DP)
    assert full_cov.stats_width(S, D) == 2 + S + S * S + S + S * D + S * D * D
    pack = full_cov.pack_models([(sp, A, mu, cv), (sp[:S - 1] / sp[:S - 1].sum(), A[:S - 1, :S - 1] /
                                                   A[:S - 1, :S - 1].sum(axis=1, keepdims=True), mu[:S - 1], cv[:S - 1])])
    assert pack.shape == (2, full_cov.pack_layout(S, D)[2]) and pack.dtype == np.float64
    for w, s in enumerate((S, S - 1)):
        row, o = pack[w], 0
        ls = row[o:o + SP]
        o += SP
        lt = row[o:o + SP * SP].reshape(SP, SP)
        o += SP * SP
        ltT = row[o:o + SP * SP].reshape(SP, SP)
        o += SP * SP
        cc = row[o:o + SP]
        o += SP
        pmu = row[o:o + SP * DP].reshape(SP, DP)
        o += SP * DP
        wi = row[o:].reshape(SP, DP, DP)
        assert np.all(ls[s:] == -np.inf) and np.all(lt[s:] == -np.inf) and np.all(lt[:, s:] == -np.inf)
        assert np.array_equal(ltT, lt.T) and np.all(cc[s:] == -np.inf)
        if w == 0:
            np.testing.assert_array_equal(ls[:s], np.log(sp))
            assert lt[0, S - 1] == -np.inf
        assert np.all(pmu[s:] == 0) and np.all(pmu[:, D:] == 0) and np.array_equal(pmu[:s, :D], mu[:s])
        assert np.all(wi[s:] == 0) and np.all(wi[:, D:] == 0) and np.all(wi[:, :, D:] == 0)
        assert np.all(np.triu(wi, 1) == 0)      # exactly lower triangular
        for k in range(s):
            np.testing.assert_allclose(wi[k, :D, :D] @ cv[k] @ wi[k, :D, :D].T, np.eye(D), rtol=0, atol=1e-10)
            np.testing.assert_allclose(cc[k], -0.5 * (D * np.log(2 * np.pi) + np.linalg.slogdet(cv[k])[1]), rtol=1e-12)


def test_not_positive_definite_is_refused():
    from sapr_amd import full_cov
    S, D = 2, 3
    sp, A, mu = np.full(S, 0.5), np.full((S, S), 0.5), np.zeros((S, D))
    good = np.tile(np.eye(D), (S, 1, 1))
    indefinite = good.copy()
    indefinite[1, 2, 2] = -1.0
    skew = good.copy()
    skew[0, 0, 1] = 0.5
    for cv in (indefinite, skew):
        with pytest.raises(ValueError, match="'full' covars must be symmetric, positive-definite"):
            full_cov.pack_models([(sp, A, mu, cv)])
        with pytest.raises(ValueError, match="'tied' covars must be symmetric, positive-definite"):
            full_cov.pack_models([(sp, A, mu, cv)], name="tied")
    full_cov.pack_models([(sp, A, mu, good)])


def test_pickle_round_trip():
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    c = fc.case("d5_s3_dense")
    for ct in ("full", "tied", "spherical"):
        m = GaussianHMM(n_components=3, covariance_type=ct, init_params="")
        m.startprob_, m.transmat_, m.means_ = c["params"][0][:3]
        m.covars_ = fc.start_covars(c["params"][0], ct)
        m2 = pickle.loads(pickle.dumps(m))
        assert m2.covariance_type == ct
        for k in ("startprob_", "transmat_", "means_", "_covars_", "covars_"):
            assert np.array_equal(getattr(m, k), getattr(m2, k)), k
        assert all(not type(v).__module__.startswith(("torch", "ctypes")) for v in vars(m2).values())


def test_new_symbols_are_exported_and_check_their_arguments():
    from sapr_amd import _lib
    from sapr_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    for name in ("sapr_full_pack_layout", "sapr_full_stats_width", "sapr_full_workspace_bytes", "sapr_full_estep",
                 "sapr_full_viterbi"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    assert lib.sapr_full_workspace_bytes(1000, 2, 18, 39, ctypes.byref(n)) == 0
    K1 = 2 + 18 + 18 * 18 + 18
    assert n.value == 8 * (2 * 1000 * 18 + K1 * 257 * 2 + 4 * 2 * 18 * 39 * 40)
    w = ctypes.c_int32(0)
    assert lib.sapr_full_stats_width(19, 13, ctypes.byref(w)) == ERR_UNSUPPORTED
    assert lib.sapr_full_workspace_bytes(10, 1, 10, 40, ctypes.byref(n)) == ERR_UNSUPPORTED
    assert lib.sapr_full_stats_width(0, 13, ctypes.byref(w)) == ERR_ARG

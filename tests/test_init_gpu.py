"""GPU: what ``GaussianHMM.fit`` and ``GMMHMM.fit`` initialise from scratch (``n_iter=0``: the initialiser alone) against
the restatement of tests/_init_ref.py — the draws to the bit, the k-means means at the bar of
tests/test_kmeans_gpu.py::test_kmeans_against_reference_lloyd, the covariances of all four types against ``np.cov`` —
and mixed batches, in which only some models need only some attributes, bit for bit against each model fitted alone.
tests/test_init_cpu.py asserts the margins and gaps these comparisons rest on."""
import numpy as np
import pytest

from tests import _init_ref as iref
from tests import _kmeans_ref as ref

pytestmark = pytest.mark.gpu


def _matches_one(got, candidates, rtol=1e-9):
    err = [np.abs(got / c - 1).max() for c in candidates if c.shape == got.shape]
    return min(err) if err and min(err) <= rtol else None


def _covariance_deviation(got, X, S, covariance_type):
    """``_covars_`` against the restated rule: every entry within 1e-10 sqrt(cv_ii cv_jj) (a float64 product sum over
    n <= 500 frames in another order differs by at most n eps sqrt(sum x^2 sum y^2), about 6e-14 of that scale), the
    spherical value at rtol 1e-10.  -> the largest deviation in units of its scale."""
    want = iref.covars(X, S, covariance_type)
    assert got.shape == want.shape
    cv = iref.data_cov(X)
    scale = np.sqrt(np.outer(np.diag(cv), np.diag(cv)))
    if covariance_type == "spherical":
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
        return float(np.abs(got / want - 1).max())
    dev = float((np.abs(got - want) / (np.diag(scale) if covariance_type == "diag" else scale)).max())
    assert dev <= 1e-10, (covariance_type, dev)
    return dev


@pytest.mark.parametrize("covariance_type", iref.COVARIANCE_TYPES)
@pytest.mark.parametrize("name", sorted(iref.GAUSSIAN_WORDS))
def test_gaussian_initialisation(name, covariance_type):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    X, lengths, S, want = iref.gaussian_case(name, covariance_type)
    D = X.shape[1]
    rs = iref.GAUSSIAN_RANDOM_STATE[name]
    assert rs is not None and want["km"]["margin"] > 1e-9              # (no Gaussian case needed the tie rule)
    m = GaussianHMM(n_components=S, covariance_type=covariance_type, random_state=rs, n_iter=0).fit(X.copy(), lengths)
    assert np.asarray(m.startprob_).tobytes() == want["startprob"].tobytes()
    assert np.asarray(m.transmat_).tobytes() == want["transmat"].tobytes()
    best = want["km"]["runs"][want["km"]["best"]]
    np.testing.assert_allclose(m.means_, best["centers"], rtol=1e-9, atol=0)
    dev = _covariance_deviation(np.asarray(m._covars_), X, S, covariance_type)
    print(f"{name} {covariance_type}: means deviate by {np.abs(m.means_ / best['centers'] - 1).max():.2e} (bound 1e-9), "
          f"covariances by {dev:.2e} of sqrt(cv_ii cv_jj) (bound 1e-10)")
    assert m.covars_.shape == (S, D, D) and len(m.monitor_.history) == 0


@pytest.mark.parametrize("name", sorted(iref.GMM_CASES))
def test_gmm_initialisation(name):
    """Both cases run under the tie rule of tests/_init_ref.py (no ``random_state`` below 50 separates the restarts):
    ``means_`` must equal the restatement continued from one of the tied stage-1 restarts, state by state from one of
    that state's tied stage-2 restarts."""
    from sapr_amd.gmm_hmm import GMMHMM
    X, lengths, S, M, want = iref.gmm_case(name)
    rs = iref.GMM_RANDOM_STATE[name]
    m = GMMHMM(n_components=S, n_mix=M, random_state=iref.FALLBACK_RANDOM_STATE if rs is None else rs,
               n_iter=0).fit(X.copy(), lengths)
    assert np.asarray(m.startprob_).tobytes() == want["startprob"].tobytes()
    assert np.asarray(m.transmat_).tobytes() == want["transmat"].tobytes()
    np.testing.assert_array_equal(m.weights_, want["weights"])
    np.testing.assert_allclose(m.covars_, want["covars"], rtol=1e-10, atol=0)
    assert m.means_.shape == (S, M, X.shape[1])
    if rs is not None:
        assert min(want["margins"]) > 1e-9
        np.testing.assert_allclose(m.means_, want["means"], rtol=1e-9, atol=0)
        return
    found = []
    for per_state in iref.gmm_candidates(X, want):
        errs = [_matches_one(m.means_[s], per_state[s]) for s in range(S)]
        if all(e is not None for e in errs):
            found.append(max(errs))
    print(f"{name}: covariances deviate by {np.abs(m.covars_ / want['covars'] - 1).max():.2e} (bound 1e-10), means by "
          f"{min(found) if found else None} (bound 1e-9) from a tied restart")
    assert found, "means_ equal the restatement from none of the tied restarts"


def _attrs(m, names=("startprob_", "transmat_", "means_", "_covars_")):
    return {n: np.array(getattr(m, n), dtype=np.float64, copy=True) for n in names}


def _same_bits(a, b, what):
    for n in a:
        assert a[n].shape == b[n].shape and a[n].tobytes() == b[n].tobytes(), (what, n)


def _mixed_models(types):
    """Four models of one ``n_components``: 0 fully preset, 1 needs ``c`` only, 2 ``m`` only, 3 everything."""
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    S, D = iref.MIXED_S, 13
    data = iref.mixed_data(D)
    rng = np.random.default_rng(77)
    models = []
    for w, (ct, params) in enumerate(zip(types, ("", "c", "m", "stmc"))):
        m = GaussianHMM(n_components=S, covariance_type=ct, random_state=iref.MIXED_RANDOM_STATE[w], n_iter=0,
                        init_params=params)
        X64 = data[w][0].astype(np.float64)
        if w < 3:
            m.startprob_ = rng.dirichlet(np.ones(S))
            m.transmat_ = rng.dirichlet(np.ones(S), size=S)
        if w in (0, 1):
            m.means_ = X64[rng.choice(X64.shape[0], S, replace=False)]
        if w in (0, 2):
            m.covars_ = iref.covars(X64, S, ct) * 1.5
        models.append(m)
    return models, data


@pytest.mark.parametrize("types", [("diag",) * 4, ("diag", "tied", "full", "spherical")], ids=["all_diag", "four_types"])
def test_mixed_batch_equals_each_model_alone(types):
    """``len(sel) != len(models)`` and ``len(msel) != len(sel)`` in ``_init_models``: the selected models' frames and
    moments are gathered, and must be the models' own."""
    from sapr_amd.hmmlearn_hmm import fit_models
    together, data = _mixed_models(types)
    preset = _attrs(together[0])
    given = [_attrs(m, [n for n in ("startprob_", "transmat_", "means_", "_covars_") if hasattr(m, n)]) for m in together]
    fit_models(together, [(X.copy(), ln) for X, ln in data])
    _same_bits(_attrs(together[0]), preset, "the preset model")
    alone, _ = _mixed_models(types)
    for w, m in enumerate(alone):
        m.fit(data[w][0].copy(), data[w][1])
        _same_bits(_attrs(together[w]), _attrs(m), f"model {w} ({types[w]})")
    # what was preset and not asked for stays; what was asked for is new
    for w, keep in ((1, ("startprob_", "transmat_", "means_")), (2, ("startprob_", "transmat_", "_covars_"))):
        for n in keep:
            assert np.asarray(getattr(together[w], n)).tobytes() == given[w][n].tobytes(), (w, n)
    # and the initialised parts are the restatement's (model 1: covariances of ITS data, model 2: means from ITS moments)
    S = iref.MIXED_S
    _covariance_deviation(np.asarray(together[1]._covars_), data[1][0], S, types[1])
    want = ref.kmeans_seeded(data[2][0], S, iref.N_INIT, iref.seed_of_preset_topology(iref.MIXED_RANDOM_STATE[2]))
    err = _matches_one(np.asarray(together[2].means_), [want["runs"][r]["centers"] for r in want["tied"]])
    assert err is not None, "model 2's means are not the restatement's from any tied restart"


def test_gmm_mixed_n_components_equals_each_model_alone():
    """The loop over distinct ``n_components`` in ``_init_gmm_models``: models of 3, 4 and 3 states in one batch."""
    from sapr_amd.gmm_hmm import GMMHMM, fit_gmm_models
    data = [iref.word(g, 13) for g, _ in iref.GMM_MIXED]
    make = lambda: [GMMHMM(n_components=S, n_mix=2, random_state=20 + w, n_iter=0)
                    for w, (_, S) in enumerate(iref.GMM_MIXED)]
    names = ("startprob_", "transmat_", "weights_", "means_", "covars_")
    together = make()
    fit_gmm_models(together, [(X.copy(), ln) for X, ln in data])
    for w, m in enumerate(make()):
        m.fit(data[w][0].copy(), data[w][1])
        assert m.means_.shape == (iref.GMM_MIXED[w][1], 2, 13)
        _same_bits(_attrs(together[w], names), _attrs(m, names), f"model {w}")

"""CPU: the cases of tests/_init_ref.py are what tests/test_init_gpu.py needs them to be, from the restatement alone — the
committed ``random_state`` of every case is the first of 50 whose best restart wins clearly at every stage (or none of
the 50 does, and the tie rule applies), every Lloyd run behind a comparison is clear of near-ties, and the restated
covariance rules are numpy's.  No compute call is made."""
import numpy as np
import pytest

from tests import _init_ref as iref
from tests import _kmeans_ref as ref


def test_draws_follow_the_documented_order():
    sp, tm, seeds = iref.draws(3, 4, 5)
    rs = np.random.RandomState(3)
    assert np.array_equal(sp, rs.dirichlet(np.full(4, 0.25))) and np.array_equal(tm, rs.dirichlet(np.full(4, 0.25), size=4))
    assert seeds == [int(rs.randint(2 ** 31 - 1)) for _ in range(5)]
    from sapr_amd.hmmlearn_hmm import kmeans_seed
    rs2 = np.random.RandomState(3)
    rs2.dirichlet(np.full(4, 0.25))
    rs2.dirichlet(np.full(4, 0.25), size=4)
    assert kmeans_seed(rs2) == seeds[0]


@pytest.mark.parametrize("name", sorted(iref.GAUSSIAN_WORDS))
def test_covariance_rules(name):
    g, D, S = iref.GAUSSIAN_WORDS[name]
    X, lengths = iref.word(g, D)
    assert X.shape == (sum(lengths), D) and X.shape[0] <= 500          # (the n behind the 1e-10 covariance bound)
    X64 = X.astype(np.float64)
    cv = np.cov(X64.T) + 1e-3 * np.eye(D)
    assert np.array_equal(iref.covars(X, S, "tied"), cv)
    assert np.array_equal(iref.covars(X, S, "full"), np.tile(cv, (S, 1, 1)))
    sph = iref.covars(X, S, "spherical")
    assert sph.shape == (S,) and (sph == cv.mean()).all() and cv.mean() != np.diag(cv).mean()
    diag = iref.covars(X, S, "diag")
    assert diag.shape == (S, D)
    np.testing.assert_allclose(diag[0], np.diag(cv), rtol=1e-13)
    np.linalg.cholesky(cv)


@pytest.mark.parametrize("name", sorted(iref.GAUSSIAN_WORDS))
def test_gaussian_random_state_is_the_first_with_a_clear_margin(name):
    g, D, S = iref.GAUSSIAN_WORDS[name]
    X, _ = iref.word(g, D)
    found = iref.search_random_state(lambda rs: [iref.gaussian_init(X, S, "diag", rs)["km"]["margin"]])
    assert found == iref.GAUSSIAN_RANDOM_STATE[name]
    km = iref.gaussian_case(name, "diag")[3]["km"]
    print(f"{name}: random_state {found} margin {km['margin']:.3e} best {km['best']} "
          f"min_gap {min(r['min_gap'] for r in km['runs']):.3e} n_iter {[r['n_iter'] for r in km['runs']]}")
    assert km["margin"] > 1e-9 and km["tied"] == [km["best"]]
    assert iref.runs_are_clear(km) and iref.tie_set_is_clear(km)
    assert (km["pick"].size < X.shape[0]) == (X.shape[0] > 256 * S)
    assert len({c.tobytes() for c in km["runs"][km["best"]]["centers"]}) == S


@pytest.mark.parametrize("name", sorted(iref.GMM_CASES))
def test_gmm_random_state_or_tie_rule(name):
    g, D, S, M = iref.GMM_CASES[name]
    X, _ = iref.word(g, D)

    def margins(rs):
        try:
            return iref.gmm_init(X, S, M, rs)["margins"]
        except ValueError:
            return None
    found = iref.search_random_state(margins)
    assert found == iref.GMM_RANDOM_STATE[name]                        # None: the tie rule (see _init_ref's docstring)
    init = iref.gmm_case(name)[4]
    print(f"{name}: random_state {found} margins {['%.2e' % m for m in init['margins']]} "
          f"tied {[init['stage1']['tied']] + [k['tied'] for k in init['stage2']]} label gap {init['label_gap']:.3e} "
          f"state sizes {np.bincount(init['labels']).tolist()}")
    stages = [init["stage1"]] + init["stage2"]
    assert all(iref.runs_are_clear(k) and iref.tie_set_is_clear(k) for k in stages)
    assert init["label_gap"] > 1e-8 and np.bincount(init["labels"], minlength=S).min() >= max(M, 2)
    # what the tie rule admits differs from the best restart's result by the order of states or mixtures only
    srt = lambda c: c[np.lexsort(c.T[::-1])]
    want = srt(init["means"].reshape(S * M, D))
    cands = iref.gmm_candidates(X, init)
    assert len(cands) == len(init["stage1"]["tied"]) >= 1
    for per_state in cands:
        assert len(per_state) == S
        for picks in zip(*[[c[0], c[-1]] for c in per_state]):
            np.testing.assert_allclose(srt(np.concatenate(picks)), want, rtol=1e-9)
    if M == 1:
        assert all(len(k["tied"]) == iref.N_INIT for k in init["stage2"])   # one cluster: every restart reaches the mean


def test_mixed_batch_models_see_different_scales():
    """The mixed-batch test hands model 1 (covariances only) data 10 000 times as wide as the others': a threshold taken
    from the wrong model's moments would stop the k-means of model 2 or 3 at another iteration."""
    data = iref.mixed_data()
    var = [np.var(X.astype(np.float64), axis=0).mean() for X, _ in data]
    assert var[1] > 1e7 * max(var[0], var[2], var[3])
    # with model 1's threshold, the reference Lloyd of model 2 stops at another iteration in some restart
    S = iref.MIXED_S
    seed = iref.seed_of_preset_topology(iref.MIXED_RANDOM_STATE[2])
    assert seed != iref.draws(iref.MIXED_RANDOM_STATE[2], S, 1)[2][0]
    init, _ = ref.seed_centres(data[2][0], S, iref.N_INIT, seed)
    own = [ref.lloyd(data[2][0], c)["n_iter"] for c in init]
    other = [ref.lloyd(data[2][0], c, tol=1e-4 * var[1] / var[2])["n_iter"] for c in init]
    print("n_iter with the own threshold", own, "with model 1's", other)
    assert own != other
    km = ref.kmeans_seeded(data[2][0], S, iref.N_INIT, seed)
    assert iref.runs_are_clear(km) and iref.tie_set_is_clear(km)

"""CPU checks of the inputs and of the reference that tests/test_fullcov_regimes_gpu.py compares the full-covariance
kernels with.

1. Every case of tests/_fullcov_regimes.py meets its regime's conditions, computed from the longdouble reference alone.
2. The longdouble ``log_density`` (a Cholesky factorisation and a forward substitution written out) agrees with
   ``scipy.stats.multivariate_normal.logpdf`` to rtol 1e-12 at a well-conditioned shape (D = 13, condition number 10).
3. The longdouble reference agrees with the float64 restatement tests/_fullcov_ref.py on a soft case at the float64
   side's own accuracy: a quarter of the project's pins (rtol 1e-11 on log scores, rtol 1e-9 with atol 1e-12 on
   posteriors and statistics, 1e-9 norm-wise on oo), which is what lets the pin and not 4 * E_ref decide the GPU test's
   tolerance in the soft regime, and the same paths on every frame.
4. The measured table of the module docstring of tests/_fullcov_regimes.py is printed (-s shows it)."""
import numpy as np
import pytest
from scipy.stats import multivariate_normal

from tests import _fullcov_regimes as R


@pytest.mark.parametrize("fn_args", R.all_cases(), ids=R.case_id)
def test_regime_conditions_hold(fn_args):
    fn, args = fn_args
    case = fn(*args)
    assert case.utt_model.shape == case.lengths.shape == (len(case.utts),)
    assert case.feats.dtype == np.float32 and case.feats.shape == (case.lengths.sum(), case.D)
    assert all(len(prm[0]) == case.S and prm[3].shape == (case.S, case.D, case.D) for prm in case.params)
    if case.regime != "ragged":
        assert case.W == 3 and case.lengths.tolist() == list(R.SOFT_LENGTHS) * 3
    m = R.check_conditions(case, R.reference(case))
    print(R.case_id(fn_args), m)


def test_seed_skips_are_recorded_for_cases_that_exist():
    known = {(fn.__name__, *args[:2]) for fn, args in R.all_cases() if args}
    assert set(R.SEED_SKIPS) <= known


def test_longdouble_log_density_against_scipy():
    rng = np.random.default_rng(8)
    D, S = 13, 3
    sp, A, means, covars = R.word_model(rng, D, S, "dense", 10.0, R.A_SOFT)
    assert max(np.linalg.cond(cv) for cv in covars) < 100
    X = R.sample(rng, sp, A, means, np.linalg.cholesky(covars), 50)
    got = R.log_density(X, means, covars)
    assert got.dtype == R.LD and got.shape == (50, S)
    for s in range(S):
        want = multivariate_normal(means[s], covars[s]).logpdf(X.astype(np.float64))
        np.testing.assert_allclose(got[:, s].astype(np.float64), want, rtol=1e-12)


def test_reference_agrees_with_the_float64_restatement():
    case = R.soft(13, 10, "bidiag")
    want, o64, e = R.reference(case), R.float64_oracle(case), R.e_ref(case)
    print(e)
    for k in ("logb", "ll", "vit", "forward", "viterbi", "logprob"):
        assert 4 * e[k] <= 1e-11, (k, e[k])
    for k in ("gamma", "start", "trans", "post", "obs", "oo"):
        assert 4 * e[k] <= 1e-9, (k, e[k])
    assert np.array_equal(o64.path, want.path) and np.array_equal(o64.vit_path, want.vit_path)
    for m in ("forward", "viterbi"):
        assert np.array_equal(np.argmax(o64.scores[m], axis=1), np.argmax(want.scores[m], axis=1))
    # the reference's zeros are exact: a state the bidiagonal chain cannot have reached yet
    first = want.gamma[case.offs[2]:case.offs[3]]          # word 0's utterance of 63 frames
    for t in range(case.S - 1):
        assert (first[t, t + 1:] == 0).all() and (o64.gamma[case.offs[2] + t, t + 1:] == 0).all()


def test_measured_table():
    print()
    print(R.TABLE_HEAD)
    for fn, args in R.all_cases():
        case = fn(*args)
        want = R.reference(case)
        print(R.table_row(case, R.measure(case, want), R.e_ref(case)))

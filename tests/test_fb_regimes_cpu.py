"""CPU checks of the inputs and of the reference that tests/test_fb_regimes_gpu.py compares the forward family with.

1. Every regime of tests/_fb_regimes.py meets its conditions, computed from the longdouble reference alone.
2. The longdouble reference (tests/_fb_ref.py) agrees with the float64 numpy restatement of hmmlearn
   (oracle/hmmlearn_oracle.py: forward_log, backward_log, posteriors, accumulate's sums) to 1e-12 relative in the soft
   regime at (13, 8): element-wise on the log-likelihoods, relative to the largest entry of the array on the posterior
   lattice (largest entry 1) and on each word's statistics.  Measured: log-likelihoods 1.9e-15, posteriors 5.4e-13,
   trans 8.5e-13, post 3.5e-14, obs 3.5e-14, obs**2 3.4e-14, start 0.  (Element by element the float64 side cannot
   hold 1e-12: an obs entry is a sum of terms of both signs and the oracle's xi subtract a log-likelihood of 4e3 in
   float64 — trans 1.4e-12, obs 1.6e-12 element-wise.)
3. The reference itself against a 50-digit evaluation by path enumeration (mpmath) on a 3-state, 5-frame case at 1e-16:
   three orders below the float64 errors (1e-13 .. 1e-11) it is used to measure."""
import itertools

import numpy as np
import pytest

from tests import _fb_ref as F
from tests import _fb_regimes as R


@pytest.mark.parametrize("fn_args", R.all_cases(), ids=R.case_id)
def test_regime_conditions_hold(fn_args):
    fn, args = fn_args
    case = fn(*args)
    assert case.W == 3 and case.utt_model.shape == (len(case.utts),)
    assert all(X.dtype == np.float32 and X.shape[1] == case.D and X.shape[0] >= 1 for X in case.utts)
    if case.name != "long":
        lens = [X.shape[0] for X in case.utts]
        assert len(case.utts) == 48 and 1 <= min(lens) and max(lens) <= 109
    m = R.check_conditions(case, F.reference(case))
    print(R.case_id(fn_args), m)


def test_sep_1p5_is_not_soft_enough():
    """Why sep = 0.7: at 1.5 fewer than 10 % of the frames are soft at (39, 16)."""
    case = R.soft(39, 16, 1.5)
    m = R.measure(case, F.reference(case))
    print(m)
    assert m["soft_frames"] < 0.10 or m["gaps_lt2"] < 0.15


@pytest.mark.parametrize("D,ns", R.SHAPES)
def test_contained_batches(D, ns):
    b, bp, touched = R.contained(D, ns)
    assert [int((b.utt_model == w).sum()) for w in range(3)] == list(R.CONTAINED_COUNTS)
    assert sorted(touched.values()) == ["+inf", "-inf last", "nan", "nan frame"]
    assert [b.utt_model[u] for u in touched] == [1, 1, 1, 2]
    for u, (x, y) in enumerate(zip(b.utts, bp.utts)):
        assert np.isfinite(x).all()
        if u in touched:
            assert x.shape == y.shape and x.shape[0] >= 3 and not np.isfinite(y).all()
            bad = ~np.isfinite(y)
            assert np.array_equal(x[~bad], y[~bad])
            lls = [float(F.loglik(y, bp.sp[v], bp.A[v], bp.mu[v], bp.cv[v])) for v in range(3)]
            if touched[u].startswith("nan"):
                assert np.isnan(lls).all()
            else:
                assert all(v == -np.inf for v in lls)
        else:
            assert y is x
    assert bad.all(axis=1).sum() == 1           # (the last one touched: a whole NaN frame)


def test_reference_agrees_with_the_float64_oracle():
    case = R.soft(13, 8)
    ref, o64 = F.reference(case), F.float64_oracle(case)
    errs = {"ll": F.rel_err(o64.scores, ref.scores), "gamma": float(np.abs(o64.gamma - ref.gamma).max())}
    for k in F.STAT_KEYS:
        errs[k] = max(float(np.abs(o64.stats[w][k] - ref.stats[w][k]).max() / np.abs(ref.stats[w][k]).max())
                      for w in range(case.W))
    print(errs)
    for k, e in errs.items():
        assert e <= 1e-12, (k, e)
    assert np.array_equal(o64.path, ref.path)


def test_reference_against_path_enumeration_in_50_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    rng = np.random.default_rng(4)
    S, T, D = 3, 5, 2
    sp = rng.dirichlet(np.ones(S))
    A = rng.dirichlet(np.ones(S), S)
    A[2, 0] = 0.0                                           # a structural zero
    A[2] /= A[2].sum()
    mu, cv = rng.normal(0, 2, (S, D)), rng.uniform(0.5, 2.0, (S, D))
    X = rng.normal(0, 2, (T, D)).astype(np.float32)
    got = F.utterance(X, sp, A, mu, cv)

    f = mp.mpf
    b = [[mp.mpf(1) for _ in range(S)] for _ in range(T)]
    for t in range(T):
        for s in range(S):
            for d in range(D):
                v = f(float(cv[s, d]))
                b[t][s] *= mp.exp(-(f(float(X[t, d])) - f(float(mu[s, d]))) ** 2 / (2 * v)) / mp.sqrt(2 * mp.pi * v)
    total = f(0)
    gamma = [[f(0)] * S for _ in range(T)]
    xi = [[f(0)] * S for _ in range(S)]
    for q in itertools.product(range(S), repeat=T):
        p = f(float(sp[q[0]])) * b[0][q[0]]
        for t in range(1, T):
            p *= f(float(A[q[t - 1], q[t]])) * b[t][q[t]]
        total += p
        for t in range(T):
            gamma[t][q[t]] += p
        for t in range(1, T):
            xi[q[t - 1]][q[t]] += p

    def close(x, want, what):        # (a longdouble goes to mpmath through its decimal expansion, 30 digits)
        err = abs(mp.mpf(np.format_float_scientific(F.LD(x), precision=30, unique=False)) - want)
        assert err <= f("1e-16") * max(abs(want), 1), (what, err)

    close(got["ll"], mp.log(total), "ll")
    x2 = (X * X).astype(np.float64)
    for s in range(S):
        close(got["start"][s], gamma[0][s] / total, "start")
        close(got["post"][s], sum(gamma[t][s] for t in range(T)) / total, "post")
        for t in range(T):
            close(got["gamma"][t, s], gamma[t][s] / total, "gamma")
        for j in range(S):
            close(got["trans"][s, j], xi[s][j] / total, "trans")
        for d in range(D):
            close(got["obs"][s, d], sum(gamma[t][s] * f(float(X[t, d])) for t in range(T)) / total, "obs")
            close(got["obs2"][s, d], sum(gamma[t][s] * f(float(x2[t, d])) for t in range(T)) / total, "obs2")
    assert got["trans"][2, 0] == 0

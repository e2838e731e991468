"""CPU checks of the inputs tests/test_viterbi_cases_gpu.py decodes (tests/_viterbi_cases.py), from the two oracles alone.

For every case: the C oracle (oracle/hmm_oracle.c, what the GPU file compares with) and the numpy oracle
(oracle/hmmlearn_oracle.py) agree bit for bit on all W scores, on the best word and on the best word's path under both tie
rules; every score is finite; a structure case has the topology and the unreachable states it claims; in a tie case the
two rules give equal scores and paths that differ on at least half of the frames.

The numpy side is _viterbi_cases.numpy_viterbi — hmmlearn_oracle.log_density_diag (numpy's own summation order) and the
lattice of hmmlearn_oracle.viterbi evaluated a row at a time — on every utterance (every fifth one of a case with
utterances longer than 300 frames, the longest among them); hmmlearn_oracle.decode itself, a Python loop per state and
frame, runs on the best word of every fifth utterance and must give the same bits."""
import numpy as np
import pytest

from tests import _fb_regimes as R
from tests import _viterbi_cases as V

ALL = V.dense_cases() + V.bidiag_cases()


def _tview(u):
    """(T, D) transposed view of (D, T) storage: the layout whose numpy reduction is sum_order = 1."""
    return np.ascontiguousarray(u.T).T


def _check_oracles_agree(case, step_long=5):
    from oracle import hmmlearn_oracle as ho
    res = {tie: V.oracle(case, tie, 1) for tie in ("high", "low")}
    np.testing.assert_array_equal(res["high"][0], res["low"][0])           # the tie rule never changes a score
    np.testing.assert_array_equal(res["high"][1], res["low"][1])
    sc, bw, _ = res["high"]
    assert np.isfinite(sc).all() and (bw >= 0).all()
    _, offs = V.packed(case)
    lens = np.diff(offs)
    n = len(case.utts)
    picked = list(range(n)) if lens.max() <= 300 else sorted(set(range(0, n, step_long)) | {int(np.argmax(lens))})
    for u in picked:
        X = _tview(case.utts[u])
        for w in range(case.W):
            lp, st = V.numpy_viterbi(X, case.sp[w], case.A[w], case.mu[w], case.cv[w])
            assert lp == sc[u, w], (case, u, w)
            if w == bw[u]:
                for tie in ("high", "low"):
                    np.testing.assert_array_equal(st[tie], res[tie][2][offs[u]:offs[u + 1]])
                if u % 5 == 0 and lens[u] <= 300:
                    for tie in ("high", "low"):
                        lp2, st2 = ho.decode(X, case.sp[w], case.A[w], case.mu[w], case.cv[w], tie=tie)
                        assert lp2 == lp
                        np.testing.assert_array_equal(st2, st[tie])
    return res


@pytest.mark.parametrize("fn_args", ALL, ids=V.case_id)
def test_oracles_agree_and_case_is_what_it_claims(fn_args):
    case = V.make(fn_args)
    assert case.W == 3 and case.utt_model.shape == (len(case.utts),)
    assert all(X.dtype == np.float32 and X.shape[1] == case.D and X.shape[0] >= 1 for X in case.utts)
    assert case.bidiag == (fn_args in V.bidiag_cases()) == R.is_bidiagonal(case.A)
    np.testing.assert_allclose(case.sp.sum(axis=-1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(case.A.sum(axis=-1), 1.0, rtol=0, atol=1e-12)
    res = _check_oracles_agree(case)
    lens = [X.shape[0] for X in case.utts]
    kind = case.name
    if fn_args[0] is V.structure:
        assert len(case.utts) == 48 and 1 <= min(lens) and max(lens) <= 109
        want_dead = V.DEAD_STATES.get(kind, lambda S: [])(case.S)
        for w in range(case.W):
            dead = np.nonzero(~R.reachable(case.sp[w], case.A[w]))[0].tolist()
            assert dead == want_dead, (case, w, dead)
        path = res["high"][2]
        um = np.repeat(res["high"][1], lens)
        for w in range(case.W):                       # no path of a word visits one of its unreachable states
            assert not np.isin(path[um == w], want_dead).any()
        if kind in ("no_self_loop", "no_self_loop_48"):
            gone = (4, 7) if kind == "no_self_loop" else (4, 8)
            assert all((case.A[:, s, s] == 0).all() and (case.A[:, s, s + 1] == 1).all() for s in gone)
        if kind == "two_chains":                      # both halves of the chain are used
            first = path[np.r_[0, np.cumsum(lens)[:-1]]]
            assert set(first.tolist()) == {0, 6}
    elif fn_args[0] is V.long:
        want = R.LONG_LENGTHS if (case.D, case.ns) == (13, 8) else R.LONG_LENGTHS[:-1]
        assert lens == want + want and lens[0] == 1 and max(lens) == want[-1]
    elif kind == "dense_ties":
        assert lens == V.DENSE_TIE_LENGTHS
    else:
        assert kind == "bidiag_ties" and lens == V.bidiag_tie_lengths(case.S)
    if V.is_tie_case(case):
        differ = int((res["high"][2] != res["low"][2]).sum())
        print(f"{V.case_id(fn_args)}: the two tie rules' paths differ on {differ} of {sum(lens)} frames")
        assert 2 * differ >= sum(lens), (differ, sum(lens))
        if kind == "dense_ties":
            assert differ == sum(lens) - len(lens)    # every frame but each utterance's last
    else:
        # sampled data, no exact ties: the tie rule changes nothing (what makes the tie cases necessary)
        np.testing.assert_array_equal(res["high"][2], res["low"][2])


@pytest.mark.parametrize("D,ns", [(13, 8), (39, 16)])
def test_pairwise_order_differs_from_the_decoders_order(D, ns):
    """sum_order = 0 is another summation, not another name: some score bits differ, and the C oracle follows numpy's
    pair-wise reduction of a C-contiguous array."""
    case = V.structure(D, ns, "skips")
    s1, s0 = V.oracle(case, "high", 1)[0], V.oracle(case, "high", 0)[0]
    assert (s1 != s0).any()
    np.testing.assert_allclose(s0, s1, rtol=1e-13)
    for u in range(0, len(case.utts), 6):
        for w in range(case.W):
            lp, _ = V.numpy_viterbi(np.ascontiguousarray(case.utts[u]), case.sp[w], case.A[w], case.mu[w], case.cv[w],
                                    ties=())
            assert lp == s0[u, w]


@pytest.mark.parametrize("D,ns", R.SHAPES)
@pytest.mark.parametrize("dense", [False, True])
def test_contained_batches_are_finite_where_untouched(D, ns, dense):
    b, bp, touched = V.contained(D, ns, dense)
    assert b.bidiag != dense and len(touched) == 4
    sc, bw, _ = V.oracle(b, "high", 1)
    assert np.isfinite(sc).all() and (bw >= 0).all()
    sc2, bw2, path2 = V.oracle(bp, "high", 1)
    clean = np.asarray([u not in touched for u in range(len(b.utts))])
    np.testing.assert_array_equal(sc2[clean], sc[clean])
    # the touched utterances are not compared with an oracle on the GPU: the two oracles disagree about them (the C
    # oracle's strict '>' maximum drops a NaN candidate and ends at -inf or a finite number, numpy's max propagates it)
    assert not np.isfinite(sc2[~clean]).any()

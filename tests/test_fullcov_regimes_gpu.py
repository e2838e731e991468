"""The full-covariance family (sapr_full_estep, sapr_full_viterbi, sapr_full_vocab in both modes,
sapr_connected_emit_full) on models whose states differ in their covariance matrices, on soft posteriors, at the edges of
the 16-wide matrix-core tiles and of the 64-frame chunks, against the np.longdouble reference of
tests/_fullcov_regimes.py (which see for the regimes and the conditions each one meets; they are asserted here before
anything is compared).  Everything goes through the C ABI by way of sapr_amd/full_cov.py and sapr_amd/connected.py.

Tolerances.  The project's pins for this family: rtol 1e-11 on log-likelihoods, Viterbi scores and logb; rtol 1e-9 with
atol 1e-12 on posteriors and on start / trans / post / obs (measured as |x - ref| / (1e-3 + |ref|) <= 1e-9, the same
statement); every oo[s] within 1e-9 of its own largest entry and exactly symmetric.  For every case E_ref, the deviation
of the float64 restatement tests/_fullcov_ref.py from the longdouble reference on the same inputs, is computed on the
CPU in the same measure, and the kernel is allowed max(pin, 4 * E_ref): the factor covers the explicit inverse in place
of a triangular solve and a different summation order, both at float64.  Every test prints the kernel's error, E_ref
and the tolerance used.

MEASURED on an MI355X, kernel error / E_ref, the largest over the cases of a regime (relative on logb, log-likelihoods
and scores; |x - ref| / (1e-3 + |ref|) on gamma, start, trans, post, obs; norm-wise per state on oo; "vocab" = both
modes of sapr_full_vocab over every (utterance, word) pair, "logb" = sapr_connected_emit_full; * = 4 * E_ref is above the
pin in a case of the regime and decides its tolerance):
    regime  logb                 loglik               viterbi              vocab                gamma                start                trans                post                 obs                  oo                   logprob
    soft    4.2e-13 / 4.2e-13    5.4e-15 / 5.4e-15    8.2e-15 / 8.0e-15    1.9e-13 / 1.9e-13    7.1e-12 / 5.9e-12    2.3e-13 / 1.7e-13    3.8e-12 / 3.6e-12    3.0e-13 / 4.5e-13    1.9e-10 / 1.6e-10    2.8e-13 / 4.2e-13    7.5e-16 / 5.9e-16
    ill     3.2e-11 / 3.2e-11*   2.5e-13 / 2.5e-13    2.5e-13 / 2.5e-13    2.1e-11 / 2.1e-11*   1.3e-10 / 1.3e-10    6.0e-12 / 6.0e-12    1.0e-11 / 9.6e-12    2.9e-12 / 2.9e-12    2.7e-09 / 2.6e-09*   6.1e-12 / 6.2e-12    6.9e-15 / 6.9e-15
    tied    -                    3.2e-15 / 3.5e-15    3.4e-15 / 3.6e-15    1.2e-13 / 1.2e-13    5.0e-12 / 5.0e-12    7.8e-14 / 1.7e-13    3.3e-12 / 2.6e-12    7.2e-13 / 5.6e-13    2.8e-09 / 1.5e-09*   7.2e-13 / 5.4e-13    4.1e-16 / 4.1e-16
    ragged  -                    1.1e-15 / 1.0e-15    2.6e-15 / 2.3e-15    -                    3.7e-12 / 3.1e-12    7.2e-13 / 7.1e-13    6.5e-12 / 6.5e-12    5.0e-13 / 5.1e-13    4.0e-11 / 6.4e-11    5.0e-13 / 5.1e-13    4.7e-16 / 5.0e-16
The pin decides everywhere except: logb and the vocabulary scores of the three ill-conditioned cases (E_ref 1.1e-11 ..
3.2e-11, tolerance 4.4e-11 .. 1.3e-10), and obs in ill-13-10, ill-17-5, ill-39-18 and tied-33-17 (E_ref 3.2e-10 ..
2.6e-9; the largest ratio kernel / E_ref is 1.9, in tied-33-17: an entry of obs[s] that nearly cancels, see the CPU
table).  On the densities the kernel's error EQUALS the float64 restatement's to three digits, in every regime: both start
from the same float64 np.linalg.cholesky, and a longdouble forward substitution with that float64 factor has the same
error (3.16e-11 at ill-13-10), so the error of the ill-conditioned regime is the factorisation's; the explicit inverse
of full_cov._inv_lower and the device's dot-product chains add nothing that can be measured beside it.

The MAP path and the Viterbi path are compared on every frame and the best word on every utterance: the conditions
assert that the reference's smallest gap between the two largest posteriors of a frame exceeds 1e-6, its smallest
relative Viterbi arg-max gap 1e-9, and the vocabulary test that the relative gap between an utterance's best and
second-best word exceeds 1e-9.  Where the reference holds an exact zero (a state the chain has not reached yet, a
padding state, a word without utterances) the device must hold one too."""
import functools

import numpy as np
import pytest

from tests import _fullcov_regimes as R

pytestmark = pytest.mark.gpu

RTOL_LL = 1e-11
TOL = 1e-9
FACTOR = 4
CASES = R.all_cases()


def _prepare(fn_args):
    """The case, its longdouble reference and E_ref; the regime's conditions are asserted here."""
    fn, args = fn_args
    case = fn(*args)
    want = R.reference(case)
    R.check_conditions(case, want)
    return case, want, R.e_ref(case)


def _within(what, err, pin, e_ref):
    tol = max(pin, FACTOR * e_ref)
    print(f"    {what:8s} kernel error {err:.3e}   E_ref {e_ref:.3e}   tolerance {tol:.3e}"
          f"{'   (E_ref decides)' if tol > pin else ''}")
    assert err <= tol, (what, err, tol)


@functools.lru_cache(maxsize=None)
def _batch(case, S=None):
    from sapr_amd import full_cov
    S = case.S if S is None else S
    return (full_cov.FullCovBatch(np.array(case.feats), case.lengths, case.utt_model, case.W, S),
            full_cov.pack_models(case.params, S))


@functools.lru_cache(maxsize=None)
def _gpu_estep(case):
    """(loglik, stats, post, path) as host arrays, one launch over all of the case's models."""
    batch, pack = _batch(case)
    return tuple(t.cpu().numpy() for t in batch.estep(pack, want_stats=True, want_post=True, want_path=True))


@functools.lru_cache(maxsize=None)
def _gpu_viterbi(case):
    batch, pack = _batch(case)
    return tuple(t.cpu().numpy() for t in batch.viterbi(pack))


def _split(row, S, D, S_model=None):
    from sapr_amd import full_cov
    st = full_cov.split_stats(row, S, D, S_model)
    st["oo"] = st["obs*obs.T"]
    return st


@pytest.mark.parametrize("fn_args", CASES, ids=R.case_id)
def test_estep(fn_args):
    case, want, e = _prepare(fn_args)
    S, D = case.S, case.D
    loglik, stats, post, path = _gpu_estep(case)
    print(f"{case!r} sapr_full_estep; reference's smallest top-two gap {float(want.top_gap.min()):.3e}")
    assert loglik.shape == want.ll.shape and np.isfinite(loglik[case.lengths > 0]).all()
    _within("loglik", R.rel_err(loglik, want.ll), RTOL_LL, e["ll"])
    assert post.shape == want.gamma.shape and post.dtype == np.float64
    _within("gamma", R.mixed_err(post, want.gamma), TOL, e["gamma"])
    assert (post[np.asarray(want.gamma == 0)] == 0).all()            # a state the chain cannot have reached: exactly 0
    print(f"    MAP path differs on {int((path != want.path).sum())} of {path.size} frames")
    assert path.dtype == np.int32 and np.array_equal(path, want.path)       # every frame, none left out
    got = [_split(stats[w], S, D) for w in range(case.W)]
    errs = R.stat_errs(case, lambda w: got[w], want)
    for k in ("start", "trans", "post", "obs"):
        _within(k, errs[k], TOL, e[k])
    _within("oo", errs["oo"], TOL, e["oo"])
    _within("logprob", errs["logprob"], RTOL_LL, e["logprob"])
    for w in range(case.W):
        assert got[w]["nobs"] == want.stats[w]["nobs"]
        for s in range(S):
            assert np.array_equal(got[w]["oo"][s], got[w]["oo"][s].T), (w, s)
        for k in R.STAT_KEYS:                                         # the reference's exact zeros are exact here too
            assert (got[w][k][np.asarray(want.stats[w][k] == 0)] == 0).all(), (w, k)
        if want.stats[w]["nobs"] == 0:
            assert not stats[w].any(), w                              # a word without utterances: an all-zero row
    if (case.regime, D, S) == ("soft", 5, 3):
        # the same models at 4 kernel states: the padding state gives exact zeros, the rest the same bits
        wide, pack4 = _batch(case, 4)
        l4, s4, p4, q4 = (t.cpu().numpy() for t in wide.estep(pack4, True, True, True))
        assert np.array_equal(l4, loglik) and np.array_equal(p4[:, :3], post) and np.all(p4[:, 3] == 0)
        assert np.array_equal(q4, path)
        for w in range(case.W):
            whole, own = _split(s4[w], 4, D), _split(s4[w], 4, D, 3)
            for k in R.STAT_KEYS:
                assert np.array_equal(own[k], got[w][k]), k
                assert np.all(whole[k][3:] == 0), k
            assert np.all(whole["trans"][:, 3] == 0)


@pytest.mark.parametrize("fn_args", CASES, ids=R.case_id)
def test_viterbi(fn_args):
    case, want, e = _prepare(fn_args)
    logprob, path = _gpu_viterbi(case)
    print(f"{case!r} sapr_full_viterbi; reference's smallest relative arg-max gap {want.vit_gap:.3e}")
    _within("viterbi", R.rel_err(logprob, want.vit_score), RTOL_LL, e["vit"])
    assert path.dtype == np.int32 and path.shape == (case.feats.shape[0],)
    print(f"    path differs on {int((path != want.vit_path).sum())} of {path.size} frames")
    assert np.array_equal(path, want.vit_path)                        # every frame


@pytest.mark.parametrize("fn_args", R.vocab_cases(), ids=R.case_id)
def test_vocabulary_scores(fn_args):
    """Both modes against the reference of every (utterance, word) pair; column w carries the bits of the per-model
    entry points for the utterances of word w — with a covariance matrix of its own in every state."""
    from sapr_amd import full_cov
    case, want, e = _prepare(fn_args)
    pack = full_cov.FullPack.from_params(case.params)
    own = {"forward": _gpu_estep(case)[0], "viterbi": _gpu_viterbi(case)[0]}
    for mode in ("forward", "viterbi"):
        ref_sc = want.scores[mode]
        top = np.sort(ref_sc, axis=1)
        gap = float(((top[:, -1] - top[:, -2]) / np.abs(top[:, -1])).min())
        assert gap > 1e-9, gap
        vs = full_cov.vocab_scores(np.array(case.feats), case.lengths, pack, mode=mode)
        sc, bw = vs.score.cpu().numpy(), vs.best_word.cpu().numpy()
        print(f"{case!r} sapr_full_vocab, {mode}; reference's smallest relative gap best / second-best {gap:.3e}")
        assert sc.shape == ref_sc.shape and sc.dtype == np.float64
        _within(mode, R.rel_err(sc, ref_sc), RTOL_LL, e[mode])
        print(f"    best word differs on {int((bw != np.argmax(ref_sc, axis=1)).sum())} of {bw.size} utterances")
        assert np.array_equal(bw, np.argmax(ref_sc, axis=1))          # every utterance
        rows = np.arange(len(case.utts))
        assert np.array_equal(sc[rows, case.utt_model], own[mode]), mode


@pytest.mark.parametrize("fn_args", R.emit_cases(), ids=R.case_id)
def test_connected_emission(fn_args):
    """sapr_connected_emit_full: logb[T, W, S] of the same frames against the longdouble log density; padded columns
    are -inf."""
    import torch
    from sapr_amd import connected, full_cov
    case, want, e = _prepare(fn_args)
    W, S = case.W, case.S
    pack = full_cov.FullPack.from_params(case.params)
    with np.errstate(divide="ignore"):
        net = connected.ConnectedNetwork(np.log([p[0] for p in case.params]), np.log([p[1] for p in case.params]),
                                         np.zeros((W, S)), 0.0, family="full", pack=pack)
    logb = connected.emit_full(torch.from_numpy(np.array(case.feats)).cuda(), net).cpu().numpy()
    assert logb.shape == (case.feats.shape[0], net.R) and net.R == W * net.SP
    logb = logb.reshape(-1, W, net.SP)
    print(f"{case!r} sapr_connected_emit_full")
    assert np.isfinite(logb[:, :, :S]).all()
    _within("logb", max(R.rel_err(logb[:, w, :S], want.logb[w]) for w in range(W)), RTOL_LL, e["logb"])
    assert np.all(logb[:, :, S:] == -np.inf)


@pytest.mark.parametrize("fn_args", [(R.soft, (13, 10, "bidiag")), (R.soft, (17, 5, "dense")), (R.ragged, ())],
                         ids=R.case_id)
def test_determinism_and_batch_independence(fn_args):
    """A second launch returns the same bytes, and every word alone the bits it gave inside the batch."""
    from sapr_amd import full_cov
    case, want, _ = _prepare(fn_args)
    batch, pack = _batch(case)
    first = _gpu_estep(case)
    again = tuple(t.cpu().numpy() for t in batch.estep(pack, want_stats=True, want_post=True, want_path=True))
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    vit = _gpu_viterbi(case)
    for a, b in zip(vit, (t.cpu().numpy() for t in batch.viterbi(pack))):
        assert a.tobytes() == b.tobytes()
    loglik, stats, post, path = first
    for w in range(case.W):
        sel = np.nonzero(case.utt_model == w)[0]
        if sel.size == 0:
            continue
        rows = slice(case.offs[sel[0]], case.offs[sel[-1] + 1])      # (a word's utterances are consecutive)
        one = full_cov.FullCovBatch(np.array(case.feats[rows]), case.lengths[sel], np.zeros(sel.size, np.int64), 1,
                                    case.S)
        pack1 = full_cov.pack_models([case.params[w]])
        l1, s1, p1, q1 = (t.cpu().numpy() for t in one.estep(pack1, True, True, True))
        assert np.array_equal(l1, loglik[sel]) and np.array_equal(s1[0], stats[w])
        assert np.array_equal(p1, post[rows]) and np.array_equal(q1, path[rows])
        v1 = tuple(t.cpu().numpy() for t in one.viterbi(pack1))
        assert np.array_equal(v1[0], vit[0][sel]) and np.array_equal(v1[1], vit[1][rows])


def _model(prm, ct):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    m = GaussianHMM(n_components=prm[2].shape[0], covariance_type=ct, init_params="")
    m.startprob_, m.transmat_, m.means_ = (np.array(a) for a in prm[:3])
    m.covars_ = np.array(prm[3][0] if ct == "tied" else prm[3])
    return m


@pytest.mark.parametrize("fn_args", [(R.tied, s) for s in R.TIED_SHAPES], ids=R.case_id)
def test_tied_carries_the_bits_of_full(fn_args):
    """One matrix per word as a "tied" GaussianHMM and as a "full" one with S copies: the same operand block and so the
    same bits from the device (their accuracy is test_estep's and test_viterbi's business)."""
    from sapr_amd import full_cov
    case, want, _ = _prepare(fn_args)
    tied_models = [_model(prm, "tied") for prm in case.params]
    full_models = [_model(prm, "full") for prm in case.params]
    assert tied_models[0]._covars_.shape == (case.D, case.D)
    assert full_models[0]._covars_.shape == (case.S, case.D, case.D)
    pt = full_cov.pack_models([m._full_params() for m in tied_models], name="tied")
    pf = full_cov.pack_models([m._full_params() for m in full_models])
    assert pt.tobytes() == pf.tobytes() == _batch(case)[1].tobytes()
    batch, _ = _batch(case)
    a = tuple(t.cpu().numpy() for t in batch.estep(pt, True, True, True))
    for x, y in zip(a, _gpu_estep(case)):
        assert x.tobytes() == y.tobytes()
    for x, y in zip((t.cpu().numpy() for t in batch.viterbi(pt)), _gpu_viterbi(case)):
        assert x.tobytes() == y.tobytes()
    w = 1
    sel = case.utt_model == w
    X, lengths = np.array(case.feats[case.offs[8]:case.offs[16]]), case.lengths[sel]
    (lt, gt), (lf, gf) = tied_models[w].score_samples(X, lengths), full_models[w].score_samples(X, lengths)
    assert lt == lf == a[0][sel].sum() and np.array_equal(gt, gf)
    (vt, st), (vf, sf) = tied_models[w].decode(X, lengths), full_models[w].decode(X, lengths)
    assert vt == vf and np.array_equal(st, sf) and np.array_equal(st, want.vit_path[case.offs[8]:case.offs[16]])

"""The forward family (sapr_forward_diag, sapr_estep_diag — fused, SAPR_ESTEP_OBS=split and dense routes —,
sapr_forward_vocab, sapr_state_posteriors_diag) on soft posteriors and numeric edges, against the np.longdouble
forward-backward of tests/_fb_ref.py on the inputs of tests/_fb_regimes.py (which see for the regimes and the conditions
each one meets; they are asserted here before anything is compared).

Tolerances.  The project's pins: rtol 1e-11 on log-likelihoods, rtol = atol = 1e-9 on posteriors and statistics
(|x - ref| / (1 + |ref|) <= 1e-9).  For every case E_ref, the deviation of the float64 numpy oracle
(oracle/hmmlearn_oracle.py) from the longdouble reference on the same inputs, is computed on the CPU in the same
measure, and the kernel is allowed max(pin, 4 * E_ref): the factor covers a different summation order, the quick
emission form's extra rounding per term and the 4.5 ulp of lse_unit.h, all at float64.  Every test prints the kernel's
error, E_ref and the tolerance used.

MEASURED on an MI355X, kernel error / E_ref, the largest over the entry points and the shapes of a regime (relative on
log-likelihoods, |x - ref| / (1 + |ref|) otherwise; "lattice" = the posterior rows of sapr_state_posteriors_diag):
    regime                 loglik             lattice            trans              post               obs                obs**2
    soft                   2.8e-15 / 2.8e-15  7.6e-13 / 7.2e-13  7.2e-13 / 1.7e-11  8.0e-13 / 5.1e-13  2.2e-12 / 1.7e-11  1.9e-12 / 1.3e-12
    soft, split route      2.5e-15 / 2.8e-15  -                  3.8e-13 / 1.7e-11  4.5e-13 / 4.0e-13  2.2e-12 / 1.7e-11  1.4e-12 / 1.3e-12
    separated              1.9e-15 / 1.9e-15  0 / 0              0 / 9.4e-12        0 / 0              0 / 0              7.7e-17 / 7.7e-17
    clamp boundary         2.5e-15 / 2.5e-15  4.3e-29 / 2.3e-41  8e-141 / 1.1e-11   8e-141 / 8e-141    2e-138 / 2e-138    8.3e-17 / 8.3e-17
    far                    2.5e-15 / 2.5e-15  0 / 0              0 / 2.6e-06        0 / 0              0 / 0              0 / 0
    long                   5.6e-14 / 5.6e-14  4.7e-13 / 1.2e-11  1.7e-13 / 1.3e-10  1.3e-13 / 1.9e-12  3.1e-12 / 4.4e-11  4.0e-13 / 3.8e-12
    structure, bidiagonal  2.9e-15 / 2.9e-15  7.6e-13 / 8.7e-13  3.9e-13 / 1.6e-11  4.5e-13 / 4.0e-13  1.9e-12 / 1.4e-11  1.4e-12 / 1.7e-12
    structure, dense       2.4e-15 / 2.4e-15  8.4e-13 / 9.0e-13  7.4e-12 / 7.4e-12  2.1e-13 / 4.0e-13  1.1e-11 / 2.2e-11  8.9e-13 / 1.1e-12
start: at most 3.4e-13 / 3.9e-13 (dense), summed log-prob of a word: at most 1.5e-15.  The pin decides in every case
but one: trans in the far regime, where the oracle's exp(fwd + log a + b + bwd - logprob) loses seven digits to a
log-likelihood of 1e9 (E_ref 2.6e-6, tolerance 1.0e-5) while the bidiagonal kernel, whose smoothing recursion never forms
that difference, has no error at all.  Everything else is two orders or more below its pin.

The MAP path is compared on every frame and the best word on every utterance: each case asserts first that the
reference's smallest gap between the two largest posteriors of a frame exceeds 1e-6 and that the relative gap between
the best and the second-best score of an utterance exceeds 1e-9.

Contained regime: batch B' is batch B with a NaN, a +inf, a -inf (last frame) in three utterances of word 1 and a whole
NaN frame in one utterance of word 2.  Every other utterance keeps its bits in all four entry points, word 0's
statistics keep theirs, and a touched utterance's log-likelihood is NaN where the reference's is NaN and -inf where
the reference's is -inf."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _fb_ref as F
from tests import _fb_regimes as R

pytestmark = pytest.mark.gpu

RTOL_LL = 1e-11
TOL = 1e-9
FACTOR = 4
CASES = R.all_cases()
STAT_NAMES = (("start", "start"), ("trans", "trans"), ("post", "post"), ("obs", "obs"), ("obs2", "obs**2"))


def _batch(utts):
    import torch
    from sapr_amd.trellis import FeatureBatch
    packed = np.ascontiguousarray(np.concatenate(utts, axis=0), dtype=np.float32)
    return FeatureBatch.from_packed(torch.from_numpy(packed).cuda(), np.asarray([u.shape[0] for u in utts]))


def _pack(case):
    from sapr_amd import _lib
    from sapr_amd.trellis import DiagModelPack, kernel_dims, kernel_states
    pack = DiagModelPack.from_params(case.sp, case.A, case.mu, case.cv)
    assert pack.topology == (_lib.TOPO_BIDIAG if case.bidiag else _lib.TOPO_DENSE)
    assert (pack.S_model, pack.D_model) == (case.S, case.D)
    assert (pack.S, pack.D) == (kernel_states(case.S), kernel_dims(case.D)) and pack.S in (10, 18) and pack.D in (13, 39)
    return pack


def _prepare(fn_args):
    """The case, its longdouble reference and E_ref; the regime's conditions are asserted here."""
    fn, args = fn_args
    case = fn(*args)
    ref = F.reference(case)
    R.check_conditions(case, ref)
    return case, ref, F.e_ref(case)


def _within(what, err, pin, e_ref):
    tol = max(pin, FACTOR * e_ref)
    print(f"    {what:8s} kernel error {err:.3e}   E_ref {e_ref:.3e}   tolerance {tol:.3e}"
          f"{'   (E_ref decides)' if tol > pin else ''}")
    assert err <= tol, (what, err, tol)


def _check_loglik(ll, ref_ll, e):
    assert np.isfinite(ll).all()
    _within("loglik", F.rel_err(ll, ref_ll), RTOL_LL, e["ll"])


def _check_stats(case, ref, e, es_split, stats, ll):
    _check_loglik(ll, ref.ll, e)
    for k_ref, k_got in STAT_NAMES:
        err = max(F.scaled_err(es_split(stats[w])[k_got], ref.stats[w][k_ref]) for w in range(case.W))
        _within(k_got, err, TOL, e[k_ref])
    for w in range(case.W):
        got = es_split(stats[w])
        assert got["nobs"] == ref.stats[w]["nobs"]
        if ref.stats[w]["nobs"]:
            _within("logprob", F.rel_err(got["logprob"], ref.stats[w]["logprob"]), RTOL_LL, e["logprob"])
        assert got["trans"].shape == (case.S, case.S) and got["obs"].shape == (case.S, case.D)
        for k_ref, k_got in STAT_NAMES:          # structural zeros and unreachable states: exact zeros
            assert (got[k_got][np.asarray(ref.stats[w][k_ref] == 0)] == 0).all(), k_got


@pytest.mark.parametrize("fn_args", CASES, ids=R.case_id)
def test_forward_loglik(fn_args):
    from sapr_amd.trellis import forward_loglik
    case, ref, e = _prepare(fn_args)
    ll = forward_loglik(_batch(case.utts), _pack(case), case.utt_model).cpu().numpy()
    print(f"{case!r} sapr_forward_diag")
    _check_loglik(ll, ref.ll, e)


@pytest.mark.parametrize("fn_args", CASES, ids=R.case_id)
def test_estep_statistics(fn_args):
    """EStep.run twice: the second call reads the features it staged in the first."""
    from sapr_amd.trellis import EStep
    case, ref, e = _prepare(fn_args)
    pack = _pack(case)
    es = EStep(_batch(case.utts), case.utt_model, case.W, case.S)
    first = es.run(pack).cpu().numpy().copy()
    ll_first = es.loglik.cpu().numpy().copy()
    second = es.run(pack).cpu().numpy().copy()
    assert es._staged
    print(f"{case!r} sapr_estep_diag, {'bidiagonal' if case.bidiag else 'dense'} route")
    _check_stats(case, ref, e, es.split, first, ll_first)
    np.testing.assert_array_equal(second, first)
    np.testing.assert_array_equal(es.loglik.cpu().numpy(), ll_first)


@pytest.mark.parametrize("fn_args", CASES, ids=R.case_id)
def test_state_posteriors_and_map_path(fn_args):
    from sapr_amd.trellis import state_posteriors
    case, ref, e = _prepare(fn_args)
    res = state_posteriors(_batch(case.utts), _pack(case), case.utt_model)
    ll, post, path = res.loglik.cpu().numpy(), res.post.cpu().numpy(), res.path.cpu().numpy()
    print(f"{case!r} sapr_state_posteriors_diag; reference's smallest top-two gap {float(ref.top_gap.min()):.3e}")
    _check_loglik(ll, ref.ll, e)
    assert post.shape == ref.gamma.shape and post.dtype == np.float64
    _within("post", F.scaled_err(post, ref.gamma), TOL, e["gamma"])
    assert (post >= 0).all()
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0.0, atol=1e-12)
    assert (post[np.asarray(ref.gamma == 0)] == 0).all()          # unreachable states: exactly 0
    print(f"    path differs on {int((path != ref.path).sum())} of {path.size} frames")
    np.testing.assert_array_equal(path, ref.path)                  # every frame, none left out


@pytest.mark.parametrize("fn_args", CASES, ids=R.case_id)
def test_forward_scores_and_best_word(fn_args):
    from sapr_amd.trellis import forward_scores
    case, ref, e = _prepare(fn_args)
    top = np.sort(ref.scores, axis=1)
    gap = float(((top[:, -1] - top[:, -2]) / np.abs(top[:, -1])).min())
    assert gap > 1e-9, gap
    fs = forward_scores(_batch(case.utts), _pack(case))
    ll, bw = fs.loglik.cpu().numpy(), fs.best_word.cpu().numpy()
    print(f"{case!r} sapr_forward_vocab; reference's smallest relative gap best / second-best {gap:.3e}")
    assert ll.shape == ref.scores.shape
    _check_loglik(ll, ref.scores, e)
    print(f"    best word differs on {int((bw != np.argmax(ref.scores, axis=1)).sum())} of {bw.size} utterances")
    np.testing.assert_array_equal(bw, np.argmax(ref.scores, axis=1))          # every utterance


SPLIT_WORKER = r'''
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from sapr_amd.trellis import DiagModelPack, EStep, FeatureBatch
from tests import _fb_regimes as R
case = R.soft(int(sys.argv[3]), int(sys.argv[4]))
packed = np.ascontiguousarray(np.concatenate(case.utts, axis=0), dtype=np.float32)
batch = FeatureBatch.from_packed(torch.from_numpy(packed).cuda(), np.asarray([u.shape[0] for u in case.utts]))
es = EStep(batch, case.utt_model, case.W, case.S)
pack = DiagModelPack.from_params(case.sp, case.A, case.mu, case.cv)
a = es.run(pack).cpu().numpy().copy()
b = es.run(pack).cpu().numpy().copy()      # second call: staged features
assert np.array_equal(a, b)
np.savez(sys.argv[2], stats=a, loglik=es.loglik.cpu().numpy())
print("ok")
'''


@pytest.mark.parametrize("D,ns", R.SHAPES)
def test_estep_split_route(D, ns, tmp_path):
    """SAPR_ESTEP_OBS=split is read once per process: a fresh child runs the soft regime through the split pair."""
    from sapr_amd.trellis import split_stats
    case, ref, e = _prepare((R.soft, (D, ns)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "w.py"
    script.write_text(SPLIT_WORKER)
    env = dict(os.environ)
    env["SAPR_ESTEP_OBS"] = "split"
    out = str(tmp_path / "split.npz")
    p = subprocess.run([sys.executable, str(script), root, out, str(D), str(ns)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0 and "ok" in p.stdout, (p.stdout + p.stderr)[-3000:]
    got = dict(np.load(out))
    print(f"{case!r} sapr_estep_diag, SAPR_ESTEP_OBS=split")
    _check_stats(case, ref, e, lambda row: split_stats(row, case.S, case.D), got["stats"], got["loglik"])


def _same_class(got, want):
    """NaN where the reference gives NaN, -inf where it gives -inf; never a finite number."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert not np.isfinite(want).any()
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == -np.inf, want == -np.inf))


@pytest.mark.parametrize("D,ns", R.SHAPES)
def test_non_finite_features_are_contained(D, ns):
    import torch
    from sapr_amd.trellis import EStep, forward_loglik, forward_scores, state_posteriors
    b, bp, touched = R.contained(D, ns)
    pack = _pack(b)
    um = b.utt_model
    n = len(b.utts)
    clean = np.asarray([u not in touched for u in range(n)])
    hit = np.asarray(sorted(touched))
    assert clean.sum() == n - 4 and [int(um[u]) for u in hit] == [1, 1, 1, 2]
    want = np.asarray([[float(F.loglik(bp.utts[u], bp.sp[v], bp.A[v], bp.mu[v], bp.cv[v])) for v in range(b.W)]
                       for u in hit])                               # the reference's class, under every model
    own = want[np.arange(4), um[hit]]
    print(f"contained ({D}, {ns}): touched {touched}, reference log-likelihoods {own}")
    batches = [_batch(b.utts), _batch(bp.utts)]
    keep = torch.from_numpy(clean).cuda()
    rows = torch.from_numpy(np.repeat(clean, [x.shape[0] for x in b.utts])).cuda()
    wrong = []                # every entry point is run and printed before the first of these fails the test

    def expect(ok, what):
        if not ok:
            wrong.append(what)

    fl = [forward_loglik(x, pack, um) for x in batches]
    print(f"    sapr_forward_diag          {fl[1].cpu().numpy()[hit]}")
    expect(torch.equal(fl[0][keep], fl[1][keep]) and bool(torch.isfinite(fl[0]).all()), "forward_diag: untouched bits")
    expect(_same_class(fl[1].cpu().numpy()[hit], own), "forward_diag: class of the touched utterances")

    sp = [state_posteriors(x, pack, um) for x in batches]
    print(f"    sapr_state_posteriors_diag {sp[1].loglik.cpu().numpy()[hit]}")
    expect(torch.equal(sp[0].loglik[keep], sp[1].loglik[keep]), "state_posteriors: untouched log-likelihoods")
    expect(torch.equal(sp[0].post[rows], sp[1].post[rows]), "state_posteriors: untouched posterior rows")
    expect(torch.equal(sp[0].path[rows], sp[1].path[rows]), "state_posteriors: untouched paths")
    expect(_same_class(sp[1].loglik.cpu().numpy()[hit], own), "state_posteriors: class of the touched utterances")

    fs = [forward_scores(x, pack) for x in batches]
    print(f"    sapr_forward_vocab         {fs[1].loglik.cpu().numpy()[hit].tolist()}, best word "
          f"{fs[1].best_word.cpu().numpy()[hit]}")
    expect(torch.equal(fs[0].loglik[keep], fs[1].loglik[keep]), "forward_vocab: all W columns of an untouched row")
    expect(torch.equal(fs[0].best_word[keep], fs[1].best_word[keep]), "forward_vocab: untouched best words")
    expect(torch.equal(fs[0].word_post[keep], fs[1].word_post[keep]), "forward_vocab: untouched word posteriors")
    expect(_same_class(fs[1].loglik.cpu().numpy()[hit], want), "forward_vocab: class of the touched rows")
    # include/sapr_hip.h: the first strict maximum from -inf; neither NaN nor -inf beats -inf, so such a row has no word
    expect(bool((fs[1].best_word.cpu().numpy()[hit] == -1).all()), "forward_vocab: best word of a touched row is -1")

    stats, lls = [], []
    for x in batches:
        es = EStep(x, um, b.W, b.S)
        es.run(pack)
        stats.append(es.run(pack).cpu().numpy().copy())                     # (the staged second call)
        lls.append(es.loglik.clone())
    print(f"    sapr_estep_diag            {lls[1].cpu().numpy()[hit]}, logprob of words 1, 2: {stats[1][1:, 1]}")
    expect(torch.equal(lls[0][keep], lls[1][keep]), "estep: untouched log-likelihoods")
    expect(np.array_equal(stats[0][0], stats[1][0]), "estep: word 0's statistics keep their bits")
    expect(bool(np.isfinite(stats[0]).all()), "estep: the clean batch is finite")
    expect(_same_class(lls[1].cpu().numpy()[hit], own), "estep: class of the touched utterances")
    expect(not np.isfinite(stats[1][1, 1]) and not np.isfinite(stats[1][2, 1]), "estep: logprob of words 1 and 2")
    assert not wrong, wrong

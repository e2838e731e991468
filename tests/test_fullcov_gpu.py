"""GaussianHMM with "full", "tied" and "spherical" covariances on the GPU (the family of csrc/fullcov_ops.h over the
engine of csrc/tile_trellis.h, through sapr_amd/full_cov.py and sapr_amd/hmmlearn_hmm.py) against the numpy restatement tests/_fullcov_ref.py on the
seeded cases of tests/_fullcov_cases.py (shapes, seeds and the reference results, computed once per case; their
conditioning is established by tests/test_fullcov_cpu.py).

Tolerances are the project's pins for the mixture kernels: loglik and Viterbi scores rtol 1e-11;
start / trans / post / obs and the posteriors rtol 1e-9 with atol 1e-12; every oo[s] within 1e-9 of its own
largest-magnitude entry (norm-wise on purpose: the features sit near -300 in c0, so small entries carry the rounding of
the large ones) and exactly symmetric.  Trained parameters after three EM iterations: history rtol 1e-9, means rtol
1e-7, every covariance matrix within 1e-7 of its largest entry and exactly symmetric."""
import ctypes
import functools

import numpy as np
import pytest

from tests import _fullcov_cases as fc
from tests import _fullcov_ref as ref

pytestmark = pytest.mark.gpu

NAMES = list(fc.CASES)
MULTI = ["d13_s10_bidiag", "d5_s3_dense"]      # the cases with three words


@functools.lru_cache(maxsize=None)
def _batch(name):
    from sapr_amd import full_cov
    c = fc.case(name)
    return (full_cov.FullCovBatch(c["feats"], c["lengths"], c["utt_model"], len(c["utts"]), c["S"]),
            full_cov.pack_models(c["params"]))


@functools.lru_cache(maxsize=None)
def _gpu_estep(name):
    """(loglik, stats, post, path) as host arrays, one launch over all of the case's models."""
    batch, pack = _batch(name)
    return tuple(t.cpu().numpy() for t in batch.estep(pack, want_stats=True, want_post=True, want_path=True))


def _model(prm, ct, **kw):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    m = GaussianHMM(n_components=prm[2].shape[0], covariance_type=ct, init_params="", **kw)
    m.startprob_, m.transmat_, m.means_ = (np.array(a) for a in prm[:3])
    m.covars_ = fc.start_covars(prm, ct)
    return m


def _word_data(c, w=0):
    utts = [x for x in c["utts"][w]]
    return np.concatenate(utts, axis=0), [x.shape[0] for x in utts]


@pytest.mark.parametrize("name", NAMES)
def test_estep_matches_reference(name):
    from sapr_amd import full_cov
    c = fc.case(name)
    S, D = c["S"], c["D"]
    ref_stats, ref_utts = fc.reference_estep(name)
    loglik, stats, post, path = _gpu_estep(name)
    want = np.array([r["loglik"] for r in ref_utts])
    fin = np.isfinite(want)
    print("loglik max rel err", np.max(np.abs(loglik[fin] - want[fin]) / np.abs(want[fin])))
    np.testing.assert_allclose(loglik, want, rtol=1e-11)
    gamma = np.concatenate([r["gamma"] for r in ref_utts], axis=0)
    assert post.shape == gamma.shape == (c["feats"].shape[0], S)
    print("post max abs err", np.max(np.abs(post - gamma)))
    np.testing.assert_allclose(post, gamma, rtol=1e-9, atol=1e-12)
    assert path.dtype == np.int32 and np.array_equal(path, np.argmax(post, axis=1))
    for w, rs in enumerate(ref_stats):
        st = full_cov.split_stats(stats[w], S, D)
        assert st["nobs"] == rs["nobs"]
        np.testing.assert_allclose(st["logprob"], rs["logprob"], rtol=1e-11)
        for k in ("start", "trans", "post", "obs"):
            np.testing.assert_allclose(st[k], rs[k], rtol=1e-9, atol=1e-12, err_msg=k)
        for s in range(S):
            got, exp = st["obs*obs.T"][s], rs["oo"][s]
            print("oo", w, s, "norm-wise err", np.max(np.abs(got - exp)) / np.max(np.abs(exp)))
            assert np.max(np.abs(got - exp)) <= 1e-9 * np.max(np.abs(exp)), (w, s)
            assert np.array_equal(got, got.T), (w, s)
    if name == "d5_s3_dense":
        # the utterance without frames scores -inf and adds nothing (nobs counted above)
        last = len(c["utts"][0]) - 1      # word 0 carries them, after its own utterances
        assert c["lengths"][last] == 0 and c["lengths"][last - 1] == 1
        assert loglik[last] == -np.inf and np.isfinite(loglik[last - 1])
        # the same models at 4 kernel states: the padding state gives exact zeros, the rest the same bits
        wide = full_cov.FullCovBatch(c["feats"], c["lengths"], c["utt_model"], len(c["utts"]), 4)
        l4, s4, p4, _ = (t.cpu().numpy() for t in wide.estep(full_cov.pack_models(c["params"], 4), True, True, True))
        assert np.array_equal(l4, loglik) and np.array_equal(p4[:, :3], post) and np.all(p4[:, 3] == 0)
        for w in range(len(c["utts"])):
            whole, own = full_cov.split_stats(s4[w], 4, D), full_cov.split_stats(s4[w], 4, D, 3)
            mine = full_cov.split_stats(stats[w], S, D)
            for k in ("start", "trans", "post", "obs", "obs*obs.T"):
                assert np.array_equal(own[k], mine[k]), k
                assert np.all(whole[k][3:] == 0), k
            assert np.all(whole["trans"][:, 3] == 0)


@pytest.mark.parametrize("name", NAMES)
def test_viterbi_matches_reference(name):
    c = fc.case(name)
    want = fc.reference_viterbi(name)
    assert min(g for _, _, g in want) > 1e-9      # (the condition of tests/test_fullcov_cpu.py on the inputs)
    batch, pack = _batch(name)
    logprob, path = (t.cpu().numpy() for t in batch.viterbi(pack))
    np.testing.assert_allclose(logprob, [r[0] for r in want], rtol=1e-11)
    assert path.dtype == np.int32 and path.shape == (c["feats"].shape[0],)
    assert np.array_equal(path, np.concatenate([r[1] for r in want]))


def test_map_path_and_posteriors():
    """``want_post`` / ``want_path`` in all four combinations: the same bits."""
    name = "d5_s3_dense"
    batch, pack = _batch(name)
    loglik, stats, post, path = _gpu_estep(name)
    for want_post in (False, True):
        for want_path in (False, True):
            ll, s, p, q = batch.estep(pack, True, want_post, want_path)
            assert np.array_equal(ll.cpu().numpy(), loglik) and np.array_equal(s.cpu().numpy(), stats)
            assert (p is None) == (not want_post) and (q is None) == (not want_path)
            if want_post:
                assert np.array_equal(p.cpu().numpy(), post)
            if want_path:
                assert np.array_equal(q.cpu().numpy(), path)
            l2 = batch.estep(pack, False, want_post, want_path)[0]
            assert np.array_equal(l2.cpu().numpy(), loglik)


@pytest.mark.parametrize("name", MULTI)
def test_launch_independence(name):
    from sapr_amd import full_cov
    c = fc.case(name)
    S = c["S"]
    off = np.concatenate([[0], np.cumsum(c["lengths"])])
    loglik, stats, post, path = _gpu_estep(name)
    batch, pack = _batch(name)
    again = tuple(t.cpu().numpy() for t in batch.estep(pack, want_stats=True, want_post=True, want_path=True))
    for a, b in zip((loglik, stats, post, path), again):
        assert np.array_equal(a, b, equal_nan=True)
    vit = tuple(t.cpu().numpy() for t in batch.viterbi(pack))
    for w, (utts, prm) in enumerate(zip(c["utts"], c["params"])):
        sel = np.nonzero(c["utt_model"] == w)[0]
        one = full_cov.FullCovBatch(np.concatenate(utts, axis=0), c["lengths"][sel], np.zeros(sel.size, np.int64), 1, S)
        l1, s1, p1, q1 = (t.cpu().numpy() for t in one.estep(full_cov.pack_models([prm]), True, True, True))
        rows = slice(off[sel[0]], off[sel[-1] + 1])
        assert np.array_equal(l1, loglik[sel]) and np.array_equal(s1[0], stats[w], equal_nan=True)
        assert np.array_equal(p1, post[rows]) and np.array_equal(q1, path[rows])
        v1 = tuple(t.cpu().numpy() for t in one.viterbi(full_cov.pack_models([prm])))
        assert np.array_equal(v1[0], vit[0][sel]) and np.array_equal(v1[1], vit[1][rows])


def test_tied_equals_full_with_equal_matrices():
    from sapr_amd import full_cov
    c = fc.case("d13_s10_bidiag")
    prm = c["params"][0]            # (the case starts every state from one matrix)
    assert all(np.array_equal(cv, prm[3][0]) for cv in prm[3])
    X, lengths = _word_data(c)
    tied, full = _model(prm, "tied"), _model(prm, "full")
    assert tied._covars_.shape == (13, 13) and full._covars_.shape == (10, 13, 13)
    assert np.array_equal(full_cov.pack_models([tied._full_params()], name="tied"),
                          full_cov.pack_models([full._full_params()]))
    (lt, pt), (lf, pf) = tied.score_samples(X, lengths), full.score_samples(X, lengths)
    assert lt == lf and np.array_equal(pt, pf)
    assert tied.score(X, lengths) == full.score(X, lengths)
    (vt, st), (vf, sf) = tied.decode(X, lengths), full.decode(X, lengths)
    assert vt == vf and np.array_equal(st, sf)


def _check_trained(models, want):
    for m, (prm, hist, cvs) in zip(models, want):
        np.testing.assert_allclose(list(m.monitor_.history), hist, rtol=1e-9)
        np.testing.assert_allclose(m.startprob_, prm[0], rtol=0, atol=1e-7)
        np.testing.assert_allclose(m.transmat_, prm[1], rtol=0, atol=1e-7)
        np.testing.assert_allclose(m.means_, prm[2], rtol=1e-7)
        got = m.covars_
        assert got.shape == cvs[-1].shape
        for s in range(got.shape[0]):
            print("covariance", s, "norm-wise err", np.max(np.abs(got[s] - cvs[-1][s])) / np.max(np.abs(cvs[-1][s])))
            assert np.max(np.abs(got[s] - cvs[-1][s])) <= 1e-7 * np.max(np.abs(cvs[-1][s])), s
            assert np.array_equal(got[s], got[s].T), s


@pytest.mark.parametrize("ct", ["full", "tied"])
@pytest.mark.parametrize("name", NAMES)
def test_em_three_iterations(name, ct):
    from sapr_amd.hmmlearn_hmm import fit_models
    c = fc.case(name)
    models = [_model(prm, ct, n_iter=fc.EM_ITERS, tol=0) for prm in c["params"]]
    fit_models(models, [_word_data(c, w) for w in range(len(c["utts"]))])
    _check_trained(models, fc.reference_em(name, ct))


def test_spherical_runs_on_the_diag_kernels():
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    name = "d13_s10_bidiag"
    c = fc.case(name)
    prm = c["params"][0]
    X, lengths = _word_data(c)
    m = _model(prm, "spherical", n_iter=fc.EM_ITERS, tol=0)
    assert m._covars_.shape == (10,)
    d = GaussianHMM(n_components=10, covariance_type="diag", init_params="")
    d.startprob_, d.transmat_, d.means_ = m.startprob_, m.transmat_, m.means_
    d.covars_ = np.broadcast_to(m._covars_[:, None], (10, 13))
    assert m.score(X, lengths) == d.score(X, lengths)
    for alg in ("viterbi", "map"):
        (a, p), (b, q) = m.decode(X, lengths, algorithm=alg), d.decode(X, lengths, algorithm=alg)
        assert a == b and np.array_equal(p, q)
    (a, p), (b, q) = m.score_samples(X, lengths), d.score_samples(X, lengths)
    assert a == b and np.array_equal(p, q)
    m.fit(X, lengths)
    assert m._covars_.shape == (10,)
    _check_trained([m], fc.reference_em(name, "spherical")[:1])


@functools.lru_cache(maxsize=None)
def _scratch_fit(ct):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    X, lengths = _word_data(fc.case("d13_s10_bidiag"))
    return GaussianHMM(n_components=4, covariance_type=ct, random_state=0).fit(X, lengths)


def test_public_api_full():
    name = "d13_s10_bidiag"
    c = fc.case(name)
    n0 = len(c["utts"][0])
    X, lengths = _word_data(c)
    n = X.shape[0]
    _, ref_utts = fc.reference_estep(name)
    loglik, _, post, path = _gpu_estep(name)
    m = _model(c["params"][0], "full")
    np.testing.assert_allclose(m.score(X, lengths), sum(r["loglik"] for r in ref_utts[:n0]), rtol=1e-11)
    lp, pr = m.score_samples(X, lengths)
    assert isinstance(lp, float) and pr.dtype == np.float64 and np.array_equal(pr, post[:n])
    assert lp == loglik[:n0].sum() == m.score(X, lengths)
    assert np.array_equal(m.predict_proba(X, lengths), pr)
    mlp, mstates = m.decode(X, lengths, algorithm="map")
    assert mstates.dtype == np.int64 and np.array_equal(mstates, path[:n])
    assert mlp == pytest.approx(pr.max(axis=1).sum(), rel=1e-12)
    vlp, states = m.decode(X, lengths)
    want = fc.reference_viterbi(name)[:n0]
    np.testing.assert_allclose(vlp, sum(r[0] for r in want), rtol=1e-11)
    assert states.dtype == np.int64 and np.array_equal(states, np.concatenate([r[1] for r in want]))
    assert np.array_equal(m.predict(X, lengths), states)
    one = m.score(c["utts"][0][0])
    assert one == loglik[0]


@pytest.mark.parametrize("ct", ref.COVARIANCE_TYPES)
def test_fit_from_scratch(ct):
    X, lengths = _word_data(fc.case("d13_s10_bidiag"))
    m = _scratch_fit(ct)
    hist = list(m.monitor_.history)
    print(ct, "history", hist)
    assert 2 <= len(hist) <= 10 and np.all(np.isfinite(hist))
    assert all(b >= a - 1e-6 * abs(a) for a, b in zip(hist, hist[1:])), hist
    shape = {"diag": (4, 13), "spherical": (4,), "tied": (13, 13), "full": (4, 13, 13)}[ct]
    assert m._covars_.shape == shape and m.covars_.shape == (4, 13, 13) and m.means_.shape == (4, 13)
    for cv in m.covars_:
        assert np.array_equal(cv, cv.T) and np.linalg.eigvalsh(cv)[0] > 0
    np.testing.assert_allclose(m.transmat_.sum(axis=1), 1.0, atol=1e-12)
    assert np.isfinite(m.score(X, lengths))


def test_errors():
    from sapr_amd import _lib, full_cov
    from sapr_amd.trellis import DiagModelPack
    lib = _lib.load()
    for S, D in ((19, 13), (10, 40)):
        rc = lib.sapr_full_estep(None, None, None, None, None, 1, 10, 1, D, 10, None, 1, S, None, 0, None, None, None,
                                 None, None)
        assert rc == -2 and b"full-covariance" in lib.sapr_last_error()     # SAPR_ERR_UNSUPPORTED
        rc = lib.sapr_full_viterbi(None, None, None, None, 1, 10, 1, D, 10, None, 1, S, None, 0, None, None, None)
        assert rc == -2
        with pytest.raises(_lib.SaprHipError):
            full_cov.pack_layout(S, D)
    batch, pack = _batch("d5_s3_dense")
    real = batch.ws_bytes
    batch.ws_bytes = real - 8
    try:
        with pytest.raises(_lib.SaprHipError, match=f"workspace too small: {real - 8} < {real}"):
            batch.estep(pack)
        with pytest.raises(_lib.SaprHipError, match=f"workspace too small: {real - 8} < {real}"):
            batch.viterbi(pack)
    finally:
        batch.ws_bytes = real
    c = fc.case("d5_s3_dense")
    for ct in ("full", "tied"):
        with pytest.raises(ValueError, match=ct):
            DiagModelPack.from_models([_model(c["params"][0], ct)])
    n = ctypes.c_size_t(0)
    assert lib.sapr_full_workspace_bytes(batch.total_frames, batch.layout.n_tiles, 3, 5, ctypes.byref(n)) == 0
    assert n.value == real

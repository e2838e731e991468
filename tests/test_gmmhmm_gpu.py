"""GMMHMM on the GPU (csrc/gmm_hmm.hip through sapr_amd/gmm_hmm.py) against the numpy restatement
tests/_gmmhmm_ref.py on multi-modal synthetic words (tests/_gmmhmm_cases.py: shapes, seeds and the reference results,
computed once per case).

Tolerances: loglik rtol 1e-11 (the project's pin for forward scores); statistics, posteriors and their row sums rtol
1e-9 / atol 1e-9 (the pin of tests/test_state_posteriors_gpu.py); a component's statistics are compared wherever the
reference's post_mix is >= 1e-6, below that only |post_mix_gpu - post_mix_ref| <= 1e-9.  Trained parameters after three
EM iterations: history rtol 1e-9, weights atol 1e-7, means and covariances rtol 1e-7, components whose
reference occupancy fell below 1e-6 in any iteration left out (at most one in ten)."""
import functools

import numpy as np
import pytest

from tests import _gmmhmm_cases as gc
from tests._synth import VOCAB, synth_utterance, word_prototypes

pytestmark = pytest.mark.gpu

NAMES = list(gc.CASES)


@functools.lru_cache(maxsize=None)
def _batch(name):
    from sapr_amd import gmm_hmm as gh
    c = gc.case(name)
    W = len(c["utts"])
    return gh.GmmBatch(c["feats"], c["lengths"], c["utt_model"], W, c["S"], c["M"]), gh.pack_models(c["params"])


@functools.lru_cache(maxsize=None)
def _gpu_estep(name):
    """(loglik, stats, post, path) as host arrays, one launch over all of the case's models."""
    batch, pack = _batch(name)
    return tuple(t.cpu().numpy() for t in batch.estep(pack, want_stats=True, want_post=True, want_path=True))


@pytest.mark.parametrize("name", NAMES)
def test_estep_fixed_parameters(name):
    from sapr_amd import gmm_hmm as gh
    c = gc.case(name)
    S, M, D = c["S"], c["M"], c["D"]
    ref_stats, ref_utts = gc.reference_estep(name)
    loglik, stats, post, path = _gpu_estep(name)
    np.testing.assert_allclose(loglik, [r["loglik"] for r in ref_utts], rtol=1e-11)
    gamma = np.concatenate([r["gamma"] for r in ref_utts], axis=0)
    assert post.shape == gamma.shape == (c["feats"].shape[0], S)
    np.testing.assert_allclose(post, gamma, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=1e-9, atol=1e-9)
    assert path.dtype == np.int32 and np.array_equal(path, np.argmax(post, axis=1))   # the MAP path
    for w, rs in enumerate(ref_stats):
        st = gh.split_stats(stats[w], S, M, D)
        assert st["nobs"] == rs["nobs"]
        np.testing.assert_allclose(st["logprob"], rs["logprob"], rtol=1e-11)
        for k in ("start", "trans", "post"):
            np.testing.assert_allclose(st[k], rs[k], rtol=1e-9, atol=1e-9, err_msg=k)
        seen = rs["post_mix"] >= 1e-6
        np.testing.assert_allclose(st["post_mix"][~seen], rs["post_mix"][~seen], rtol=0, atol=1e-9)
        np.testing.assert_allclose(st["post_mix"][seen], rs["post_mix"][seen], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(st["obs"][seen], rs["obs"][seen], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(st["obs**2"][seen], rs["obs2"][seen], rtol=1e-9, atol=1e-9)
    if name == "d5_s3_m3_dense":   # the utterance without frames scores -inf and adds nothing (nobs counted above)
        last = len(c["utts"][0]) - 1      # word 0 carries them, after its own utterances
        assert c["lengths"][last] == 0 and c["lengths"][last - 1] == 1
        assert loglik[last] == -np.inf and np.isfinite(loglik[last - 1])


@pytest.mark.parametrize("name", NAMES)
def test_viterbi(name):
    c = gc.case(name)
    ref = gc.reference_viterbi(name)
    # a condition on the INPUTS: every arg-max the reference took, on every utterance, is decided by far more than
    # the rounding error of the scores
    assert min(g for _, _, g in ref) > 1e-9
    batch, pack = _batch(name)
    logprob, path = (t.cpu().numpy() for t in batch.viterbi(pack))
    np.testing.assert_allclose(logprob, [r[0] for r in ref], rtol=1e-11)
    assert path.dtype == np.int32 and path.shape == (c["feats"].shape[0],)
    assert np.array_equal(path, np.concatenate([r[1] for r in ref]))


def test_m1_matches_the_existing_gpu_estep():
    """One component of weight 1 against sapr_estep_diag and GaussianHMM.score on the same batch."""
    import torch
    from sapr_amd import _lib, gmm_hmm as gh
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    from sapr_amd.trellis import DiagModelPack, EStep, FeatureBatch
    c = gc.case("d13_s10_m2_bidiag")
    S, D, W = c["S"], c["D"], len(c["utts"])
    prm = [(sp, A, np.ones((S, 1)), mu[:, :1], cv[:, :1]) for sp, A, _, mu, cv in c["params"]]
    batch = gh.GmmBatch(c["feats"], c["lengths"], c["utt_model"], W, S, 1)
    loglik, stats, _, _ = (None if t is None else t.cpu().numpy() for t in batch.estep(gh.pack_models(prm)))
    dev = _lib.require_gpu()
    fb = FeatureBatch.from_packed(torch.from_numpy(c["feats"]).to(dev), c["lengths"])
    old = EStep(fb, c["utt_model"], W, S)
    pack = DiagModelPack.from_params(np.stack([p[0] for p in prm]), np.stack([p[1] for p in prm]),
                                     np.stack([p[3][:, 0] for p in prm]), np.stack([p[4][:, 0] for p in prm]),
                                     device=dev, exact_only=True)
    old_stats = old.run(pack).cpu().numpy()
    np.testing.assert_allclose(loglik, old.loglik.cpu().numpy(), rtol=1e-11)
    for w in range(W):
        a, b = gh.split_stats(stats[w], S, 1, D), old.split(old_stats[w])
        assert a["nobs"] == b["nobs"]
        np.testing.assert_allclose(a["logprob"], b["logprob"], rtol=1e-11)
        for k in ("start", "trans", "post"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-9, err_msg=k)
        np.testing.assert_allclose(a["post_mix"][:, 0], b["post"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(a["obs"][:, 0], b["obs"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(a["obs**2"][:, 0], b["obs**2"], rtol=1e-9, atol=1e-9)
    g = GaussianHMM(n_components=S, init_params="")
    g.startprob_, g.transmat_, g.means_, g.covars_ = prm[0][0], prm[0][1], prm[0][3][:, 0], prm[0][4][:, 0]
    n0 = len(c["utts"][0])
    X0, len0 = np.concatenate(c["utts"][0], axis=0), c["lengths"][:n0]
    np.testing.assert_allclose(loglik[:n0].sum(), g.score(X0, len0), rtol=1e-11)
    m = gh.GMMHMM(n_components=S, n_mix=1, init_params="")
    m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_ = prm[0]
    np.testing.assert_allclose(m.score(X0, len0), g.score(X0, len0), rtol=1e-11)


@pytest.mark.parametrize("name", ["d13_s10_m2_bidiag", "d5_s3_m3_dense"])
def test_launch_independence(name):
    from sapr_amd import gmm_hmm as gh
    c = gc.case(name)
    S, M = c["S"], c["M"]
    off = np.concatenate([[0], np.cumsum(c["lengths"])])
    loglik, stats, post, path = _gpu_estep(name)
    # two runs: bit-equal
    batch, pack = _batch(name)
    again = tuple(t.cpu().numpy() for t in batch.estep(pack, want_stats=True, want_post=True, want_path=True))
    for a, b in zip((loglik, stats, post, path), again):
        assert np.array_equal(a, b, equal_nan=True)
    vit = tuple(t.cpu().numpy() for t in batch.viterbi(pack))
    # one launch over 3 models against 3 single-model launches: bit-equal
    for w, (utts, prm) in enumerate(zip(c["utts"], c["params"])):
        sel = np.nonzero(c["utt_model"] == w)[0]
        one = gh.GmmBatch(np.concatenate(utts, axis=0), c["lengths"][sel], np.zeros(sel.size, np.int64), 1, S, M)
        l1, s1, p1, q1 = (t.cpu().numpy() for t in one.estep(gh.pack_models([prm]), True, True, True))
        rows = slice(off[sel[0]], off[sel[-1] + 1])
        assert np.array_equal(l1, loglik[sel]) and np.array_equal(s1[0], stats[w], equal_nan=True)
        assert np.array_equal(p1, post[rows]) and np.array_equal(q1, path[rows])
        v1 = tuple(t.cpu().numpy() for t in one.viterbi(gh.pack_models([prm])))
        assert np.array_equal(v1[0], vit[0][sel]) and np.array_equal(v1[1], vit[1][rows])
    # permuted utterance order: every utterance's outputs bit-equal
    perm = np.random.default_rng(5).permutation(c["lengths"].size)
    flat = [x for lst in c["utts"] for x in lst]
    pb = gh.GmmBatch(np.concatenate([flat[i] for i in perm], axis=0), c["lengths"][perm], c["utt_model"][perm],
                     len(c["utts"]), S, M)
    l2, _, p2, q2 = (None if t is None else t.cpu().numpy() for t in pb.estep(pack, False, True, True))
    v2 = tuple(t.cpu().numpy() for t in pb.viterbi(pack))
    off2 = np.concatenate([[0], np.cumsum(c["lengths"][perm])])
    for k, u in enumerate(perm):
        a, b = slice(off2[k], off2[k + 1]), slice(off[u], off[u + 1])
        assert l2[k] == loglik[u] and np.array_equal(p2[a], post[b]) and np.array_equal(q2[a], path[b])
        assert v2[0][k] == vit[0][u] and np.array_equal(v2[1][a], vit[1][b])


@pytest.mark.parametrize("name", NAMES)
def test_fit_gmm_models_from_fixed_parameters(name):
    from sapr_amd import gmm_hmm as gh
    c = gc.case(name)
    S, M = c["S"], c["M"]
    ref = gc.reference_em(name, 3)
    models = []
    for prm in c["params"]:
        m = gh.GMMHMM(n_components=S, n_mix=M, init_params="", n_iter=3, tol=-np.inf)
        m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_ = (np.array(a) for a in prm)
        models.append(m)
    gh.fit_gmm_models(models, [(np.concatenate(u, axis=0), [x.shape[0] for x in u]) for u in c["utts"]])
    left_out = total = 0
    for m, (prm, hist, occ) in zip(models, ref):
        np.testing.assert_allclose(list(m.monitor_.history), hist, rtol=1e-9)
        keep = np.min(np.stack(occ), axis=0) >= 1e-6
        left_out += int((~keep).sum())
        total += keep.size
        np.testing.assert_allclose(m.startprob_, prm[0], rtol=0, atol=1e-7)
        np.testing.assert_allclose(m.transmat_, prm[1], rtol=0, atol=1e-7)
        np.testing.assert_allclose(m.weights_, prm[2], rtol=0, atol=1e-7)
        np.testing.assert_allclose(m.means_[keep], prm[3][keep], rtol=1e-7)
        np.testing.assert_allclose(m.covars_[keep], prm[4][keep], rtol=1e-7)
    assert left_out * 10 <= total, (left_out, total)


@functools.lru_cache(maxsize=None)
def _scratch_data():
    rng = np.random.default_rng(21)
    protos = [word_prototypes(VOCAB[:1], 13, seed=5), word_prototypes(VOCAB[:1], 13, seed=6)]
    utts = [np.ascontiguousarray(synth_utterance(rng, protos[k % 2][VOCAB[0]], int(rng.integers(40, 90))).T)
            for k in range(12)]
    return np.concatenate(utts, axis=0), [u.shape[0] for u in utts]


def test_fit_from_scratch():
    from sapr_amd import GMMHMM
    X, lengths = _scratch_data()
    m = GMMHMM(n_components=4, n_mix=2, random_state=0).fit(X, lengths)
    hist = list(m.monitor_.history)
    assert 2 <= len(hist) <= 10 and np.all(np.isfinite(hist))
    assert all(b >= a - 1e-6 * abs(a) for a, b in zip(hist, hist[1:])), hist
    assert m.means_.shape == (4, 2, 13) and m.covars_.shape == (4, 2, 13) and m.weights_.shape == (4, 2)
    np.testing.assert_allclose(m.weights_.sum(axis=1), 1.0, atol=1e-12)
    np.testing.assert_allclose(m.transmat_.sum(axis=1), 1.0, atol=1e-12)
    assert np.all(m.covars_ >= 1e-3) and np.isfinite(m.score(X, lengths))
    m2 = GMMHMM(n_components=4, n_mix=2, random_state=0).fit(X, lengths)
    assert list(m2.monitor_.history) == hist
    for k in ("startprob_", "transmat_", "weights_", "means_", "covars_"):
        assert np.array_equal(getattr(m, k), getattr(m2, k)), k
    with pytest.raises(ValueError, match="n_mix"):     # 5 frames in 4 clusters: some label group holds one frame
        GMMHMM(n_components=4, n_mix=2, random_state=0).fit(X[:5], [5])
    with pytest.raises(NotImplementedError):
        GMMHMM(n_components=4, n_mix=2, covariance_type="full")
    with pytest.raises(ValueError, match="n_mix"):
        from sapr_amd import fit_gmm_models
        fit_gmm_models([GMMHMM(2, 1), GMMHMM(2, 2)], [(X, lengths), (X, lengths)])


def test_api_shapes_and_dtypes():
    from sapr_amd import GMMHMM
    c = gc.case("d5_s3_m3_dense")
    prm = c["params"][0]
    m = GMMHMM(n_components=3, n_mix=3, init_params="")
    m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_ = prm
    a, b = c["utts"][0][0], c["utts"][0][1]
    X, lengths = np.concatenate([a, b], axis=0), [a.shape[0], b.shape[0]]
    n = X.shape[0]
    lp, post = m.score_samples(X, lengths)
    assert isinstance(lp, float) and post.shape == (n, 3) and post.dtype == np.float64
    np.testing.assert_allclose(post.sum(axis=1), 1.0, atol=1e-9)
    assert lp == pytest.approx(m.score(X, lengths), rel=1e-12)
    assert lp == pytest.approx(m.score(a) + m.score(b), rel=1e-12)
    assert np.array_equal(m.predict_proba(X, lengths), post)
    vlp, states = m.decode(X, lengths)
    assert isinstance(vlp, float) and states.shape == (n,) and states.dtype == np.int64 and vlp <= lp
    assert np.array_equal(m.predict(X, lengths), states)
    mlp, mstates = m.decode(X, lengths, algorithm="map")
    assert np.array_equal(mstates, np.argmax(post, axis=1)) and mlp == pytest.approx(post.max(axis=1).sum())
    assert states.min() >= 0 and states.max() < 3
    with pytest.raises(ValueError):
        m.decode(X, lengths, algorithm="beam")

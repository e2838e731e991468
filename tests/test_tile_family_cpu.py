"""What the mixture and the full-covariance families share on the host (``sapr_amd/tile_family.py``): the validation
of a packed batch and the common heads of a statistics row and of an operand block.  Host arrays only, no device."""
import numpy as np
import pytest


def test_packed_utterances_accepts_an_empty_utterance_and_needs_no_device():
    from sapr_amd.tile_family import packed_utterances
    x = np.arange(10, dtype=np.float32).reshape(5, 2)
    feats, lengths, offsets = packed_utterances(x, [3, 0, 2])
    assert isinstance(feats, np.ndarray) and feats.dtype == np.float32 and np.array_equal(feats, x)
    assert lengths.dtype == np.int64 and lengths.tolist() == [3, 0, 2]
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 3, 3, 5]
    # float32 values in a float64 array pass, as everywhere else
    assert packed_utterances(x.astype(np.float64), [5])[0].dtype == np.float32


def test_packed_utterances_refuses_what_the_batches_refused():
    from sapr_amd.tile_family import packed_utterances
    x = np.arange(10, dtype=np.float32).reshape(5, 2)
    with pytest.raises(ValueError, match="lengths must be >= 0"):
        packed_utterances(x, [6, -1])
    with pytest.raises(ValueError, match="feats rows do not match sum\\(lengths\\)"):
        packed_utterances(x, [3, 1])
    with pytest.raises(ValueError, match="do not round-trip through float32"):
        packed_utterances(x.astype(np.float64) + 1e-9, [3, 2])
    with pytest.raises(ValueError, match="feats must be a contiguous float32 \\[total_frames, D\\] tensor"):
        packed_utterances(np.arange(5, dtype=np.float32), [3, 2])


def test_the_two_split_stats_share_their_head():
    from sapr_amd import full_cov, gmm_hmm
    S, S_model, M, D = 3, 2, 2, 2
    head = 2 + S + S * S + S
    g = gmm_hmm.split_stats(np.arange(head + S * M * (2 * D + 1), dtype=np.float64), S, M, D, S_model)
    f = full_cov.split_stats(np.arange(head + S * D + S * D * D, dtype=np.float64), S, D, S_model)
    for key in ("nobs", "logprob", "start", "trans", "post"):
        assert np.array_equal(g[key], f[key]), key
    assert (g["nobs"], g["logprob"]) == (0.0, 1.0)
    assert g["start"].tolist() == [2.0, 3.0]
    assert g["trans"].tolist() == [[5.0, 6.0], [8.0, 9.0]]
    assert g["post"].tolist() == [14.0, 15.0]
    # what follows the head is the family's own
    assert g["post_mix"].tolist() == [[17.0, 18.0], [19.0, 20.0]] and f["obs"].tolist() == [[17.0, 18.0], [19.0, 20.0]]
    assert set(g) == {"nobs", "logprob", "start", "trans", "post", "post_mix", "obs", "obs**2"}
    assert set(f) == {"nobs", "logprob", "start", "trans", "post", "obs", "obs*obs.T"}


def test_the_two_pack_models_share_their_head():
    from sapr_amd import full_cov, gmm_hmm
    rng = np.random.default_rng(3)
    S, D, SP = 3, 2, 4
    startprob, transmat = np.array([0.5, 0.5, 0.0]), rng.dirichlet(np.ones(S), size=S)
    transmat[2] = [0.0, 0.0, 1.0]
    means = rng.normal(0, 1, (S, D))
    g = gmm_hmm.pack_models([(startprob, transmat, np.ones((S, 1)), means[:, None, :], np.ones((S, 1, D)))])
    f = full_cov.pack_models([(startprob, transmat, means, np.tile(np.eye(D), (S, 1, 1)))])
    assert gmm_hmm.pack_layout(S, 1, D)[0] == full_cov.pack_layout(S, D)[0] == SP
    n = SP + 2 * SP * SP
    assert np.array_equal(g[0, :n], f[0, :n])
    with np.errstate(divide="ignore"):
        assert np.array_equal(g[0, :S], np.log(startprob)) and np.isneginf(g[0, S:SP]).all()
        lt = np.full((SP, SP), -np.inf)
        lt[:S, :S] = np.log(transmat)
    assert np.array_equal(g[0, SP:SP + SP * SP].reshape(SP, SP), lt)
    assert np.array_equal(g[0, SP + SP * SP:n].reshape(SP, SP), lt.T)

"""GPU: sapr_kmeans_step against the float64 numpy reference (tests/_kmeans_ref.py) on every frame of the recipe, its
determinism and batch independence, ``kmeans()`` against the reference Lloyd, and ``GaussianHMM.fit`` from scratch
(hmmlearn's ``_init``: Dirichlet draws, k-means means, data covariance)."""
import numpy as np
import pytest

from tests import _kmeans_ref as ref

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _upload(groups):
    import torch
    D = groups[0].shape[1]
    packed = np.concatenate(groups, axis=0) if sum(g.shape[0] for g in groups) else np.zeros((0, D), np.float32)
    return torch.from_numpy(np.ascontiguousarray(packed, dtype=np.float32)).to(_dev()), [g.shape[0] for g in groups]


def _step(groups, centres, want_labels=True):
    from sapr_amd.kmeans import FrameTiles, kmeans_step
    feats, lengths = _upload(groups)
    tiles = FrameTiles.build(lengths, _dev())
    out = kmeans_step(feats, tiles, centres, want_labels=want_labels)
    if want_labels:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def _check_against_reference(groups, centres, stats, labels, tag=""):
    """Every frame of every (group, restart): labels and counts equal, sum_x within 1e-11 of sum|x| per column, sqdev at
    rtol 1e-11 (the project's pin for float64 sums that differ by association).  First, from the reference alone: the
    nearest-centre decisions are clear of the last ulps (gap > 1e-8, exact ties only between identical centre rows)."""
    D = groups[0].shape[1]
    at = 0
    for g, X in enumerate(groups):
        n = X.shape[0]
        X64 = X.astype(np.float64)
        for r in range(centres.shape[1]):
            c = centres[g, r]
            want_labels, want, dist = ref.step(X64, c)
            finite = np.isfinite(dist).all(axis=1)
            gaps = ref.relative_gaps(dist[finite])
            print(f"{tag} g={g} r={r} n={n} min non-zero gap {gaps[gaps > 0].min() if (gaps > 0).any() else None}")
            assert not (gaps > 0).any() or gaps[gaps > 0].min() > 1e-8
            assert ref.zero_gaps_come_from_identical_centres(dist[finite], c)
            np.testing.assert_array_equal(labels[r, at:at + n], want_labels, err_msg=f"{tag} labels g={g} r={r}")
            got = stats[g, r]
            np.testing.assert_array_equal(got[:, 0], want[:, 0], err_msg=f"{tag} counts g={g} r={r}")
            for k in range(c.shape[0]):
                Xk = X64[want_labels == k]
                bound = 1e-11 * np.abs(Xk).sum(axis=0)
                err = np.abs(got[k, 1:1 + D] - want[k, 1:1 + D])
                ok = (err <= bound) | (np.isnan(got[k, 1:1 + D]) & np.isnan(want[k, 1:1 + D]))
                assert ok.all(), (tag, g, r, k, err.max(), bound.min())
            np.testing.assert_allclose(got[:, 1 + D:], want[:, 1 + D:], rtol=1e-11, atol=0, equal_nan=True,
                                       err_msg=f"{tag} sqdev g={g} r={r}")
        at += n


@pytest.mark.parametrize("D, K", ref.SHAPES)
def test_step_parity_on_every_frame(D, K):
    groups = list(ref.recipe_groups(D))
    centres = np.array(ref.recipe_init(D, K))
    stats, labels = _step(groups, centres)
    assert stats.shape == (len(groups), ref.R, K, 2 * D + 1) and labels.shape == (ref.R, sum(map(len, groups)))
    _check_against_reference(groups, centres, stats, labels, tag=f"D={D} K={K}")


@pytest.mark.parametrize("D", [13, 39, 26])
def test_step_edge_groups_and_centres(D):
    """Groups of 0, 1, 255, 256 and 257 frames cut from the recipe; a centre far from all data (count 0, zeros), two
    identical centres (the lower index takes all) and one NaN frame (label 0, NaN in the sums of cluster 0)."""
    pool = np.concatenate(ref.recipe_groups(D), axis=0)
    cuts = np.cumsum([0, 0, 1, 255, 256, 257])
    groups = [pool[a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]
    groups[4][100, 2] = np.nan
    K = 5
    centres = np.empty((5, 2, K, D))
    for g in range(5):
        src = groups[g] if groups[g].shape[0] >= 3 else pool[1000:1010]
        for r in range(2):
            rows = np.random.default_rng(77 * g + r).choice(src.shape[0], 3, replace=False)
            rows = rows[~np.isnan(src[rows]).any(axis=1)] if g == 4 else rows
            rows = np.resize(rows, 3)
            centres[g, r, 0], centres[g, r, 2] = src[rows[0]], src[rows[1]]
            centres[g, r, 1] = 1e6                       # far from all data
            centres[g, r, 3] = centres[g, r, 2]          # identical rows: index 2 takes all of them
            centres[g, r, 4] = src[rows[2]] + 0.25
    stats, labels = _step(groups, centres)
    _check_against_reference(groups, centres, stats, labels, tag=f"edge D={D}")
    assert not stats[0].any()                                           # a group without frames: exact zeros
    assert not stats[:, :, 1].any() and not stats[:, :, 3].any()        # far centre / shadowed twin: exact zeros
    assert labels[0, cuts[4] + 100] == 0 and np.isnan(stats[4, 0, 0, 1 + 2]) and np.isnan(stats[4, 0, 0, 1 + D + 2])
    assert np.isfinite(stats[4, 0, 0, 1]) and np.isfinite(stats[4, :, 2:]).all()
    assert stats[..., 0].sum(axis=2).tolist() == [[0, 0], [1, 1], [255, 255], [256, 256], [257, 257]]


def test_step_is_deterministic_and_batch_independent():
    D, K = 13, 10
    groups = list(ref.recipe_groups(D))
    centres = np.array(ref.recipe_init(D, K))
    a_stats, a_labels = _step(groups, centres)
    b_stats, b_labels = _step(groups, centres)
    assert a_stats.tobytes() == b_stats.tobytes() and a_labels.tobytes() == b_labels.tobytes()
    at = 0
    for g, X in enumerate(groups):                      # one launch over 11 groups == 11 single-group launches
        s, lb = _step([X], centres[g:g + 1])
        assert s.tobytes() == a_stats[g:g + 1].tobytes(), g
        assert np.array_equal(lb, a_labels[:, at:at + X.shape[0]]), g
        at += X.shape[0]
    # and without labels the statistics are the same
    assert _step(groups, centres, want_labels=False).tobytes() == a_stats.tobytes()


def test_step_past_2_31_workspace_elements():
    """The per-tile partial statistics of the LAST group sit past element 2^31 of the workspace (160 001 tiles x 16
    restarts x 32 clusters x 27 values = 2.2e9 doubles): that group's results must be the bits of a launch of its own,
    and the filler group in front of it must account for every one of its frames."""
    import torch
    from sapr_amd.kmeans import FrameTiles, kmeans_step
    D, K, R, n_fill = 13, 32, 16, 160000 * 256
    X = ref.recipe_groups(D)[0][:200]
    gen = torch.Generator(device=_dev()).manual_seed(3)
    feats = torch.empty((n_fill + X.shape[0], D), dtype=torch.float32, device=_dev())
    feats[:n_fill].normal_(0.0, 20.0, generator=gen)
    feats[:n_fill, 0] -= 300.0
    feats[n_fill:] = torch.from_numpy(X.copy()).to(_dev())
    rows = np.random.default_rng(8).choice(X.shape[0], (2, R, K))
    centres = X.astype(np.float64)[rows]                                # both groups start from rows of the small one
    tiles = FrameTiles.build([n_fill, X.shape[0]], _dev())
    assert (tiles.n_tiles - 1) * R * K * (2 * D + 1) > 2 ** 31
    stats, labels = kmeans_step(feats, tiles, centres, want_labels=True)
    alone_stats, alone_labels = kmeans_step(feats[n_fill:].contiguous(), FrameTiles.build([X.shape[0]], _dev()),
                                            centres[1:], want_labels=True)
    assert torch.equal(stats[1:], alone_stats) and torch.equal(labels[:, n_fill:], alone_labels)
    assert torch.equal(stats[0, :, :, 0].sum(dim=1), torch.full((R,), float(n_fill), dtype=torch.float64, device=_dev()))
    assert int(labels[:, :n_fill].min()) >= 0 and int(labels[:, :n_fill].max()) < K
    assert torch.isfinite(stats).all()


@pytest.mark.parametrize("D, K", ref.SHAPES)
def test_kmeans_against_reference_lloyd(D, K):
    from sapr_amd.kmeans import kmeans
    groups = list(ref.recipe_groups(D))
    feats, lengths = _upload(groups)
    centers, inertia, n_iter, best = kmeans(feats, lengths, K, init=np.array(ref.recipe_init(D, K)))
    runs = ref.recipe_lloyd(D, K)
    assert centers.shape == (len(groups), K, D) and inertia.shape == n_iter.shape == best.shape == (len(groups),)
    for g in range(len(groups)):
        ri = np.array([run["inertia"] for run in runs[g]])
        order = np.argsort(ri, kind="stable")
        margin = (ri[order[1]] - ri[order[0]]) / ri[order[1]] if ri[order[1]] > 0 else 0.0
        print(f"D={D} K={K} g={g} ref inertias {ri} margin {margin:.3e} got best {best[g]} n_iter {n_iter[g]}")
        if margin > 1e-9:
            assert best[g] == order[0], (g, ri, best[g])
            want = runs[g][order[0]]
            np.testing.assert_allclose(centers[g], want["centers"], rtol=1e-9, atol=0, err_msg=str(g))
        else:  # two restarts reach the same optimum: the centres as row-sorted sets
            assert abs(ri[best[g]] - ri[order[0]]) <= 1e-9 * ri[order[0]], (g, ri, best[g])
            want = runs[g][int(best[g])]
            srt = lambda c: c[np.lexsort(c.T[::-1])]
            np.testing.assert_allclose(srt(centers[g]), srt(runs[g][order[0]]["centers"]), rtol=1e-9, atol=0,
                                       err_msg=str(g))
        assert n_iter[g] == want["n_iter"], (g, n_iter[g], want["n_iter"])
        np.testing.assert_allclose(inertia[g], want["inertia"], rtol=1e-9, atol=0)


def test_kmeans_refuses_too_few_frames():
    from sapr_amd.kmeans import kmeans
    X = ref.recipe_groups(13)[0]
    feats, lengths = _upload([X[:9], X[9:200]])
    with pytest.raises(ValueError, match="at least 10 frames"):
        kmeans(feats, lengths, 10, n_init=1, seeds=[1, 2])
    feats, lengths = _upload([X[:1]])
    with pytest.raises(ValueError, match="at least 2 frames"):
        kmeans(feats, lengths, 1, n_init=1, seeds=[1])


def _word(g, D=13):
    return ref.recipe_groups(D)[g].copy(), list(ref.recipe_lengths(D)[g])


def test_fit_from_scratch_initialises_like_hmmlearn():
    """The test that fails without the feature: ``GaussianHMM(n_components=5).fit(X, lengths)`` raised AttributeError."""
    from sapr_amd.hmmlearn_hmm import GaussianHMM, kmeans_seed
    from sapr_amd.kmeans import kmeans
    X, lengths = _word(0)
    m = GaussianHMM(n_components=5, random_state=0, n_iter=0).fit(X, lengths)
    rs = np.random.RandomState(0)
    np.testing.assert_array_equal(m.startprob_, rs.dirichlet(np.full(5, 0.2)))
    np.testing.assert_array_equal(m.transmat_, rs.dirichlet(np.full(5, 0.2), size=5))
    seed = kmeans_seed(rs)
    feats, _ = _upload([X])
    centers, _, _, _ = kmeans(feats, [X.shape[0]], 5, n_init=10, seeds=[seed])
    np.testing.assert_array_equal(m.means_, centers[0])
    assert len({row.tobytes() for row in m.means_}) == 5
    want = np.var(X.astype(np.float64), axis=0, ddof=1) + m.min_covar
    np.testing.assert_allclose(m._covars_, np.tile(want, (5, 1)), rtol=1e-10, atol=0)
    assert m.covars_.shape == (5, 13, 13) and len(m.monitor_.history) == 0
    again = GaussianHMM(n_components=5, random_state=0, n_iter=0).fit(X, lengths)
    for a, b in ((m.startprob_, again.startprob_), (m.transmat_, again.transmat_), (m.means_, again.means_),
                 (m._covars_, again._covars_)):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    other = GaussianHMM(n_components=5, random_state=1, n_iter=0).fit(X, lengths)
    assert not np.array_equal(other.startprob_, m.startprob_)


def test_fit_from_scratch_trains():
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    X, lengths = _word(0)
    m = GaussianHMM(n_components=5, random_state=0, n_iter=5).fit(X, lengths)
    h = np.asarray(list(m.monitor_.history))
    print("history", h)
    assert 2 <= len(h) <= 5 and np.isfinite(h).all()
    assert (np.diff(h) >= -1e-9 * np.abs(h[:-1])).all()
    assert np.isfinite(m.score(X, lengths))


def test_partial_initialisation_keeps_preset_topology():
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    from sapr_amd.trellis import is_bidiagonal
    X, lengths = _word(3)
    S = 5
    sp = np.zeros(S)
    sp[0] = 1.0
    A = np.zeros((S, S))
    for i in range(S - 1):
        A[i, i], A[i, i + 1] = 0.8, 0.2
    A[S - 1, S - 1] = 1.0

    def make(n_iter):
        m = GaussianHMM(n_components=S, random_state=4, n_iter=n_iter, init_params="mc")
        m.startprob_, m.transmat_ = sp.copy(), A.copy()
        return m.fit(X, lengths)
    m0 = make(0)
    np.testing.assert_array_equal(m0.startprob_, sp)
    np.testing.assert_array_equal(m0.transmat_, A)
    assert m0.means_.shape == (S, 13) and m0._covars_.shape == (S, 13)
    m3 = make(3)
    assert is_bidiagonal(m3.transmat_) and m3.startprob_[0] == 1.0 and not np.array_equal(m3.transmat_, A)
    assert np.isfinite(np.asarray(list(m3.monitor_.history))).all()


def test_batched_training_equals_separate_fits():
    from sapr_amd.hmmlearn_hmm import GaussianHMM, fit_models
    G = len(ref.VOCAB)
    data = [_word(g) for g in range(G)]
    together = [GaussianHMM(n_components=5, random_state=g, n_iter=2) for g in range(G)]
    fit_models(together, data)
    for g in range(G):
        alone = GaussianHMM(n_components=5, random_state=g, n_iter=2).fit(*data[g])
        for name in ("startprob_", "transmat_", "means_", "_covars_"):
            assert np.asarray(getattr(alone, name)).tobytes() == np.asarray(getattr(together[g], name)).tobytes(), \
                (g, name)
        assert list(alone.monitor_.history) == list(together[g].monitor_.history), g


def test_torch_op_equals_ctypes_path():
    import torch
    import sapr_amd.torch_ops  # noqa: F401  (registers the ops)
    from sapr_amd.kmeans import FrameTiles, kmeans_step
    D, K = 39, 18
    groups = list(ref.recipe_groups(D))
    feats, lengths = _upload(groups)
    tiles = FrameTiles.build(lengths, _dev())
    centres = torch.from_numpy(np.array(ref.recipe_init(D, K))).to(_dev())
    stats, labels = kmeans_step(feats, tiles, centres, want_labels=True)
    o_stats, o_labels = torch.ops.sapr.kmeans_step(feats, tiles.tile_begin, tiles.tile_len, tiles.tile_group,
                                                   tiles.group_tile_off, centres, True)
    assert torch.equal(stats, o_stats) and torch.equal(labels, o_labels)
    o_stats, o_labels = torch.ops.sapr.kmeans_step(feats, tiles.tile_begin, tiles.tile_len, tiles.tile_group,
                                                   tiles.group_tile_off, centres, False)
    assert torch.equal(stats, o_stats) and o_labels.numel() == 0

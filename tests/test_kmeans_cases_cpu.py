"""CPU: every case of tests/_kmeans_cases.py is what it claims to be, from the float64 numpy reference alone — the
conditions tests/test_kmeans_cases_gpu.py rests on (nearest-centre gaps above 1e-8, exact ties only between bit-identical
centre rows, the intended labels of the skewed tiles, centre shifts clear of the threshold, ``emptied``) — and the
restated seeding of tests/_kmeans_ref.py draws what ``sapr_amd.kmeans`` draws.  No compute call is made."""
import numpy as np
import pytest

from tests import _kmeans_cases as cases
from tests import _kmeans_ref as ref


def _step_is_clear(groups, centres, tag):
    """gap > 1e-8 and ties only between identical centre rows, on every (group, restart); -> the smallest gap."""
    low = np.inf
    for g, X in enumerate(groups):
        for r in range(centres.shape[1]):
            _, _, dist = ref.step(X.astype(np.float64), centres[g, r])
            finite = np.isfinite(dist).all(axis=1)
            gaps = ref.relative_gaps(dist[finite])
            if (gaps > 0).any():
                low = min(low, gaps[gaps > 0].min())
            assert ref.zero_gaps_come_from_identical_centres(dist[finite], centres[g, r]), (tag, g, r)
    print(f"{tag}: smallest non-zero gap {low:.3e}")
    assert low > 1e-8, (tag, low)
    return low


@pytest.mark.parametrize("D, K", cases.SHAPES)
def test_shapes_have_no_near_ties(D, K):
    groups = ref.recipe_groups(D)
    assert all(X.shape == (X.shape[0], D) and X.shape[0] >= 64 for X in groups)
    _step_is_clear(groups, ref.recipe_init(D, K), f"shape-{D}-{K}")


def test_shapes_cover_the_branches_they_name():
    passes = {(D, K): -(-K * (39 if D > 13 else 13) // 256) for D, K in cases.SHAPES}
    assert passes[(39, 32)] == 5 and passes[(39, 26)] == 4 and passes[(39, 20)] == 4 and passes[(13, 20)] == 2
    assert 39 * 20 % 256 != 0 and {K for _, K in cases.SHAPES} >= {17, 31, 32}
    assert {D for D, _ in cases.SHAPES} >= {1, 14}                     # padded to 13 and to 39 columns


@pytest.mark.parametrize("D, K, R", cases.RESTART_CASES)
def test_restart_cases(D, K, R):
    centres = cases.restart_init(D, K, R)
    assert centres.shape[1] == R
    if R == 10:
        assert np.array_equal(centres[:, 7], centres[:, 0]) and not np.array_equal(centres[:, 6], centres[:, 0])
    _step_is_clear(ref.recipe_groups(D), centres, f"restarts-{D}-{K}-{R}")


@pytest.mark.parametrize("D", [13, 39])
def test_skewed_tiles_get_their_intended_labels(D):
    groups, centres, intended, names = cases.skewed(D)
    K = cases.SKEW_K
    assert [X.shape[0] for X in groups] == [256, 512] * 4 and centres.shape == (8, 2, K, D)
    for X, c, lab, name in zip(groups, centres, intended, names):
        for r in range(2):
            got, st, _ = ref.step(X.astype(np.float64), c[r])
            assert np.array_equal(got, lab if r == 0 else K - 1 - lab), (name, r)
        tile = lab[-256:]                                              # the tile that carries the pattern
        counts = np.bincount(tile, minlength=K).tolist()
        if name.startswith("all_first"):
            assert counts == [256, 0, 0, 0, 0]
        elif name.startswith("all_last"):
            assert counts == [0, 0, 0, 0, 256]
        elif name.startswith("one_wave"):
            assert np.nonzero(tile == 2)[0].tolist() == list(range(64, 128)) and counts == [48, 48, 64, 48, 48]
        else:
            assert counts == [3, 253, 0, 0, 0] and np.nonzero(tile == 0)[0].tolist() == list(cases.THREE)
    _step_is_clear(groups, centres, f"skewed-{D}")


@pytest.mark.parametrize("D", [13, 39])
def test_nan_centre_labels(D):
    groups, centres, expected = cases.nan_centre(D)
    for g, X in enumerate(groups):
        for r, want in enumerate(expected):
            labels, st, _ = ref.step(X.astype(np.float64), centres[g, r])
            if want is None:
                assert len(set(labels.tolist())) > 1 and np.isfinite(st).all()
                continue
            assert (labels == want).all() and st[want, 0] == X.shape[0]
            assert np.isfinite(st[want, 1:1 + D]).all()                # the frames are finite: so are their sums
            assert np.isnan(st[want, 1 + D:]).sum() == 1               # the one column of the centre that holds NaN
            assert not np.delete(st, want, axis=0).any()
    _step_is_clear(groups, centres[:, 2:], f"nan_centre-{D}")


@pytest.mark.parametrize("D", [13, 39])
@pytest.mark.filterwarnings("ignore:invalid value encountered")     # inf - inf in numpy's own sums
def test_inf_frames_labels(D):
    groups, centres, rows = cases.inf_frames(D)
    assert [len(r) for r in rows] == [2, 2, 0] and rows[0][0] // 256 != rows[0][1] // 256
    for g, X in enumerate(groups):
        for r in range(centres.shape[1]):
            labels, st, dist = ref.step(X.astype(np.float64), centres[g, r])
            for i in rows[g]:
                assert labels[i] == 0 and np.isposinf(dist[i]).all()
            assert np.isfinite(st[1:]).all()
            assert np.isfinite(st[0]).all() == (len(rows[g]) == 0)
    _, st, _ = ref.step(groups[0].astype(np.float64), centres[0, 0])
    assert np.isposinf(st[0, 1 + 3]) and np.isneginf(st[0, 1 + 7]) and np.isposinf(st[0, 1 + D + 3])
    _, st, _ = ref.step(groups[1].astype(np.float64), centres[1, 0])
    assert np.isnan(st[0, 1 + 2]) and np.isposinf(st[0, 1 + D + 2])
    _step_is_clear(groups, centres, f"inf_frames-{D}")


def test_table_case_layout():
    from sapr_amd.kmeans import FrameTiles
    groups, centres = cases.tables()
    t = FrameTiles.build([X.shape[0] for X in groups])
    assert t.n_tiles == 4 and t.tile_len.tolist() == [256, 44, 256, 100] and t.tile_group.tolist() == [0, 0, 1, 2]
    assert t.group_tile_off.tolist() == [0, 2, 3, 4]
    total, G = t.total_frames, t.G
    for name, table, idx, value in cases.TABLE_EDITS:
        v = value(total, int(t.tile_len[cases.TABLE_TILE]), t.n_tiles, G)
        good = getattr(t, table)[G if idx == "G" else idx]
        assert v != int(good), name
    # each edit is one the guards name: outside 0..256, outside [0, total - len], outside 0..G-1, outside 0..n_tiles
    values = {name: value(total, 44, 4, G) for name, _, _, value in cases.TABLE_EDITS}
    assert values == dict(len_257=257, len_minus_1=-1, begin_one_past=total - 43, begin_minus_1=-1, group_G=3,
                          group_minus_1=-1, off_last_past=9, off_first_negative=-3)
    _step_is_clear(groups, centres, "tables")


@pytest.mark.parametrize("D", [13, 39])
def test_many_tiles_case(D):
    groups, centres = cases.many_tiles(D)
    lengths = [X.shape[0] for X in groups]
    assert [-(-n // 256) for n in lengths] == list(cases.MANY_TILES[D])
    assert all(1 <= n % 256 <= 255 for n in lengths)                   # a partial last tile everywhere
    if D == 13:
        assert cases.MANY_TILES[D][0] == 1 and sum(lengths) < 88000   # no interesting group starts at tile 0
    assert all(abs(X[:, 0].mean() + 300) < 30 for X in groups)        # the offset that makes the order visible
    _step_is_clear(groups, centres, f"many_tiles-{D}")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restated_seeding_is_the_products(seed):
    """``_kmeans_ref.kmeans_pp`` returns ``sapr_amd.kmeans.kmeans_pp_seeds``' indices, also through the uniform branch,
    and ``seed_centres`` subsamples exactly when the group holds more than 256 K rows."""
    from sapr_amd.kmeans import kmeans_pp_seeds
    X = np.random.default_rng(100 + seed).normal(size=(300, 6))
    X[40:90] = X[7]
    for K in (1, 2, 9):
        a = kmeans_pp_seeds(X, K, np.random.default_rng(seed))
        assert np.array_equal(a, ref.kmeans_pp(X, K, np.random.default_rng(seed)))
    Z = np.ones((9, 3))
    assert np.array_equal(kmeans_pp_seeds(Z, 4, np.random.default_rng(seed)), ref.kmeans_pp(Z, 4, np.random.default_rng(seed)))
    # the subsample: drawn first, sorted, shared by the restarts; the restarts' draws follow on the same stream
    big = np.random.default_rng(seed).normal(size=(600, 3)).astype(np.float32)
    c, pick = ref.seed_centres(big, 2, 3, seed)
    rng = np.random.default_rng(seed)
    want_pick = np.sort(rng.choice(600, 512, replace=False))
    assert np.array_equal(pick, want_pick) and pick.size == 512
    for r in range(3):
        assert np.array_equal(c[r], big[want_pick][kmeans_pp_seeds(big[want_pick], 2, rng)].astype(np.float64))
    c, pick = ref.seed_centres(big[:512], 2, 1, seed)                  # exactly 256 K rows: no draw for the subsample
    assert np.array_equal(pick, np.arange(512))
    assert np.array_equal(c[0], big[kmeans_pp_seeds(big[:512], 2, np.random.default_rng(seed))].astype(np.float64))


@pytest.mark.parametrize("D, K", sorted(cases.SEEDED))
def test_seeded_cases(D, K):
    groups, seeds, want = cases.seeded(D, K)
    for g, (X, run) in enumerate(zip(groups, want)):
        assert (run["pick"].size < X.shape[0]) == (X.shape[0] > 256 * K)
        assert run["init"].shape == (cases.SEEDED_N_INIT, K, D)
        print(f"seeded-{D}-{K} g={g} n={X.shape[0]} margin {run['margin']:.3e} tied {run['tied']} "
              f"min_gap {min(r['min_gap'] for r in run['runs']):.3e} n_iter {[r['n_iter'] for r in run['runs']]}")
        for r in run["runs"]:
            assert r["min_gap"] > 1e-8
            assert all(s == 0.0 or s >= 2 * r["threshold"] for s in r["shifts"]), (r["shifts"], r["threshold"])
    if (D, K) == (13, 2):
        assert want[0]["pick"].size == 512 and want[1]["pick"].size == 300


def test_emptied_case():
    X, init, run = cases.emptied()
    assert run["emptied"] and run["min_gap"] > 1e-8
    assert all(s == 0.0 or s >= 2 * run["threshold"] for s in run["shifts"])
    print(f"emptied: n_iter {run['n_iter']} min_gap {run['min_gap']:.3e}")
    # the far centre takes no frame in any step: the reference leaves it where it started (up to its own centring)
    np.testing.assert_allclose(run["centers"][cases.EMPTIED_FAR], init[0, 0, cases.EMPTIED_FAR], rtol=1e-12)
    labels, st, _ = ref.step(X.astype(np.float64), run["centers"])
    assert st[cases.EMPTIED_FAR, 0] == 0 and (np.delete(st[:, 0], cases.EMPTIED_FAR) > 0).all()

"""CPU: the k-means entry points (sapr_kmeans_workspace_bytes, sapr_kmeans_step) are exported, bound and report
argument errors without a device; the tile tables, the k-means++ seeding and the initialisation rules of ``GaussianHMM``
are host logic; and the numpy reference the GPU tests compare against (tests/_kmeans_ref.py) is scikit-learn's Lloyd
wherever no cluster empties.  No compute call is made — there is no GPU in the build container."""
import ctypes
import logging

import numpy as np
import pytest

from sapr_amd import _lib
from tests import _kmeans_ref as ref

ERR_ARG, ERR_UNSUPPORTED = -1, -2
P = ctypes.c_void_p(256)      # dummy non-NULL pointer (never dereferenced on the paths exercised here)
BIG = 1 << 40


def _call(lib, feats=P, total=1000, tb=P, tl=P, tg=P, off=P, n_tiles=4, G=2, R=3, K=10, D=13, centres=P, ws=P,
          ws_bytes=BIG, stats=P, labels=P):
    return lib.sapr_kmeans_step(feats, total, tb, tl, tg, off, n_tiles, G, R, K, D, centres, ws, ws_bytes, stats,
                                labels, None)


def test_symbols_are_exported_and_bound():
    for name, arity in (("sapr_kmeans_workspace_bytes", 5), ("sapr_kmeans_step", 17)):
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == arity
        assert hasattr(_lib.load(), name)
    assert _lib.load().sapr_abi_version() == 2          # additive: the ABI version does not move


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    for bad in (dict(total=-1), dict(n_tiles=-1), dict(G=-1), dict(R=0), dict(K=0), dict(D=0), dict(G=0)):
        assert _call(lib, **bad) == ERR_ARG, bad
        assert b"bad sizes" in lib.sapr_last_error()
    for bad in (dict(D=12), dict(D=40), dict(K=33)):
        assert _call(lib, **bad) == ERR_UNSUPPORTED, bad
    for name in ("feats", "tb", "tl", "tg", "off", "centres", "ws", "stats"):
        assert _call(lib, **{name: None}) == ERR_ARG, name
        assert b"NULL" in lib.sapr_last_error()
    assert _call(lib, labels=None, ws_bytes=0) == ERR_ARG          # labels may be NULL: the next check speaks
    assert b"workspace too small" in lib.sapr_last_error()
    n = ctypes.c_size_t(0)
    assert lib.sapr_kmeans_workspace_bytes(4, 3, 10, 13, ctypes.byref(n)) == 0
    assert n.value == 4 * 3 * 10 * (2 * 13 + 1) * 8
    assert _call(lib, ws_bytes=n.value - 1) == ERR_ARG
    assert b"workspace too small" in lib.sapr_last_error()
    assert lib.sapr_kmeans_workspace_bytes(0, 1, 1, 39, ctypes.byref(n)) == 0 and n.value == 0
    for bad in ((-1, 1, 1, 13), (1, 0, 1, 13), (1, 1, 0, 13), (1, 1, 1, 0)):
        assert lib.sapr_kmeans_workspace_bytes(*bad, ctypes.byref(n)) == ERR_ARG
    assert lib.sapr_kmeans_workspace_bytes(1, 1, 1, 13, None) == ERR_ARG


def test_no_tiles_returns_without_touching_the_other_pointers():
    lib = _lib.load()
    # no group at all: nothing to fill, success with every pointer NULL
    assert lib.sapr_kmeans_step(None, 0, None, None, None, None, 0, 0, 1, 1, 13, None, None, 0, None, None, None) == 0
    # groups but no statistics array to zero-fill: refused; the sizes are still checked
    assert _call(lib, n_tiles=0, stats=None) == ERR_ARG
    assert _call(lib, n_tiles=0, K=0) == ERR_ARG
    assert _call(lib, n_tiles=0, D=7) == ERR_UNSUPPORTED


@pytest.mark.parametrize("lengths", [[0], [1], [255], [256], [257], [0, 1, 255, 256, 257, 0, 600], []])
def test_frame_tiles(lengths):
    from sapr_amd.kmeans import FrameTiles
    t = FrameTiles.build(lengths)
    beg, ln, grp, off = (x.numpy() for x in (t.tile_begin, t.tile_len, t.tile_group, t.group_tile_off))
    assert beg.dtype == np.int64 and ln.dtype == np.int32 and grp.dtype == np.int32 and off.dtype == np.int32
    assert t.G == len(lengths) and t.total_frames == sum(lengths) and t.n_tiles == len(beg) == off[-1]
    assert off[0] == 0 and len(off) == len(lengths) + 1
    assert (np.diff(grp) >= 0).all()                                   # sorted by group
    covered, at = [], 0
    for g, n in enumerate(lengths):
        tiles = np.arange(off[g], off[g + 1])
        assert len(tiles) == -(-n // 256) and (grp[tiles] == g).all()
        assert ((ln[tiles] >= 1) & (ln[tiles] <= 256)).all() and ln[tiles].sum() == n
        assert (ln[tiles[:-1]] == 256).all()                           # only the last tile is partial
        for i in tiles:
            covered += list(range(beg[i], beg[i] + ln[i]))
        at += n
    assert covered == list(range(sum(lengths)))                        # every frame once, in order
    with pytest.raises(ValueError):
        FrameTiles.build([3, -1])


def test_kmeans_pp_seeds():
    from sapr_amd.kmeans import kmeans_pp_seeds
    rng = np.random.default_rng(5)
    X = rng.normal(size=(200, 7))
    X[50:120] = X[3]                                                   # many duplicates of one row
    a = kmeans_pp_seeds(X, 12, np.random.default_rng(1))
    b = kmeans_pp_seeds(X, 12, np.random.default_rng(1))
    assert a.dtype == np.int64 and np.array_equal(a, b)                # reproducible
    assert len({X[i].tobytes() for i in a}) == 12                      # distinct rows, not just distinct indices
    assert not np.array_equal(a, kmeans_pp_seeds(X, 12, np.random.default_rng(2)))
    # exactly K distinct rows exist: all of them are found
    Y = np.repeat(np.arange(4.0)[:, None], 3, axis=1)[np.array([0, 0, 1, 1, 1, 2, 3, 3])]
    for s in range(5):
        got = kmeans_pp_seeds(Y, 4, np.random.default_rng(s))
        assert sorted(Y[got][:, 0]) == [0.0, 1.0, 2.0, 3.0]
    # all-identical data: every D^2 is zero -> uniform picks among the rows not chosen yet
    Z = np.ones((9, 3))
    got = kmeans_pp_seeds(Z, 4, np.random.default_rng(0))
    assert len(set(got.tolist())) == 4 and got.min() >= 0 and got.max() < 9
    assert np.array_equal(got, kmeans_pp_seeds(Z, 4, np.random.default_rng(0)))
    assert kmeans_pp_seeds(Z, 1, np.random.default_rng(0)).shape == (1,)
    with pytest.raises(ValueError):
        kmeans_pp_seeds(Z[:3], 4, np.random.default_rng(0))


def test_too_few_frames_are_refused_before_any_device_work():
    from sapr_amd.kmeans import kmeans
    X = np.zeros((209, 13), dtype=np.float32)
    with pytest.raises(ValueError, match="at least 10 frames"):
        kmeans(X, [9, 200], 10, n_init=1, seeds=[1, 2])
    with pytest.raises(ValueError, match="at least 2 frames"):
        kmeans(X[:1], [1], 1, n_init=1, seeds=[1])
    with pytest.raises(ValueError, match="at least 2 frames"):
        kmeans(X[:5], [5, 0], 1)
    for bad_k in (0, 33):
        with pytest.raises(ValueError, match="n_clusters"):
            kmeans(X, [209], bad_k)


def test_needs_init_truth_table_and_warning(caplog):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    attrs = dict(GaussianHMM._INIT_ATTRS)
    assert attrs == {"s": "startprob_", "t": "transmat_", "m": "means_", "c": "covars_"}
    for code, name in attrs.items():
        for in_params in (True, False):
            for preset in (True, False):
                m = GaussianHMM(n_components=2, init_params=code if in_params else "")
                if preset:
                    setattr(m, name, {"startprob_": np.array([0.5, 0.5]), "transmat_": np.full((2, 2), 0.5),
                                      "means_": np.zeros((2, 3)), "covars_": np.ones((2, 3))}[name])
                caplog.clear()
                with caplog.at_level(logging.WARNING):
                    got = m._needs_init(code, name)
                assert got == (in_params or not preset), (code, in_params, preset)
                warned = any("will be overwritten" in r.getMessage() and name in r.getMessage()
                             for r in caplog.records)
                assert warned == (in_params and preset), (code, in_params, preset)
    # the default constructor initialises everything
    m = GaussianHMM(n_components=2)
    assert all(m._needs_init(c, n) for c, n in attrs.items())


def test_random_state_handling():
    from sapr_amd.hmmlearn_hmm import check_random_state, kmeans_seed
    assert check_random_state(None) is np.random.mtrand._rand
    a, b = check_random_state(7), check_random_state(np.int64(7))
    assert isinstance(a, np.random.RandomState) and a is not b
    assert a.randint(1 << 30) == b.randint(1 << 30) == np.random.RandomState(7).randint(1 << 30)
    rs = np.random.RandomState(3)
    assert check_random_state(rs) is rs
    for bad in ("x", 1.5, True, np.random.default_rng(0)):
        with pytest.raises(ValueError):
            check_random_state(bad)
    # the k-means seed is one draw from the stream, after whatever the s / t draws consumed
    r1, r2 = np.random.RandomState(0), np.random.RandomState(0)
    r1.dirichlet(np.full(5, 0.2))
    r1.dirichlet(np.full(5, 0.2), size=5)
    s1 = kmeans_seed(r1)
    assert 0 <= s1 < 2 ** 31 and s1 != kmeans_seed(r2)
    r3 = np.random.RandomState(0)
    r3.dirichlet(np.full(5, 0.2))
    r3.dirichlet(np.full(5, 0.2), size=5)
    assert kmeans_seed(r3) == s1


def test_reference_step_rules():
    """The reference's own step on a hand-made case: ties go to the lowest k, a NaN frame gets label 0, an empty
    cluster has zeros."""
    X = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 0.0], [np.nan, 1.0]])
    c = np.array([[0.0, 0.0], [2.0, 0.0], [50.0, 50.0]])
    labels, st, _ = ref.step(X, c)
    assert labels.tolist() == [0, 1, 0, 0]
    assert st[2].tolist() == [0.0] * 5 and st[1].tolist() == [1.0, 2.0, 0.0, 0.0, 0.0]
    assert st[0, 0] == 3 and np.isnan(st[0, 1]) and st[0, 2] == 1.0


@pytest.mark.parametrize("D, K", ref.SHAPES)
def test_reference_lloyd_is_sklearn_lloyd_where_no_cluster_empties(D, K):
    pytest.importorskip("sklearn")
    from sklearn.cluster import KMeans
    groups, init, runs = ref.recipe_groups(D), ref.recipe_init(D, K), ref.recipe_lloyd(D, K)
    compared = 0
    for g, X in enumerate(groups):
        assert 182 <= X.shape[0] <= 484
        for r in range(ref.R):
            run = runs[g][r]
            if run["emptied"]:
                continue
            km = KMeans(n_clusters=K, init=np.array(init[g, r]), n_init=1, algorithm="lloyd", tol=1e-4,
                        max_iter=300).fit(X.astype(np.float64))
            # rtol 1e-12, plus the absolute floor that two float64 summation orders of the same cluster can differ by:
            # a centre coordinate is the mean of n_k <= n centred values of magnitude <= A, whose sum in any order
            # is within (n - 1) eps sum|x_i| <= n^2 eps A of the exact one, i.e. the mean within n eps A — it decides
            # only for coordinates that land near zero (|c| ~ 1e-2 against A ~ 50)
            atol = X.shape[0] * np.finfo(np.float64).eps * np.abs(X.astype(np.float64) - X.mean(axis=0)).max()
            np.testing.assert_allclose(run["centers"], km.cluster_centers_, rtol=1e-12, atol=atol, err_msg=f"{g} {r}")
            assert run["n_iter"] == km.n_iter_, (g, r)
            compared += 1
    assert compared >= 18, compared


@pytest.mark.parametrize("D, K", ref.SHAPES)
def test_recipe_has_no_near_ties(D, K):
    """What the GPU parity tests rely on: nearest-centre decisions are clear of the last ulps, and no centre shift
    sits near the threshold."""
    for runs in ref.recipe_lloyd(D, K):
        for run in runs:
            assert run["min_gap"] > 1e-8
            thr = run["threshold"]
            assert all(s == 0.0 or s >= 2 * thr for s in run["shifts"]), (run["shifts"], thr)

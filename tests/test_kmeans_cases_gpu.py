"""GPU: sapr_kmeans_step against the float64 numpy reference on the cases of tests/_kmeans_cases.py — every accumulator
pass and scan width of the tile kernel, R = 1 and R = 10, skewed tiles, NaN centres and infinite frames, tables that
leave the batch, the reduce kernel over up to 130 tiles — and ``kmeans()`` with its own seeding and with a cluster that
stays empty.  The bar is tests/test_kmeans_gpu.py's ``_check_against_reference``, which also asserts, from the reference,
the gap and tie conditions each comparison rests on (tests/test_kmeans_cases_cpu.py asserts them without a device)."""
import ctypes as C

import numpy as np
import pytest

from tests import _kmeans_cases as cases
from tests import _kmeans_ref as ref
from tests.test_kmeans_gpu import _check_against_reference, _dev, _step, _upload

pytestmark = pytest.mark.gpu


def _report(groups, centres, stats, tag):
    """The largest deviations from the reference, relative to their bounds' scales (printed: DESIGN.md §6.0e)."""
    D = groups[0].shape[1]
    worst_sum = worst_sq = 0.0
    with np.errstate(all="ignore"):
        for g, X in enumerate(groups):
            X64 = X.astype(np.float64)
            for r in range(centres.shape[1]):
                labels, want, _ = ref.step(X64, centres[g, r])
                for k in range(centres.shape[2]):
                    scale = np.abs(X64[labels == k]).sum(axis=0)
                    e = np.abs(stats[g, r, k, 1:1 + D] - want[k, 1:1 + D]) / scale
                    worst_sum = max(worst_sum, np.nanmax(np.where(np.isfinite(e), e, 0.0), initial=0.0))
                    e = np.abs(stats[g, r, k, 1 + D:] - want[k, 1 + D:]) / np.abs(want[k, 1 + D:])
                    worst_sq = max(worst_sq, np.nanmax(np.where(np.isfinite(e), e, 0.0), initial=0.0))
    print(f"{tag}: largest sum_x deviation {worst_sum:.2e} of sum|x| (bound 1e-11), sqdev {worst_sq:.2e} relative "
          f"(bound 1e-11)")


@pytest.mark.parametrize("D, K", cases.SHAPES)
def test_step_parity_at_every_accumulator_pass_and_scan_width(D, K):
    groups = list(ref.recipe_groups(D))
    centres = np.array(ref.recipe_init(D, K))
    stats, labels = _step(groups, centres)
    assert stats.shape == (len(groups), ref.R, K, 2 * D + 1)
    _check_against_reference(groups, centres, stats, labels, tag=f"shape-{D}-{K}")
    _report(groups, centres, stats, f"shape-{D}-{K}")


@pytest.mark.parametrize("D, K, R", cases.RESTART_CASES)
def test_step_parity_at_one_and_ten_restarts(D, K, R):
    groups = list(ref.recipe_groups(D))
    centres = cases.restart_init(D, K, R)
    stats, labels = _step(groups, centres)
    assert stats.shape[1] == R and labels.shape[0] == R
    _check_against_reference(groups, centres, stats, labels, tag=f"restarts-{D}-{K}-{R}")
    if R == 10:   # the copy of restart 0 behind six other restarts: the same bits (the LDS copy is rewritten cleanly)
        assert stats[:, 7].tobytes() == stats[:, 0].tobytes() and labels[7].tobytes() == labels[0].tobytes()
        assert stats[:, 6].tobytes() != stats[:, 0].tobytes()


@pytest.mark.parametrize("D", [13, 39])
def test_step_parity_on_skewed_tiles(D):
    groups, centres, intended, names = cases.skewed(D)
    K = cases.SKEW_K
    for X, c, lab in zip(groups, centres, intended):                   # first, from the reference: the intended labels
        for r in range(2):
            assert np.array_equal(ref.step(X.astype(np.float64), c[r])[0], lab if r == 0 else K - 1 - lab)
    stats, labels = _step(list(groups), np.array(centres))
    _check_against_reference(list(groups), centres, stats, labels, tag=f"skewed-{D}")
    _report(groups, centres, stats, f"skewed-{D}")
    assert np.array_equal(labels[0], np.concatenate(intended))
    assert np.array_equal(labels[1], K - 1 - np.concatenate(intended))
    all_first = names.index("all_first-256")
    assert stats[all_first, 0, :, 0].tolist() == [256, 0, 0, 0, 0] and not stats[all_first, 0, 1:].any()
    assert stats[all_first, 1, :, 0].tolist() == [0, 0, 0, 0, 256] and not stats[all_first, 1, :4].any()
    three = names.index("three_253-256")
    assert stats[three, 0, :, 0].tolist() == [3, 253, 0, 0, 0] and stats[three, 1, :, 0].tolist() == [0, 0, 0, 253, 3]


@pytest.mark.parametrize("D", [13, 39])
def test_step_nan_centre_takes_every_frame(D):
    groups, centres, expected = cases.nan_centre(D)
    stats, labels = _step(list(groups), np.array(centres))
    _check_against_reference(list(groups), centres, stats, labels, tag=f"nan_centre-{D}")
    for r, want in enumerate(expected):
        if want is not None:
            assert (labels[r] == want).all()


@pytest.mark.parametrize("D", [13, 39])
def test_step_infinite_frames_go_to_cluster_0(D):
    """The reference defines the result.  Where it is not finite (cluster 0's sums in the columns that hold an infinity)
    the kernel's value must be the same infinity or NaN; every finite value meets the bar of
    ``_check_against_reference`` (whose ``|got - want| <= bound`` cannot compare inf with inf)."""
    groups, centres, rows = cases.inf_frames(D)
    stats, labels = _step(list(groups), np.array(centres))
    at = 0
    for g, X in enumerate(groups):
        n, X64 = X.shape[0], X.astype(np.float64)
        for r in range(centres.shape[1]):
            with np.errstate(invalid="ignore"):
                want_labels, want, dist = ref.step(X64, centres[g, r])
            finite = np.isfinite(dist).all(axis=1)
            assert (~finite).sum() == len(rows[g])
            gaps = ref.relative_gaps(dist[finite])
            assert gaps[gaps > 0].min() > 1e-8 and ref.zero_gaps_come_from_identical_centres(dist[finite], centres[g, r])
            np.testing.assert_array_equal(labels[r, at:at + n], want_labels)
            assert all(labels[r, at + i] == 0 for i in rows[g])
            got = stats[g, r]
            np.testing.assert_array_equal(got[:, 0], want[:, 0])
            odd = ~np.isfinite(want)
            assert not odd[1:].any() and odd[0].any() == bool(rows[g])
            np.testing.assert_array_equal(got[odd], want[odd])         # the same infinity, or NaN where the reference has
            assert np.isfinite(got[~odd]).all()
            for k in range(centres.shape[2]):
                ok = ~odd[k, 1:1 + D]
                Xk = X64[want_labels == k][:, ok]
                err = np.abs(got[k, 1:1 + D][ok] - want[k, 1:1 + D][ok])
                assert (err <= 1e-11 * np.abs(Xk).sum(axis=0)).all(), (g, r, k)
            ok = ~odd[:, 1 + D:]
            np.testing.assert_allclose(got[:, 1 + D:][ok], want[:, 1 + D:][ok], rtol=1e-11, atol=0)
        at += n


# ---- tables that leave the batch -------------------------------------------------------------------------------------
def _raw_step(feats, tables, G, R, K, D, centres):
    """``sapr_kmeans_step`` through the C interface on explicit tables -> (return code, stats, labels filled with -7)."""
    import torch
    from sapr_amd import _lib
    lib = _lib.load()
    tb, tl, tg, off = tables
    n_tiles, total = int(tb.numel()), int(feats.shape[0])
    nb = C.c_size_t(0)
    assert lib.sapr_kmeans_workspace_bytes(n_tiles, R, K, D, C.byref(nb)) == 0
    ws = torch.zeros(int(nb.value), dtype=torch.uint8, device=feats.device)
    stats = torch.full((G, R, K, 2 * D + 1), -5.0, dtype=torch.float64, device=feats.device)
    labels = torch.full((R, total), -7, dtype=torch.int32, device=feats.device)
    rc = lib.sapr_kmeans_step(_lib.ptr(feats), total, _lib.ptr(tb), _lib.ptr(tl), _lib.ptr(tg), _lib.ptr(off), n_tiles,
                              G, R, K, D, _lib.ptr(centres), _lib.ptr(ws), int(nb.value), _lib.ptr(stats),
                              _lib.ptr(labels), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, stats.cpu().numpy(), labels.cpu().numpy()


@pytest.fixture(scope="module")
def table_case():
    import torch
    from sapr_amd.kmeans import FrameTiles
    groups, centres = cases.tables()
    feats, lengths = _upload(list(groups))
    t = FrameTiles.build(lengths, _dev())
    dcentres = torch.from_numpy(np.array(centres)).to(_dev())
    G, R, K, D = t.G, cases.TABLE_R, cases.TABLE_K, cases.TABLE_D
    tabs = dict(tile_begin=t.tile_begin, tile_len=t.tile_len, tile_group=t.tile_group, group_tile_off=t.group_tile_off)
    order = ("tile_begin", "tile_len", "tile_group", "group_tile_off")
    rc, stats, labels = _raw_step(feats, [tabs[n] for n in order], G, R, K, D, dcentres)
    assert rc == 0
    _check_against_reference(list(groups), centres, stats, labels, tag="tables, unedited")
    # group 0 without the frames of tile 1: its first 256 frames as a group of their own
    first, _ = _step([groups[0][:256]], np.array(centres[:1]))
    return feats, t, tabs, order, dcentres, stats, labels, first


@pytest.mark.parametrize("edit", cases.TABLE_EDITS, ids=[e[0] for e in cases.TABLE_EDITS])
def test_step_serves_a_table_that_leaves_the_batch_as_empty(table_case, edit):
    """One entry of a valid four-tile layout is edited.  The call returns 0, the edited tile contributes exact zeros
    (group 0 is left with the bits of its first tile alone), every other group has the bits of the unedited call, and
    so have the labels of every other tile; the edited tile's label slots are unspecified.  An edited
    ``group_tile_off`` end is cut to the workspace's rows, which restores the true range."""
    feats, t, tabs, order, dcentres, base_stats, base_labels, first = table_case
    name, table, idx, value = edit
    tile = cases.TABLE_TILE
    edited = dict(tabs)
    edited[table] = tabs[table].clone()
    edited[table][t.G if idx == "G" else idx] = value(t.total_frames, int(t.tile_len[tile]), t.n_tiles, t.G)
    rc, stats, labels = _raw_step(feats, [edited[n] for n in order], t.G, cases.TABLE_R, cases.TABLE_K, cases.TABLE_D,
                                  dcentres)
    assert rc == 0
    if table == "group_tile_off":
        assert stats.tobytes() == base_stats.tobytes() and labels.tobytes() == base_labels.tobytes()
        return
    assert stats[1:].tobytes() == base_stats[1:].tobytes()
    assert stats[0].tobytes() == first[0].tobytes()
    assert stats[0, :, :, 0].sum(axis=1).tolist() == [256.0] * cases.TABLE_R
    lo, hi = 256, 300                                                  # the edited tile's frames
    assert np.array_equal(labels[:, :lo], base_labels[:, :lo]) and np.array_equal(labels[:, hi:], base_labels[:, hi:])


# ---- the reduce kernel over many tiles -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [13, 39])
def test_reduce_over_many_tiles(D):
    groups, centres = cases.many_tiles(D)
    groups, centres = list(groups), np.array(centres)
    stats, labels = _step(groups, centres)
    _check_against_reference(groups, centres, stats, labels, tag=f"many_tiles-{D}")
    _report(groups, centres, stats, f"many_tiles-{D}")
    # a second identical launch, and the long groups launched alone: the same bits
    again, again_labels = _step(groups, centres)
    assert again.tobytes() == stats.tobytes() and again_labels.tobytes() == labels.tobytes()
    off = np.concatenate([[0], np.cumsum([X.shape[0] for X in groups])])
    for g, tiles in enumerate(cases.MANY_TILES[D]):
        if tiles in (65, 130):
            alone, alone_labels = _step([groups[g]], centres[g:g + 1])
            assert alone.tobytes() == stats[g:g + 1].tobytes(), (D, tiles)
            assert np.array_equal(alone_labels, labels[:, off[g]:off[g + 1]]), (D, tiles)


# ---- kmeans() ----------------------------------------------------------------------------------------------------------
def check_kmeans_result(centers, inertia, n_iter, best, runs, tag=""):
    """The bar of tests/test_kmeans_gpu.py::test_kmeans_against_reference_lloyd for one group: the best restart equal
    where the reference's margin exceeds 1e-9 (else the centres as row-sorted sets), centres and inertia at rtol 1e-9,
    ``n_iter`` equal.  -> the largest relative centre deviation."""
    ri = np.array([run["inertia"] for run in runs])
    order = np.argsort(ri, kind="stable")
    margin = np.inf if len(ri) < 2 else (ri[order[1]] - ri[order[0]]) / ri[order[1]] if ri[order[1]] > 0 else 0.0
    print(f"{tag} ref inertias {ri} margin {margin:.3e} got best {best} n_iter {n_iter}")
    if margin > 1e-9:
        assert best == order[0], (tag, ri, best)
        want = runs[order[0]]
        got_c, want_c = centers, want["centers"]
    else:
        assert abs(ri[best] - ri[order[0]]) <= 1e-9 * ri[order[0]], (tag, ri, best)
        want = runs[int(best)]
        srt = lambda c: c[np.lexsort(c.T[::-1])]
        got_c, want_c = srt(centers), srt(runs[order[0]]["centers"])
    np.testing.assert_allclose(got_c, want_c, rtol=1e-9, atol=0, err_msg=tag)
    assert n_iter == want["n_iter"], (tag, n_iter, want["n_iter"])
    np.testing.assert_allclose(inertia, want["inertia"], rtol=1e-9, atol=0)
    return float(np.abs(got_c / want_c - 1).max())


@pytest.mark.parametrize("D, K", sorted(cases.SEEDED))
def test_kmeans_with_its_own_seeding(D, K):
    from sapr_amd.kmeans import kmeans
    groups, seeds, want = cases.seeded(D, K)
    feats, lengths = _upload(list(groups))
    centers, inertia, n_iter, best = kmeans(feats, lengths, K, n_init=cases.SEEDED_N_INIT, seeds=list(seeds))
    assert centers.shape == (len(groups), K, D)
    for g, run in enumerate(want):
        dev = check_kmeans_result(centers[g], inertia[g], n_iter[g], best[g], run["runs"], tag=f"seeded-{D}-{K} g={g}")
        print(f"seeded-{D}-{K} g={g}: largest centre deviation {dev:.2e} (bound 1e-9)")


def test_kmeans_keeps_the_centre_of_a_cluster_that_stays_empty():
    from sapr_amd.kmeans import kmeans
    X, init, run = cases.emptied()
    feats, lengths = _upload([X])
    centers, inertia, n_iter, best = kmeans(feats, lengths, cases.EMPTIED_K, init=np.array(init))
    far = cases.EMPTIED_FAR
    assert centers[0, far].tobytes() == init[0, 0, far].tobytes()     # unchanged to the bit
    keep = np.delete(np.arange(cases.EMPTIED_K), far)
    np.testing.assert_allclose(centers[0, keep], run["centers"][keep], rtol=1e-9, atol=0)
    assert n_iter[0] == run["n_iter"] and best[0] == 0
    np.testing.assert_allclose(inertia[0], run["inertia"], rtol=1e-9, atol=0)

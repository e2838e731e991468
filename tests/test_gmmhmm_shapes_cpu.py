"""The conditions tests/test_gmmhmm_shapes_gpu.py sets on its INPUTS, checked from the numpy reference alone
(tests/_gmmhmm_ref.py over the cases of tests/_gmmhmm_sweep.py); no GPU.  These are caps, not measurements: a generator
or seed change must keep them.

* the sweep pads to all 36 (SP, MP, DP) triples of the kernels, each at least twice;
* everything the reference returns for an utterance with frames is finite (no impossible utterance: both sides would
  give NaN statistics by design);
* every arg-max the reference's Viterbi took is decided by more than 1e-9 of the score (far above the rounding error
  of float64 scores compared at rtol 1e-11), so paths are comparable;
* the two best word scores of every utterance are more than 1e-4 apart while |score| stays below 1e6: rtol 1e-11
  moves a score by less than 1e-5 and cannot flip a word;
* at most one (state, component) cell in five over the sweep, and one in two in any single model, has a reference
  occupancy below 1e-6 (such a cell's observation sums are left out of the comparison).
"""
import numpy as np
import pytest

from tests import _gmmhmm_ref as ref
from tests import _gmmhmm_sweep as sw

VITERBI_GAP, WORD_GAP, SCORE_CAP = 1e-9, 1e-4, 1e6


def _all_finite(name):
    stats, utts = sw.reference_estep(name)
    for st in stats:
        for k, v in st.items():
            assert np.all(np.isfinite(v)), (name, k)
    for r, T in zip(utts, sw.case(name)["lengths"]):
        assert np.isfinite(r["loglik"]) == (T > 0), name
        assert np.all(np.isfinite(r["gamma"])), name


def _viterbi_gap(name):
    return min(g for _, _, g in sw.reference_viterbi(name))


def _check_word_scores(name):
    for mode in sw.MODES:
        sc = sw.reference_scores(name)[mode][0]
        live = sw.case(name)["lengths"] > 0
        assert np.all(np.isfinite(sc[live])) and np.all(sc[~live] == -np.inf), (name, mode)
        assert sw.word_gap(sc) > WORD_GAP, (name, mode, sw.word_gap(sc))
        assert np.abs(sc[live]).max() < SCORE_CAP, (name, mode)


def test_sweep_covers_every_padded_triple_twice():
    from sapr_amd import gmm_hmm as gh
    assert len(sw.SHAPES) == len(set(sw.SHAPES)) == 72
    count = {}
    for k, (S, M, D) in enumerate(sw.SHAPES):
        tri = gh.pack_layout(S, M, D)[:3]
        count[tri] = count.get(tri, 0) + 1
        c = sw.case(sw.SWEEP[k])
        assert (c["S"], c["M"], c["D"]) == (S, M, D) and len(c["utts"]) == 2
        tmin = max(S, 6)
        assert [x.shape[0] for x in c["utts"][0][5:]] == [1, 2, 0] and len(c["utts"][1]) == 5
        assert all(tmin <= x.shape[0] < tmin + 12 for lst in c["utts"] for x in lst[:5])
        assert c["feats"].dtype == np.float32 and c["feats"].shape == (int(c["lengths"].sum()), D)
        dense = bool(np.all(c["params"][0][1] > 0))
        assert dense == (k % 2 == 1) or S == 1      # alternates along the list (one state: the same matrix)
    assert sorted(count) == sorted((s, m, d) for s in sw.SPS for m in sw.MPS for d in sw.DPS)
    assert min(count.values()) >= 2, count


def test_sweep_inputs_meet_the_conditions():
    low = total = 0
    gap = np.inf
    for name in sw.SWEEP:
        _all_finite(name)
        gap = min(gap, _viterbi_gap(name))
        _check_word_scores(name)
        for st in sw.reference_estep(name)[0]:
            below = st["post_mix"] < 1e-6
            assert 2 * int(below.sum()) <= below.size, (name, int(below.sum()), below.size)
            low += int(below.sum())
            total += below.size
    assert gap > VITERBI_GAP, gap
    assert 5 * low <= total, (low, total)


@pytest.mark.parametrize("name", list(sw.RAGGED))
def test_ragged_inputs(name):
    c = sw.case(name)
    own = np.array(sorted((x.shape[0] for x in c["utts"][0]), reverse=True))
    assert tuple(own) == sw.RAGGED_LENGTHS
    run = np.cumsum(own)[:-1]          # the frames in front of every utterance but the first, longest first
    assert list(run) == [1024, 1280, 1472, 1600, 1665, 1729, 1792, 1794, 1795]
    assert int((run % 64 == 0).sum()) == 5 and int((run % 256 == 0).sum()) == 3
    assert not np.array_equal(c["order"], np.arange(c["order"].size))      # fed shuffled
    assert [len(lst) for lst in c["utts"]] == [len(own), 1, 0] and c["utts"][1][0].shape[0] == 1
    _all_finite(name)
    assert _viterbi_gap(name) > VITERBI_GAP
    _check_word_scores(name)
    st = sw.reference_estep(name)[0]
    assert not np.any(st[0]["post_mix"] < 1e-6)       # the long word sees every component
    assert st[2]["nobs"] == 0 and all(not np.any(v) for v in st[2].values())


def test_tiles_inputs():
    c = sw.case("tiles")
    n0, n1 = (len(lst) for lst in c["utts"])
    assert n0 <= 256 and 2049 <= n1 <= 2304           # one tile, then nine: 8 + 1 rows, 32 + 4 partial rows
    assert all(3 <= x.shape[0] < 8 for lst in c["utts"] for x in lst)
    _all_finite("tiles")
    assert _viterbi_gap("tiles") > VITERBI_GAP
    for st in sw.reference_estep("tiles")[0]:
        assert not np.any(st["post_mix"] < 1e-6)


@pytest.mark.parametrize("name", sw.DEGENERATE)
def test_degenerate_inputs(name):
    c = sw.case(name)
    S = c["S"]
    _all_finite(name)
    assert _viterbi_gap(name) > VITERBI_GAP
    _check_word_scores(name)
    stats, utts = sw.reference_estep(name)
    for (sp, A, wt, mu, cv), st in zip(c["params"], stats):
        np.testing.assert_allclose([sp.sum(), *A.sum(axis=1), *wt.sum(axis=1)], 1.0, atol=1e-12)
        if name == "zero_weight":
            assert np.all(wt[:, 1] == 0) and np.all(wt[:, [0, 2]] > 0)
            assert not np.any(st["post_mix"][:, 1]) and not np.any(st["obs"][:, 1]) and not np.any(st["obs2"][:, 1])
        elif name == "unreachable":
            assert sp[1] == sp[2] == 0 and not np.any(A[:, 2]) and np.all(A[:, [0, 1, 3, 4]] > 0)
            assert st["post"][2] == 0 and st["start"][2] == 0 and not np.any(st["post_mix"][2])
            assert not np.any(st["trans"][2]) and not np.any(st["trans"][:, 2])
        elif name == "skips":
            assert np.array_equal(A > 0, np.triu(np.ones((S, S), bool)) & ~np.triu(np.ones((S, S), bool), 3))
            np.testing.assert_allclose(A[0, :3], (0.7, 0.2, 0.1))
        elif name == "absorbing":
            assert np.array_equal(A[3], np.eye(S)[3]) and np.all(A[:3] > 0)
    if name == "unreachable":
        assert all(not np.any(r["gamma"][:, 2]) for r in utts)
    if name == "outlier":
        # the frame's log components spread over more than exp_unit's clamp of 800 within every state, and its
        # responsibilities are one-hot in float64
        w, u, t = sw.OUTLIER_AT
        x, plain = c["utts"][w][u], sw.case(sw.SWEEP[sw.SHAPES.index((4, 4, 13))])["utts"][w][u]
        assert np.array_equal(np.nonzero(np.any(x != plain, axis=1))[0], [t])
        assert np.all(x[t] - plain[t] > 0.99 * sw.OUTLIER_SHIFT)
        lc = ref.log_components(x.astype(np.float64), *c["params"][w][2:])[t]
        assert np.all(lc.max(axis=1) - lc.min(axis=1) > 800.0)
        resp = np.exp(lc - ref._lse(lc, axis=1)[:, None])
        assert np.all(np.sort(resp, axis=1)[:, -2] < 1e-30) and np.all(resp.max(axis=1) == 1.0)

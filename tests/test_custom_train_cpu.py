"""The conditions test_custom_train_gpu.py relies on, asserted from the references alone (no GPU): the E-step batches
hold every class of c0 in the numbers the kernel's branches need, every tile / block / chunk / run / loop threshold of
custom_estep.hip and custom_update.hip is straddled by the case sizes, the zero-occupancy state and the empty model exist, a plain
float64 evaluation stays under every pin (so the pin decides), and the long-double references agree with the oracle."""
import numpy as np
import pytest

from oracle import custom_hmm_oracle as co
from tests import _custom_train_ref as R


# ------------------------------------------------------------------------------------------------------------ part 5
@pytest.mark.parametrize("ns, D", R.FAST_SHAPES)
def test_estep_batches_hold_every_class(ns, D):
    b = R.estep_batch(ns, D)
    S = ns + 2
    assert b.n_utts > 3 * 64                                   # more than three workgroups of 64
    assert set(b.utt_model[:4]) == {0, 1} and b.W == 2
    c0 = b.c0
    smooth, band, zero = (b.kinds == k for k in ("smooth", "band", "zero"))
    assert smooth.sum() >= 40 and band.sum() >= 70 and zero.sum() >= 40
    assert band.sum() > 64                                     # the redo list spans more than one workgroup
    assert np.sum(smooth & (c0 < -677.0)) >= 3                 # inside (-679, -677), on either side of -678
    assert np.sum(band & (c0 > -679.0)) >= 3
    assert np.sum(band & (c0 < -749.0)) >= 3                   # within 1 of the lower end, on either side
    assert np.sum(zero & (c0 > -751.0)) >= 3
    assert b.count("unreachable") >= 4                         # c0 = -inf: T < S - 1
    assert all(u.T < S - 1 for u in b.utts if u.kind == "unreachable")
    assert {0, 1, 2} <= set(int(t) for t in b.lens) and b.count("empty") == 1
    bad = [u for u in b.utts if u.kind == "nan"]
    assert len(bad) == 2 and any(np.isnan(u.x).any() for u in bad) and any(np.isinf(u.x).any() for u in bad)
    assert np.isfinite(b.x[np.repeat(~np.isin(b.kinds, ["nan"]), b.lens)]).all()
    # a model in which one state is always left at once
    assert any(np.any(np.diagonal(A)[1:-1] == 0) for A in b.A) and not all(np.any(np.diagonal(A)[1:-1] == 0) for A in b.A)
    # every workgroup of 64 meets every class (the utterances are shuffled)
    for g in range(0, b.n_utts - 63, 64):
        assert {"smooth", "band", "zero"} <= set(b.kinds[g:g + 64])
    # the band's frames whose denormal terms leave no usable comparison with the oracle: at most one in four
    assert b.band_frame_share_outside_oracle() <= 0.25
    assert sum(u.xi_in_oracle for u in b.utts if u.kind == "band") >= 50
    # densities above 1: the forward scale grows with the length
    assert np.median([u.sc for u in b.utts if u.kind in ("smooth", "band", "zero")]) > 300


@pytest.mark.parametrize("which", ["smooth", "band"])
def test_estep_single_class_batches(which):
    b = R.estep_batch(8, 13, which)
    assert b.n_utts > 2 * 64 and np.all(b.kinds == which)      # redo_count = 0 / = n_utts, over more than one workgroup
    if which == "band":
        assert b.band_frame_share_outside_oracle() <= 0.25


def test_xi_totals_restate_the_oracle_bit_for_bit():
    b = R.estep_batch(8, 13)
    seen = set()
    for u in b.utts:
        if u.T < 2 or u.kind in seen:
            continue
        seen.add(u.kind)
        s, xi = R.xi_totals(u.al, u.be, u.E, b.A[u.w])
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(xi, co.xi(u.al, u.be, u.E, b.A[u.w]))
            g, x, ll = co.e_step(u.x, b.A[u.w], b.means[u.w], b.covs[u.w])
        np.testing.assert_array_equal(g, u.gamma)
        np.testing.assert_array_equal(x.sum(axis=0), u.xi_sum)
        if u.kind == "zero":
            assert not s.any() and not u.xi_sum.any()          # every term underflows: no transition counts
        if u.kind == "band":
            assert 0 < s[0] < 2.0 ** -1022 * 64                # denormal (or nearly) totals
    assert {"smooth", "band", "zero", "unreachable", "nan"} <= seen


@pytest.mark.parametrize("S, D", R.GENERIC_SHAPES)
def test_generic_batches(S, D):
    for dense in (False, True):
        b = R.generic_batch(S, D, dense)
        assert b.n_utts > 64 and {0, 1, 2} <= set(int(t) for t in b.lens)
        finite = [u for u in b.utts if u.kind in ("smooth", "band", "zero")]
        assert len(finite) >= 40
        if dense and S > 3:
            assert max(u.sc for u in finite) > 100


# ------------------------------------------------------------------------------------------------------ parts 1 to 4
def test_fold_cases_straddle_every_threshold():
    rows, cols = R.FOLD_ROWS, R.FOLD_COLS
    assert 0 in rows and 1 in rows
    # 32 row lanes, four accumulators (128 rows per round of the unrolled loop) and its tail
    for edge in (32, 128):
        assert {edge - 1, edge, edge + 1} <= set(rows)
    assert {r % 128 for r in rows} >= {0, 1, 127} and any(r % 4 == 1 for r in rows)
    # eight columns per workgroup and the column tail
    assert {7, 8, 9} <= set(cols) and any(k % 8 for k in cols) and any(k % 8 == 0 for k in cols)
    # two-level branch: n_rows >= 8192 and fewer than 64 column blocks
    assert R.fold_branch(8191, 504) == "single" and R.fold_branch(8192, 504) == "two-level"
    assert R.fold_branch(8192, 512) == "single" and (504 + 7) // 8 == 63 and (512 + 7) // 8 == 64
    # runs of per = ceil(n / 128) rows: full, short and empty last runs
    shapes = set()
    for n in (r for r in rows if r >= R.FOLD_TWO_LEVEL_ROWS):
        per = -(-n // R.FOLD_RUNS)
        last = [max(0, min(n, (i + 1) * per) - i * per) for i in range(R.FOLD_RUNS)]
        shapes |= {"full" if last[-1] == per else ("empty" if last[-1] == 0 else "short")}
        shapes |= {"some-empty"} if last.count(0) > 1 else set()
    assert {"full", "short", "empty"} <= shapes
    # LDS-staged ordered fold (K <= 64) against the plain chain kernel (K > 64)
    assert 64 in cols and 65 in cols
    part1, _ = R.fold_case(8193, 1)                      # one contiguous column: still the chain, not numpy's pair-wise sum
    acc = 0.0
    for v in part1[:, 0]:
        acc += v
    assert R.fold_chain(part1)[0] == acc
    for n, K in ((33, 9), (8193, 13)):
        part, nan_row = R.fold_case(n, K)
        cancel, nan = R.fold_columns(n, K)
        assert np.isnan(part[:, nan]).sum() == 1 and np.isfinite(np.delete(part, nan, axis=1)).all()
        import math
        assert math.fsum(part[:, cancel]) == 0.0 and np.abs(part[:, cancel]).sum() > 0
        mags = np.abs(part[np.isfinite(part) & (part != 0)])
        assert mags.min() < 1e-5 and mags.max() > 1e3 and (part < 0).any() and (part > 0).any()
        ref, mag = R.fold_ref(part)
        chain = R.fold_chain(part)
        acc = np.zeros(K)
        for r in range(n):
            acc += part[r]
        np.testing.assert_array_equal(chain, acc)
        fin = np.arange(K) != nan
        assert np.all(np.abs(chain.astype(R.LD)[fin] - ref[fin]) <= n * R.U64 * mag[fin])


def test_mstep_cases_straddle_tiles_chunks_and_hold_the_edges():
    lane_n = sorted({n for n, _ in R.LANE_CASES})
    assert {255, 256, 257} <= set(lane_n) and 1 in lane_n and max(lane_n) > 2 * 256       # 1, 2 and 3 tiles of 256
    assert {-(-n // 256) for n in lane_n} >= {1, 2, 3}
    assert {S for _, S in R.LANE_CASES} >= {3, 20}                                         # check_dims' limits
    assert {D for _, _, D in R.GENERIC_D_CASES} >= {1, 39, 40}
    multi_n = sorted({n for n, _, _ in R.MULTI_CASES})
    assert {-(-n // 32) for n in multi_n} >= {2, 3, 4} and any(n % 32 == 0 for n in multi_n)  # 32-utterance chunks
    for args in ([(n, S, 13) for n, S in R.LANE_CASES] + list(R.GENERIC_D_CASES)
                 + [(n, 10, D, W) for n, D, W in R.MULTI_CASES]):
        c = R.mstep_case(*args)
        if c.n_utts >= 2:
            assert 0 in c.lens and 1 in c.lens
        if c.S > 3:
            assert not c.gamma[:, c.zero_state].any() and 1 <= c.zero_state <= c.S - 2
        assert not c.gamma[:, 0].any() and not c.gamma[:, -1].any()
        np.testing.assert_allclose(c.gamma.sum(axis=1), 1.0, atol=1e-12)
        assert 90 < c.x.mean() < 110 and 4 < c.x.std() < 6
        if c.W == 3:
            assert list(c.utt_model[:6]) == [0, 1, 2, 0, 1, 2]
        if c.W == 4:
            assert c.empty_model == 2 and 2 not in c.utt_model and {0, 1, 3} == set(c.utt_model)
        g = c.gamma_slots()
        assert c.slots % 64 == 0 and c.slots >= c.n_utts and np.isnan(g[:, :, c.n_utts:]).all()
        for u in (0, c.n_utts - 1):
            np.testing.assert_array_equal(g[:c.lens[u], :, u], c.gamma[c.offs[u]:c.offs[u + 1]])


def test_moments_and_flat_start_cases_straddle_blocks_and_loops():
    n = R.MOM_UTTS
    assert {15, 16, 17, 63, 64, 65} <= set(n)                                              # 16-utterance blocks, 4 per workgroup
    blocks = -(-max(n) // 16)
    assert blocks > 4096 and blocks % 4096 != 0 and max(n) % 16 != 0                # the loop runs, ends unevenly
    assert max(R.MOM_STATES) == 16 and min(R.MOM_STATES) == 3
    f = R.COV_MFMA_FRAMES
    assert {1, 2, 3, 4, 5} <= set(f)                                                       # 4-frame groups
    groups = [-(-x // 4) for x in f]
    assert any(g == 8192 for g in groups) and any(g == 8191 + 1 for g in groups)
    assert any(8192 < g <= 2 * 8192 for g in groups) and any(g > 2 * 8192 + 8192 for g in groups)  # second accumulator, then the loop
    assert any(g < 8192 and g % 4 for g in groups)                                         # idle wavefronts in the last workgroup
    c = R.COV_FALLBACK_FRAMES
    assert {4095, 4096, 4097} <= set(c) and max(-(-x // 4096) for x in c) >= 4            # 4096-frame chunks


# --------------------------------------------------------------------------------------- E_64 against the pins
def _e64_mstep(c):
    (occ, occ_mag), (sx, sx_mag) = R.sums_ref(c)
    occ64, sx64 = R.sums_ref(c, f64=True)
    means = R.means_of(c)
    sc, sc_mag = R.scatter_ref(c, means)
    return (R.measure(occ64, occ, occ_mag), R.measure(sx64, sx, sx_mag),
            R.measure(R.scatter_ref(c, means, f64=True), sc, sc_mag))


def test_float64_in_frame_order_stays_under_every_pin():
    """E_64 <= pin / 4 everywhere, so the allowance max(pin, 4 E_64) is the pin: no exception to name."""
    cases = ([(n, S, 13) for n, S in R.LANE_CASES if n in (1, 257, 700)] + list(R.GENERIC_D_CASES)
             + [(n, 10, D, W) for n, D, W in R.MULTI_CASES if n == 97])
    for args in cases:
        e_occ, e_sum, e_sc = _e64_mstep(R.mstep_case(*args))
        assert 4 * e_occ <= R.PIN_OCC and 4 * e_sum <= R.PIN_MOMENT and 4 * e_sc <= R.PIN_MOMENT, args
    for n in (65, 65553):
        _, _, _, _, e64 = R.moments_reference(n, 10)
        for name, _, pin in R.MOM_PARTS:
            assert 4 * e64[name] <= pin, (n, name, e64[name])
    for n, D in ((100003, 13), (12289, 40), (4097, 1)):
        x = R.flat_features(n, D)
        mean = x.astype(np.float64).mean(axis=0)
        ref, mag = R.global_cov_ref(x, mean)
        assert 4 * R.measure(R.global_cov_ref(x, mean, f64=True), ref, mag) <= R.PIN_OCC, (n, D)


# ------------------------------------------------------------------------------------- references against the oracle
def test_long_double_mstep_reference_agrees_with_the_oracle():
    c = R.mstep_case(33, 10, 13)
    feats = [np.ascontiguousarray(c.x[c.offs[u]:c.offs[u + 1]].T) for u in range(c.n_utts)]
    gammas = [c.gamma[c.offs[u]:c.offs[u + 1]] for u in range(c.n_utts)]
    want_mean, want_cov = co.update_B(feats, gammas, np.eye(13), 0.0)       # no floor: the plain two-pass estimate
    (occ, _), (sx, _) = R.sums_ref(c)
    means = R.means_of(c)
    sc, _ = R.scatter_ref(c, means)
    live = (occ[0] > 0)
    assert list(np.flatnonzero(~live)) == [0, c.zero_state, c.S - 1]
    np.testing.assert_allclose(means[0], want_mean, rtol=1e-13, atol=0)
    cov = np.zeros((c.S, 13, 13))
    cov[live] = (sc[0][live] / occ[0][live][:, None, None]).astype(np.float64)
    np.testing.assert_allclose(cov, want_cov, rtol=1e-9, atol=1e-9)
    # moments: the same statistics about a fixed centre
    centre = c.x.astype(np.float64).mean(axis=0)
    m, _ = R.moments_ref(c, centre)
    iu = np.triu_indices(13)
    for s in np.flatnonzero(live):
        o, d = m[s, 104], m[s, 91:104] / m[s, 104]
        np.testing.assert_allclose((centre + d).astype(np.float64), want_mean[s], rtol=1e-13)
        s2 = np.zeros((13, 13), R.LD)
        s2[iu] = m[s, :91]
        full = s2 + s2.T - np.diag(np.diag(s2))
        np.testing.assert_allclose((full / o - np.outer(d, d)).astype(np.float64), want_cov[s], rtol=1e-9, atol=1e-9)
    assert not m[~np.r_[live, np.zeros(16 - c.S, bool)]].any() and not m[:, 105:].any()


def test_flat_start_references_agree_with_the_oracle():
    rng = np.random.default_rng(3)
    feats = [(rng.standard_normal((13, int(rng.integers(5, 30)))) * 5 + 100).astype(np.float32) for _ in range(40)]
    np.testing.assert_array_equal(R.global_sum_chain(feats) / sum(f.shape[1] for f in feats), co.global_mean(feats))
    mean = co.global_mean(feats)
    x = np.ascontiguousarray(np.concatenate([f.T for f in feats], axis=0))
    ref, _ = R.global_cov_ref(x, mean)
    want = co.global_covariance(feats, mean, var_floor_factor=0.0)          # diagonal of the biased covariance
    np.testing.assert_allclose(np.diag((ref / len(x)).astype(np.float64)), np.diag(want), rtol=1e-12)

"""The training units custom_estep.hip and custom_update.hip at every dispatch branch and size, through the C ABI
(references, case builders and the derivation of every tolerance: tests/_custom_train_ref.py; the conditions on the
inputs: test_custom_train_cpu.py).

1. sapr_custom_fold_rows: tree (single- and two-level) within n 2^-53 sum|x| of the long-double sum per column — a
   bound that holds for any order of summation — and the same bits twice; SAPR_CUSTOM_FOLD=ordered bit-equal to the
   float64 chain in row order.
2. sapr_custom_update_b_sums / _scatter / _normalise / sapr_custom_update_b: lane kernels (256-utterance tiles), generic
   kernels (any D), several models through utt_model (one of them without utterances), both posterior layouts.
3. sapr_custom_update_b_moments up to 65 553 utterances (the persistent loop ends unevenly); it reads posteriors through
   gamma_at, so both layouts are run; S = 17 and D = 12 are refused.
4. sapr_custom_global_cov on the matrix cores and on the chunked fallback (three ways in); sapr_custom_global_sum at
   D = 1 and D = 40 (D <= 40, so no D gives 64 or 65 columns).
5. The E-step's three classes of c0, the redo list across workgroups, unreachable exits, NaN / inf features, T = 0, 1, 2
   on all four register-resident shapes against the float64 oracle and the run-time-shaped kernel; the latter alone at
   four more shapes.

Parts 2-4 measure |got - ref| / sum|terms| against the long-double reference and allow max(pin, 4 E_64).

Largest measured errors (MI355X):
  1  tree fold: 0.077 of n 2^-53 sum|x| (single- and two-level); ordered fold: bit-equal
  2  occupancies 9.4e-16 (pin 1e-12), sums 9.7e-16 (1e-10) — both in the ordered mode; 2.7e-16 / 3.0e-16 in the lane
     kernels; scatter 6.6e-16 (1e-10)
  3  moments: occupancy 3.5e-16 (1e-12), first 2.0e-16 (1e-10), second 5.4e-16 (1e-10)
  4  global covariance 2.3e-16 on the matrix cores, 1.5e-14 in 4096-frame chunks (1e-12)
  5  against the oracle 2.2e-13 (register-resident) / 3.9e-13 (run-time-shaped) of the 1e-9; band xi 1.1e-4 of its
     allowance; register-resident against run-time-shaped 2.4e-13
"""
import ctypes as C

import numpy as np
import pytest

from tests import _custom_train_ref as R

pytestmark = pytest.mark.gpu
RT = dict(rtol=1e-9, atol=1e-9)
SENTINEL = 7.25          # what a lattice holds where no kernel wrote
LD = np.longdouble


def _close(a, b, **kw):
    kw = {**RT, **kw}
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    np.testing.assert_array_equal(np.isneginf(a), np.isneginf(b))
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    m = np.isfinite(b)
    np.testing.assert_allclose(a[m], b[m], **kw)


def _relerr(a, b):
    """the largest |a - b| / max(|b|, 1) over the finite entries of b (what RT bounds by 1e-9), for the report"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.isfinite(b) & np.isfinite(a)
    return float(np.max(np.abs(a[m] - b[m]) / np.maximum(np.abs(b[m]), 1.0))) if m.any() else 0.0


class Dev:
    def __init__(self):
        import torch
        from sapr_amd import _lib
        self.torch, self._lib = torch, _lib
        self.lib = _lib.load()
        self.dev = torch.device("cuda", 0)
        self.st = _lib.current_stream()
        self.p = _lib.ptr

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def full(self, n, value, dtype=None):
        return self.torch.full((max(int(n), 1),), value, dtype=dtype or self.torch.float64, device=self.dev)

    def ok(self, rc, what):
        self._lib.check(rc, what)


@pytest.fixture(scope="module")
def G():
    return Dev()


def _report(name, value):
    print(f"MEASURED {name} {value:.3g}")


# ----------------------------------------------------------------------------------------------------------------
# 1. fold kernels
@pytest.mark.parametrize("n_rows", R.FOLD_ROWS)
def test_fold_rows_tree_within_the_summation_bound_and_ordered_bit_exact(G, n_rows, monkeypatch):
    worst = 0.0
    for K in R.FOLD_COLS:
        part, _ = R.fold_case(n_rows, K)
        cancel, nan = R.fold_columns(n_rows, K)
        d_part = G.put(part) if n_rows else G.full(K, SENTINEL)
        got = {}
        for mode in ("", "ordered"):
            if mode:
                monkeypatch.setenv("SAPR_CUSTOM_FOLD", mode)
            else:
                monkeypatch.delenv("SAPR_CUSTOM_FOLD", raising=False)
            runs = []
            for _ in range(2):
                out = G.full(K, SENTINEL)
                G.ok(G.lib.sapr_custom_fold_rows(G.p(d_part), n_rows, K, G.p(out), G.st), "sapr_custom_fold_rows")
                runs.append(out.cpu().numpy())
            np.testing.assert_array_equal(runs[0], runs[1], err_msg=f"{mode or 'tree'} K={K}: two runs differ")
            got[mode] = runs[0]
        fin = np.ones(K, bool)
        if nan is not None:
            fin[nan] = False
            assert np.isnan(got[""][nan]) and np.isnan(got["ordered"][nan]), K
        assert np.isfinite(got[""][fin]).all() and np.isfinite(got["ordered"][fin]).all(), K
        if n_rows == 0:
            assert not got[""].any() and not got["ordered"].any()
            continue
        np.testing.assert_array_equal(got["ordered"], R.fold_chain(part), err_msg=f"ordered K={K}")
        ref, mag = R.fold_ref(part)
        err = np.abs(got[""].astype(LD)[fin] - ref[fin])
        bound = n_rows * R.U64 * mag[fin]
        assert np.all(err <= bound), (K, float(np.max(err / bound)))
        worst = max(worst, float(np.max(err / bound)))
    _report(f"fold n_rows={n_rows} err/bound", worst)


# ----------------------------------------------------------------------------------------------------------------
# 2. M-step accumulators
def _gamma_dev(G, c, layout):
    return (G.put(c.gamma.reshape(-1)), 0) if layout == "rows" else (G.put(c.gamma_slots().reshape(-1)), c.slots)


def _workspace(G, n_utts, W, D, S):
    nb = C.c_size_t(0)
    G.ok(G.lib.sapr_custom_update_b_workspace_bytes(n_utts, W, D, S, C.byref(nb)), "workspace_bytes")
    return G.full(nb.value, 0, G.torch.uint8), int(nb.value)


def _mstep_device(G, c, layout):
    """the four calls, then the convenience entry point: every result as numpy"""
    W, S, D, N = c.W, c.S, c.D, c.n_utts
    feats = G.put(c.x) if len(c.x) else G.full(D, 0.0, G.torch.float32)
    offs = G.put(c.offs)
    um = G.put(c.utt_model) if c.utt_model is not None else None
    gam, slots = _gamma_dev(G, c, layout)
    ws, nb = _workspace(G, N, W, D, S)
    nan = float("nan")
    sum_x, occ, scat = G.full(W * S * D, nan), G.full(W * S, nan), G.full(W * S * D * D, nan)
    G.ok(G.lib.sapr_custom_update_b_sums(G.p(feats), G.p(offs), G.p(um), N, W, D, S, G.p(gam), slots, G.p(sum_x),
                                         G.p(occ), G.p(ws), nb, G.st), "sapr_custom_update_b_sums")
    means = sum_x.clone()
    G.ok(G.lib.sapr_custom_normalise(G.p(means), G.p(occ), W * S, D, G.st), "sapr_custom_normalise")
    G.ok(G.lib.sapr_custom_update_b_scatter(G.p(feats), G.p(offs), G.p(um), N, W, D, S, G.p(gam), slots, G.p(means),
                                            G.p(scat), G.p(ws), nb, G.st), "sapr_custom_update_b_scatter")
    covs = scat.clone()
    G.ok(G.lib.sapr_custom_normalise(G.p(covs), G.p(occ), W * S, D * D, G.st), "sapr_custom_normalise")
    means_b, occ_b, covs_b = G.full(W * S * D, nan), G.full(W * S, nan), G.full(W * S * D * D, nan)
    G.ok(G.lib.sapr_custom_update_b(G.p(feats), G.p(offs), G.p(um), N, W, D, S, G.p(gam), slots, G.p(means_b),
                                    G.p(occ_b), G.p(covs_b), G.p(ws), nb, G.st), "sapr_custom_update_b")
    shapes = dict(sum_x=(W, S, D), occ=(W, S), means=(W, S, D), scat=(W, S, D, D), covs=(W, S, D, D),
                  means_b=(W, S, D), occ_b=(W, S), covs_b=(W, S, D, D))
    loc = dict(sum_x=sum_x, occ=occ, means=means, scat=scat, covs=covs, means_b=means_b, occ_b=occ_b, covs_b=covs_b)
    return {k: loc[k].cpu().numpy().reshape(shapes[k]) for k in shapes}


def _check_mstep(G, c, layout, tag):
    r = _mstep_device(G, c, layout)
    again = _mstep_device(G, c, layout)
    for k in r:
        assert np.isfinite(r[k]).all(), f"{k}: a value was not written or is not finite"
        np.testing.assert_array_equal(r[k], again[k], err_msg=f"{k}: two runs differ")
    # the convenience entry point is the four calls, bit for bit
    np.testing.assert_array_equal(r["means_b"], r["means"])
    np.testing.assert_array_equal(r["occ_b"], r["occ"])
    np.testing.assert_array_equal(r["covs_b"], r["covs"])
    (occ, occ_mag), (sx, sx_mag) = R.sums_ref(c)
    occ64, sx64 = R.sums_ref(c, f64=True)
    sc, sc_mag = R.scatter_ref(c, r["means"])
    sc64 = R.scatter_ref(c, r["means"], f64=True)
    e = {}
    for name, got, ref, mag, f64, pin in (("occ", r["occ"], occ, occ_mag, occ64, R.PIN_OCC),
                                          ("sums", r["sum_x"], sx, sx_mag, sx64, R.PIN_MOMENT),
                                          ("scatter", r["scat"], sc, sc_mag, sc64, R.PIN_MOMENT)):
        e[name] = R.measure(got, ref, mag)                      # (asserts exact zeros where there are no terms)
        allow = R.allowance(pin, R.measure(f64, ref, mag))
        assert e[name] <= allow, (tag, name, e[name], allow)
        _report(f"mstep {tag} {layout} {name}", e[name])
    # normalisation: x / occ where occ > 0, untouched (zero) elsewhere — the zero-occupancy state, the empty model
    live = r["occ"] > 0
    np.testing.assert_array_equal(r["means"][live], r["sum_x"][live] / r["occ"][live][:, None])
    np.testing.assert_array_equal(r["covs"][live], r["scat"][live] / r["occ"][live][:, None, None])
    assert not r["means"][~live].any() and not r["covs"][~live].any() and not r["scat"][~live].any()
    assert not live[:, 0].any() and not live[:, -1].any()
    if c.zero_state is not None:
        assert not live[:, c.zero_state].any()
    if c.empty_model is not None:
        assert not live[c.empty_model].any() and not r["sum_x"][c.empty_model].any()
    return r


@pytest.mark.parametrize("layout", ["rows", "slots"])
@pytest.mark.parametrize("n_utts, S", R.LANE_CASES)
def test_update_b_lane_kernels_across_256_utterance_tiles(G, n_utts, S, layout, monkeypatch):
    monkeypatch.delenv("SAPR_CUSTOM_FOLD", raising=False)
    _check_mstep(G, R.mstep_case(n_utts, S, 13), layout, f"lane N={n_utts} S={S}")


@pytest.mark.parametrize("layout", ["rows", "slots"])
@pytest.mark.parametrize("n_utts, S, D", R.GENERIC_D_CASES)
def test_update_b_generic_kernels_at_every_dimension(G, n_utts, S, D, layout, monkeypatch):
    monkeypatch.delenv("SAPR_CUSTOM_FOLD", raising=False)
    _check_mstep(G, R.mstep_case(n_utts, S, D), layout, f"generic N={n_utts} S={S} D={D}")


@pytest.mark.parametrize("layout", ["rows", "slots"])
@pytest.mark.parametrize("n_utts, D, W", R.MULTI_CASES)
def test_update_b_several_models_through_utt_model(G, n_utts, D, W, layout, monkeypatch):
    monkeypatch.delenv("SAPR_CUSTOM_FOLD", raising=False)
    _check_mstep(G, R.mstep_case(n_utts, 10, D, W), layout, f"multi N={n_utts} D={D} W={W}")


@pytest.mark.parametrize("layout", ["rows", "slots"])
def test_update_b_ordered_mode_takes_the_per_utterance_chain_at_13_dimensions(G, layout, monkeypatch):
    """SAPR_CUSTOM_FOLD=ordered sends pass 1 of the single-model 13-dimensional case to update_b_utt_sums_kernel and the
    list-order fold: sums and occupancies are then the float64 chain over frames, then over utterances, bit for bit."""
    monkeypatch.setenv("SAPR_CUSTOM_FOLD", "ordered")
    c = R.mstep_case(257, 10, 13)
    r = _check_mstep(G, c, layout, "ordered N=257")
    want_x, want_o = np.zeros((10, 13)), np.zeros(10)
    x64 = c.x.astype(np.float64)
    for u in range(c.n_utts):
        mu, ou = np.zeros((10, 13)), np.zeros(10)
        for f in range(c.offs[u], c.offs[u + 1]):
            mu += c.gamma[f][:, None] * x64[f]
            ou += c.gamma[f]
        want_x += mu
        want_o += ou
    np.testing.assert_array_equal(r["sum_x"][0], want_x)
    np.testing.assert_array_equal(r["occ"][0], want_o)


# ----------------------------------------------------------------------------------------------------------------
# 3. moments kernel
def _moments(G, c, layout, centre, S=None, D=None):
    S, D = S or c.S, D or c.D
    feats, offs = G.put(c.x), G.put(c.offs)
    gam, slots = _gamma_dev(G, c, layout)
    ws, nb = _workspace(G, c.n_utts, 1, min(D, 13), min(S, 16))
    out, cen = G.full(16 * R.MOM_COLS, SENTINEL), G.put(centre)
    rc = G.lib.sapr_custom_update_b_moments(G.p(feats), G.p(offs), c.n_utts, D, S, G.p(gam), slots, G.p(cen),
                                            G.p(out), G.p(ws), nb, G.st)
    return rc, out.cpu().numpy().reshape(16, R.MOM_COLS)


@pytest.mark.parametrize("n_utts", R.MOM_UTTS)
@pytest.mark.parametrize("S", R.MOM_STATES)
@pytest.mark.parametrize("layout", ["rows", "slots"])
def test_update_b_moments_across_blocks_and_the_persistent_loop(G, n_utts, S, layout):
    c, centre, ref, mag, e64 = R.moments_reference(n_utts, S)
    rc, m = _moments(G, c, layout, centre)
    G.ok(rc, "sapr_custom_update_b_moments")
    rc2, m2 = _moments(G, c, layout, centre)
    np.testing.assert_array_equal(m, m2)
    assert not m[0].any() and not m[S - 1:].any() and not m[:, 105:].any()
    for name, cols, pin in R.MOM_PARTS:
        e = R.measure(m[:, cols], ref[:, cols], mag[:, cols])
        allow = R.allowance(pin, e64[name])
        assert e <= allow, (name, e, allow)
        _report(f"moments N={n_utts} S={S} {layout} {name}", e)


@pytest.mark.parametrize("S, D", [(17, 13), (10, 12)])
def test_update_b_moments_refuse_what_the_kernel_cannot_hold(G, S, D):
    c = R.mstep_case(17, S, D)
    rc, m = _moments(G, c, "slots", np.zeros(D), S=S, D=D)
    assert rc == -2  # SAPR_ERR_UNSUPPORTED
    assert np.all(m == SENTINEL)


# ----------------------------------------------------------------------------------------------------------------
# 4. flat-start statistics
def _global_cov(G, x, mean, ws_doubles=None):
    n, D = x.shape
    nb = C.c_size_t(0)
    G.ok(G.lib.sapr_custom_global_workspace_bytes(1, n, D, C.byref(nb)), "global_workspace_bytes")
    nbytes = int(nb.value) if ws_doubles is None else 8 * ws_doubles
    ws = G.full(nbytes, 0, G.torch.uint8)
    out, feats, mu = G.full(D * D, float("nan")), G.put(x), G.put(mean)    # (every buffer held until the result is read)
    G.ok(G.lib.sapr_custom_global_cov(G.p(feats), n, D, G.p(mu), G.p(out), G.p(ws), nbytes, G.st),
         "sapr_custom_global_cov")
    return out.cpu().numpy().reshape(D, D)


def _check_cov(x, mean, got, tag):
    ref, mag = R.global_cov_ref(x, mean)
    allow = R.allowance(R.PIN_OCC, R.measure(R.global_cov_ref(x, mean, f64=True), ref, mag))
    e = R.measure(got, ref, mag)
    assert e <= allow, (tag, e, allow)
    _report(f"global_cov {tag}", e)
    return ref, mag, allow


@pytest.mark.parametrize("total_frames", R.COV_MFMA_FRAMES)
def test_global_cov_matrix_core_route_across_groups_and_the_persistent_loop(G, total_frames, monkeypatch):
    monkeypatch.delenv("SAPR_CUSTOM_FOLD", raising=False)
    x = R.flat_features(total_frames, 13)
    mean = x.astype(np.float64).mean(axis=0)
    got = _global_cov(G, x, mean)
    np.testing.assert_array_equal(got, _global_cov(G, x, mean))
    np.testing.assert_array_equal(got, got.T)
    _check_cov(x, mean, got, f"mfma n={total_frames}")


@pytest.mark.parametrize("total_frames", R.COV_FALLBACK_FRAMES)
@pytest.mark.parametrize("D", R.COV_FALLBACK_D)
def test_global_cov_chunked_route_at_other_dimensions(G, total_frames, D, monkeypatch):
    monkeypatch.delenv("SAPR_CUSTOM_FOLD", raising=False)
    x = R.flat_features(total_frames, D)
    mean = x.astype(np.float64).mean(axis=0)
    _check_cov(x, mean, _global_cov(G, x, mean), f"chunked D={D} n={total_frames}")


@pytest.mark.parametrize("total_frames", R.COV_FALLBACK_FRAMES)
def test_global_cov_both_routes_on_the_same_data(G, total_frames, monkeypatch):
    """D = 13: the matrix-core route, and the chunked one reached through SAPR_CUSTOM_FOLD=ordered and through a
    workspace too small for the partial tiles — all against the reference, and against one another"""
    x = R.flat_features(total_frames, 13)
    mean = x.astype(np.float64).mean(axis=0)
    monkeypatch.delenv("SAPR_CUSTOM_FOLD", raising=False)
    mfma = _global_cov(G, x, mean)
    chunks = (total_frames + 4095) // 4096
    small = _global_cov(G, x, mean, ws_doubles=chunks * 169)
    monkeypatch.setenv("SAPR_CUSTOM_FOLD", "ordered")
    ordered = _global_cov(G, x, mean)
    np.testing.assert_array_equal(small, ordered)           # the same kernels
    assert not np.array_equal(small, mfma) or total_frames < 8, "the small workspace did not change the route"
    ref, mag, allow = _check_cov(x, mean, mfma, f"both/mfma n={total_frames}")
    _check_cov(x, mean, small, f"both/chunked n={total_frames}")
    assert R.measure(mfma, small.astype(LD), mag) <= allow


@pytest.mark.parametrize("n_utts, D", [(1, 1), (700, 1), (1, 40), (700, 40)])
def test_global_sum_list_order_fold_at_the_dimension_limits(G, n_utts, D):
    rng = np.random.default_rng([n_utts, D])
    feats = []
    for _ in range(n_utts):
        T = int(rng.integers(1, 40))
        feats.append((10.0 ** rng.integers(-6, 4) * rng.standard_normal((D, T))).astype(np.float32))
    lens = np.array([f.shape[1] for f in feats])
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    x = np.ascontiguousarray(np.concatenate([f.T for f in feats], axis=0))
    nb = C.c_size_t(0)
    G.ok(G.lib.sapr_custom_global_workspace_bytes(n_utts, int(lens.sum()), D, C.byref(nb)), "global_workspace_bytes")
    ws = G.full(nb.value, 0, G.torch.uint8)
    out, d_x, d_offs = G.full(D, float("nan")), G.put(x), G.put(offs)
    G.ok(G.lib.sapr_custom_global_sum(G.p(d_x), G.p(d_offs), n_utts, D, G.p(out), G.p(ws), int(nb.value), G.st),
         "sapr_custom_global_sum")
    np.testing.assert_array_equal(out.cpu().numpy(), R.global_sum_chain(feats))


# ----------------------------------------------------------------------------------------------------------------
# 5. E-step
def _estep_device(G, b, mode):
    """mode: 'generic' (row layout, custom_estep_kernel) or 0 / 1 / 2 (slot layout: frame-major features, staged
    features, staged features and frame sums).  Returns (utt_out[N][K], gamma[N] list of (T, S))."""
    S, D, N = b.S, b.D, b.n_utts
    K = 2 + S + S * S
    total, max_T = int(b.offs[-1]), int(b.lens.max())
    feats, offs, um = G.put(b.x), G.put(b.offs), G.put(b.utt_model)
    arrs = [G.put(a) for a in b.arrays()]
    out = G.full(N * K, SENTINEL)
    if mode == "generic":
        lat = [G.full(total * S, SENTINEL) for _ in range(4)]
        G.ok(G.lib.sapr_custom_estep(G.p(feats), G.p(offs), G.p(um), N, D, S, b.W, *[G.p(a) for a in arrs], 0,
                                     *[G.p(a) for a in lat], None, G.p(out), G.st), "sapr_custom_estep")
        g = lat[3].cpu().numpy().reshape(total, S)
        return out.cpu().numpy().reshape(N, K), [g[b.offs[u]:b.offs[u + 1]] for u in range(N)], None
    slots = ((N + 63) // 64) * 64
    feat_t = fsum = None
    if mode:
        feat_t = G.full(max_T * D * slots, float("nan"), G.torch.float32)
        fsum = G.full(D * slots, float("nan"))
        G.ok(G.lib.sapr_custom_stage_features(G.p(feats), G.p(offs), N, D, max_T, slots, G.p(feat_t), G.p(fsum), G.st),
             "sapr_custom_stage_features")
    lat = [G.full(max_T * S * slots, SENTINEL) for _ in range(4)]
    G.ok(G.lib.sapr_custom_estep_staged(G.p(feats), G.p(offs), G.p(um), N, D, S, b.W, *[G.p(a) for a in arrs], slots,
                                        *[G.p(a) for a in lat], None, G.p(out), G.p(feat_t),
                                        G.p(fsum) if mode == 2 else None, G.st), "sapr_custom_estep_staged")
    g = lat[3].cpu().numpy().reshape(max_T, S, slots)
    return out.cpu().numpy().reshape(N, K), [g[:b.lens[u], :, u] for u in range(N)], g


def _check_against_oracle(b, out, gammas, tag, zero_class_exact):
    S = b.S
    worst, worst_band = 0.0, 0.0
    for u, o in enumerate(b.utts):
        got_xi = out[u, 2 + S:].reshape(S, S)
        if o.kind == "empty":
            assert not out[u].any(), (tag, u)
            continue
        _close(out[u, 0], o.ll)
        _close(out[u, 1], o.sc)
        _close(out[u, 2:2 + S], o.gamma[:-1].sum(axis=0))
        _close(gammas[u], o.gamma)
        worst = max(worst, _relerr(out[u, 0], o.ll), _relerr(out[u, 1], o.sc), _relerr(gammas[u], o.gamma),
                    _relerr(out[u, 2:2 + S], o.gamma[:-1].sum(axis=0)))
        if o.kind == "zero" and zero_class_exact:
            assert not got_xi.any(), (tag, u, o.c0)
        if o.kind == "band":
            # the reference's terms are denormal here: quantised, and the device's exp may land one step away
            if o.xi_in_oracle:
                allow = float(np.sum(o.xi_allow))
                err = float(np.max(np.abs(got_xi - o.xi_sum)))
                assert err <= allow, (tag, u, o.c0, err, allow)
                worst_band = max(worst_band, err / allow)
        else:
            _close(got_xi, o.xi_sum)
            worst = max(worst, _relerr(got_xi, o.xi_sum))
    _report(f"estep {tag} vs oracle", worst)
    _report(f"estep {tag} band xi err/allowance", worst_band)


@pytest.mark.parametrize("ns, D, which", [(ns, D, "mixed") for ns, D in R.FAST_SHAPES]
                         + [(8, 13, "smooth"), (8, 13, "band")])
def test_estep_every_class_of_c0_on_the_register_resident_shapes(G, ns, D, which):
    b = R.estep_batch(ns, D, which)
    runs = {m: [_estep_device(G, b, m) for _ in range(2)] for m in (0, 1, 2)}
    for m in (0, 1, 2):
        # a second run: the redo list fills in another order, the results may not depend on it
        np.testing.assert_array_equal(runs[m][0][0], runs[m][1][0], err_msg=f"staged={m}: two runs differ")
        np.testing.assert_array_equal(runs[m][0][2], runs[m][1][2], err_msg=f"staged={m}: two runs differ (gamma)")
    for m in (1, 2):  # the three ways to hand over the features: the same operations, NaN positions included
        np.testing.assert_array_equal(runs[0][0][0], runs[m][0][0], err_msg=f"staged={m} against frame-major")
        np.testing.assert_array_equal(runs[0][0][2], runs[m][0][2], err_msg=f"staged={m} against frame-major (gamma)")
    out, gammas, lattice = runs[1][0]
    # nothing is written past an utterance's end, into the empty utterance's slot or into the unused slots
    for u in range(b.n_utts):
        assert np.all(lattice[b.lens[u]:, :, u] == SENTINEL), u
    assert np.all(lattice[:, :, b.n_utts:] == SENTINEL)
    _check_against_oracle(b, out, gammas, f"fast ns={ns} D={D} {which}", zero_class_exact=True)
    # against the run-time-shaped kernel: the device's own exp in the reference's order, so the band agrees too
    gout, ggam, _ = _estep_device(G, b, "generic")
    _close(out, gout)
    worst = _relerr(out, gout)
    for u in range(b.n_utts):
        _close(gammas[u], ggam[u])
        worst = max(worst, _relerr(gammas[u], ggam[u]))
    _report(f"estep fast ns={ns} D={D} {which} vs generic", worst)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("S, D", R.GENERIC_SHAPES)
def test_estep_run_time_shaped_kernel_against_the_oracle(G, S, D, dense):
    b = R.generic_batch(S, D, dense)
    out, gammas, _ = _estep_device(G, b, "generic")
    out2, _, _ = _estep_device(G, b, "generic")
    np.testing.assert_array_equal(out, out2)
    _check_against_oracle(b, out, gammas, f"generic S={S} D={D} dense={dense}", zero_class_exact=False)

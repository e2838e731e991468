"""CPU: the numpy definition of MMI training (tests/_mmi_ref.py) against path enumeration and hand-worked numbers,
the host-side update of ``sapr_amd.connected`` against it, the conditions the GPU cases of tests/test_mmi_gpu.py rely
on, and the C ABI of ``sapr_connected_loop_stats`` without a device."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _embedded_ref as eref
from tests import _loop_fb_ref as fref
from tests import _mmi_cases as cases
from tests import _mmi_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -np.inf


# ---- F(u) is the log of the transcript's share of all paths ---------------------------------------------------------
def _tiny(seed, T, dense):
    """2 words x 2 states x T <= 4 frames under a random bigram; ``dense``: every transition and exit is allowed."""
    rng = np.random.default_rng(seed)
    W, S = 2, 2
    with np.errstate(divide="ignore"):
        ls = np.log(rng.dirichlet(np.ones(S), W)) if dense else np.log(np.array([[1.0, 0.0]] * W))
        lt = np.log(rng.dirichlet(np.ones(S), (W, S)))
        if not dense:
            lt[:, 1, 0] = NEG
        lx = np.log(rng.uniform(0.2, 1.0, (W, S))) if dense else np.array([[NEG, 0.0]] * W)
    lm = np.log(rng.dirichlet(np.ones(W + 1), W))[:, :W]
    lm_start = np.log(rng.dirichlet(np.ones(W)))
    lm_end = np.log(rng.uniform(0.1, 0.9, W))
    logb = rng.normal(-3.0, 2.0, (T, W, S))
    return logb, ls, lt, lx, lm, lm_start, lm_end


@pytest.mark.parametrize("dense", (True, False))
@pytest.mark.parametrize("T,words", ((1, [1]), (2, [0, 1]), (3, [1, 1]), (4, [0, 1]), (4, [1]), (4, [0, 0])))
def test_objective_is_the_log_share_of_the_transcripts_paths(T, words, dense):
    logb, ls, lt, lx, lm, lm_start, lm_end = _tiny(31 * T + len(words) + 7 * words[0], T, dense)
    got = mref.objective(logb, [T], [words], ls, lt, lx, lm, lm_start, lm_end)
    num = eref.brute(logb, words, ls, lt, lx, 0.0)["loglik"] + mref.lm_score(words, lm, lm_start, lm_end)
    den = fref.brute(logb, ls, lt, lx, lm, lm_start, lm_end)[0]
    if not np.isfinite(num):                                     # (the sparse topology cannot place the words)
        assert not got["keep"][0] and got["F"] == 0.0
        return
    assert got["keep"][0]
    assert got["F"] == pytest.approx(num - den, rel=1e-12, abs=1e-12)
    assert got["F"] <= 1e-12
    assert np.exp(got["F"]) <= 1.0 + 1e-12


def test_a_forbidden_transcript_scores_minus_infinity_and_two_words_cannot_share_one_frame():
    logb, ls, lt, lx, lm, lm_start, lm_end = _tiny(5, 3, True)
    lm = lm.copy()
    lm[0, 1] = NEG
    assert mref.lm_score([0, 1], lm, lm_start, lm_end) == NEG
    got = mref.objective(logb[:1], [1], [[1, 0]], ls, lt, lx, lm, lm_start, lm_end)   # 2 words, 1 frame
    assert not got["keep"][0] and np.isfinite(got["den_loglik"][0]) and got["F"] == 0.0


def test_den_stats_leaves_out_what_keep_drops():
    rng = np.random.default_rng(3)
    post = rng.uniform(0, 1, (7, 2, 3))
    x = rng.normal(0, 1, (7, 2)).astype(np.float32)
    poisoned_post, poisoned_x = post.copy(), x.copy()
    poisoned_post[3:5], poisoned_x[3:5] = np.nan, np.nan
    got = mref.den_stats(poisoned_post, poisoned_x, [3, 2, 0, 2], [1, 0, 1, 1])
    rows = [0, 1, 2, 5, 6]
    assert got["nobs"] == 2
    np.testing.assert_allclose(got["post"], post[rows].sum(axis=0), rtol=1e-14)
    np.testing.assert_allclose(got["obs"], np.einsum("tws,td->wsd", post[rows], x[rows].astype(np.float64)),
                               rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(got["obs2"], np.einsum("tws,td->wsd", post[rows], (x[rows] * x[rows]).astype(float)),
                               rtol=1e-13, atol=1e-14)


# ---- the extended Baum-Welch update ---------------------------------------------------------------------------------
def _updates():
    from sapr_amd.connected import mmi_update
    return (("reference", mref.update), ("connected.mmi_update", mmi_update))


@pytest.mark.parametrize("which", (0, 1))
def test_update_reproduces_a_hand_worked_number_set(which):
    """Four states of one feature, worked by hand (E = 2, tau = 0):

    state 0: mu 1, var 2; num (3, 6, 20), den (1, 1, 3): occ 2, th1 5, th2 17; a 2, b 13, c 9: both roots negative,
             D_min 0, D = E den.post = 2; mu' = 7 / 4, var' = 23 / 4 - 49 / 16 = 2.6875
    state 1: mu 0, var 1; num (1, 0, 1), den (2, 2, 6): occ -1, th1 -2, th2 -5; a 1, b -6, c 1: larger root
             3 + 2 sqrt 2 = D_min (> -occ = 1), D = 2 D_min = 6 + 4 sqrt 2 (> E den.post = 4);
             mu' = -2 / (5 + 4 sqrt 2), var' = (1 + 4 sqrt 2) / (5 + 4 sqrt 2) - mu'^2
    state 2: nothing seen on either side: occ 0, D 0: kept as it is
    state 3: mu 2, var 1; num (2, 4, 10) = den (2, 4, 10): theta 0, D = E den.post = 4: unchanged
    """
    name, update = _updates()[which]
    mu = np.array([[1.0], [0.0], [5.0], [2.0]])
    var = np.array([[2.0], [1.0], [3.0], [1.0]])
    num = {"post": np.array([3.0, 1.0, 0.0, 2.0]), "obs": np.array([[6.0], [0.0], [0.0], [4.0]]),
           "obs**2": np.array([[20.0], [1.0], [0.0], [10.0]])}
    den = {"post": np.array([1.0, 2.0, 0.0, 2.0]), "obs": np.array([[1.0], [2.0], [0.0], [4.0]]),
           "obs**2": np.array([[3.0], [6.0], [0.0], [10.0]])}
    got_mu, got_var = update(num, den, mu, var, "diag", E=2.0, tau=0.0, min_covar=1e-3)
    r2 = np.sqrt(2.0)
    m1 = -2.0 / (5.0 + 4.0 * r2)
    want_mu = np.array([[1.75], [m1], [5.0], [2.0]])
    want_var = np.array([[2.6875], [(1.0 + 4.0 * r2) / (5.0 + 4.0 * r2) - m1 * m1], [3.0], [1.0]])
    np.testing.assert_allclose(got_mu, want_mu, rtol=1e-14, err_msg=name)
    np.testing.assert_allclose(got_var, want_var, rtol=1e-13, err_msg=name)
    assert got_mu[2, 0] == 5.0 and got_var[2, 0] == 3.0          # the empty state keeps its bytes
    assert mref.d_min(-1.0, np.array([-2.0]), np.array([-5.0]), mu[1], var[1]) == pytest.approx(3.0 + 2.0 * r2, 1e-15)
    # I-smoothing: tau = 1 scales state 3's numerator by 1 + 1 / 2: occ 1, th1 2, th2 5; a 1, b 5 + 5 - 8 = 2,
    # c 5 - 4 = 1: a double root at -1, D_min 0, D = 4; mu' = (2 + 8) / 5 = 2, var' = (5 + 20) / 5 - 4 = 1
    got_mu, got_var = update(num, den, mu, var, "diag", E=2.0, tau=1.0, min_covar=1e-3)
    assert got_mu[3, 0] == pytest.approx(2.0, rel=1e-15) and got_var[3, 0] == pytest.approx(1.0, rel=1e-14)
    assert got_mu[2, 0] == 5.0 and got_var[2, 0] == 3.0          # num.post = 0: unscaled, and still empty
    # state 0 with tau = 3: scale 2: occ 5, th1 11, th2 37; b = 37 + 15 - 22 = 30, c = 185 - 121 = 64: roots negative,
    # D = 2; mu' = 13 / 7, var' = (37 + 6) / 7 - 169 / 49
    got_mu, got_var = update(num, den, mu, var, "diag", E=2.0, tau=3.0, min_covar=1e-3)
    assert got_mu[0, 0] == pytest.approx(13.0 / 7.0, rel=1e-15)
    assert got_var[0, 0] == pytest.approx(43.0 / 7.0 - 169.0 / 49.0, rel=1e-14)
    # the variance floor
    _, got_var = update(num, den, mu, var, "diag", E=2.0, tau=0.0, min_covar=4.0)
    assert got_var[0, 0] == 4.0 and got_var[2, 0] == 3.0


@pytest.mark.parametrize("which", (0, 1))
def test_spherical_takes_the_mean_over_the_features(which):
    name, update = _updates()[which]
    rng = np.random.default_rng(8)
    S, D = 3, 4
    mu, var = rng.normal(0, 2, (S, D)), rng.uniform(1, 2, S)
    num = {"post": rng.uniform(5, 9, S), "obs": rng.normal(0, 9, (S, D)), "obs**2": rng.uniform(40, 60, (S, D))}
    den = {"post": rng.uniform(1, 4, S), "obs": rng.normal(0, 3, (S, D)), "obs**2": rng.uniform(5, 20, (S, D))}
    mu_d, var_d = update(num, den, mu, np.repeat(var[:, None], D, 1), "diag")
    mu_s, var_s = update(num, den, mu, var, "spherical")
    assert var_s.shape == (S,)
    np.testing.assert_array_equal(mu_s, mu_d)
    np.testing.assert_allclose(var_s, var_d.mean(axis=1), rtol=1e-15, err_msg=name)
    with pytest.raises(NotImplementedError, match="'full'"):
        _updates()[1][1](num, den, mu, np.zeros((S, D, D)), "full")


def test_both_updates_agree_on_random_statistics():
    from sapr_amd.connected import mmi_update
    rng = np.random.default_rng(21)
    for trial in range(50):
        S, D = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        mu, var = rng.normal(0, 3, (S, D)), rng.uniform(0.5, 4, (S, D))
        num = {"post": rng.uniform(0, 9, S), "obs": rng.normal(0, 20, (S, D)), "obs**2": rng.uniform(0, 90, (S, D))}
        den = {"post": rng.uniform(0, 9, S), "obs": rng.normal(0, 20, (S, D)), "obs**2": rng.uniform(0, 90, (S, D))}
        if trial % 5 == 0:
            num["post"][0] = 0.0
        tau = (0.0, 2.5)[trial % 2]
        a = mref.update(num, den, mu, var, "diag", E=1.5, tau=tau, min_covar=1e-3)
        b = mmi_update(num, den, mu, var, "diag", E=1.5, tau=tau, min_covar=1e-3)
        np.testing.assert_allclose(b[0], a[0], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(b[1], a[1], rtol=1e-12, atol=1e-12)


def test_the_variance_is_positive_for_every_constant_above_d_min():
    rng = np.random.default_rng(55)
    for _ in range(300):
        D = int(rng.integers(1, 5))
        mu, var = rng.normal(0, 3, (1, D)), rng.uniform(0.1, 4, (1, D))
        num = {"post": rng.uniform(0, 9, 1), "obs": rng.normal(0, 20, (1, D)), "obs2": rng.uniform(0, 90, (1, D))}
        den = {"post": rng.uniform(0, 9, 1), "obs": rng.normal(0, 20, (1, D)), "obs2": rng.uniform(0, 90, (1, D))}
        occ = num["post"][0] - den["post"][0]
        dm = mref.d_min(occ, num["obs"][0] - den["obs"][0], num["obs2"][0] - den["obs2"][0], mu[0], var[0])
        assert dm >= 0.0 and dm >= -occ
        for factor in (1.0 + 1e-9, 1.5, 2.0, 10.0, 1e4):
            Ds = dm * factor + 1e-9                              # (D_min = 0: any positive constant)
            assert occ + Ds > 0.0
            _, v = mref.update(num, den, mu, var, "diag", min_covar=0.0, D_s=[Ds])
            assert (v > 0.0).all(), (dm, factor, v)


@pytest.mark.parametrize("which", (0, 1))
def test_equal_statistics_change_nothing(which):
    """theta = 0: mu' = D mu / D and var' = D (var + mu^2) / D - mu^2.  With |mu| <= 1 / 2 and var in [1, 2] the
    roundings (the sum, the product, the quotient, the square, the difference) add up to less than 4 ulp of 2.25 against
    a variance of at least 1: below 1e-15."""
    name, update = _updates()[which]
    rng = np.random.default_rng(13)
    S, D = 6, 5
    mu, var = rng.uniform(-0.5, 0.5, (S, D)), rng.uniform(1.0, 2.0, (S, D))
    st = {"post": rng.uniform(1, 50, S), "obs": rng.normal(0, 30, (S, D)), "obs**2": rng.uniform(10, 900, (S, D))}
    got_mu, got_var = update(st, copy.deepcopy(st), mu, var, "diag", E=2.0)
    np.testing.assert_allclose(got_mu, mu, rtol=1e-15, atol=0, err_msg=name)
    np.testing.assert_allclose(got_var, var, rtol=1e-15, atol=0, err_msg=name)


# ---- what the GPU cases rely on, from the reference alone -------------------------------------------------------------
def test_the_confusable_case_trains_and_drops_two_utterances():
    models, utts, truth, lm = cases.confusable_case()
    assert np.array_equal(models[0].means_, models[1].means_)    # the pair shares its Gaussians
    _, history, last = mref.fit(models, utts, truth, lm, n_iter=4)
    assert len(history) == 4 and all(b > a for a, b in zip(history, history[1:])), history
    assert all(h <= 1e-9 for h in history)
    keep = last["keep"]
    assert keep[:16].all() and not keep[16:].any()
    assert np.isfinite(last["terms"][keep]).all() and np.isfinite(last["lmscore"]).all()
    assert np.isfinite(last["den_loglik"][16]) and last["num_loglik"][16] == NEG     # more words than frames
    assert last["den_loglik"][17] == NEG                                             # no frames


def test_the_chain_case_has_numerator_equal_to_denominator():
    models, utts, truth, lm = cases.chain_case()
    _, history, last = mref.fit(models, utts, truth, lm, n_iter=1)
    keep = last["keep"]
    assert keep.sum() == 11 and not keep[5]
    assert np.isfinite(last["terms"][keep]).all() and (last["lmscore"] == 0.0).all()
    frames = sum(len(x) for x, k in zip(utts, keep) if k)
    assert abs(history[0]) <= 1e-9 * frames
    for key_n, key_d in (("post_sum", "post"), ("obs", "obs"), ("obs2", "obs2")):
        np.testing.assert_allclose(last["den"][key_d], last["num"][key_n], rtol=1e-9, atol=1e-9)
    assert len(set(cases.CHAIN)) == len(cases.CHAIN)


@pytest.mark.parametrize("W,S,D", cases.SWEEP)
def test_the_sweep_cases_hold_what_the_device_test_looks_for(W, S, D):
    (ls, lt, lx), n_states, post, feats, keep, loglik = cases.sweep_case(W, S, D)
    lengths = cases.SWEEP_LENGTHS
    assert sorted(lengths) == [0, 1, 3, 4, 5, 64, 65, 300]
    assert 0 < cases.SWEEP_MASKED < len(lengths) - 1 and not keep[cases.SWEEP_MASKED] and keep.sum() == len(lengths) - 1
    offs = np.r_[0, np.cumsum(lengths)]
    z = cases.SWEEP_ZERO
    assert loglik[z] == NEG and not post[offs[z]:offs[z + 1]].any() and lengths[z] > 0
    with_path = [u for u, n in enumerate(lengths) if n > 0 and u != z]
    assert np.isfinite(loglik[with_path]).all()
    assert n_states[1] < S and not post[:, 1, n_states[1]:].any()
    want = mref.den_stats(post, feats, lengths, keep)
    frames = sum(lengths[u] for u in with_path if keep[u])
    assert want["nobs"] == sum(1 for u, n in enumerate(lengths) if n > 0 and keep[u])
    assert want["post"].sum() == pytest.approx(frames, rel=1e-9)


# ---- the C ABI, without a device --------------------------------------------------------------------------------------
NAMES = ("sapr_connected_loop_stats_workspace_bytes", "sapr_connected_loop_stats")


def test_symbols_are_declared_bound_and_exported():
    from sapr_amd import _lib
    with open(os.path.join(ROOT, "include", "sapr_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "tests/_mmi_ref.py" in header
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    import sapr_amd
    from sapr_amd import connected
    for name in ("loop_stats", "loop_stats_workspace_bytes", "MmiStats", "mmi_estep", "mmi_update", "mmi_fit"):
        assert getattr(sapr_amd, name) is getattr(connected, name)
    from sapr_amd.decoder import Decoder
    assert callable(Decoder.train_discriminative)
    with open(os.path.join(ROOT, "sapr_amd", "build.py"), encoding="utf-8") as fh:
        assert '"connected_loop_stats.hip"' in fh.read()


def _run(lib, n_utts=1, total=10, W=2, S=4, D=3, ws=None, ws_bytes=0, stats=False):
    """``sapr_connected_loop_stats`` with every pointer NULL except the workspace and, where asked, ``stats`` (a host
    address the checks never dereference)."""
    dummy = (C.c_double * 1)()
    return lib.sapr_connected_loop_stats(None, None, D, None, n_utts, total, None, W, S, ws, ws_bytes,
                                         C.cast(dummy, C.c_void_p) if stats else None, None)


def test_size_function_and_refusals_before_any_launch():
    from sapr_amd import _lib
    from sapr_amd.connected import loop_stats_workspace_bytes
    lib = _lib.load()
    n = C.c_size_t(0)
    size = lib.sapr_connected_loop_stats_workspace_bytes
    # 1000 frames: spans of 256 frames, 4 partial rows of R * (2 D + 1) = 110 * 27 doubles
    assert size(1000, 7, 11, 10, 13, C.byref(n)) == 0 and n.value == 8 * 4 * 110 * 27
    assert loop_stats_workspace_bytes(1000, 7, 11, 10, 13) == n.value
    # 10 000 x 505 frames: ceil(5 050 000 / 1024) = 4932 -> spans of 4992 frames, 1012 of them
    assert size(5_050_000, 10_000, 11, 18, 39, C.byref(n)) == 0 and n.value == 8 * 1012 * 198 * 79
    assert size(256, 1, 3, 3, 1, C.byref(n)) == 0 and n.value == 8 * 1 * 12 * 3
    assert size(257, 1, 3, 3, 1, C.byref(n)) == 0 and n.value == 8 * 2 * 12 * 3
    assert size(0, 0, 1, 1, 1, C.byref(n)) == 0 and n.value == 0
    # unsupported: S = 19, W * SP = 260, D = 40 — from the size function and the entry point
    assert size(10, 1, 2, 19, 3, C.byref(n)) == -2
    assert size(10, 1, 26, 10, 3, C.byref(n)) == -2
    assert b"W * SP" in lib.sapr_last_error()
    assert size(10, 1, 2, 4, 40, C.byref(n)) == -2
    assert b"D in 1..39" in lib.sapr_last_error()
    assert size(10, 1, 14, 18, 39, C.byref(n)) == 0
    assert _run(lib, W=2, S=19) == -2 and _run(lib, W=26, S=10) == -2 and _run(lib, D=40) == -2
    # bad sizes
    for bad in ((-1, 1, 2, 4, 3), (10, -1, 2, 4, 3), (10, 1, 0, 4, 3), (10, 1, 2, 0, 3), (10, 1, 2, 4, 0)):
        assert size(*bad, C.byref(n)) == -1
        assert b"bad sizes" in lib.sapr_last_error()
    assert size(10, 1, 2, 4, 3, None) == -1
    assert _run(lib, D=0) == -1 and _run(lib, n_utts=-1) == -1 and _run(lib, total=-1) == -1
    # the workspace: 10 frames, R = 8, 7 columns
    need = 8 * 1 * 8 * 7
    buf = (C.c_uint8 * need)()
    assert _run(lib, ws=None, ws_bytes=0, stats=True) == -1
    assert b"workspace too small" in lib.sapr_last_error()
    assert _run(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=need - 1, stats=True) == -1
    assert _run(lib, ws=None, ws_bytes=need, stats=True) == -1
    # NULL pointers, behind the workspace check and before any launch
    assert _run(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=need) == -1
    assert b"stats" in lib.sapr_last_error()
    assert _run(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=need, stats=True) == -1
    assert b"NULL pointer" in lib.sapr_last_error()


def test_host_side_refusals_need_no_device():
    """A forbidden transcript, an unknown word and the families without a denominator kernel are refused before a
    device is asked for."""
    from sapr_amd.connected import ConnectedNetwork, WordBigram, mmi_estep, mmi_fit, mmi_update
    models, utts, truth, _ = cases.chain_case()
    W = len(models)
    grammar = WordBigram.from_grammar(W, [(2, 0), (0, 3), (3, 1)], starts=[2], ends=[1])
    net = ConnectedNetwork.from_models(models, bigram=grammar)
    with pytest.raises(ValueError, match="utterance 1"):
        mmi_estep(utts[:2], [truth[0], [2, 3, 0, 1]], net)
    with pytest.raises(ValueError, match="utterance 0"):
        mmi_fit(copy.deepcopy(models), utts[:1], [[0, 3, 1]], bigram=grammar)        # may not begin with word 0
    with pytest.raises(ValueError, match="word 7"):
        mmi_fit(copy.deepcopy(models), utts[:1], [[2, 7]], names=cases.NAMES)
    with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
        mmi_estep(utts[:2], truth[:1], net)
    with pytest.raises(ValueError, match="acoustic_scale"):
        mmi_estep(utts[:2], truth[:2], net, acoustic_scale=0.0)
    with pytest.raises(NotImplementedError, match="'full'"):
        mmi_update({}, {}, np.zeros((2, 2)), np.zeros((2, 2, 2)), "full")
    full = copy.deepcopy(models)
    full[2].covariance_type = "full"
    full[2]._covars_ = np.tile(np.eye(cases.D_FIT) * 40.0, (cases.S_FIT, 1, 1))
    with pytest.raises(NotImplementedError, match="'full'"):
        mmi_fit(full, utts, truth)

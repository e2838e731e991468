"""GPU: every padded instantiation of the GMMHMM kernels (csrc/gmm_hmm.hip: gmm_emit_kernel / gmm_accum_kernel<MP, DP>,
the trellis kernels<SP>; csrc/gmm_vocab.hip: gmm_vocab_kernel<SP, MP, DP> in both modes) and the branches only some
shapes reach, against the numpy restatement tests/_gmmhmm_ref.py on the cases of tests/_gmmhmm_sweep.py (reference
results computed once per case; tests/test_gmmhmm_shapes_cpu.py checks the conditions on the inputs).

    sweep      72 cases: (S, M, D) = (SP, MP, DP) for all 36 triples, and the smallest sizes every padded width serves
               (S in {1, 5, 11}, M in {1, 2, 3, 5}, D in {1, 14, 27}: most of the instantiation is padding)
    ragged     utterances of 1024 .. 0 frames whose running frame counts land on and off the 64-frame chunks of
               gmm_accum_kernel and the 256-frame blocks of gmm_emit_kernel; a word without utterances
    tiles      nine tiles of one model behind another model's tile: the eight-wide loop of gmm_reduce_kernel and its
               tail, on the per-tile rows (8 + 1) and on the partial rows (32 + 4)
    degenerate a component of weight 0, zeros in startprob and an unreachable state, left-to-right with skips, an
               absorbing state, a frame 1000 away from every mean

The comparisons and pins are those of tests/test_gmmhmm_gpu.py and tests/test_gmm_vocab_gpu.py: loglik, logprob and
vocabulary scores rtol 1e-11; statistics and posteriors rtol 1e-9 / atol 1e-9, a component's observation sums compared
wherever the reference's post_mix is >= 1e-6 (below that only |post_mix_gpu - post_mix_ref| <= 1e-9); paths and best
words equal; the columns of the vocabulary launch against the per-model entry points with np.array_equal.  Every test
prints its largest errors against the reference; test_sweep_error_record prints the largest over the sweep (a record of
the margin under the pins, not a threshold)."""
import functools

import numpy as np
import pytest

from tests import _gmmhmm_sweep as sw

pytestmark = pytest.mark.gpu

RTOL_SCORE, TOL_STAT, SEEN = 1e-11, 1e-9, 1e-6
STAT_KEYS = (("start", "start"), ("trans", "trans"), ("post", "post"), ("post_mix", "post_mix"), ("obs", "obs"),
             ("obs**2", "obs2"))
RECORD = {}        # figure -> largest value over the sweep cases that ran


def _host(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


@functools.lru_cache(maxsize=None)
def _batch(name):
    from sapr_amd import gmm_hmm as gh
    c = sw.case(name)
    W = len(c["utts"])
    return gh.GmmBatch(c["feats"], c["lengths"], c["utt_model"], W, c["S"], c["M"]), gh.pack_models(c["params"])


def _rel(got, want):
    """Largest |got - want| / |want| over the finite, non-zero reference values."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    sel = np.isfinite(want) & (want != 0)
    return float((np.abs(got[sel] - want[sel]) / np.abs(want[sel])).max()) if sel.any() else 0.0


def _note(figs, name, sweep):
    print(f"{name}: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    if sweep:
        for k, v in figs.items():
            RECORD[k] = max(RECORD.get(k, 0.0), v)


def _covered(S, M, D, S_model):
    """The cells of a raw statistics row (kernel state count S) that split_stats hands out for S_model states."""
    def block(shape, keep):
        m = np.zeros(shape, dtype=bool)
        m[keep] = True
        return m.ravel()
    s = slice(0, S_model)
    return np.concatenate([np.ones(2, dtype=bool), block((S,), s), block((S, S), (s, s)), block((S,), s),
                           block((S, M), s), block((S, M, D), s), block((S, M, D), s)])


def _check_estep(name, out, figs):
    """loglik, the statistics rows, post and path of one all-on E-step launch against the reference."""
    from sapr_amd import gmm_hmm as gh
    c = sw.case(name)
    S, M, D = c["S"], c["M"], c["D"]
    ref_stats, ref_utts = sw.reference_estep(name)
    loglik, stats, post, path = out
    want = np.array([r["loglik"] for r in ref_utts])
    figs["loglik rel"] = _rel(loglik, want)
    np.testing.assert_allclose(loglik, want, rtol=RTOL_SCORE)
    assert np.all(loglik[c["lengths"] == 0] == -np.inf) and np.all(np.isfinite(loglik[c["lengths"] > 0]))
    gamma = np.concatenate([r["gamma"] for r in ref_utts], axis=0)
    assert post.shape == gamma.shape == (c["feats"].shape[0], S)
    figs["post abs"] = float(np.abs(post - gamma).max())
    np.testing.assert_allclose(post, gamma, rtol=TOL_STAT, atol=TOL_STAT)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=TOL_STAT, atol=TOL_STAT)
    assert path.dtype == np.int32 and np.array_equal(path, np.argmax(post, axis=1))   # the MAP path
    assert stats.shape == (len(ref_stats), gh.stats_width(S, M, D))
    rel = ab = 0.0
    for w, rs in enumerate(ref_stats):
        st = gh.split_stats(stats[w], S, M, D)
        assert st["nobs"] == rs["nobs"]                  # an utterance without frames adds nothing
        if rs["nobs"] == 0:                              # a word without utterances: an exact zero row
            assert not np.any(stats[w])
            continue
        figs["logprob rel"] = max(figs.get("logprob rel", 0.0), _rel(st["logprob"], rs["logprob"]))
        np.testing.assert_allclose(st["logprob"], rs["logprob"], rtol=RTOL_SCORE)
        for k, rk in STAT_KEYS:
            assert st[k].shape == rs[rk].shape, k        # the model's own shape
        for k in ("start", "trans", "post"):
            np.testing.assert_allclose(st[k], rs[k], rtol=TOL_STAT, atol=TOL_STAT, err_msg=k)
        seen = rs["post_mix"] >= SEEN
        np.testing.assert_allclose(st["post_mix"][~seen], rs["post_mix"][~seen], rtol=0, atol=TOL_STAT)
        np.testing.assert_allclose(st["post_mix"][seen], rs["post_mix"][seen], rtol=TOL_STAT, atol=TOL_STAT)
        np.testing.assert_allclose(st["obs"][seen], rs["obs"][seen], rtol=TOL_STAT, atol=TOL_STAT)
        np.testing.assert_allclose(st["obs**2"][seen], rs["obs2"][seen], rtol=TOL_STAT, atol=TOL_STAT)
        for k, rk in STAT_KEYS:
            a, b = (st[k], rs[rk]) if k in ("start", "trans", "post") else (st[k][seen], rs[rk][seen])
            big = np.abs(b) >= SEEN
            rel = max(rel, _rel(a[big], b[big]))
            ab = max(ab, float(np.abs(a[~big] - b[~big]).max()) if (~big).any() else 0.0)
        # padding holds zeros exactly: whatever of the raw row split_stats does not hand out
        own = sum(v.size for k, v in st.items() if k not in ("nobs", "logprob")) + 2
        cov = _covered(S, M, D, c["params"][w][0].shape[0])
        assert own == int(cov.sum()) and cov.size == stats[w].size and not np.any(stats[w][~cov])
    figs["stats rel (|ref| >= 1e-6)"], figs["stats abs (|ref| < 1e-6)"] = rel, ab


def _check_viterbi(name, out, figs):
    c = sw.case(name)
    ref = sw.reference_viterbi(name)
    assert min(g for _, _, g in ref) > 1e-9           # a condition on the inputs (tests/test_gmmhmm_shapes_cpu.py)
    logprob, path = out
    want = np.array([r[0] for r in ref])
    figs["viterbi logprob rel"] = _rel(logprob, want)
    np.testing.assert_allclose(logprob, want, rtol=RTOL_SCORE)
    assert np.all(logprob[c["lengths"] == 0] == -np.inf)
    assert path.dtype == np.int32 and path.shape == (c["feats"].shape[0],)
    assert np.array_equal(path, np.concatenate([r[1] for r in ref]))


def _check_vocab(name, estep_loglik, vit_logprob, figs):
    """Both modes of the vocabulary launch over the case's models: the reference, the best word on every utterance,
    and every column bit for bit against the per-model entry points."""
    from sapr_amd import gmm_hmm as gh
    c = sw.case(name)
    N, W = len(c["lengths"]), len(c["params"])
    want = sw.reference_scores(name)
    vpack, pack = gh.GmmPack.from_params(c["params"]), _batch(name)[1]
    got = {}
    for mode in sw.MODES:
        vs = gh.vocab_scores(c["feats"], c["lengths"], vpack, mode=mode)
        sc, bw = vs.score.cpu().numpy(), vs.best_word.cpu().numpy()
        rsc, rbw = want[mode]
        assert sc.shape == (N, W) and sc.dtype == np.float64 and bw.dtype == np.int32
        figs[f"vocab {mode} rel"] = _rel(sc, rsc)
        np.testing.assert_allclose(sc, rsc, rtol=RTOL_SCORE)
        np.testing.assert_array_equal(bw, rbw)          # every utterance; -1 for the one without frames
        empty = c["lengths"] == 0
        assert np.all(sc[empty] == -np.inf) and np.all(bw[empty] == -1) and np.all(bw[~empty] >= 0)
        got[mode] = sc
    for w in range(W):
        batch = gh.GmmBatch(c["feats"], c["lengths"], np.full(N, w), W, c["S"], c["M"])
        loglik = batch.estep(pack, want_stats=False)[0].cpu().numpy()
        logprob = batch.viterbi(pack)[0].cpu().numpy()
        assert np.array_equal(got["forward"][:, w], loglik), (name, w, "forward")
        assert np.array_equal(got["viterbi"][:, w], logprob), (name, w, "viterbi")
        own = c["utt_model"] == w                       # and the case's own launch, where the utterance is the word's
        assert np.array_equal(loglik[own], estep_loglik[own]) and np.array_equal(logprob[own], vit_logprob[own])


def _check_all(name, sweep=False):
    batch, pack = _batch(name)
    figs = {}
    est = _host(batch.estep(pack, want_stats=True, want_post=True, want_path=True))
    _check_estep(name, est, figs)
    vit = _host(batch.viterbi(pack))
    _check_viterbi(name, vit, figs)
    _check_vocab(name, est[0], vit[0], figs)
    _note(figs, name, sweep)
    return est, vit


# ---- 1: the shape sweep -------------------------------------------------------------------------------------------------
def _sweep_id(k):
    S, M, D = sw.SHAPES[k]
    return f"{k:03d}-s{S}m{M}d{D}-{sw.sweep_topology(k)}"


@pytest.mark.parametrize("k", range(len(sw.SHAPES)), ids=_sweep_id)
def test_shape_sweep(k):
    from sapr_amd import gmm_hmm as gh
    name = sw.SWEEP[k]
    c = sw.case(name)
    S, M, D = sw.SHAPES[k]
    SP, MP, DP, _ = gh.pack_layout(S, M, D)
    assert (SP, MP, DP) == (S, M, D) if k < len(sw.TIGHT) else (S < SP or M < MP or D < DP)
    n0 = len(c["utts"][0])
    assert list(c["lengths"][n0 - 3:n0]) == [1, 2, 0]
    est, vit = _check_all(name, sweep=True)
    assert est[0][n0 - 1] == vit[0][n0 - 1] == -np.inf and np.isfinite(est[0][n0 - 3]) and np.isfinite(vit[0][n0 - 3])
    _batch.cache_clear()      # (the workspace of a case is not kept on the device)


def test_sweep_error_record():
    """The largest errors against the reference over the sweep cases that ran in this process."""
    for k, v in RECORD.items():
        print(f"sweep, largest {k}: {v:.3e}")


# ---- 2: ragged tiles and long utterances ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sw.RAGGED))
def test_ragged_tiles_and_long_utterances(name):
    c = sw.case(name)
    assert c["lengths"].max() == 1024 and len(c["params"]) == 3 and not np.any(c["utt_model"] == 2)
    est, _ = _check_all(name)
    stats = est[1]
    assert not np.any(stats[2])                         # the word without utterances: nobs 0 and an exact zero row
    assert stats[1][0] == 1.0 and stats[0][0] == len(sw.RAGGED_LENGTHS) - 1
    # each combination of outputs returns, for what it returns, the bits of the all-on run
    batch, pack = _batch(name)
    for flags in [(a, b, d) for a in (False, True) for b in (False, True) for d in (False, True)]:
        out = _host(batch.estep(pack, want_stats=flags[0], want_post=flags[1], want_path=flags[2]))
        assert np.array_equal(out[0], est[0]), flags
        for got, full, on in zip(out[1:], est[1:], flags):
            assert (got is not None) == on and (not on or np.array_equal(got, full)), flags
    _batch.cache_clear()


# ---- 3: many tiles ----------------------------------------------------------------------------------------------------
def test_many_tiles():
    from sapr_amd import gmm_hmm as gh
    name = "tiles"
    c = sw.case(name)
    S, M, D = c["S"], c["M"], c["D"]
    batch, pack = _batch(name)
    assert batch.layout.n_tiles == 10 and list(batch.layout.model_tile_off.cpu().numpy()) == [0, 1, 10]
    ref_stats, ref_utts = sw.reference_estep(name)
    loglik, stats, _, _ = _host(batch.estep(pack))
    figs = {"loglik rel": _rel(loglik, [r["loglik"] for r in ref_utts])}
    np.testing.assert_allclose(loglik, [r["loglik"] for r in ref_utts], rtol=RTOL_SCORE)
    for w, rs in enumerate(ref_stats):
        st = gh.split_stats(stats[w], S, M, D)
        assert st["nobs"] == rs["nobs"] == len(c["utts"][w])
        figs["logprob rel"] = max(figs.get("logprob rel", 0.0), _rel(st["logprob"], rs["logprob"]))
        np.testing.assert_allclose(st["logprob"], rs["logprob"], rtol=RTOL_SCORE)
        assert np.all(rs["post_mix"] >= SEEN)
        for k, rk in STAT_KEYS:
            figs["stats rel"] = max(figs.get("stats rel", 0.0), _rel(st[k], rs[rk]))
            np.testing.assert_allclose(st[k], rs[rk], rtol=TOL_STAT, atol=TOL_STAT, err_msg=k)
    _note(figs, name, False)
    again = _host(batch.estep(pack))                    # two runs: bit-equal
    assert np.array_equal(again[0], loglik) and np.array_equal(again[1], stats)
    sel = np.nonzero(c["utt_model"] == 1)[0]            # word 1 alone: its tiles start at tile 0 there
    one = gh.GmmBatch(np.concatenate(c["utts"][1], axis=0), c["lengths"][sel], np.zeros(sel.size, np.int64), 1, S, M)
    assert one.layout.n_tiles == 9
    l1, s1, _, _ = _host(one.estep(gh.pack_models([c["params"][1]])))
    assert np.array_equal(l1, loglik[sel]) and np.array_equal(s1[0], stats[1])
    _batch.cache_clear()


# ---- 4: degenerate but valid models -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sw.DEGENERATE)
def test_degenerate_models(name):
    from sapr_amd import gmm_hmm as gh
    c = sw.case(name)
    S, M, D = c["S"], c["M"], c["D"]
    est, _ = _check_all(name)
    loglik, stats, post, path = est
    if name == "zero_weight":                            # the component's cells: exactly 0.0
        for w in range(2):
            st = gh.split_stats(stats[w], S, M, D)
            assert not np.any(st["post_mix"][:, 1]) and not np.any(st["obs"][:, 1]) and not np.any(st["obs**2"][:, 1])
            assert np.all(st["post_mix"][:, [0, 2]] > 0)
    if name == "unreachable":                            # state 2: exactly 0.0 wherever it appears
        assert not np.any(post[:, 2]) and not np.any(path == 2)
        np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=TOL_STAT, atol=TOL_STAT)
        for w in range(2):
            st = gh.split_stats(stats[w], S, M, D)
            assert st["post"][2] == 0.0 and st["start"][2] == 0.0 and st["start"][1] == 0.0
            assert not np.any(st["trans"][2]) and not np.any(st["trans"][:, 2])
            assert not np.any(st["post_mix"][2]) and not np.any(st["obs"][2]) and not np.any(st["obs**2"][2])
    _batch.cache_clear()

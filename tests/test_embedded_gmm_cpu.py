"""CPU: the restatement of embedded Baum-Welch for Gaussian-mixture word models (tests/_embedded_gmm_ref.py) against
the enumeration of every path and against the isolated-word restatement, its host EM loop, the new symbols of the C ABI
with their size functions and refusals, and the refusals of the Python layer that come before a device is asked for."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _connected_family_cases as cases
from tests import _embedded_gmm_ref as mref
from tests import _gmmhmm_ref as gref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mixtures(rng, W, S, M, D):
    weights = rng.dirichlet(np.full(M, 5.0), (W, S))
    means = rng.normal(0.0, 4.0, (W, S, M, D))
    covars = rng.uniform(1.0, 9.0, (W, S, M, D))
    return weights, means, covars


# ---- the definition against the enumeration ---------------------------------------------------------------------
@pytest.mark.parametrize("exits", aref.EXITS)
@pytest.mark.parametrize("topology", aref.TOPOLOGIES)
def test_mixture_sums_equal_those_of_the_enumerated_posteriors(topology, exits):
    """W 2-3, S 1-2, M = 2, K 1-3, T <= 6, a non-zero word penalty for two of three K; the transcripts of K >= 2
    repeat a word.  ``logb`` is the mixtures' own emission, so that ``post_mix`` is a share of ``post``."""
    finite = 0
    for W in (2, 3):
        for S in (1, 2):
            for K in (1, 2, 3):
                rng = np.random.default_rng(2000 * W + 100 * S + 10 * K)
                pen = aref.PENALTIES[K % 3]
                ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
                weights, means, covars = _mixtures(rng, W, S, 2, 3)
                T = int(rng.integers(max(K, 3), 7))
                x = rng.normal(0.0, 4.0, (T, 3)).astype(np.float32)
                logb = mref.emit_gmm(x, weights, means, covars)
                words = rng.integers(0, W, K).tolist()
                if K >= 2:
                    words[-1] = words[0]                         # a word repeated in the transcript
                got = mref.estep_batch_gmm(logb, [T], [words], ls, lt, lx, pen, x, weights, means, covars)
                want = mref.brute_mix(logb, words, ls, lt, lx, pen, x, weights, means, covars)
                if not np.isfinite(got["loglik"][0]):
                    assert not any(got[k].any() for k in ("post_mix", "obs", "obs2"))
                    assert not any(a.any() for a in want)
                    continue
                finite += 1
                for key, exp in zip(("post_mix", "obs", "obs2"), want):
                    err = np.max(np.abs(got[key] - exp) / (1.0 + np.abs(exp)))
                    assert err <= 1e-12, (W, S, K, key, err)
                np.testing.assert_allclose(got["post_mix"].sum(axis=2), got["post_sum"], rtol=1e-12, atol=1e-13)
    assert finite >= 8                                           # (of the 12 cases; the rest have no path)


def test_a_switched_off_component_gets_exact_zeros_and_a_dead_state_no_nan():
    rng = np.random.default_rng(11)
    W, S, M, D = 2, 2, 3, 2
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    weights, means, covars = _mixtures(rng, W, S, M, D)
    weights[0, 1] = [0.25, 0.0, 0.75]                            # one component of weight exactly 0
    weights[1, 0] = 0.0                                          # a state with every component off: it emits -inf
    lengths, transcripts = [6, 5, 4], [[0, 1], [1, 0, 1], [0]]
    x = rng.normal(0.0, 4.0, (sum(lengths), D)).astype(np.float32)
    logb = mref.emit_gmm(x, weights, means, covars)
    assert np.isneginf(logb[:, 1, 0]).all()
    got = mref.estep_batch_gmm(logb, lengths, transcripts, ls, lt, lx, -1.0, x, weights, means, covars)
    assert np.isfinite(got["loglik"]).all()
    for key in ("post_mix", "obs", "obs2"):
        assert np.isfinite(got[key]).all(), key
        assert not got[key][0, 1, 1].any() and not got[key][1, 0].any(), key
    assert got["post_mix"][0, 1, 0] > 0 and got["post_mix"][0, 1, 2] > 0
    np.testing.assert_allclose(got["post_mix"].sum(axis=2), got["post_sum"], rtol=1e-12, atol=1e-13)


def test_a_pathless_utterance_adds_nothing():
    rng = np.random.default_rng(3)
    W, S, M, D = 2, 2, 2, 2
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    weights, means, covars = _mixtures(rng, W, S, M, D)
    x = rng.normal(0.0, 4.0, (9, D)).astype(np.float32)
    logb = mref.emit_gmm(x, weights, means, covars)
    both = mref.estep_batch_gmm(logb, [5, 1, 3], [[0, 1], [0, 1], [1]], ls, lt, lx, -1.0, x, weights, means, covars)
    assert both["loglik"][1] == NEG                              # (K > T in the middle)
    only = mref.estep_batch_gmm(np.delete(logb, 5, 0), [5, 3], [[0, 1], [1]], ls, lt, lx, -1.0, np.delete(x, 5, 0),
                                weights, means, covars)
    for key in ("nobs", "post_mix", "obs", "obs2"):
        assert np.array_equal(both[key], only[key]), key


def test_one_word_utterances_with_any_exit_equal_the_isolated_word_restatement():
    """K = 1 and every state an exit: the chain is the word model itself, and the rows are ``_gmmhmm_ref.estep``'s over
    the word's own utterances.  Short utterances: the two restatements form gamma differently (``exp(alpha + beta -
    loglik)`` here, a softmax there) and differ by about ulp(|loglik|) per posterior."""
    model, utts, _ = cases.gmm_case(208, 2, 3, 2, 2, 9)          # (seed, W, S, M, D, utterances)
    W, S = model["log_start"].shape
    rng = np.random.default_rng(5)
    utts = [u[:int(rng.integers(2, 7))] for u in utts]
    words = rng.integers(0, W, len(utts)).tolist()
    logb = mref.emit_gmm(np.concatenate(utts), model["weights"], model["means"], model["covars"])
    got = mref.estep_batch_gmm(logb, [len(u) for u in utts], [[w] for w in words], model["log_start"],
                               model["log_trans"], cases.log_exit(W, S, "any"), -3.0, np.concatenate(utts),
                               model["weights"], model["means"], model["covars"])
    for w in range(W):
        mine = [u for u, v in zip(utts, words) if v == w]
        st, res = gref.estep(mine, model["startprob"][w], model["transmat"][w], model["weights"][w], model["means"][w],
                             model["covars"][w])
        assert st["nobs"] == got["nobs"][w] == len(mine) and len(mine) >= 1
        np.testing.assert_allclose(got["loglik"][[v == w for v in words]], [r["loglik"] for r in res], rtol=1e-13)
        for key in ("post_mix", "obs", "obs2"):
            err = np.max(np.abs(got[key][w] - st[key]) / (1.0 + np.abs(st[key])))
            assert err <= 1e-12, (w, key, err)


# ---- the host EM loop ---------------------------------------------------------------------------------------------
def test_fit_gmm_does_not_decrease_the_likelihood():
    model, utts, truth = cases.gmm_case(*cases.GMM_DECODER_CASE)
    models = cases.models_of("gmm", model)
    before = [pickle.dumps(m) for m in models]
    trained, history = mref.fit_gmm(models, utts, truth, n_iter=3, tol=0.0)
    assert len(history) == 3 and history[0] <= history[1] <= history[2] and history[2] > history[0]
    assert [pickle.dumps(m) for m in models] == before           # (the caller's models are not touched)
    spoken = sorted({w for t in truth for w in t})
    for w in spoken:
        assert not np.array_equal(trained[w].means_, models[w].means_)
        np.testing.assert_allclose(trained[w].weights_.sum(axis=1), 1.0, rtol=1e-12)


def test_fit_gmm_leaves_a_word_in_no_transcript_untouched():
    model, utts, truth = cases.gmm_case(*cases.GMM_DECODER_CASE)
    models = cases.models_of("gmm", model)
    extra = cases.models_of("gmm", cases.gmm_case(*cases.GMM_DECODER_CASE[:5], 1)[0])[0]
    extra.means_ = extra.means_ + 100.0
    before = pickle.dumps(extra)
    trained, history = mref.fit_gmm(models + [extra], utts[:4], truth[:4], n_iter=1, tol=0.0)
    assert pickle.dumps(trained[-1]) == before and len(history) == 1


# ---- the C ABI ------------------------------------------------------------------------------------------------------
NEW = {"sapr_connected_embed_gmm_stats_width": 4, "sapr_connected_embed_gmm_workspace_bytes": 9,
       "sapr_connected_embed_gmm": 24}


def test_new_symbols_are_declared_bound_and_exported():
    import sapr_amd
    from sapr_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sapr_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, arity in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    # the arguments of sapr_connected_embed[_full] in their order, with (pack, M) behind D
    sig, base = _lib.SIGNATURES["sapr_connected_embed_gmm"][1], _lib.SIGNATURES["sapr_connected_embed_full"][1]
    assert sig[:3] == base[:3] and sig[3:5] == [C.c_void_p, C.c_int32] and sig[5:] == base[3:]
    for name in ("embed_gmm_stats_width", "embed_gmm_workspace_bytes"):
        assert getattr(sapr_amd, name) is getattr(sapr_amd.connected, name)
    fields = sapr_amd.EmbeddedStats.__dataclass_fields__
    assert fields["M"].default == 0 and fields["layout"].default == "diag"


def test_size_functions_and_refusals():
    from sapr_amd import _lib
    from sapr_amd.gmm_hmm import stats_width
    lib = _lib.load()
    n, m, w = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    for S, M, D in ((3, 1, 1), (10, 2, 13), (7, 3, 26), (18, 8, 39)):
        assert lib.sapr_connected_embed_gmm_stats_width(S, M, D, C.byref(w)) == 0
        assert w.value == stats_width(S, M, D) == 2 + S + S * S + S + S * M * (2 * D + 1)
    assert lib.sapr_connected_embed_gmm_stats_width(19, 2, 13, C.byref(w)) == -2
    assert lib.sapr_connected_embed_gmm_stats_width(10, 9, 13, C.byref(w)) == -2
    assert lib.sapr_connected_embed_gmm_stats_width(10, 2, 40, C.byref(w)) == -2
    assert lib.sapr_connected_embed_gmm_stats_width(0, 2, 13, C.byref(w)) == -1
    assert lib.sapr_connected_embed_gmm_stats_width(10, 0, 13, C.byref(w)) == -1
    assert lib.sapr_connected_embed_gmm_stats_width(10, 2, 13, None) == -1
    # what sapr_connected_embed takes at D = 0, W heads, and one partial row per (group of 8 utterances, word; at most
    # 96 groups): the groups of sapr_connected_embed_full
    for n_utts, groups in ((7, 1), (8, 1), (9, 2), (32, 4), (768, 96), (769, 86), (3073, 94), (10000, 96)):
        assert lib.sapr_connected_embed_workspace_bytes(1000, n_utts, 35, 5, 10, 0, C.byref(m)) == 0
        assert lib.sapr_connected_embed_gmm_workspace_bytes(1000, n_utts, 35, 5, 11, 10, 2, 13, C.byref(n)) == 0
        head = 8 * 11 * (2 + 10 + 100 + 10)
        assert n.value == m.value + (head + 15) // 16 * 16 + 8 * groups * 11 * (10 * 2 * 27), n_utts
    # unsupported: S = 19, M = 9, D = 40, max_words * SP = 260, W * SP = 260
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 2, 19, 2, 13, C.byref(n)) == -2
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 2, 10, 9, 13, C.byref(n)) == -2
    assert b"M in 1..8" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 2, 10, 2, 40, C.byref(n)) == -2
    assert b"D in 0..39" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 26, 26, 2, 10, 2, 13, C.byref(n)) == -2
    assert b"max_words * SP" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 26, 10, 2, 13, C.byref(n)) == -2
    assert lib.sapr_connected_embed_gmm_workspace_bytes(-1, 1, 2, 2, 2, 4, 2, 1, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 0, 4, 2, 1, C.byref(n)) == -1
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 2, 4, 0, 1, C.byref(n)) == -1
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 2, 4, 2, 1, None) == -1

    def call(D, M, n_utts, total, total_words, max_words, W, S, stats=None, ws=None, ws_bytes=0, feats=None,
             pack=None):
        return lib.sapr_connected_embed_gmm(None, feats, D, pack, M, None, n_utts, total, None, None, total_words,
                                            max_words, None, None, None, 0.0, W, S, ws, ws_bytes, None, stats, None,
                                            None)

    assert call(1, 2, 1, 10, 26, 26, 2, 10) == -2
    assert call(1, 2, 1, 10, 2, 2, 26, 10) == -2
    assert call(40, 2, 1, 10, 2, 2, 2, 10) == -2
    assert call(1, 9, 1, 10, 2, 2, 2, 10) == -2
    assert call(1, 2, 1, 10, -1, 2, 2, 4) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert call(1, 0, 1, 10, 2, 2, 2, 4) == -1
    assert call(1, 2, 1, 10, 2, 2, 2, 4) == -1
    assert b"workspace too small" in lib.sapr_last_error()
    # (host memory stands in for the buffers: every refusal below comes before anything is launched or read)
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 2, 4, 2, 0, C.byref(n)) == 0
    buf, row = C.create_string_buffer(n.value), (C.c_double * 64)()
    assert call(0, 2, 1, 10, 2, 2, 2, 4, stats=row, ws=buf, ws_bytes=n.value) == -1
    assert b"D >= 1" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_gmm_workspace_bytes(10, 1, 2, 2, 2, 4, 2, 1, C.byref(n)) == 0
    buf, some = C.create_string_buffer(n.value), (C.c_double * 8)()
    assert call(1, 2, 1, 10, 2, 2, 2, 4, stats=row, ws=buf, ws_bytes=n.value, feats=some) == -1
    assert b"pack" in lib.sapr_last_error()
    assert call(1, 2, 1, 10, 2, 2, 2, 4, stats=row, ws=buf, ws_bytes=n.value, pack=some) == -1
    assert b"NULL" in lib.sapr_last_error()
    assert call(1, 2, 0, 0, 0, 2, 2, 4, ws=buf, ws_bytes=n.value) == 0


# ---- the Python layer ---------------------------------------------------------------------------------------------
class _Pack:
    """As much of a ``GmmPack`` as ``ConnectedNetwork`` and the refusals look at."""
    W, S, D, M = 3, 7, 2, 2


def _networks():
    from sapr_amd.connected import ConnectedNetwork
    z = np.zeros((3, 7))
    diag = ConnectedNetwork(z, np.zeros((3, 7, 7)), z)
    gmm = ConnectedNetwork(z, np.zeros((3, 7, 7)), z, family="gmm", pack=_Pack())
    full = ConnectedNetwork(z, np.zeros((3, 7, 7)), z, family="full", pack=_Pack())
    return diag, gmm, full


def test_the_switch_is_refused_where_it_does_not_apply_before_a_device_is_asked_for():
    from sapr_amd.connected import embedded_estep, embedded_forward_backward
    diag, gmm, full = _networks()
    x = np.zeros((8, 2), np.float32)
    utts, logb = [x[:5], x[5:]], np.zeros((8, 3, 7))
    tr = [[0, 1], [2]]
    for net in (diag, full):
        with pytest.raises(ValueError, match="mixtures=True serves a network of the 'gmm' family"):
            embedded_estep(utts, tr, net, mixtures=True)
        with pytest.raises(ValueError, match="mixtures=True serves a network of the 'gmm' family"):
            embedded_forward_backward(logb, [5, 3], tr, net, feats=x, mixtures=True)
    with pytest.raises(ValueError, match="exclude each other"):
        embedded_estep(utts, tr, gmm, mixtures=True, second_moments=True)
    with pytest.raises(ValueError, match="exclude each other"):
        embedded_forward_backward(logb, [5, 3], tr, gmm, feats=x, mixtures=True, second_moments=True)
    with pytest.raises(ValueError, match="needs the frames"):
        embedded_forward_backward(logb, [5, 3], tr, gmm, mixtures=True)
    # the transcripts come first
    for call in (lambda t: embedded_estep(utts, t, diag, mixtures=True),
                 lambda t: embedded_forward_backward(logb, [5, 3], t, gmm, feats=x, mixtures=True,
                                                     second_moments=True)):
        with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
            call([[0]])
        with pytest.raises(ValueError, match="outside the vocabulary"):
            call([[0, 3], [1]])
        with pytest.raises(ValueError, match=r"K \* SP = 260 exceeds the limit of 256"):
            call([[0] * 26, [1]])


def test_without_the_switch_mixtures_are_refused_as_before():
    from sapr_amd.connected import embedded_estep
    _, gmm, _ = _networks()
    utts = [np.zeros((5, 2), np.float32)]
    with pytest.raises(NotImplementedError, match="'gmm'") as err:
        embedded_estep(utts, [[0, 1]], gmm)
    assert "mixture responsibilities" in str(err.value) and "mixtures=True" in str(err.value)
    with pytest.raises(NotImplementedError, match="mixture responsibilities") as err:
        embedded_estep(utts, [[0, 1]], gmm, second_moments=True)
    assert "'gmm'" in str(err.value)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        embedded_estep(utts, [[5]], gmm)


def test_embedded_fit_refusals_before_a_device_is_asked_for():
    from sapr_amd.connected import embedded_fit
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    model, utts, truth = cases.gmm_case(*cases.GMM_DECODER_CASE)
    models = cases.models_of("gmm", model)
    before = [pickle.dumps(m) for m in models]
    g = GaussianHMM(n_components=5, covariance_type="diag")
    g.startprob_, g.transmat_ = model["startprob"][0], model["transmat"][0]
    g.means_, g._covars_ = model["means"][0][:, 0], model["covars"][0][:, 0]
    with pytest.raises(ValueError, match="is not a GMMHMM"):
        embedded_fit(models[:2] + [g], utts[:1], [[0, 1]])
    with pytest.raises(ValueError, match="is not a GMMHMM"):
        embedded_fit([g] + models[:2], utts[:1], [[0, 1]], second_moments=True)
    with pytest.raises(ValueError, match="second_moments=True serves GaussianHMM"):
        embedded_fit(models, utts[:1], [[0, 1]], second_moments=True)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        embedded_fit(models, utts[:1], [[0, 4]])
    with pytest.raises(ValueError, match="is empty"):
        embedded_fit(models, utts[:1], [[]])
    with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
        embedded_fit(models, utts[:2], [[0]])
    other = cases.models_of("gmm", cases.gmm_case(206, 1, 5, 3, 13, 1)[0])     # another n_mix
    with pytest.raises(ValueError, match="share n_mix"):
        embedded_fit(models + other, utts[:1], [[0, 1]])
    assert [pickle.dumps(m) for m in models] == before           # (nothing was noted on the caller's objects)


def test_decoder_train_embedded_still_refuses_custom(tmp_path):
    from sapr_amd.decoder import Decoder
    d = tmp_path / "trained_models" / "custom"
    d.mkdir(parents=True)
    with open(d / "zero_custom_15.pkl", "wb") as f:
        pickle.dump({"placeholder": "custom"}, f)
    with pytest.raises(ValueError, match="implementation='custom'"):
        Decoder(models_dir=str(tmp_path / "trained_models"), implementation="custom").train_embedded(
            [np.zeros((13, 4), np.float32)], [["zero"]])


def test_embedded_stats_split_of_the_gmm_layout():
    from sapr_amd.connected import EmbeddedStats
    from sapr_amd.gmm_hmm import stats_width
    S, SP, M, D = 3, 4, 2, 2
    width = stats_width(S, M, D)
    stats = np.arange(2 * width, dtype=np.float64).reshape(2, -1)
    res = EmbeddedStats(loglik=np.array([-1.0]), stats=stats, post=None, offsets=np.array([0, 3]),
                        word_offsets=np.array([0, 2]), words=np.array([1, 0], np.int32), S=S, SP=SP, D=D,
                        n_states=(3, 2), layout="gmm", M=M)
    st = res.split(1)
    assert st["nobs"] == stats[1, 0] and st["start"].shape == (2,) and st["trans"].shape == (2, 2)
    assert st["post"].shape == (2,) and st["post_mix"].shape == (2, M)
    assert st["obs"].shape == (2, M, D) and st["obs**2"].shape == (2, M, D) and "obs*obs.T" not in st
    o = 2 + S + S * S + S
    whole = res.split(0)
    assert np.array_equal(whole["post_mix"], stats[0, o:o + S * M].reshape(S, M))
    assert np.array_equal(whole["obs"], stats[0, o + S * M:o + S * M + S * M * D].reshape(S, M, D))
    assert np.array_equal(whole["obs**2"], stats[0, o + S * M + S * M * D:].reshape(S, M, D))
    assert np.array_equal(st["obs**2"], stats[1, o + S * M + S * M * D:].reshape(S, M, D)[:2])

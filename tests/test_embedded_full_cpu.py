"""CPU: the restatement of embedded Baum-Welch with second-moment matrices (tests/_embedded_full_ref.py) against the
enumeration of every path, its host EM loop over a mixed vocabulary, the new symbols of the C ABI with their size
functions and refusals, and the refusals of the Python layer that come before a device is asked for."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _embedded_full_ref as fref
from tests import _embedded_ref as eref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("exits", aref.EXITS)
@pytest.mark.parametrize("topology", aref.TOPOLOGIES)
def test_moments_equal_those_of_the_enumerated_posteriors(topology, exits):
    """W 2-3, S 2-3, K 1-3, T <= 6: ``obs`` and ``oo`` equal the sums built from the posteriors of the path
    enumeration; ``oo`` is symmetric; its diagonal is ``obs2`` up to the rounding of the float32 square (2^-24
    relative per term, every term being non-negative)."""
    finite = 0
    for W in (2, 3):
        for S in (2, 3):
            for K in (1, 2, 3):
                rng = np.random.default_rng(1000 * W + 100 * S + 10 * K)
                pen = aref.PENALTIES[K % 3]
                ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
                T = int(rng.integers(max(K, 3), 7))
                logb = rng.normal(-5.0, 3.0, (T, W, S))
                x = rng.normal(0.0, 4.0, (T, 3)).astype(np.float32)
                words = rng.integers(0, W, K).tolist()
                got = fref.estep_batch_full(logb, [T], [words], ls, lt, lx, pen, x)
                obs, oo = fref.brute_moments(logb, words, ls, lt, lx, pen, x, W)
                if not np.isfinite(got["loglik"][0]):
                    assert not got["oo"].any() and not oo.any()
                    continue
                finite += 1
                np.testing.assert_allclose(got["obs"], obs, rtol=0, atol=1e-11)
                np.testing.assert_allclose(got["oo"], oo, rtol=0, atol=1e-10)
                assert np.array_equal(got["oo"], np.swapaxes(got["oo"], 2, 3))
                diag = np.diagonal(got["oo"], axis1=2, axis2=3)
                np.testing.assert_allclose(diag, got["obs2"], rtol=2.0 ** -23, atol=1e-300)
    assert finite >= 8                                           # (of the 12 cases; the rest have no path)


def test_a_pathless_utterance_adds_nothing():
    rng = np.random.default_rng(3)
    W, S = 2, 2
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    logb = rng.normal(-5.0, 3.0, (9, W, S))
    x = rng.normal(0.0, 4.0, (9, 2)).astype(np.float32)
    both = fref.estep_batch_full(logb, [5, 1, 3], [[0, 1], [0, 1], [1]], ls, lt, lx, -1.0, x)     # (K > T in the middle)
    assert both["loglik"][1] == NEG
    only = fref.estep_batch_full(np.delete(logb, 5, 0), [5, 3], [[0, 1], [1]], ls, lt, lx, -1.0, np.delete(x, 5, 0))
    for key in ("nobs", "obs", "oo"):
        assert np.array_equal(both[key], only[key]), key


# ---- the host EM loop over a mixed vocabulary -----------------------------------------------------------------
def mixed_vocabulary(S=3, D=3, seed=9, n_utts=10):
    """Words "diag", "full", "tied", and one ("spherical") in no transcript; short recordings of 2-3 words."""
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    rng = np.random.default_rng(seed)
    types = ["diag", "full", "tied", "spherical"]
    centres = rng.normal(0.0, 6.0, (4, S, D))
    utts, truth = [], []
    for _ in range(n_utts):
        words = rng.integers(0, 3, int(rng.integers(2, 4))).tolist()
        utts.append(np.concatenate([np.repeat(centres[w], int(rng.integers(2, 4)), axis=0) for w in words])
                    .astype(np.float32) + rng.normal(0.0, 1.0, (1, D)).astype(np.float32))
        utts[-1] += rng.normal(0.0, 1.0, utts[-1].shape).astype(np.float32)
        truth.append(words)
    tm = np.zeros((S, S))
    for i in range(S):
        tm[i, i] = 0.6 if i + 1 < S else 1.0
        if i + 1 < S:
            tm[i, i + 1] = 0.4
    models = []
    for w, ct in enumerate(types):
        m = GaussianHMM(n_components=S, covariance_type=ct)
        m.startprob_ = np.r_[1.0, np.zeros(S - 1)]
        m.transmat_ = tm.copy()
        m.means_ = centres[w] + rng.normal(0.0, 1.0, (S, D))
        m._covars_ = {"diag": np.full((S, D), 9.0), "spherical": np.full(S, 9.0), "tied": 9.0 * np.eye(D),
                      "full": np.tile(9.0 * np.eye(D), (S, 1, 1))}[ct]
        models.append(m)
    return models, utts, truth


def test_fit_full_on_a_mixed_vocabulary():
    models, utts, truth = mixed_vocabulary()
    before = pickle.dumps(models[3])
    trained, history = fref.fit_full(models, utts, truth, n_iter=3, tol=0.0)
    assert len(history) == 3 and history[-1] > history[0]
    S, D = 3, 3
    assert trained[0]._covars_.shape == (S, D) and trained[1]._covars_.shape == (S, D, D)
    assert trained[2]._covars_.shape == (D, D) and trained[3]._covars_.shape == (S,)
    for m in trained[1:3]:
        cv = np.asarray(m._covars_)
        assert np.array_equal(cv, np.swapaxes(cv, -1, -2))
        np.linalg.cholesky(cv)
    for w in range(3):
        assert not np.array_equal(trained[w].means_, models[w].means_)
    assert pickle.dumps(trained[3]) == before                     # the word in no transcript keeps its bytes
    assert pickle.dumps(models[3]) == before                      # (and the caller's models are not touched)


def test_all_diagonal_vocabulary_differs_from_the_diagonal_route_by_the_float32_square_only():
    """The documented difference: on an all-diagonal vocabulary ``fit_full`` reads ``diag(oo)`` (float64 squares),
    ``_embedded_ref.fit`` the float32 squares; the emission is the Cholesky form in one and the diagonal form in the
    other.  Both are float64 roundings of the same quantities."""
    models, utts, truth = mixed_vocabulary()
    for m in models:
        if m.covariance_type in ("full", "tied"):
            m.covariance_type, m._covars_ = "diag", np.full((3, 3), 9.0)
    a, ha = fref.fit_full(models, utts, truth, n_iter=2, tol=0.0)
    b, hb = eref.fit(models, utts, truth, n_iter=2, tol=0.0)
    np.testing.assert_allclose(ha, hb, rtol=1e-6)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x._covars_, y._covars_, rtol=1e-5)


# ---- the C ABI --------------------------------------------------------------------------------------------------
NEW = {"sapr_connected_embed_full_stats_width": 3, "sapr_connected_embed_full_workspace_bytes": 8,
       "sapr_connected_embed_full": 22}


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
    assert _lib.SIGNATURES["sapr_connected_embed_full"] == _lib.SIGNATURES["sapr_connected_embed"]
    assert lib.sapr_abi_version() == 2
    for name in ("embed_full_stats_width", "embed_full_workspace_bytes"):
        assert getattr(sapr_amd, name) is getattr(sapr_amd.connected, name)
    assert "layout" in sapr_amd.EmbeddedStats.__dataclass_fields__


def test_size_functions_and_refusals():
    from sapr_amd import _lib
    from sapr_amd.full_cov import stats_width
    lib = _lib.load()
    n, m, w = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    for S, D in ((3, 1), (10, 13), (18, 39)):
        assert lib.sapr_connected_embed_full_stats_width(S, D, C.byref(w)) == 0
        assert w.value == stats_width(S, D) == 2 + S + S * S + S + S * D + S * D * D
    assert lib.sapr_connected_embed_full_stats_width(19, 13, C.byref(w)) == -2
    assert lib.sapr_connected_embed_full_stats_width(10, 40, C.byref(w)) == -2
    assert lib.sapr_connected_embed_full_stats_width(0, 13, C.byref(w)) == -1
    assert lib.sapr_connected_embed_full_stats_width(10, 13, None) == -1
    # what sapr_connected_embed takes at D = 0, W heads, and one partial row per (group of 8 utterances, word; at most 96 groups)
    for n_utts, groups in ((7, 1), (8, 1), (9, 2), (32, 4), (768, 96), (769, 86), (3073, 94), (10000, 96)):
        assert lib.sapr_connected_embed_workspace_bytes(1000, n_utts, 35, 5, 10, 0, C.byref(m)) == 0
        assert lib.sapr_connected_embed_full_workspace_bytes(1000, n_utts, 35, 5, 11, 10, 13, C.byref(n)) == 0
        head = 8 * 11 * (2 + 10 + 100 + 10)
        assert n.value == m.value + (head + 15) // 16 * 16 + 8 * groups * 11 * (10 * 13 + 10 * 13 * 13), n_utts
    assert lib.sapr_connected_embed_full_workspace_bytes(0, 0, 0, 1, 1, 1, 1, C.byref(n)) == 0 and n.value == 48
    # unsupported: S = 19, D = 40, max_words * SP = 260, W * SP = 260
    assert lib.sapr_connected_embed_full_workspace_bytes(10, 1, 2, 2, 2, 19, 13, C.byref(n)) == -2
    assert lib.sapr_connected_embed_full_workspace_bytes(10, 1, 2, 2, 2, 10, 40, C.byref(n)) == -2
    assert b"D in 0..39" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_full_workspace_bytes(10, 1, 26, 26, 2, 10, 13, C.byref(n)) == -2
    assert b"max_words * SP" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_full_workspace_bytes(10, 1, 2, 2, 26, 10, 13, C.byref(n)) == -2
    assert lib.sapr_connected_embed_full_workspace_bytes(-1, 1, 2, 2, 2, 4, 1, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_full_workspace_bytes(10, 1, 2, 2, 0, 4, 1, C.byref(n)) == -1
    assert lib.sapr_connected_embed_full_workspace_bytes(10, 1, 2, 2, 2, 4, 1, None) == -1

    def call(D, n_utts, total, total_words, max_words, W, S, stats=None, ws=None, ws_bytes=0):
        return lib.sapr_connected_embed_full(None, None, D, None, n_utts, total, None, None, total_words, max_words,
                                             None, None, None, 0.0, W, S, ws, ws_bytes, None, stats, None, None)

    assert call(1, 1, 10, 26, 26, 2, 10) == -2
    assert call(1, 1, 10, 2, 2, 26, 10) == -2
    assert call(40, 1, 10, 2, 2, 2, 10) == -2
    assert call(1, 1, 10, -1, 2, 2, 4) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert call(1, 1, 10, 2, 2, 2, 4) == -1
    assert b"workspace too small" in lib.sapr_last_error()
    # (host memory stands in for the buffers: every refusal below comes before anything is launched or read)
    assert lib.sapr_connected_embed_full_workspace_bytes(10, 1, 2, 2, 2, 4, 0, C.byref(n)) == 0
    buf, row = C.create_string_buffer(n.value), (C.c_double * 64)()
    assert call(0, 1, 10, 2, 2, 2, 4, stats=row, ws=buf, ws_bytes=n.value) == -1
    assert b"D >= 1" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_full_workspace_bytes(10, 1, 2, 2, 2, 4, 1, C.byref(n)) == 0
    buf = C.create_string_buffer(n.value)
    assert call(1, 1, 10, 2, 2, 2, 4, stats=row, ws=buf, ws_bytes=n.value) == -1
    assert b"NULL" in lib.sapr_last_error()
    assert call(1, 0, 0, 0, 2, 2, 4, ws=buf, ws_bytes=n.value) == 0


# ---- the Python layer ---------------------------------------------------------------------------------------------
def test_python_layer_refuses_bad_transcripts_before_a_device_is_asked_for():
    from sapr_amd.connected import ConnectedNetwork, embedded_estep, embedded_forward_backward
    W, S = 3, 7                                  # SP = 10: at most 25 words
    z = np.zeros((W, S))
    net = ConnectedNetwork(z, np.zeros((W, S, S)), z)
    logb = np.zeros((8, W, S))
    x = np.zeros((8, 2), np.float32)
    utts = [x[:5], x[5:]]
    for call in (lambda tr: embedded_forward_backward(logb, [5, 3], tr, net, feats=x, second_moments=True),
                 lambda tr: embedded_estep(utts, tr, net, second_moments=True)):
        with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
            call([[0]])
        with pytest.raises(ValueError, match="utterance 1 is empty"):
            call([[0], []])
        with pytest.raises(ValueError, match="outside the vocabulary"):
            call([[0, 3], [1]])
        with pytest.raises(ValueError, match=r"K \* SP = 260 exceeds the limit of 256"):
            call([[0] * 26, [1]])
    with pytest.raises(ValueError, match="needs the frames"):
        embedded_forward_backward(logb, [5, 3], [[0], [1]], net, second_moments=True)


class _Pack:
    """As much of a ``VocabPack`` as ``ConnectedNetwork`` looks at."""
    W, S, D = 3, 7, 2


def test_mixtures_are_still_refused_and_the_default_still_refuses_full():
    from sapr_amd.connected import ConnectedNetwork, embedded_estep
    z = np.zeros((3, 7))
    utts = [np.zeros((5, 2), np.float32)]
    gmm = ConnectedNetwork(z, np.zeros((3, 7, 7)), z, family="gmm", pack=_Pack())
    with pytest.raises(NotImplementedError, match="mixture responsibilities"):
        embedded_estep(utts, [[0, 1]], gmm, second_moments=True)
    with pytest.raises(ValueError, match="outside the vocabulary"):      # (the transcripts come first)
        embedded_estep(utts, [[5]], gmm, second_moments=True)
    full = ConnectedNetwork(z, np.zeros((3, 7, 7)), z, family="full", pack=_Pack())
    with pytest.raises(NotImplementedError, match="'full'"):
        embedded_estep(utts, [[0, 1]], full)
    with pytest.raises(NotImplementedError, match="'full'"):
        embedded_estep(utts, [[0, 1]], full, second_moments=False)


def test_embedded_fit_refusals_before_a_device_is_asked_for():
    from sapr_amd.connected import embedded_fit
    models, utts, _ = mixed_vocabulary()
    with pytest.raises(ValueError, match="'full' or 'tied'") as err:
        embedded_fit(models[:2], utts[:1], [[0, 1]])
    assert "second_moments=True" in str(err.value)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        embedded_fit(models, utts[:1], [[0, 4]], second_moments=True)
    with pytest.raises(ValueError, match="is empty"):
        embedded_fit(models, utts[:1], [[]], second_moments=True)
    with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
        embedded_fit(models, utts[:2], [[0]], second_moments=True)


def test_embedded_stats_split_by_layout():
    from sapr_amd.connected import EmbeddedStats
    from sapr_amd.full_cov import stats_width
    S, SP, D = 3, 4, 2
    stats = np.arange(2 * stats_width(S, D), dtype=np.float64).reshape(2, -1)
    res = EmbeddedStats(loglik=np.array([-1.0]), stats=stats, post=None, offsets=np.array([0, 3]),
                        word_offsets=np.array([0, 2]), words=np.array([1, 0], np.int32), S=S, SP=SP, D=D,
                        n_states=(3, 2), layout="full")
    st = res.split(1)
    assert st["nobs"] == stats[1, 0] and st["start"].shape == (2,) and st["trans"].shape == (2, 2)
    assert st["obs"].shape == (2, D) and st["obs*obs.T"].shape == (2, D, D) and "obs**2" not in st
    o = 2 + S + S * S + S
    assert np.array_equal(res.split(0)["obs*obs.T"], stats[0, o + S * D:].reshape(S, D, D))
    assert EmbeddedStats.__dataclass_fields__["layout"].default == "diag"

"""CPU: the embedded Baum-Welch restatement (tests/_embedded_ref.py) against an exhaustive enumeration of every path,
the invariants of the definition, its tie to the isolated-word forward-backward, the new symbols of the C ABI with
their size function and refusals, and the refusals of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _embedded_ref as eref
from tests import _fb_ref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("exits", aref.EXITS)
@pytest.mark.parametrize("topology", aref.TOPOLOGIES)
def test_restatement_equals_exhaustive_enumeration(topology, exits):
    """W 2-3, S 2-3, K 1-3, T <= 6, real-valued tables, every penalty: likelihood, posteriors, expected entries and
    expected transitions equal the sums over all paths to 1e-12."""
    finite = 0
    for W in (2, 3):
        for S in (2, 3):
            for K in (1, 2, 3):
                for pen in aref.PENALTIES:
                    rng = np.random.default_rng(1000 * W + 100 * S + 10 * K + int(abs(pen)))
                    ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
                    T = int(rng.integers(max(K, 3), 7))
                    logb = rng.normal(-5.0, 3.0, (T, W, S))
                    words = rng.integers(0, W, K).tolist()
                    got = eref.forward_backward(logb, words, ls, lt, lx, pen)
                    want = eref.brute(logb, words, ls, lt, lx, pen)
                    if not np.isfinite(want["loglik"]):
                        assert got["loglik"] == NEG and not got["gamma"].any() and not got["trans"].any()
                        continue
                    finite += 1
                    assert abs(got["loglik"] - want["loglik"]) <= 1e-12 * max(1.0, abs(want["loglik"]))
                    for key in ("gamma", "start", "trans"):
                        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=1e-12, err_msg=key)
    assert finite >= 30


def test_restatement_without_a_path():
    z = np.zeros((2, 1))
    lt = np.zeros((2, 1, 1))
    for logb, words in ((np.zeros((0, 2, 1)), [0]), (np.zeros((3, 2, 1)), []), (np.zeros((2, 2, 1)), [0, 1, 0]),
                        (np.zeros((3, 2, 1)), [0, 2]), (np.zeros((3, 2, 1)), [-1])):
        r = eref.forward_backward(logb, words, z, lt, z, 0.0)
        assert r["loglik"] == NEG and not r["gamma"].any() and not r["start"].any() and not r["trans"].any()
    nan = np.zeros((4, 2, 1))
    nan[2] = np.nan
    r = eref.estep_batch(np.concatenate([nan, np.zeros((4, 2, 1))]), [4, 4], [[0, 1], [1, 1]], z, lt, z, 0.0)
    assert np.isnan(r["loglik"][0]) and np.isfinite(r["loglik"][1])
    assert not r["post"][:4].any() and r["nobs"].tolist() == [0, 2] and np.isfinite(r["trans"]).all()
    # sized for fewer words than the transcript has: no path
    r = eref.estep_batch(np.zeros((4, 2, 1)), [4], [[0, 1, 0]], z, lt, z, 0.0, max_words=2)
    assert r["loglik"][0] == NEG and not r["nobs"].any()


CASES = [(3, 4, "skip", "last"), (5, 7, "dense", "any"), (11, 10, "bidiag", "last")]
LENGTHS = [3, 24, 1, 30, 0, 17, 2, 12]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "-".join(str(v) for v in c))
def batch(request):
    """Short utterances with emission scores around -5: a posterior is exp(alpha + beta - loglik), whose argument
    carries a rounding error of about ulp(|loglik|) per frame of the recursion.  With T <= 30 and |loglik| below about
    250 (ulp 2.8e-14) that stays below the 1e-12 the invariants are held to; at the magnitudes of
    ``_align_ref.recursion_case`` (|loglik| in the thousands) float64 itself does not reach 1e-12.  K = T + 1 at the
    1- and 2-frame utterances and the empty utterance have no path."""
    W, S, topology, exits = request.param
    rng = np.random.default_rng(100 * W + S)
    ls, lt, lx = aref.network(rng, W, S, topology, exits, False)
    logb = rng.normal(-5.0, 3.0, (sum(LENGTHS), W, S))
    transcripts = [rng.integers(0, W, T + 1 if T in (1, 2) else max(1, T // (S + 1))).tolist() for T in LENGTHS]
    feats = rng.normal(0.0, 3.0, (logb.shape[0], 3)).astype(np.float32)
    res = {pen: eref.estep_batch(logb, LENGTHS, transcripts, ls, lt, lx, pen, feats) for pen in (0.0, -20.0)}
    return W, S, LENGTHS, transcripts, res


def test_invariants_of_the_definition(batch):
    W, S, lengths, transcripts, res = batch
    r = res[0.0]
    offs = np.r_[0, np.cumsum(lengths)]
    ok = np.isfinite(r["loglik"])
    assert ok.sum() >= 4 and not ok[[2, 4, 6]].any()
    count = np.zeros(W)
    frames = 0
    for u in range(len(lengths)):
        rows = r["post"][offs[u]:offs[u + 1]].sum(axis=(1, 2))
        if ok[u]:
            np.testing.assert_allclose(rows, 1.0, rtol=0, atol=1e-12)
            frames += lengths[u]
            for w in transcripts[u]:
                count[w] += 1
        else:
            assert not rows.any()
    np.testing.assert_array_equal(r["nobs"], count)
    np.testing.assert_allclose(r["start"].sum(axis=1), count, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["post"].sum(), frames, rtol=1e-12)
    np.testing.assert_allclose(r["post_sum"].sum(), frames, rtol=1e-12)
    # every frame but a slot's first is reached by a transition inside the slot
    np.testing.assert_allclose(r["trans"].sum() + r["start"].sum(), frames, rtol=1e-12)


def test_word_penalty_shifts_the_likelihood_and_nothing_else(batch):
    W, S, lengths, transcripts, res = batch
    a, b = res[0.0], res[-20.0]
    ok = np.isfinite(a["loglik"])
    assert np.array_equal(ok, np.isfinite(b["loglik"]))
    K = np.array([len(t) for t in transcripts])
    np.testing.assert_allclose(b["loglik"][ok], a["loglik"][ok] + (K[ok] - 1) * -20.0, rtol=1e-12)
    for key in ("post", "nobs", "start", "trans", "post_sum", "obs", "obs2"):
        np.testing.assert_allclose(b[key], a[key], rtol=1e-9, atol=1e-9, err_msg=key)


def test_one_word_with_any_exit_is_the_isolated_word_forward_backward():
    """K = 1 and ``exit_states="any"`` (log_exit 0 everywhere): the chain is the word model itself, and the statistics
    are those of hmmlearn's E-step (tests/_fb_ref.py, longdouble) over the same frames."""
    rng = np.random.default_rng(11)
    W, S, D = 3, 4, 5
    sp = rng.dirichlet(np.ones(S), W)
    A = rng.dirichlet(np.ones(S), (W, S))
    mu = rng.normal(0.0, 3.0, (W, S, D))
    cv = rng.uniform(0.5, 2.0, (W, S, D))
    lengths = [7, 1, 30]
    words = [[2], [0], [2]]
    feats = rng.normal(0.0, 3.0, (sum(lengths), D)).astype(np.float32)
    gconst = D * np.log(2 * np.pi) + np.log(cv).sum(axis=-1)
    logb = eref.emit_diag(feats.astype(np.float64), mu, cv, gconst)
    r = eref.estep_batch(logb, lengths, words, np.log(sp), np.log(A), np.zeros((W, S)), -3.0, feats)
    offs = np.r_[0, np.cumsum(lengths)]
    want = {k: np.zeros_like(r[k]) for k in ("start", "trans", "post_sum", "obs", "obs2")}
    for u, (w,) in enumerate(words):
        one = _fb_ref.utterance(feats[offs[u]:offs[u + 1]], sp[w], A[w], mu[w], cv[w])
        assert abs(r["loglik"][u] - float(one["ll"])) <= 1e-11 * abs(float(one["ll"]))
        np.testing.assert_allclose(r["post"][offs[u]:offs[u + 1], 0], one["gamma"].astype(np.float64), rtol=1e-9,
                                   atol=1e-9)
        for key, src in (("start", "start"), ("trans", "trans"), ("post_sum", "post"), ("obs", "obs"),
                         ("obs2", "obs2")):
            want[key][w] += one[src].astype(np.float64)
    assert r["nobs"].tolist() == [1, 0, 2]
    for key in want:
        np.testing.assert_allclose(r[key], want[key], rtol=1e-9, atol=1e-9, err_msg=key)


# ---- the C ABI --------------------------------------------------------------------------------------------------
NEW = {"sapr_connected_embed_stats_width": 3, "sapr_connected_embed_workspace_bytes": 7, "sapr_connected_embed": 22}


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
    assert lib.sapr_abi_version() == 2
    for name in ("EmbeddedStats", "embedded_forward_backward", "embedded_estep", "embedded_fit"):
        assert getattr(sapr_amd, name) is getattr(sapr_amd.connected, name)
    from sapr_amd import build
    assert "connected_embed.hip" in build.SOURCES and not build.uses_sload_idiom("connected_embed.hip")


def test_size_functions_and_refusals():
    from sapr_amd import _lib
    from sapr_amd.trellis import stats_width
    lib = _lib.load()
    n, w = C.c_size_t(0), C.c_int32(0)
    for S, D in ((10, 13), (18, 39), (1, 0), (7, 26)):
        assert lib.sapr_connected_embed_stats_width(S, D, C.byref(w)) == 0 and w.value == stats_width(S, D)
    assert lib.sapr_connected_embed_stats_width(19, 13, C.byref(w)) == -2
    assert lib.sapr_connected_embed_stats_width(10, 40, C.byref(w)) == -2
    assert lib.sapr_connected_embed_stats_width(0, 13, C.byref(w)) == -1
    assert lib.sapr_connected_embed_stats_width(10, -1, C.byref(w)) == -1
    assert lib.sapr_connected_embed_stats_width(10, 13, None) == -1
    # alpha 1000 * 50 doubles, X 1000 * 5 doubles, 35 partial rows of 10 * (2 + 10 + 26) doubles, 35 bytes -> 48, and
    # the first fold level: one chunk of up to 256 slots x the 25 words SP = 10 allows x a statistics row
    assert lib.sapr_connected_embed_workspace_bytes(1000, 7, 35, 5, 10, 13, C.byref(n)) == 0
    assert n.value == 8 * (1000 * 50 + 1000 * 5 + 35 * 380) + 48 + 8 * 25 * stats_width(10, 13)
    # (3, 7): SP = 10; D = 0: rows of 10 * 12 doubles
    assert lib.sapr_connected_embed_workspace_bytes(3, 1, 3, 3, 7, 0, C.byref(n)) == 0
    # (X: 72 bytes rounded up to 80; the fold level: 13 000 rounded up to 13 008)
    assert n.value == 8 * (3 * 30 + 3 * 3 + 1 + 3 * 120) + 16 + 8 * (25 * stats_width(7, 0) + 1)
    assert lib.sapr_connected_embed_workspace_bytes(10, 2, 257, 5, 10, 0, C.byref(n)) == 0       # (two chunks)
    assert n.value == 8 * (10 * 50 + 10 * 5 + 257 * 120) + 272 + 8 * 2 * 25 * stats_width(10, 0)
    assert lib.sapr_connected_embed_workspace_bytes(0, 0, 0, 1, 1, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, 64, 64, 4, 39, C.byref(n)) == 0
    # unsupported: max_words * SP = 260, S = 19, D = 40 — the codes of sapr_connected_align
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, 26, 26, 10, 13, C.byref(n)) == -2
    assert b"max_words * SP" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, 65, 65, 4, 13, C.byref(n)) == -2
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, 2, 2, 19, 13, C.byref(n)) == -2
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, 2, 2, 10, 40, C.byref(n)) == -2
    assert b"D in 0..39" in lib.sapr_last_error()
    # bad sizes
    assert lib.sapr_connected_embed_workspace_bytes(-1, 1, 2, 2, 4, 0, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, -1, 2, 4, 0, C.byref(n)) == -1
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, 2, 0, 4, 0, C.byref(n)) == -1
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, 2, 2, 4, -1, C.byref(n)) == -1
    assert lib.sapr_connected_embed_workspace_bytes(10, 1, 2, 2, 4, 0, None) == -1

    def call(D, n_utts, total, total_words, max_words, W, S):
        return lib.sapr_connected_embed(None, None, D, None, n_utts, total, None, None, total_words, max_words, None,
                                        None, None, 0.0, W, S, None, 0, None, None, None, None)

    assert call(0, 1, 10, 26, 26, 2, 10) == -2
    assert call(0, 1, 10, 2, 2, 26, 10) == -2
    assert call(40, 1, 10, 2, 2, 2, 10) == -2
    assert call(0, 1, 10, -1, 2, 2, 4) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert call(0, 1, 10, 2, 2, 2, 4) == -1
    assert b"workspace too small" in lib.sapr_last_error()
    assert call(0, 1, 0, 0, 2, 2, 4) == -1
    assert b"NULL" in lib.sapr_last_error()
    assert call(0, 0, 0, 0, 2, 2, 4) == 0


# ---- the Python layer ---------------------------------------------------------------------------------------------
def test_python_layer_refuses_bad_transcripts_before_a_device_is_asked_for():
    from sapr_amd.connected import ConnectedNetwork, embedded_estep, embedded_forward_backward
    W, S = 3, 7                                  # SP = 10: at most 25 words
    z = np.zeros((W, S))
    net = ConnectedNetwork(z, np.zeros((W, S, S)), z)
    logb = np.zeros((8, W, S))
    utts = [np.zeros((5, 2), np.float32), np.zeros((3, 2), np.float32)]
    for call in (lambda tr: embedded_forward_backward(logb, [5, 3], tr, net),
                 lambda tr: embedded_estep(utts, tr, net),
                 lambda tr: embedded_estep(utts, tr, net, want_stats=False, want_post=True)):
        with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
            call([[0]])
        with pytest.raises(ValueError, match="utterance 1 is empty"):
            call([[0], []])
        with pytest.raises(ValueError, match="outside the vocabulary"):
            call([[0, 3], [1]])
        with pytest.raises(ValueError, match="outside the vocabulary"):
            call([[0], [-1]])
        with pytest.raises(ValueError, match=r"K \* SP = 260 exceeds the limit of 256"):
            call([[0] * 26, [1]])


class _Pack:
    """As much of a ``VocabPack`` as ``ConnectedNetwork`` looks at."""
    W, S, D = 3, 7, 2


@pytest.mark.parametrize("family", ["gmm", "full"])
def test_statistics_are_refused_for_the_other_families(family):
    from sapr_amd.connected import ConnectedNetwork, embedded_estep
    z = np.zeros((3, 7))
    net = ConnectedNetwork(z, np.zeros((3, 7, 7)), z, family=family, pack=_Pack())
    utts = [np.zeros((5, 2), np.float32)]
    with pytest.raises(NotImplementedError, match=repr(family)):
        embedded_estep(utts, [[0, 1]], net)
    with pytest.raises(ValueError, match="outside the vocabulary"):      # (the transcripts come first)
        embedded_estep(utts, [[5]], net)


def test_embedded_fit_refuses_before_a_device_is_asked_for():
    from sapr_amd.connected import embedded_fit
    from sapr_amd.hmmlearn_hmm import GaussianHMM

    def model(ct):
        m = GaussianHMM(n_components=2, covariance_type=ct)
        m.startprob_, m.transmat_, m.means_ = np.array([1.0, 0.0]), np.array([[0.5, 0.5], [0.0, 1.0]]), np.zeros((2, 3))
        m._covars_ = {"diag": np.ones((2, 3)), "spherical": np.ones(2), "full": np.tile(np.eye(3), (2, 1, 1))}[ct]
        return m

    utts = [np.zeros((6, 3), np.float32)]
    with pytest.raises(ValueError, match="outside the vocabulary"):
        embedded_fit([model("diag"), model("spherical")], utts, [[0, 2]])
    with pytest.raises(ValueError, match="is empty"):
        embedded_fit([model("diag"), model("spherical")], utts, [[]])
    with pytest.raises(ValueError, match="'full' or 'tied'"):
        embedded_fit([model("diag"), model("full")], utts, [[0, 1]])


def test_embedded_stats_accessors():
    from sapr_amd.connected import EmbeddedStats
    from sapr_amd.trellis import stats_width
    S, SP, D = 3, 4, 2
    stats = np.arange(2 * stats_width(S, D), dtype=np.float64).reshape(2, -1)
    post = np.arange(5 * 2 * SP, dtype=np.float64).reshape(5, 2 * SP)
    res = EmbeddedStats(loglik=np.array([-1.0, NEG]), stats=stats, post=post, offsets=np.array([0, 3, 5]),
                        word_offsets=np.array([0, 2, 3]), words=np.array([1, 0, 1], np.int32), S=S, SP=SP, D=D,
                        n_states=(3, 2))
    st = res.split(1)
    assert st["nobs"] == stats[1, 0] and st["start"].shape == (2,) and st["trans"].shape == (2, 2)
    assert st["obs"].shape == (2, D) and st["obs**2"].shape == (2, D)
    assert np.array_equal(res.split(0)["trans"], stats[0, 2 + S:2 + S + S * S].reshape(S, S))
    assert res.posteriors(0).shape == (3, 2, SP) and res.posteriors(1).shape == (2, 1, SP)
    assert np.array_equal(res.posteriors(0)[1, 1], post[1, SP:])

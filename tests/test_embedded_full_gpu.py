"""GPU: embedded Baum-Welch with second-moment matrices (``sapr_connected_embed_full``, csrc/connected_embed.hip)
through the C ABI and the Python layer against the CPU restatement tests/_embedded_full_ref.py.  The tolerances are the
project's pins for the same quantities: rtol 1e-11 on log-likelihoods, rtol = atol = 1e-9 on ``start`` / ``trans`` /
``post`` / ``obs`` (``TOL`` of tests/test_embedded_gpu.py), every ``oo[w][s]`` within 1e-9 of its own
largest-magnitude entry and exactly symmetric (tests/test_fullcov_gpu.py); after three iterations of EM the history at
rtol 1e-9, ``startprob_`` / ``transmat_`` at rtol 1e-7 atol 1e-12, means at rtol 1e-7 atol 1e-9 and every covariance
matrix within 1e-7 of its largest entry and exactly symmetric."""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _connected_family_cases as cases
from tests import _connected_ref as ref
from tests import _embedded_full_ref as fref
from tests._synth import VOCAB, synth_feature_set, synth_utterance, trained_like_models, word_prototypes

pytestmark = pytest.mark.gpu

NEG = -np.inf
RTOL_LL = 1e-11
TOL = dict(rtol=1e-9, atol=1e-9)
OO_TOL = 1e-9
GROUP_UTTS = 8     # kEmFullGroupUtts of connected_embed.hip: the utterances of one group of the second-moment pass
HEAD_KEYS = (("start", "start"), ("trans", "trans"), ("post_sum", "post"), ("obs", "obs"))


def _head(S):
    return 2 + S + S * S + S


def _raw(entry, logb, lengths, transcripts, ls, lt, lx, pen, max_words, feats, fill=0xA5):
    """``sapr_connected_embed`` or ``sapr_connected_embed_full`` itself: ``(loglik, stats[W, width], post)``; the
    workspace is filled with the byte ``fill`` before the call and the bytes behind it must stay untouched."""
    import torch
    from sapr_amd import _lib
    from sapr_amd.connected import layout
    W, S = ls.shape
    SP = layout(W, S)[0]
    total = int(sum(lengths))
    wide = np.full((total, W, SP), NEG)
    wide[:, :, :S] = logb
    offs = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    words = np.concatenate([np.asarray(t, np.int32) for t in transcripts]).astype(np.int32)
    woffs = np.r_[0, np.cumsum([len(t) for t in transcripts])].astype(np.int64)
    D = feats.shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    lib = _lib.load()
    n, width = C.c_size_t(0), C.c_int32(0)
    if entry == "sapr_connected_embed_full":
        assert lib.sapr_connected_embed_full_workspace_bytes(total, len(lengths), len(words), max_words, W, S, D,
                                                             C.byref(n)) == 0
        assert lib.sapr_connected_embed_full_stats_width(S, D, C.byref(width)) == 0
    else:
        assert lib.sapr_connected_embed_workspace_bytes(total, len(lengths), len(words), max_words, S, D,
                                                        C.byref(n)) == 0
        assert lib.sapr_connected_embed_stats_width(S, D, C.byref(width)) == 0
    guard = 4096
    ws = torch.full((n.value + guard,), fill, dtype=torch.uint8, device="cuda")
    ws[n.value:] = 0xA5
    t_logb, t_offs, t_woffs, t_words, t_ls, t_lt, t_lx = (dev(a) for a in (wide, offs, woffs, words, ls, lt, lx))
    t_feats = dev(np.asarray(feats, np.float32))
    loglik = torch.empty(len(lengths), dtype=torch.float64, device="cuda")
    stats = torch.full((W, width.value), np.nan, dtype=torch.float64, device="cuda")
    post = torch.zeros((total, max_words * SP), dtype=torch.float64, device="cuda")
    _lib.check(getattr(lib, entry)(
        _lib.ptr(t_logb), _lib.ptr(t_feats), D, _lib.ptr(t_offs), len(lengths), total, _lib.ptr(t_words),
        _lib.ptr(t_woffs), len(words), max_words, _lib.ptr(t_ls), _lib.ptr(t_lt), _lib.ptr(t_lx), pen, W, S,
        _lib.ptr(ws), n.value, _lib.ptr(loglik), _lib.ptr(stats), _lib.ptr(post), _lib.current_stream()), entry)
    torch.cuda.synchronize()
    assert bool((ws[n.value:] == 0xA5).all())
    return tuple(a.cpu().numpy() for a in (loglik, stats, post))


def _check_loglik(got, want, what=""):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    worst = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0
    print(f"loglik {what}: max relative difference {worst:.3g}")
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL_LL, err_msg=str(what))


def _check_rows(rows, want, S, D, what="", n_states=None):
    """``rows[W, width]`` of ``sapr_connected_embed_full`` against the dict of ``estep_batch_full``."""
    from sapr_amd.full_cov import split_stats
    assert np.isfinite(rows).all(), what
    worst = 0.0
    for w, row in enumerate(rows):
        m = S if n_states is None else n_states[w]
        st = split_stats(row, S, D, m)
        assert st["nobs"] == want["nobs"][w] and st["logprob"] == 0.0, (what, w)
        for k_ref, k_got in HEAD_KEYS:
            exp = want[k_ref][w][:m] if k_ref != "trans" else want[k_ref][w][:m, :m]
            err = np.max(np.abs(st[k_got] - exp) / (1.0 + np.abs(exp)), initial=0.0)
            print(f"{what} word {w} {k_ref}: max scaled difference {err:.3g}")
            np.testing.assert_allclose(st[k_got], exp, err_msg=f"{what} {k_ref} word {w}", **TOL)
        for s in range(m):
            got, exp = st["obs*obs.T"][s], want["oo"][w][s]
            top = np.max(np.abs(exp))
            worst = max(worst, np.max(np.abs(got - exp)) / top if top else 0.0)
            assert np.max(np.abs(got - exp)) <= OO_TOL * top, (what, w, s, np.max(np.abs(got - exp)), top)
            assert np.array_equal(got, got.T), (what, w, s)
        if want["nobs"][w] == 0:
            assert not row.any(), (what, w)
    print(f"{what} oo: max norm-wise difference {worst:.3g}")


# ---- 1. tile geometry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 13, 14, 26, 27, 39, 12, 15, 16, 17, 25, 31, 32, 33, 38])
def test_tile_geometry(D):
    """The batch of ``test_observation_sums`` (repeated words in a transcript: the slot collapse; utterance 4 has
    K > T) at every DP, on both sides of each padding boundary and with the ones column at every place it can sit;
    D = 12, 15 .. 17, 25, 31 .. 33 and 38 cut a 16-wide matrix-core tile inside a padded width (the masks on rows and
    columns and the ones column next to the last feature)."""
    W, S = 4, 5
    rng = np.random.default_rng(300)
    ls, lt, lx = aref.network(rng, W, S, "skip", "last", False)
    lengths = [33, 70, 12, 129, 2, 48]
    transcripts = [[2, 2, 2], [0, 1, 2, 3, 0], [3], [1, 1, 3, 3, 1, 1, 0], [0, 1, 2], [2, 0]]
    logb = rng.normal(-40.0, 15.0, (sum(lengths), W, S))
    feats = np.random.default_rng(300 + D).normal(0.0, 8.0, (sum(lengths), D)).astype(np.float32)
    want = fref.estep_batch_full(logb, lengths, transcripts, ls, lt, lx, -4.0, feats)
    assert np.isfinite(want["loglik"]).sum() == 5 and want["loglik"][4] == NEG
    got = _raw("sapr_connected_embed_full", logb, lengths, transcripts, ls, lt, lx, -4.0, 7, feats)
    assert got[1].shape == (W, _head(S) + S * D + S * D * D)
    _check_loglik(got[0], want["loglik"], D)
    _check_rows(got[1], want, S, D, what=f"D={D}")
    assert np.abs(want["oo"]).max() > 100.0
    diag = _raw("sapr_connected_embed", logb, lengths, transcripts, ls, lt, lx, -4.0, 7, feats)
    assert got[0].tobytes() == diag[0].tobytes() and got[2].tobytes() == diag[2].tobytes()
    h = _head(S)
    assert got[1][:, :h].tobytes() == diag[1][:, :h].tobytes()   # the head of the row: the same bytes
    np.testing.assert_allclose(got[1][:, h:h + S * D], diag[1][:, h:h + S * D], **TOL)
    # diag(oo) against obs**2: the float64 square against the float32 square, 2^-24 relative per (non-negative) term
    oo = got[1][:, h + S * D:].reshape(W, S, D, D)
    np.testing.assert_allclose(np.diagonal(oo, axis1=2, axis2=3), diag[1][:, h + S * D:].reshape(W, S, D),
                               rtol=2.0 ** -23 + 1e-9, atol=1e-9)


# ---- 2. state groups and chain widths ---------------------------------------------------------------------------
# (W, S, max_words, blocks of 64 chain positions): SP = 4, 10, 18 and the kernels with one, two and four positions per
# lane; S = 3, 7, 10 and 18 are no multiple of the four states of a pass; (14, 18, 14) sits at the edge of the backward
# kernel's LDS; S = 1 and S = 17 run the four-states-per-pass loop of the second-moment pass with one state and with one
# state in its last round
CHAIN_SHAPES = [(3, 3, 5, 1), (4, 4, 40, 3), (5, 7, 9, 2), (7, 10, 25, 4), (6, 18, 3, 1), (6, 18, 7, 2), (14, 18, 14, 4),
                (2, 1, 6, 1), (3, 17, 3, 1)]
CHAIN_LENGTHS = [40, 17, 1, 48, 23]


@pytest.mark.parametrize("W,S,max_words,blocks", CHAIN_SHAPES)
def test_state_groups_and_chain_widths(W, S, max_words, blocks):
    """D = 13, dense words that may end in any state (a word may take one frame), utterances of at most 48 frames of
    which one carries ``max_words`` words.  Word 0 is a model of S - 1 states: its padding state gives exact zeros."""
    from sapr_amd.connected import layout
    D = 13
    assert (max_words * layout(W, S)[0] + 63) // 64 == blocks    # (three blocks run the four-position kernel)
    rng = np.random.default_rng(17 * W + S + max_words)
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    logb = rng.normal(-40.0, 15.0, (sum(CHAIN_LENGTHS), W, S))
    if S > 1:
        ls[0, S - 1] = lx[0, S - 1] = NEG                        # word 0: a model of S - 1 states, padded
        lt[0, S - 1, :] = lt[0, :, S - 1] = NEG
        logb[:, 0, S - 1] = NEG
    transcripts = []
    for T in CHAIN_LENGTHS:
        K = min(max_words, T) if T == 48 else int(rng.integers(1, min(max_words, T, 6) + 1))
        transcripts.append(rng.integers(0, W, K).tolist())
    transcripts[0][0] = 0
    feats = rng.normal(0.0, 8.0, (sum(CHAIN_LENGTHS), D)).astype(np.float32)
    want = fref.estep_batch_full(logb, CHAIN_LENGTHS, transcripts, ls, lt, lx, -2.0, feats)
    assert np.isfinite(want["loglik"]).all() and want["nobs"][0] >= 1
    got = _raw("sapr_connected_embed_full", logb, CHAIN_LENGTHS, transcripts, ls, lt, lx, -2.0, max_words, feats)
    what = f"(W, S, max_words) = {(W, S, max_words)}"
    _check_loglik(got[0], want["loglik"], what)
    _check_rows(got[1], want, S, D, what=what)
    if S == 1:
        return
    from sapr_amd.full_cov import split_stats
    whole = split_stats(got[1][0], S, D)
    for key in ("start", "post", "obs", "obs*obs.T"):
        assert not whole[key][S - 1].any(), key                  # exact zeros in the padding state
    assert not whole["trans"][S - 1].any() and not whole["trans"][:, S - 1].any()
    own = split_stats(got[1][0], S, D, S - 1)
    assert own["obs*obs.T"].shape == (S - 1, D, D) and np.array_equal(own["obs*obs.T"], whole["obs*obs.T"][:S - 1])


# ---- 3. fold boundaries -------------------------------------------------------------------------------------------
def test_fold_boundaries():
    """200 utterances of 3-6 frames and one or two words (S = 3, D = 2): 25 groups of ``GROUP_UTTS`` = 8
    utterances in the second-moment pass and more than 256 transcript words, the chunk
    of the first fold level behind the head of the row."""
    W, S, D, N = 3, 3, 2, 200
    rng = np.random.default_rng(5)
    ls, lt, lx = aref.network(rng, W, S, "dense", "any", False)
    lengths = rng.integers(3, 7, N).tolist()
    transcripts = [rng.integers(0, W, int(rng.integers(1, 3))).tolist() for _ in range(N)]
    assert N > 2 * GROUP_UTTS and N <= 96 * GROUP_UTTS and sum(len(t) for t in transcripts) > 256
    logb = rng.normal(-8.0, 3.0, (sum(lengths), W, S))
    feats = rng.normal(0.0, 8.0, (sum(lengths), D)).astype(np.float32)
    want = fref.estep_batch_full(logb, lengths, transcripts, ls, lt, lx, -1.0, feats)
    assert np.isfinite(want["loglik"]).all()
    got = _raw("sapr_connected_embed_full", logb, lengths, transcripts, ls, lt, lx, -1.0, 2, feats)
    _check_loglik(got[0], want["loglik"], "fold")
    _check_rows(got[1], want, S, D, what="fold")
    diag = _raw("sapr_connected_embed", logb, lengths, transcripts, ls, lt, lx, -1.0, 2, feats)
    assert got[1][:, :_head(S)].tobytes() == diag[1][:, :_head(S)].tobytes()
    # every group matters: the sums of the first 64 utterances alone are another number
    part = fref.estep_batch_full(logb[:sum(lengths[:64])], lengths[:64], transcripts[:64], ls, lt, lx, -1.0,
                                 feats[:sum(lengths[:64])])
    assert np.abs(part["oo"] - want["oo"]).max() > 1.0


# ---- 4. containment, 5. determinism -------------------------------------------------------------------------------
def _containment_case():
    """Pathless utterances between good ones: no frames, more words than frames, a word index outside the
    vocabulary, a NaN frame.  Word 4 occurs only in pathless utterances."""
    W, S, D, max_words = 5, 6, 14, 4
    rng = np.random.default_rng(23)
    ls, lt, lx = aref.network(rng, W, S, "skip", "any", False)
    lengths = [30, 0, 41, 2, 25, 36, 19]
    transcripts = [[1, 3, 3], [2], [0, 2, 1, 0], [4, 1, 4], [2, W], [3, 4], [2, 2]]
    logb = rng.normal(-30.0, 10.0, (sum(lengths), W, S))
    feats = rng.normal(0.0, 8.0, (sum(lengths), D)).astype(np.float32)
    hit = sum(lengths[:5]) + 11                                   # a NaN frame in utterance 5
    logb[hit] = np.nan
    feats[hit] = np.nan
    return W, S, D, max_words, ls, lt, lx, lengths, transcripts, logb, feats


def test_containment_at_the_c_abi():
    W, S, D, max_words, ls, lt, lx, lengths, transcripts, logb, feats = _containment_case()
    want = fref.estep_batch_full(logb, lengths, transcripts, ls, lt, lx, -1.5, feats, max_words)
    assert want["loglik"][1] == NEG and want["loglik"][3] == NEG and want["loglik"][4] == NEG
    assert np.isnan(want["loglik"][5]) and np.isfinite(want["loglik"][[0, 2, 6]]).all()
    assert want["nobs"][4] == 0 and np.isfinite(want["oo"]).all()
    got = _raw("sapr_connected_embed_full", logb, lengths, transcripts, ls, lt, lx, -1.5, max_words, feats, fill=0xFF)
    _check_loglik(got[0], want["loglik"], "containment")
    assert np.isnan(got[0][5])
    _check_rows(got[1], want, S, D, what="containment")
    assert not got[1][4].any()                                   # only in pathless utterances: an all-zero row
    offs = np.r_[0, np.cumsum(lengths)]
    for u in (1, 3, 4, 5):
        assert not got[2][offs[u]:offs[u + 1]].any(), u
    # the good utterances alone: the same bytes
    keep = [0, 2, 6]
    rows = np.concatenate([np.arange(offs[u], offs[u + 1]) for u in keep])
    alone = _raw("sapr_connected_embed_full", logb[rows], [lengths[u] for u in keep], [transcripts[u] for u in keep],
                 ls, lt, lx, -1.5, max_words, feats[rows], fill=0xFF)
    assert alone[1].tobytes() == got[1].tobytes()


def test_two_calls_return_the_same_bytes():
    W, S, D, max_words, ls, lt, lx, lengths, transcripts, logb, feats = _containment_case()
    a = _raw("sapr_connected_embed_full", logb, lengths, transcripts, ls, lt, lx, -1.5, max_words, feats, fill=0xFF)
    b = _raw("sapr_connected_embed_full", logb, lengths, transcripts, ls, lt, lx, -1.5, max_words, feats, fill=0x00)
    assert np.isfinite(a[0]).sum() == 3 and np.isfinite(a[1]).all() and np.abs(a[1]).max() > 100.0
    for x, y, name in zip(a, b, ("loglik", "stats", "post")):
        assert x.tobytes() == y.tobytes(), name


# ---- 6. tie to the isolated-word full-covariance E-step -----------------------------------------------------------
@pytest.mark.parametrize("ns,D", [(8, 13), (16, 39)])
def test_one_word_with_any_exit_equals_the_isolated_word_full_estep(ns, D):
    """One word per utterance, every state an exit: the chain is the word model itself, and ``obs`` / ``oo`` are those
    of ``sapr_full_estep`` (``FullCovBatch.estep``) over the same models and frames.  Utterances of at most 30 frames,
    for the reason given at ``test_one_word_with_any_exit_equals_the_isolated_word_estep``: two float64
    implementations of one lattice differ in the posteriors by about ulp(|loglik|) per frame."""
    from sapr_amd import full_cov
    from sapr_amd.connected import ConnectedNetwork, embedded_estep
    W, S = 3, ns + 2
    sp, A, mu, cv = trained_like_models(W, ns, D, seed=41)
    rng = np.random.default_rng(43)
    covars = np.empty((W, S, D, D))
    for w in range(W):
        for s in range(S):
            B = rng.normal(size=(D, D))
            covars[w, s] = np.diag(cv[w, s]) + B @ B.T * (10.0 / D)
    _, flat = synth_feature_set(VOCAB[:W], 6, D=D, seed=17, tmin=1, tmax=31)
    utts = [np.ascontiguousarray(f.T) for f in flat]
    utt_model = np.repeat(np.arange(W), 6)
    lengths = np.asarray([u.shape[0] for u in utts])
    packed = np.ascontiguousarray(np.concatenate(utts, axis=0), dtype=np.float32)
    pack = full_cov.FullPack.from_params([(sp[w], A[w], mu[w], covars[w]) for w in range(W)])
    iso_ll, iso, _, _ = (None if t is None else t.cpu().numpy()
                         for t in pack.batch(packed, lengths, utt_model).estep(pack.data, want_stats=True))
    with np.errstate(divide="ignore"):
        net = ConnectedNetwork(np.log(sp), np.log(A), np.zeros((W, S)), -5.0, family="full", pack=pack)
    res = embedded_estep(utts, [[int(w)] for w in utt_model], net, second_moments=True)
    assert res.layout == "full"
    np.testing.assert_allclose(res.loglik, iso_ll, rtol=RTOL_LL)
    for w in range(W):
        want, got = full_cov.split_stats(iso[w], S, D), res.split(w)
        assert got["nobs"] == want["nobs"] == 6
        for key in ("start", "trans", "post", "obs"):
            err = np.max(np.abs(got[key] - want[key]) / (1.0 + np.abs(want[key])))
            print(f"(S, D) = ({S}, {D}) word {w} {key}: max scaled difference {err:.3g}")
            np.testing.assert_allclose(got[key], want[key], err_msg=f"{key} word {w}", **TOL)
        for s in range(S):
            a, b = got["obs*obs.T"][s], want["obs*obs.T"][s]
            top = np.max(np.abs(b))
            print(f"(S, D) = ({S}, {D}) word {w} state {s} oo: norm-wise {np.max(np.abs(a - b)) / top if top else 0.0:.3g}")
            assert np.max(np.abs(a - b)) <= OO_TOL * np.max(np.abs(b)), (w, s)
            assert np.array_equal(a, a.T)


# ---- 7. the families ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,spec", [("diag", ref.E2E_CASES[3]), ("full", cases.FULL_CASES[0])])
def test_second_moments_for_the_families(family, spec):
    """``embedded_estep(..., second_moments=True)`` against the restatement fed the emitted ``logb`` read back from
    the device."""
    from sapr_amd import connected
    from sapr_amd.connected import ConnectedNetwork, embedded_estep
    pen = -7.5
    if family == "diag":
        model, utts, truth = ref.sample_case(*spec)
        net = ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], pen, None, model["means"],
                               model["vars"], model["gconst"])
    else:
        model, utts, truth = cases.case(family, spec)
        net = ConnectedNetwork.from_models(cases.models_of(family, model), word_penalty=pen)
    feats, _, offs = connected._features(utts)
    logb = connected._EMIT[family](feats, net).cpu().numpy().reshape(-1, net.W, net.SP)[:, :, :net.S]
    lengths = np.diff(offs)
    want = fref.estep_batch_full(logb, lengths, truth, net.log_start, net.log_trans, net.log_exit, pen,
                                 np.concatenate(utts))
    assert np.isfinite(want["loglik"]).all()
    res = embedded_estep(utts, truth, net, want_post=True, second_moments=True)
    assert res.layout == "full" and res.stats.shape == (net.W, connected.embed_full_stats_width(net.S, net.D))
    _check_loglik(res.loglik, want["loglik"], family)
    got = res.post.reshape(int(offs[-1]), -1, res.SP)
    np.testing.assert_allclose(got[:, :, :net.S], want["post"], **TOL)
    _check_rows(res.stats, want, net.S, net.D, what=family)
    st = res.split(0)
    assert st["obs*obs.T"].shape == (net.n_states[0], net.D, net.D) and "obs**2" not in st
    if family == "full":                                         # the default keeps its refusal
        with pytest.raises(NotImplementedError, match="'full'"):
            embedded_estep(utts, truth, net)


# ---- 8. training ------------------------------------------------------------------------------------------------------
NAMES = ["zero", "one", "two", "three", "four"]                  # "four" is in no transcript
KINDS = ["full", "tied", "diag", "spherical", "full"]


def _fit_case():
    """The data of ``test_embedded_gpu._fit_case`` (S = 4, D = 5; 24 recordings of 2-4 words, each word 8-16 frames
    of tests/_synth.py's piecewise-constant segments) over four spoken words of the four covariance types and a fifth
    that is never spoken; models perturbed from the prototypes."""
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    rng = np.random.default_rng(78)
    S, D = 4, 5
    protos = word_prototypes(NAMES, D, n_seg=S, seed=5)
    utts, truth = [], []
    for _ in range(24):
        words = rng.integers(0, 4, int(rng.integers(2, 5))).tolist()
        utts.append(np.concatenate([synth_utterance(rng, protos[NAMES[w]], int(rng.integers(8, 17))).T
                                    for w in words]).astype(np.float32))
        truth.append(words)
    models = []
    for w, (name, kind) in enumerate(zip(NAMES, KINDS)):
        m = GaussianHMM(n_components=S, covariance_type=kind)
        m.startprob_ = np.array([1.0, 0.0, 0.0, 0.0])
        m.transmat_ = np.array([[0.7, 0.3, 0, 0], [0, 0.7, 0.3, 0], [0, 0, 0.7, 0.3], [0, 0, 0, 1.0]])
        mu = protos[name] + rng.normal(0.0, 4.0, (S, D))
        mu[:, 0] -= 300.0
        m.means_ = mu
        m._covars_ = {"full": np.tile(60.0 * np.eye(D), (S, 1, 1)), "tied": 60.0 * np.eye(D),
                      "diag": np.full((S, D), 60.0), "spherical": np.full(S, 60.0)}[kind]
        models.append(m)
    return models, utts, truth


@pytest.fixture(scope="module")
def fit_case():
    models, utts, truth = _fit_case()
    ref_models, history = fref.fit_full(models, utts, truth, n_iter=3, tol=0.0)
    return models, utts, truth, ref_models, history


def _check_params(got, want, what):
    np.testing.assert_allclose(got.startprob_, want.startprob_, rtol=1e-7, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(got.transmat_, want.transmat_, rtol=1e-7, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(got.means_, want.means_, rtol=1e-7, atol=1e-9, err_msg=what)
    a, b = np.asarray(got._covars_), np.asarray(want._covars_)
    assert a.shape == b.shape, what
    mats = zip(a.reshape(-1, *a.shape[-2:]), b.reshape(-1, *b.shape[-2:])) if got.covariance_type in ("full", "tied") \
        else [(a, b)]
    for x, y in mats:
        err = np.max(np.abs(x - y)) / np.max(np.abs(y))
        print(f"{what} ({got.covariance_type}) covariance: norm-wise difference {err:.3g}")
        assert err <= 1e-7, what
        if got.covariance_type in ("full", "tied"):
            assert np.array_equal(x, x.T), what


def test_embedded_fit_with_second_moments(fit_case):
    from sapr_amd.connected import embedded_fit
    models, utts, truth, ref_models, history = fit_case
    assert len(history) == 3 and history[-1] > history[0]
    mine = [copy.deepcopy(m) for m in models]
    before = pickle.dumps(mine[4])
    with pytest.raises(ValueError, match="'full' or 'tied'"):
        embedded_fit(mine, utts, truth, n_iter=3, tol=0.0, names=NAMES)
    assert pickle.dumps(mine[4]) == before and np.array_equal(mine[0].means_, models[0].means_)
    got = embedded_fit(mine, utts, truth, n_iter=3, tol=0.0, names=NAMES, second_moments=True)
    print("history: max relative difference", np.max(np.abs(np.array(got) - history) / np.abs(history)))
    np.testing.assert_allclose(got, history, rtol=1e-9)
    for w in range(4):
        _check_params(mine[w], ref_models[w], NAMES[w])
        assert not np.array_equal(mine[w].means_, models[w].means_)
    assert mine[0]._covars_.shape == (4, 5, 5) and mine[1]._covars_.shape == (5, 5)
    assert mine[2]._covars_.shape == (4, 5) and mine[3]._covars_.shape == (4,)
    assert pickle.dumps(mine[4]) == before                       # a word in no transcript keeps its bytes


def _pickle_models(tmp_path, models, names, sub="trained_models", n_iter=15):
    d = tmp_path / sub / "hmmlearn"
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_hmmlearn_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / sub)


def test_decoder_train_embedded_over_full_and_tied_models(tmp_path, fit_case):
    from sapr_amd.decoder import Decoder
    models, utts, truth, ref_models, history = fit_case
    dec = Decoder(models_dir=_pickle_models(tmp_path, models, NAMES), implementation="hmmlearn", n_iter=15)
    assert dec._is_full()
    said = [[NAMES[w] for w in t] for t in truth]
    dec.align([x.T for x in utts[:2]], said[:2])                  # (packs the vocabulary from the old parameters)
    untouched = pickle.dumps(dec.models["four"])
    got = dec.train_embedded([x.T for x in utts], said, n_iter=3, tol=0.0)
    # (the load order of the words does not enter: an utterance's chain and a word's slots are the same)
    np.testing.assert_allclose(got, history, rtol=1e-9)
    for w, word in enumerate(NAMES[:4]):
        _check_params(dec.models[word], ref_models[w], word)
    assert dec.models["one"]._covars_.shape == (5, 5)
    assert pickle.dumps(dec.models["four"]) == untouched
    out = dec.align([x.T for x in utts[:4]], said[:4])           # (from the new parameters: the packs were dropped)
    assert all(np.isfinite(r["log_likelihood"]) and r["words"] == s for r, s in zip(out, said))
    again = Decoder(models_dir=_pickle_models(tmp_path, [dec.models[w] for w in NAMES], NAMES, sub="retrained"),
                    implementation="hmmlearn", n_iter=15)
    b = again.align([x.T for x in utts[:4]], said[:4])
    assert [r["log_likelihood"] for r in out] == [r["log_likelihood"] for r in b]


def test_decoder_train_embedded_still_refuses_other_implementations(tmp_path):
    from sapr_amd.decoder import Decoder
    d = tmp_path / "trained_models" / "custom"
    d.mkdir(parents=True)
    with open(d / "zero_custom_15.pkl", "wb") as f:
        pickle.dump({"placeholder": "custom"}, f)
    with pytest.raises(ValueError, match="implementation='custom'"):
        Decoder(models_dir=str(tmp_path / "trained_models"), implementation="custom").train_embedded(
            [np.zeros((13, 4), np.float32)], [["zero"]])

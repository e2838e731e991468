"""GPU: embedded Baum-Welch for Gaussian-mixture word models (``sapr_connected_embed_gmm``, csrc/connected_embed.hip)
through the C ABI and the Python layer against the CPU restatement tests/_embedded_gmm_ref.py.  The tolerances are the
project's pins for the same quantities: rtol 1e-11 on log-likelihoods; ``|x - ref| / (1 + |ref|) <= 1e-9`` on
``post_mix`` / ``obs`` / ``obs2`` and rtol = atol = 1e-9 on the head of a row (``TOL`` of tests/test_embedded_gpu.py);
after three iterations of EM the history at rtol 1e-9, ``startprob_`` / ``transmat_`` / ``weights_`` / ``means_`` at
rtol 1e-7 and ``covars_`` at rtol 1e-6."""
import copy
import ctypes as C
import functools
import pickle

import numpy as np
import pytest

from tests import _connected_family_cases as cases
from tests import _embedded_gmm_ref as mref

pytestmark = pytest.mark.gpu

NEG = -np.inf
RTOL_LL = 1e-11
TOL = dict(rtol=1e-9, atol=1e-9)
PIN = 1e-9
GROUP_UTTS, MAX_GROUPS = 8, 96     # kEmFullGroupUtts, kEmFullMaxGroups of connected_embed.hip
MIX_KEYS = (("post_mix", "post_mix"), ("obs", "obs"), ("obs2", "obs**2"))
HEAD_KEYS = (("start", "start"), ("trans", "trans"), ("post_sum", "post"))


def _head(S):
    return 2 + S + S * S + S


def _network(spec, pen=0.0, exit_states="last", edit=None):
    """A committed case as ``(model, utterances, truth, ConnectedNetwork over its GMMHMM objects)``; ``edit(model)``
    may change a copy of the case's parameters first."""
    from sapr_amd.connected import ConnectedNetwork
    model, utts, truth = cases.gmm_case(*spec)
    if edit is not None:
        model = {k: np.array(v, copy=True) for k, v in model.items()}
        edit(model)
    net = ConnectedNetwork.from_models(cases.models_of("gmm", model), exit_states=exit_states, word_penalty=pen)
    return model, utts, truth, net


def _emitted(net, x):
    """The emission stage's ``logb`` of frames ``x[T, D]`` read back from the device: ``[T, W, S]``."""
    import torch
    from sapr_amd import connected
    feats = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return connected.emit_gmm(feats, net).cpu().numpy().reshape(-1, net.W, net.SP)[:, :, :net.S]


def _want(net, model, logb, lengths, transcripts, x, max_words=None):
    return mref.estep_batch_gmm(logb, lengths, transcripts, net.log_start, net.log_trans, net.log_exit,
                                net.word_penalty, x, model["weights"], model["means"], model["covars"], max_words)


def _raw(entry, net, logb, lengths, transcripts, max_words, feats, fill=0xA5):
    """``sapr_connected_embed`` at D = 0 or ``sapr_connected_embed_gmm`` itself: ``(loglik, stats[W, width], post)``;
    the workspace is filled with the byte ``fill`` before the call and the bytes behind it must stay untouched."""
    import torch
    from sapr_amd import _lib
    W, S, SP = net.W, net.S, net.SP
    total = int(sum(lengths))
    wide = np.full((total, W, SP), NEG)
    wide[:, :, :S] = logb
    offs = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    words = np.concatenate([np.asarray(t, np.int32) for t in transcripts]).astype(np.int32)
    woffs = np.r_[0, np.cumsum([len(t) for t in transcripts])].astype(np.int64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    lib = _lib.load()
    n, width = C.c_size_t(0), C.c_int32(0)
    gmm = entry == "sapr_connected_embed_gmm"
    D, M = (int(feats.shape[1]), int(net.pack.M)) if gmm else (0, 0)
    if gmm:
        assert lib.sapr_connected_embed_gmm_workspace_bytes(total, len(lengths), len(words), max_words, W, S, M, D,
                                                            C.byref(n)) == 0
        assert lib.sapr_connected_embed_gmm_stats_width(S, M, D, C.byref(width)) == 0
    else:
        assert lib.sapr_connected_embed_workspace_bytes(total, len(lengths), len(words), max_words, S, 0,
                                                        C.byref(n)) == 0
        assert lib.sapr_connected_embed_stats_width(S, 0, C.byref(width)) == 0
    guard = 4096
    ws = torch.full((n.value + guard,), fill, dtype=torch.uint8, device="cuda")
    ws[n.value:] = 0xA5
    t_logb, t_offs, t_woffs, t_words = (dev(a) for a in (wide, offs, woffs, words))
    t_ls, t_lt, t_lx, t_pack = net.device(torch.device("cuda", torch.cuda.current_device()))
    t_feats = dev(np.asarray(feats, np.float32)) if gmm else None
    loglik = torch.empty(len(lengths), dtype=torch.float64, device="cuda")
    stats = torch.full((W, width.value), np.nan, dtype=torch.float64, device="cuda")
    post = torch.zeros((total, max_words * SP), dtype=torch.float64, device="cuda")
    tail = (_lib.ptr(t_offs), len(lengths), total, _lib.ptr(t_words), _lib.ptr(t_woffs), len(words), max_words,
            _lib.ptr(t_ls), _lib.ptr(t_lt), _lib.ptr(t_lx), net.word_penalty, W, S, _lib.ptr(ws), n.value,
            _lib.ptr(loglik), _lib.ptr(stats), _lib.ptr(post), _lib.current_stream())
    mid = (_lib.ptr(t_pack), M) if gmm else ()
    _lib.check(getattr(lib, entry)(_lib.ptr(t_logb), _lib.ptr(t_feats), D, *mid, *tail), entry)
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


def _check_rows(rows, want, S, M, D, what="", n_states=None):
    """``rows[W, width]`` of ``sapr_connected_embed_gmm`` against the dict of ``estep_batch_gmm``."""
    from sapr_amd.gmm_hmm import split_stats
    assert np.isfinite(rows).all(), what
    worst = dict.fromkeys((k for k, _ in MIX_KEYS), 0.0)
    for w, row in enumerate(rows):
        m = S if n_states is None else n_states[w]
        st = split_stats(row, S, M, D, m)
        assert st["nobs"] == want["nobs"][w] and st["logprob"] == 0.0, (what, w)
        for k_ref, k_got in HEAD_KEYS:
            exp = want[k_ref][w][:m] if k_ref != "trans" else want[k_ref][w][:m, :m]
            np.testing.assert_allclose(st[k_got], exp, err_msg=f"{what} {k_ref} word {w}", **TOL)
        for k_ref, k_got in MIX_KEYS:
            exp = want[k_ref][w][:m]
            worst[k_ref] = max(worst[k_ref], float(np.max(np.abs(st[k_got] - exp) / (1.0 + np.abs(exp)), initial=0.0)))
        whole = split_stats(row, S, M, D)
        for key in ("post_mix", "obs", "obs**2"):
            assert not whole[key][m:].any(), (what, w, key)       # exact zeros in the padding states
        if want["nobs"][w] == 0:
            assert not row.any(), (what, w)
    print(f"{what}: max scaled difference " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for key, v in worst.items():
        assert v <= PIN, (what, key, v)


# ---- 1. statistics against the restatement ----------------------------------------------------------------------
SETTINGS = [(spec, 0.0, ex) for spec in cases.GMM_CASES for ex in ("last", "any")] + [(cases.GMM_CASES[1], -30.0, "last")]


@pytest.mark.parametrize("spec,pen,exit_states", SETTINGS)
def test_statistics_against_the_restatement(spec, pen, exit_states):
    """Every committed case (every SP, MP and DP instantiation; S = 7 in SP = 10 and M = 3 in MP = 4 among them)
    through ``embedded_estep(..., mixtures=True)``; the restatement is fed the emitted ``logb`` read back from the
    device."""
    from sapr_amd import connected
    from sapr_amd.connected import embedded_estep
    model, utts, truth, net = _network(spec, pen, exit_states)
    x = np.concatenate(utts)
    lengths = [len(u) for u in utts]
    assert max(lengths) > 64 or spec[2] == 4                     # (the 64-frame chunk boundary is crossed)
    want = _want(net, model, _emitted(net, x), lengths, truth, x)
    assert np.isfinite(want["loglik"]).all()
    res = embedded_estep(utts, truth, net, want_post=True, mixtures=True)
    S, M, D = spec[2], spec[3], spec[4]
    assert res.layout == "gmm" and res.M == M and res.stats.shape == (net.W, connected.embed_gmm_stats_width(S, M, D))
    _check_loglik(res.loglik, want["loglik"], (spec, pen, exit_states))
    np.testing.assert_allclose(res.post.reshape(len(x), -1, res.SP)[:, :, :S], want["post"], **TOL)
    _check_rows(res.stats, want, S, M, D, what=f"{spec} pen={pen} exit={exit_states}")
    np.testing.assert_allclose(res.stats[:, _head(S):_head(S) + S * M].reshape(net.W, S, M).sum(axis=2),
                               res.stats[:, _head(S) - S:_head(S)], **TOL)         # sum_m post_mix = post
    st = res.split(0)
    assert st["post_mix"].shape == (S, M) and st["obs"].shape == (S, M, D) and st["obs**2"].shape == (S, M, D)
    with pytest.raises(NotImplementedError, match="mixture responsibilities"):   # the default keeps its refusal
        embedded_estep(utts, truth, net)


@pytest.mark.parametrize("spec", cases.GMM_CASES)
def test_same_launches_as_the_diagonal_entry_point(spec):
    """``loglik``, ``post`` and the head of every row are byte for byte ``sapr_connected_embed``'s at D = 0; the
    Python layer over a given ``logb`` returns the C ABI's bytes."""
    from sapr_amd.connected import embedded_forward_backward
    model, utts, truth, net = _network(spec, -4.0)
    x = np.concatenate(utts)
    lengths = [len(u) for u in utts]
    logb = _emitted(net, x)
    max_words = max(len(t) for t in truth)
    got = _raw("sapr_connected_embed_gmm", net, logb, lengths, truth, max_words, x, fill=0xFF)
    base = _raw("sapr_connected_embed", net, logb, lengths, truth, max_words, x)
    h = _head(net.S)
    assert got[0].tobytes() == base[0].tobytes() and got[2].tobytes() == base[2].tobytes()
    assert got[1][:, :h].tobytes() == base[1].tobytes()
    res = embedded_forward_backward(logb, lengths, truth, net, feats=x, want_post=True, mixtures=True)
    assert res.layout == "gmm" and res.stats.tobytes() == got[1].tobytes() and res.loglik.tobytes() == got[0].tobytes()


# ---- 2. tie to the isolated-word mixture E-step ---------------------------------------------------------------------
@pytest.mark.parametrize("spec", cases.GMM_CASES)
def test_one_word_with_any_exit_equals_the_isolated_word_estep(spec):
    """One word per utterance, every state an exit: the chain is the word model itself, and ``post_mix`` / ``obs`` /
    ``obs2`` are those of ``sapr_gmm_estep_diag`` (``GmmBatch.estep``) over the same pack and frames.  The recordings
    are single words drawn from the case's own models (every state held for 1-3 frames): two float64 implementations
    of one lattice differ in the posteriors by about ulp(|loglik|) per frame, so they are kept short."""
    from sapr_amd import gmm_hmm
    from sapr_amd.connected import ConnectedNetwork, embedded_estep
    model, _, _ = cases.gmm_case(*spec)
    _, W, S, M, D, _ = spec
    rng = np.random.default_rng(spec[0])
    utt_model = np.arange(3 * W) % W
    utts = []
    for w in utt_model:
        rows = []
        for s in range(S):
            m = rng.choice(M, size=int(rng.integers(1, 4)), p=model["weights"][w, s])
            rows.append(rng.normal(model["means"][w, s, m], np.sqrt(model["covars"][w, s, m])))
        utts.append(np.concatenate(rows).astype(np.float32))
    lengths = np.asarray([len(u) for u in utts])
    packed = np.ascontiguousarray(np.concatenate(utts), dtype=np.float32)
    models = cases.models_of("gmm", model)
    pack = gmm_hmm.GmmPack.from_models([copy.copy(m) for m in models])
    iso_ll, iso, _, _ = (None if t is None else t.cpu().numpy()
                         for t in pack.batch(packed, lengths, utt_model).estep(pack, want_stats=True))
    net = ConnectedNetwork.from_models(models, exit_states="any", word_penalty=-5.0, pack=pack)
    res = embedded_estep(utts, [[int(w)] for w in utt_model], net, mixtures=True)
    np.testing.assert_allclose(res.loglik, iso_ll, rtol=RTOL_LL)
    worst = dict.fromkeys(("post_mix", "obs", "obs**2"), 0.0)
    for w in range(W):
        want, got = gmm_hmm.split_stats(iso[w], S, M, D), res.split(w)
        assert got["nobs"] == want["nobs"] == 3
        for key in worst:
            worst[key] = max(worst[key], float(np.max(np.abs(got[key] - want[key]) / (1.0 + np.abs(want[key])))))
    print(f"{spec} against sapr_gmm_estep_diag: max scaled difference " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= PIN for v in worst.values()), worst


# ---- 3. exact behaviour -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _containment_case():
    """The recordings of case (203: S = 7 in SP = 10, M = 3 in MP = 4, D = 26) with four of the twelve made pathless:
    no frames, more words than frames, more words than ``max_words``, a NaN frame.  Word 4 is taken out of every
    other transcript: it occurs only in pathless utterances."""
    spec = cases.GMM_CASES[2]
    model, utts, truth, net = _network(spec, -1.5, "any")
    W = net.W
    utts, truth = [u.copy() for u in utts], [[(w if w != 4 else 0) for w in t] for t in truth]
    max_words = 5
    utts[1], truth[1] = utts[1][:0], [2]                          # no frames
    utts[4], truth[4] = utts[4][:2], [4, 1, 4]                    # K > T
    truth[7] = [4, 0, 1, 2, 3, 4]                                 # K > max_words
    utts[9][len(utts[9]) // 2] = np.nan                           # a NaN frame: every logb of it is NaN
    truth[9] = truth[9] + [4] if len(truth[9]) < max_words else truth[9][:-1] + [4]
    assert W == 5 and max(len(t) for i, t in enumerate(truth) if i != 7) <= max_words
    return spec, model, net, utts, truth, max_words, (1, 4, 7, 9)


def _run_containment(utts, truth, fill):
    spec, model, net, _, _, max_words, _ = _containment_case()
    x = np.concatenate(utts)
    lengths = [len(u) for u in utts]
    logb = _emitted(net, x)
    return logb, lengths, x, _raw("sapr_connected_embed_gmm", net, logb, lengths, truth, max_words, x, fill=fill)


def test_pathless_utterances_contribute_exact_zeros():
    spec, model, net, utts, truth, max_words, bad = _containment_case()
    logb, lengths, x, got = _run_containment(utts, truth, 0xFF)
    want = _want(net, model, logb, lengths, truth, x, max_words)
    assert all(want["loglik"][u] == NEG for u in bad[:3]) and np.isnan(want["loglik"][9])
    assert np.isfinite(np.delete(want["loglik"], bad)).all() and want["nobs"][4] == 0
    _check_loglik(got[0], want["loglik"], "containment")
    assert np.isnan(got[0][9])
    _check_rows(got[1], want, net.S, spec[3], spec[4], what="containment")
    assert not got[1][4].any()                                   # only in pathless utterances: an all-zero row
    offs = np.r_[0, np.cumsum(lengths)]
    for u in bad:
        assert not got[2][offs[u]:offs[u + 1]].any(), u
    # path-less stand-ins (no frames) in their places — the same utterance groups: the same bytes
    utts2, truth2 = list(utts), list(truth)
    for u in bad:
        utts2[u], truth2[u] = utts[u][:0], [0]
    _, _, _, alone = _run_containment(utts2, truth2, 0xFF)
    assert alone[1].tobytes() == got[1].tobytes()
    assert np.delete(alone[0], bad).tobytes() == np.delete(got[0], bad).tobytes()


def test_two_calls_return_the_same_bytes_whatever_the_workspace_held():
    _, _, _, utts, truth, _, _ = _containment_case()
    a = _run_containment(utts, truth, 0xFF)[3]
    b = _run_containment(utts, truth, 0xFF)[3]
    c = _run_containment(utts, truth, 0x00)[3]
    assert np.isfinite(a[0]).sum() == 8 and np.isfinite(a[1]).all() and np.abs(a[1]).max() > 100.0
    for x, y, z, name in zip(a, b, c, ("loglik", "stats", "post")):
        assert x.tobytes() == y.tobytes() == z.tobytes(), name


def test_a_component_of_weight_zero_and_a_word_in_no_transcript():
    """Word 0's state 1 gets a component of weight exactly 0 (its share is an exact zero, the others' are not); word 2
    is taken out of every transcript (an all-zero row)."""
    from sapr_amd.connected import embedded_estep
    spec = cases.GMM_CASES[0]

    def edit(model):
        w0 = model["weights"][0, 1]
        model["weights"][0, 1] = [w0[0] + w0[1], 0.0]

    model, utts, truth, net = _network(spec, 0.0, "last", edit)
    truth = [[(w if w != 2 else 0) for w in t] for t in truth]
    x = np.concatenate(utts)
    lengths = [len(u) for u in utts]
    want = _want(net, model, _emitted(net, x), lengths, truth, x)
    finite = np.isfinite(want["loglik"])
    assert finite.sum() >= 8 and want["nobs"][0] > 0 and want["nobs"][2] == 0
    res = embedded_estep(utts, truth, net, mixtures=True)
    _check_loglik(res.loglik, want["loglik"], "weight 0")
    _check_rows(res.stats, want, spec[2], spec[3], spec[4], what="weight 0")
    st = res.split(0)
    for key in ("post_mix", "obs", "obs**2"):
        assert not st[key][1, 1].any() and st[key][1, 0].any(), key
    assert st["post_mix"][1, 0] == pytest.approx(st["post"][1], rel=1e-12)
    assert not res.stats[2].any()


def test_more_utterances_than_fixed_groups():
    """More than 8 * 96 tiny utterances (the ``GMM_TINY`` shape: S = 1, M = 4, D = 1, a few frames each): the groups
    grow instead of their number."""
    from sapr_amd.connected import embedded_estep
    N = 800
    spec = cases.GMM_TINY[:5] + (N,)
    assert N > GROUP_UTTS * MAX_GROUPS
    model, utts, truth, net = _network(spec, -2.0, "last")
    x = np.concatenate(utts)
    lengths = [len(u) for u in utts]
    want = _want(net, model, _emitted(net, x), lengths, truth, x)
    assert np.isfinite(want["loglik"]).all()
    res = embedded_estep(utts, truth, net, mixtures=True)
    _check_loglik(res.loglik, want["loglik"], "800 utterances")
    _check_rows(res.stats, want, spec[2], spec[3], spec[4], what="800 utterances")
    # every group matters: the sums of the first 768 utterances alone are another number
    n = sum(lengths[:768])
    part = _want(net, model, _emitted(net, x[:n]), lengths[:768], truth[:768], x[:n])
    assert np.abs(part["post_mix"] - want["post_mix"]).max() > 1.0


# ---- 4. training ------------------------------------------------------------------------------------------------------
NAMES = ["zero", "one", "two", "three", "four"]                  # "four" is in no transcript


@functools.lru_cache(maxsize=None)
def _fit_case():
    """``GMM_DECODER_CASE`` (W = 4, S = 5, M = 2, D = 13, ten recordings) with a fifth word that is never spoken;
    the models start from the case's parameters with perturbed means, so that three iterations move them."""
    model, utts, truth = cases.gmm_case(*cases.GMM_DECODER_CASE)
    rng = np.random.default_rng(79)
    models = cases.models_of("gmm", model) + cases.models_of("gmm", cases.gmm_case(306, 1, 5, 2, 13, 1)[0])
    for m in models:
        m.means_ = m.means_ + rng.normal(0.0, 2.0, m.means_.shape)
    ref_models, history = mref.fit_gmm(models, utts, truth, n_iter=3, tol=0.0)
    return models, utts, truth, ref_models, history


def _check_params(got, want, what):
    for name, rtol in (("startprob_", 1e-7), ("transmat_", 1e-7), ("weights_", 1e-7), ("means_", 1e-7),
                       ("covars_", 1e-6)):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(b != 0, np.abs(a - b) / np.abs(b), np.where(a == b, 0.0, np.inf))
        print(f"{what} {name}: max relative difference {float(rel.max()):.3g}")
        np.testing.assert_allclose(a, b, rtol=rtol, err_msg=f"{what} {name}")


def test_embedded_fit_over_gmmhmm_models():
    from sapr_amd.connected import embedded_fit
    models, utts, truth, ref_models, history = _fit_case()
    assert len(history) == 3 and history[-1] > history[0]
    mine = [copy.deepcopy(m) for m in models]
    before = pickle.dumps(mine[4])
    got = embedded_fit(mine, utts, truth, n_iter=3, tol=0.0, names=NAMES)
    print("history: max relative difference", np.max(np.abs(np.array(got) - history) / np.abs(history)))
    np.testing.assert_allclose(got, history, rtol=1e-9)
    spoken = sorted({w for t in truth for w in t})
    assert 4 not in spoken and len(spoken) >= 3
    for w in spoken:
        _check_params(mine[w], ref_models[w], NAMES[w])
        assert not np.array_equal(mine[w].means_, models[w].means_)
    assert pickle.dumps(mine[4]) == before                       # a word in no transcript keeps its bytes


def _pickle_models(tmp_path, models, names, sub="trained_models", n_iter=15):
    d = tmp_path / sub / "gmmhmm"
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_gmmhmm_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / sub)


def test_decoder_train_embedded_over_gmmhmm_models(tmp_path):
    from sapr_amd.decoder import Decoder
    models, utts, truth, ref_models, history = _fit_case()
    dec = Decoder(models_dir=_pickle_models(tmp_path, models, NAMES), implementation="gmmhmm", n_iter=15)
    said = [[NAMES[w] for w in t] for t in truth]
    old = dec.decode_connected([x.T for x in utts[:4]])          # (packs the vocabulary from the old parameters)
    untouched = pickle.dumps(dec.models["four"])
    got = dec.train_embedded([x.T for x in utts], said, n_iter=3, tol=0.0)
    # (the load order of the words does not enter: an utterance's chain and a word's slots are the same)
    np.testing.assert_allclose(got, history, rtol=1e-9)
    for w in sorted({w for t in truth for w in t}):
        _check_params(dec.models[NAMES[w]], ref_models[w], NAMES[w])
    assert pickle.dumps(dec.models["four"]) == untouched
    new = dec.decode_connected([x.T for x in utts[:4]])          # (from the new parameters: the packs were dropped)
    again = Decoder(models_dir=_pickle_models(tmp_path, [dec.models[w] for w in NAMES], NAMES, sub="retrained"),
                    implementation="gmmhmm", n_iter=15)
    fresh = again.decode_connected([x.T for x in utts[:4]])
    assert [r["log_likelihood"] for r in new] == [r["log_likelihood"] for r in fresh]
    assert [r["words"] for r in new] == [r["words"] for r in fresh]
    assert [r["log_likelihood"] for r in new] != [r["log_likelihood"] for r in old]
    assert all(np.isfinite(r["log_likelihood"]) for r in new)
    with pytest.raises(ValueError, match="'seven'"):
        dec.train_embedded([utts[0].T], [["zero", "seven"]])
    with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
        dec.train_embedded([utts[0].T, utts[1].T], [["zero"]])

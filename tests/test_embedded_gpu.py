"""GPU: embedded Baum-Welch (csrc/connected_embed.hip) through the C ABI and the Python layer against the CPU
restatement tests/_embedded_ref.py.  Tolerances are the project's pins for the same quantities: rtol 1e-11 on
log-likelihoods (``RTOL_LL`` of tests/test_state_posteriors_gpu.py), rtol = atol = 1e-9 on posteriors and statistics
and rtol 1e-7 / 1e-6 on parameters after EM (tests/test_estep_gpu.py)."""
import ctypes as C
import pickle

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _connected_family_cases as cases
from tests import _connected_ref as ref
from tests import _embedded_ref as eref
from tests._synth import VOCAB, synth_feature_set, synth_utterance, trained_like_models, word_prototypes

pytestmark = pytest.mark.gpu

NEG = -np.inf
RTOL_LL = 1e-11
TOL = dict(rtol=1e-9, atol=1e-9)
STAT_KEYS = (("start", "start"), ("trans", "trans"), ("post_sum", "post"), ("obs", "obs"), ("obs2", "obs**2"))


def _check_loglik(got, want, what=""):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.array_equal(got[~fin], want[~fin]), what           # (-inf exactly; no NaN in these cases)
    worst = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0
    print(f"loglik {what}: max relative difference {worst:.3g}")
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL_LL, err_msg=str(what))


def _check_stats(res, want, W, D_keys=True, what=""):
    """``res``: an ``EmbeddedStats``; ``want``: the dict of ``_embedded_ref.estep_batch``."""
    for w in range(W):
        st = res.split(w)
        assert st["nobs"] == want["nobs"][w] and st["logprob"] == 0.0, (what, w)
        for k_ref, k_got in STAT_KEYS:
            if k_ref.startswith("obs") and not D_keys:
                continue
            err = np.max(np.abs(st[k_got] - want[k_ref][w]) / (1.0 + np.abs(want[k_ref][w])), initial=0.0)
            print(f"{what} word {w} {k_ref}: max scaled difference {err:.3g}")
            np.testing.assert_allclose(st[k_got], want[k_ref][w], err_msg=f"{what} {k_ref} word {w}", **TOL)


def _check_post(res, want_post, S, lengths, what=""):
    total = int(sum(lengths))
    got = res.post.reshape(total, -1, res.SP)
    assert not got[:, :, S:].any(), what                         # (padded states carry exact zeros)
    err = float(np.max(np.abs(got[:, :, :S] - want_post), initial=0.0))
    print(f"post {what}: max difference {err:.3g}")
    np.testing.assert_allclose(got[:, :, :S], want_post, err_msg=str(what), **TOL)
    offs = np.r_[0, np.cumsum(lengths)]
    for u in np.flatnonzero(~np.isfinite(res.loglik)):
        assert not res.post[offs[u]:offs[u + 1]].any(), (what, u)


# ---- the recursion over a given logb ----------------------------------------------------------------------------
@pytest.mark.parametrize("exits", aref.EXITS)
@pytest.mark.parametrize("topology", aref.TOPOLOGIES)
@pytest.mark.parametrize("W,S,max_words", aref.RECURSION_SHAPES)
def test_recursion_equals_reference(W, S, max_words, topology, exits):
    from sapr_amd.connected import ConnectedNetwork, embedded_forward_backward
    lengths = aref.RECURSION_LENGTHS
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, topology, exits, False)
    assert max(len(t) for t in transcripts) == max_words or max_words == 64
    pen = aref.PENALTIES[(aref.TOPOLOGIES.index(topology) + aref.EXITS.index(exits) + W) % 3]
    res = embedded_forward_backward(logb, lengths, transcripts, ConnectedNetwork(ls, lt, lx, word_penalty=pen),
                                    want_post=True)
    want = eref.estep_batch(logb, lengths, transcripts, ls, lt, lx, pen)
    what = (W, S, topology, exits, pen)
    _check_loglik(res.loglik, want["loglik"], what)
    assert int(np.isfinite(res.loglik).sum()) >= 6
    for u in (lengths.index(0), lengths.index(1), lengths.index(2)):
        assert res.loglik[u] == NEG
    _check_post(res, want["post"], S, lengths, what)
    _check_stats(res, want, W, D_keys=False, what=str(what))
    rows = res.post.sum(axis=1)
    offs = np.r_[0, np.cumsum(lengths)]
    for u in np.flatnonzero(np.isfinite(res.loglik)):
        np.testing.assert_allclose(rows[offs[u]:offs[u + 1]], 1.0, rtol=0, atol=1e-9)


# ---- the C ABI itself -------------------------------------------------------------------------------------------
def _raw_embed(logb, lengths, transcripts, ls, lt, lx, pen, max_words, feats=None, offs=None, woffs=None):
    """``sapr_connected_embed`` itself, with what the Python layer refuses: ``(loglik, stats[W, width], post)``."""
    import torch
    from sapr_amd import _lib
    from sapr_amd.connected import layout
    W, S = ls.shape
    SP = layout(W, S)[0]
    total = int(sum(lengths))
    wide = np.full((total, W, SP), NEG)
    wide[:, :, :S] = logb
    offs = np.r_[0, np.cumsum(lengths)].astype(np.int64) if offs is None else np.asarray(offs, np.int64)
    words = np.concatenate([np.asarray(t, np.int32) for t in transcripts]).astype(np.int32)
    woffs = (np.r_[0, np.cumsum([len(t) for t in transcripts])].astype(np.int64) if woffs is None
             else np.asarray(woffs, np.int64))
    D = 0 if feats is None else feats.shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    lib = _lib.load()
    n, width = C.c_size_t(0), C.c_int32(0)
    assert lib.sapr_connected_embed_workspace_bytes(total, len(lengths), len(words), max_words, S, D, C.byref(n)) == 0
    assert lib.sapr_connected_embed_stats_width(S, D, C.byref(width)) == 0
    guard = 4096                                                 # the bytes behind the workspace must stay untouched
    ws = torch.full((n.value + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    t_logb, t_offs, t_woffs, t_words, t_ls, t_lt, t_lx = (dev(a) for a in (wide, offs, woffs, words, ls, lt, lx))
    t_feats = None if feats is None else dev(np.asarray(feats, np.float32))
    loglik = torch.empty(len(lengths), dtype=torch.float64, device="cuda")
    stats = torch.full((W, width.value), np.nan, dtype=torch.float64, device="cuda")
    post = torch.zeros((total, max_words * SP), dtype=torch.float64, device="cuda")
    _lib.check(lib.sapr_connected_embed(
        _lib.ptr(t_logb), _lib.ptr(t_feats), D, _lib.ptr(t_offs), len(lengths), total, _lib.ptr(t_words),
        _lib.ptr(t_woffs), len(words), max_words, _lib.ptr(t_ls), _lib.ptr(t_lt), _lib.ptr(t_lx), pen, W, S,
        _lib.ptr(ws), n.value, _lib.ptr(loglik), _lib.ptr(stats), _lib.ptr(post), _lib.current_stream()),
        "sapr_connected_embed")
    torch.cuda.synchronize()
    assert bool((ws[n.value:] == 0xA5).all())
    return tuple(a.cpu().numpy() for a in (loglik, stats, post))


def _raw_stats(stats, S, D):
    from sapr_amd.trellis import split_stats
    return [split_stats(row, S, D) for row in stats]


def test_pathless_utterances_at_the_c_abi():
    """What the Python layer refuses earlier — a transcript longer than ``max_words``, word indices W and -1, offsets
    that leave the batch — makes its own utterance pathless: -inf, zero posterior rows, nothing in the statistics.
    The other utterances keep their bytes."""
    W, S, max_words, D = 5, 7, 4, 3
    ls, lt, lx, logb, _ = aref.recursion_case(W, S, 25, "skip", "any", False)
    lengths = [40, 64, 30, 3, 50, 20]
    logb = logb[:sum(lengths)]
    feats = np.random.default_rng(2).normal(0.0, 3.0, (sum(lengths), D)).astype(np.float32)
    good = [[1, 4, 4], [0, 2, 3, 1], [2], [3], [4, 0], [1, 1]]
    bad = [[1, 4, 4], [0, 2, 3, 1, 0], [W], [-1], [4, 0], [1, 1]]
    offs = np.r_[0, np.cumsum(lengths)]
    clean = _raw_embed(logb, lengths, good, ls, lt, lx, -1.5, max_words, feats)
    want_all = eref.estep_batch(logb, lengths, good, ls, lt, lx, -1.5, feats, max_words)
    assert np.isfinite(want_all["loglik"]).all()
    _check_loglik(clean[0], want_all["loglik"], "clean")

    def check(got, dead, want, what):
        for u in range(len(lengths)):
            rows = slice(offs[u], offs[u + 1])
            if u in dead:
                assert got[0][u] == NEG and not got[2][rows].any(), (what, u)
            else:
                assert got[0][u:u + 1].tobytes() == clean[0][u:u + 1].tobytes(), (what, u)
                assert got[2][rows].tobytes() == clean[2][rows].tobytes(), (what, u)
        for w, st in enumerate(_raw_stats(got[1], S, D)):
            assert st["nobs"] == want["nobs"][w] and st["logprob"] == 0.0
            for k_ref, k_got in STAT_KEYS:
                np.testing.assert_allclose(st[k_got], want[k_ref][w], err_msg=f"{what} {k_ref} {w}", **TOL)

    got = _raw_embed(logb, lengths, bad, ls, lt, lx, -1.5, max_words, feats)
    check(got, (1, 2, 3), eref.estep_batch(logb, lengths, bad, ls, lt, lx, -1.5, feats, max_words), "transcripts")
    # the last utterance's frames, then its transcript, leave the batch: served as empty
    only = [t if u < 5 else [] for u, t in enumerate(good)]
    want = eref.estep_batch(logb, lengths[:5] + [0], only, ls, lt, lx, -1.5, feats[:offs[5]], max_words)
    far = offs.copy()
    far[-1] += 7
    check(_raw_embed(logb, lengths, good, ls, lt, lx, -1.5, max_words, feats, offs=far), (5,), want, "offsets")
    wfar = np.r_[0, np.cumsum([len(t) for t in good])]
    wfar[-1] += 3
    check(_raw_embed(logb, lengths, good, ls, lt, lx, -1.5, max_words, feats, woffs=wfar), (5,), want, "word_offsets")


def test_a_nan_frame_makes_its_own_utterance_pathless():
    """A NaN met in the recursion makes the utterance's likelihood NaN (the two-term log-sum-exp alone would drop it):
    zero posterior rows, nothing in the statistics, every other utterance keeps its bytes."""
    W, S, max_words = 14, 18, 14
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, "dense", "any", False)
    lengths = aref.RECURSION_LENGTHS
    offs = np.r_[0, np.cumsum(lengths)]
    clean = _raw_embed(logb, lengths, transcripts, ls, lt, lx, -2.0, max_words)
    hit = lengths.index(300)
    assert np.isfinite(clean[0][hit])
    dirty = logb.copy()
    dirty[offs[hit] + 150] = np.nan
    got = _raw_embed(dirty, lengths, transcripts, ls, lt, lx, -2.0, max_words)
    want = eref.estep_batch(dirty, lengths, transcripts, ls, lt, lx, -2.0, None, max_words)
    assert np.isnan(want["loglik"][hit]) and np.isnan(got[0][hit])
    assert not got[2][offs[hit]:offs[hit + 1]].any()
    for u in range(len(lengths)):
        if u != hit:
            assert got[0][u:u + 1].tobytes() == clean[0][u:u + 1].tobytes()
            assert got[2][offs[u]:offs[u + 1]].tobytes() == clean[2][offs[u]:offs[u + 1]].tobytes()
    assert np.isfinite(got[1]).all()
    for w, st in enumerate(_raw_stats(got[1], S, 0)):
        assert st["nobs"] == want["nobs"][w]
        for k_ref, k_got in STAT_KEYS[:3]:
            np.testing.assert_allclose(st[k_got], want[k_ref][w], err_msg=f"{k_ref} {w}", **TOL)


def test_two_calls_return_the_same_bytes():
    W, S, max_words, D = 11, 18, 5, 13
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, "dense", "any", False)
    lengths = aref.RECURSION_LENGTHS
    feats = np.random.default_rng(4).normal(0.0, 3.0, (sum(lengths), D)).astype(np.float32)
    a, b = (_raw_embed(logb, lengths, transcripts, ls, lt, lx, -2.0, max_words, feats) for _ in range(2))
    assert np.isfinite(a[0]).sum() >= 6 and np.isfinite(a[1]).all()
    for x, y, name in zip(a, b, ("loglik", "stats", "post")):
        assert x.tobytes() == y.tobytes(), name


# ---- observation sums -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 13, 26, 39])
def test_observation_sums(D):
    from sapr_amd.connected import ConnectedNetwork, embedded_forward_backward
    W, S = 4, 5
    rng = np.random.default_rng(300 + D)
    ls, lt, lx = aref.network(rng, W, S, "skip", "last", False)
    lengths = [33, 70, 12, 129, 2, 48]
    transcripts = [[2, 2, 2], [0, 1, 2, 3, 0], [3], [1, 1, 3, 3, 1, 1, 0], [0, 1, 2], [2, 0]]   # (utterance 4: K > T)
    logb = rng.normal(-40.0, 15.0, (sum(lengths), W, S))
    feats = rng.normal(0.0, 8.0, (sum(lengths), D)).astype(np.float32)
    res = embedded_forward_backward(logb, lengths, transcripts, ConnectedNetwork(ls, lt, lx, word_penalty=-4.0),
                                    feats=feats)
    want = eref.estep_batch(logb, lengths, transcripts, ls, lt, lx, -4.0, feats)
    assert np.isfinite(want["loglik"]).sum() == 5 and want["loglik"][4] == NEG
    assert res.stats.shape == (W, 2 + S + S * S + S + 2 * S * D) and res.post is None
    _check_loglik(res.loglik, want["loglik"], D)
    _check_stats(res, want, W, what=f"D={D}")
    assert np.abs(want["obs2"]).max() > 100.0


# ---- tie to the isolated-word E-step --------------------------------------------------------------------------
@pytest.mark.parametrize("ns,D", [(8, 13), (16, 39)])
def test_one_word_with_any_exit_equals_the_isolated_word_estep(ns, D):
    """Two float64 implementations of the same lattice (other emission order, other log-sum-exp order) differ in
    every alpha by the roundings of its additions: about ulp(|loglik|) / 2 per add, a random walk over the ~3 T adds
    of a path.  At D = 39 a frame scores about -125, so T = 70 gives |loglik| near 9000 and posteriors that agree to
    about 1e-11 relative; times features of magnitude 100 - 300 that is above the 1e-9 the statistics are pinned at
    wherever a sum cancels to O(1) (measured: one element of 702 off by 2.3e-9).  Utterances of at most 30 frames
    keep |loglik| below 4096 (half the ulp, 0.65 of the walk): about 4e-12 x 100 = 4e-10."""
    import torch
    from sapr_amd.connected import ConnectedNetwork, embedded_estep
    from sapr_amd.trellis import DiagModelPack, EStep, FeatureBatch, forward_loglik
    W, S = 3, ns + 2
    sp, A, mu, cv = trained_like_models(W, ns, D, seed=41)
    _, flat = synth_feature_set(VOCAB[:W], 6, D=D, seed=17, tmin=1, tmax=31)
    utts = [np.ascontiguousarray(f.T) for f in flat]
    utt_model = np.repeat(np.arange(W), 6)
    packed = np.ascontiguousarray(np.concatenate(utts, axis=0), dtype=np.float32)
    batch = FeatureBatch.from_packed(torch.from_numpy(packed).cuda(), np.asarray([u.shape[0] for u in utts]))
    pack = DiagModelPack.from_params(sp, A, mu, cv)
    es = EStep(batch, utt_model, W, S)
    iso = es.run(pack).cpu().numpy()
    ll = forward_loglik(batch, pack, utt_model).cpu().numpy()
    with np.errstate(divide="ignore"):
        net = ConnectedNetwork(np.log(sp), np.log(A), np.zeros((W, S)), -5.0, None, mu, cv,
                               D * np.log(2 * np.pi) + np.log(cv).sum(axis=-1))
    res = embedded_estep(utts, [[int(w)] for w in utt_model], net)
    np.testing.assert_allclose(res.loglik, ll, rtol=RTOL_LL)
    for w in range(W):
        want, got = es.split(iso[w]), res.split(w)
        assert got["nobs"] == want["nobs"] == 6
        for key in ("start", "trans", "post", "obs", "obs**2"):
            err = np.max(np.abs(got[key] - want[key]) / (1.0 + np.abs(want[key])))
            print(f"(S, D) = ({S}, {D}) word {w} {key}: max scaled difference {err:.3g}")
            np.testing.assert_allclose(got[key], want[key], err_msg=f"{key} word {w}", **TOL)


# ---- all three emission families ------------------------------------------------------------------------------
@pytest.mark.parametrize("family,spec", [("diag", ref.E2E_CASES[3]), ("gmm", cases.GMM_CASES[0]),
                                         ("full", cases.FULL_CASES[0])])
def test_loglik_and_posteriors_for_every_family(family, spec):
    """``embedded_estep`` against the restatement fed the emitted ``logb`` read back from the device."""
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
    want = eref.estep_batch(logb, lengths, truth, net.log_start, net.log_trans, net.log_exit, pen)
    assert np.isfinite(want["loglik"]).all()
    res = embedded_estep(utts, truth, net, want_post=True, want_stats=family == "diag")
    _check_loglik(res.loglik, want["loglik"], family)
    _check_post(res, want["post"], net.S, lengths, family)
    assert (res.stats is None) == (family != "diag")
    if family != "diag":
        with pytest.raises(NotImplementedError, match=repr(family)):
            embedded_estep(utts, truth, net)


# ---- embedded_fit and Decoder.train_embedded ------------------------------------------------------------------
NAMES = ["zero", "one", "two", "three"]                          # "three" is in no transcript


def _fit_case():
    """W = 3 spoken words (and one that never occurs), S = 4, D = 5: 24 recordings of 2-4 words, each word 8-16
    frames of tests/_synth.py's piecewise-constant segments; models perturbed from the prototypes."""
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    rng = np.random.default_rng(77)
    S, D = 4, 5
    protos = word_prototypes(NAMES, D, n_seg=S, seed=5)
    utts, truth = [], []
    for _ in range(24):
        words = rng.integers(0, 3, int(rng.integers(2, 5))).tolist()
        utts.append(np.concatenate([synth_utterance(rng, protos[NAMES[w]], int(rng.integers(8, 17))).T
                                    for w in words]).astype(np.float32))
        truth.append(words)
    models = []
    for w, name in enumerate(NAMES):
        m = GaussianHMM(n_components=S, covariance_type="spherical" if w == 1 else "diag")
        m.startprob_ = np.array([1.0, 0.0, 0.0, 0.0])
        m.transmat_ = np.array([[0.7, 0.3, 0, 0], [0, 0.7, 0.3, 0], [0, 0, 0.7, 0.3], [0, 0, 0, 1.0]])
        mu = protos[name] + rng.normal(0.0, 4.0, (S, D))
        mu[:, 0] -= 300.0
        m.means_ = mu
        m._covars_ = np.full(S, 60.0) if w == 1 else np.full((S, D), 60.0)
        models.append(m)
    return models, utts, truth


@pytest.fixture(scope="module")
def fit_case():
    models, utts, truth = _fit_case()
    ref_models, history = eref.fit(models, utts, truth, n_iter=3, tol=0.0)
    return models, utts, truth, ref_models, history


def _check_params(got, want, what):
    np.testing.assert_allclose(got.startprob_, want.startprob_, rtol=1e-7, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(got.transmat_, want.transmat_, rtol=1e-7, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(got.means_, want.means_, rtol=1e-7, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(got._covars_, want._covars_, rtol=1e-6, atol=1e-9, err_msg=what)


def test_embedded_fit(fit_case):
    import copy
    from sapr_amd.connected import embedded_fit
    models, utts, truth, ref_models, history = fit_case
    assert len(history) == 3 and history[-1] > history[0]
    mine = [copy.deepcopy(m) for m in models]
    before = pickle.dumps(mine[3])
    got = embedded_fit(mine, utts, truth, n_iter=3, tol=0.0, names=NAMES)
    np.testing.assert_allclose(got, history, rtol=1e-9)
    for w in range(3):
        _check_params(mine[w], ref_models[w], NAMES[w])
        assert not np.array_equal(mine[w].means_, models[w].means_)
    assert mine[1]._covars_.shape == (4,)
    assert pickle.dumps(mine[3]) == before                       # a word in no transcript keeps its bytes


def _pickle_models(tmp_path, models, names, sub="trained_models", n_iter=15):
    d = tmp_path / sub / "hmmlearn"
    d.mkdir(parents=True, exist_ok=True)
    for m, word in zip(models, names):
        with open(d / f"{word}_hmmlearn_{n_iter}.pkl", "wb") as f:
            pickle.dump(m, f)
    return str(tmp_path / sub)


def test_decoder_train_embedded(tmp_path, fit_case):
    from sapr_amd.decoder import Decoder
    models, utts, truth, _, _ = fit_case
    dec = Decoder(models_dir=_pickle_models(tmp_path, models, NAMES), implementation="hmmlearn", n_iter=15)
    order = [NAMES.index(w) for w in dec.vocab]                  # load order (glob) is the word order of the network
    rank = {w: k for k, w in enumerate(order)}
    ref_models, history = eref.fit([models[w] for w in order], utts, [[rank[w] for w in t] for t in truth], n_iter=3,
                                   tol=0.0)
    said = [[NAMES[w] for w in t] for t in truth]
    untouched = pickle.dumps(dec.models["three"])
    got = dec.train_embedded([x.T for x in utts], said, n_iter=3, tol=0.0)
    np.testing.assert_allclose(got, history, rtol=1e-9)
    for k, word in enumerate(dec.vocab):
        _check_params(dec.models[word], ref_models[k], word)
    assert pickle.dumps(dec.models["three"]) == untouched
    # the trained models round-trip through pickles and a fresh Decoder
    again = Decoder(models_dir=_pickle_models(tmp_path, [dec.models[w] for w in NAMES], NAMES, sub="retrained"),
                    implementation="hmmlearn", n_iter=15)
    a = dec.align([x.T for x in utts[:4]], said[:4])
    b = again.align([x.T for x in utts[:4]], said[:4])
    assert [r["log_likelihood"] for r in a] == [r["log_likelihood"] for r in b]
    assert all(np.isfinite(r["log_likelihood"]) and r["words"] == s for r, s in zip(a, said))
    with pytest.raises(ValueError, match="'seven'"):
        dec.train_embedded([utts[0].T], [["zero", "seven"]])
    with pytest.raises(ValueError, match="1 transcripts for 2 utterances"):
        dec.train_embedded([utts[0].T, utts[1].T], [["zero"]])


def test_decoder_train_embedded_refuses_other_implementations(tmp_path):
    from sapr_amd.decoder import Decoder
    d = tmp_path / "trained_models" / "custom"
    d.mkdir(parents=True)
    with open(d / "zero_custom_15.pkl", "wb") as f:
        pickle.dump({"placeholder": "custom"}, f)
    with pytest.raises(ValueError, match="implementation='custom'"):
        Decoder(models_dir=str(tmp_path / "trained_models"), implementation="custom").train_embedded(
            [np.zeros((13, 4), np.float32)], [["zero"]])

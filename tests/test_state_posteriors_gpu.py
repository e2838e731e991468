"""GPU parity of the state posteriors and MAP decoding (state_posteriors.hip: sapr_state_posteriors_diag,
trellis.state_posteriors, torch.ops.sapr.hmm_state_posteriors, GaussianHMM.score_samples / predict_proba /
decode(algorithm="map"), Decoder.state_posteriors) against the numpy restatement of hmmlearn
(oracle/hmmlearn_oracle.py: log_density_diag, forward_log, backward_log, posteriors).

float64 both sides; the quick emission form and the device exp / log differ from the CPU evaluation in the last ulps:
rtol 1e-11 on log-likelihoods (the existing pin for forward scores), rtol 1e-9 / atol 1e-9 on the posteriors (the
existing pin for posterior-derived statistics in test_estep_gpu.py).  The arg-max path must equal np.argmax of the
oracle's lattice on EVERY frame, none left out.  Smallest gap between the two largest posteriors of a frame, computed
on the CPU from the oracle alone for exactly these inputs (all log-likelihoods finite):
    68 utterances   (13, 8) 2.99e-1   (39, 16) 5.27e-1   (13, 16) 4.19e-2   (39, 8) 3.39e-1
                    dense (13, 8) 2.46e-3   dense (39, 16) 8.02e-4   padded (26, 5) 1.70e-2   (5, 1) 4.30e-1
    330 utterances  (13, 8) 1.71e-2   dense (13, 8) 4.29e-3
— the smallest is five orders of magnitude above twice the 1e-9 tolerance, so a rule that excludes near-ties would only
hide a failure (each case asserts its gap above 1e-4 before it compares paths).

Every utterance u is scored under model u % 11; the oracle's lattices are computed once per case and shared."""
import ctypes
import functools
import pickle

import numpy as np
import pytest

from oracle import hmmlearn_oracle as ho
from tests._synth import VOCAB, synth_feature_set, trained_like_models

pytestmark = pytest.mark.gpu

RTOL_LL = 1e-11
TOL_POST = 1e-9


def _batch(utts_td, lengths=None):
    import torch
    from sapr_amd.trellis import FeatureBatch
    D = utts_td[0].shape[1]
    packed = np.ascontiguousarray(np.concatenate(utts_td, axis=0), dtype=np.float32).reshape(-1, D)
    return FeatureBatch.from_packed(torch.from_numpy(packed).cuda(),
                                    np.asarray([u.shape[0] for u in utts_td] if lengths is None else lengths))


def _models(ns, D, seed, dense=False):
    sp, A, mu, cv = trained_like_models(11, ns, D, seed)
    if dense:  # drawn as in test_forward_vocab_gpu._models
        S = ns + 2
        rng = np.random.default_rng(1)
        A = rng.dirichlet(np.ones(S), (11, S))
        sp = rng.dirichlet(np.ones(S), 11)
    return sp, A, mu, cv


def _utterances(D, n_per_word):
    _, flat = synth_feature_set(VOCAB, n_per_word, D=D, seed=21, tmin=1, tmax=110)
    utts = [np.ascontiguousarray(f.T) for f in flat]
    if n_per_word == 6:  # T = 1 and T = 2, and one utterance past the first wavefront
        longest = max(utts, key=lambda a: a.shape[0])
        utts += [np.ascontiguousarray(longest[:1]), np.ascontiguousarray(longest[:2])]
    return utts


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(D, ns, dense=False, seed=3, n_per_word=6):
    """Inputs and the oracle's results of one shape, computed once: ll[N], post[total_frames, S], path, min gap."""
    c = _Case()
    c.D, c.S = D, ns + 2
    c.sp, c.A, c.mu, c.cv = _models(ns, D, seed, dense)
    c.utts = _utterances(D, n_per_word)
    c.utt_model = np.arange(len(c.utts)) % 11
    ll, rows = [], []
    for u, X in enumerate(c.utts):
        w = c.utt_model[u]
        logB = ho.log_density_diag(X, c.mu[w], c.cv[w])
        lp, fwd = ho.forward_log(c.sp[w], c.A[w], logB)
        rows.append(ho.posteriors(fwd, ho.backward_log(c.sp[w], c.A[w], logB)))
        ll.append(lp)
    c.ll, c.post = np.asarray(ll), np.concatenate(rows, axis=0)
    c.offs = np.r_[0, np.cumsum([X.shape[0] for X in c.utts])]
    c.path = np.argmax(c.post, axis=1)
    if c.S > 1:
        top = np.sort(c.post, axis=1)
        c.gap = float((top[:, -1] - top[:, -2]).min())
    else:
        c.gap = 1.0
    for a in (c.ll, c.post, c.path):
        a.setflags(write=False)
    return c


def _run(c, **kw):
    from sapr_amd.trellis import DiagModelPack, state_posteriors
    pack = DiagModelPack.from_params(c.sp, c.A, c.mu, c.cv)
    return state_posteriors(_batch(c.utts), pack, c.utt_model, **kw), pack


def _check_against_oracle(c, res):
    ll, post, path = res.loglik.cpu().numpy(), res.post.cpu().numpy(), res.path.cpu().numpy()
    assert np.isfinite(c.ll).all() and np.isfinite(ll).all()
    print(f"({c.D}, {c.S - 2}) max relative error of loglik: {(np.abs(ll - c.ll) / np.abs(c.ll)).max():.3e}; "
          f"max absolute error of post: {np.abs(post - c.post).max():.3e}; oracle min gap {c.gap:.3e}; "
          f"path differs on {int((path != c.path).sum())} of {path.size} frames")
    np.testing.assert_allclose(ll, c.ll, rtol=RTOL_LL)
    assert post.shape == c.post.shape and post.shape[1] == c.S and post.dtype == np.float64   # S_model columns
    np.testing.assert_allclose(post, c.post, rtol=TOL_POST, atol=TOL_POST)
    assert (post >= 0).all()
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0.0, atol=1e-12)
    assert c.gap > 1e-4                                 # no near-tie in these inputs: nothing is excluded below
    assert path.dtype == np.int32
    np.testing.assert_array_equal(path, c.path)          # every frame, none left out


SHAPES = [(13, 8, False, 3), (39, 16, False, 3), (13, 16, False, 3), (39, 8, False, 3), (13, 8, True, 3),
          (39, 16, True, 3), (26, 5, False, 5), (5, 1, False, 5)]


@pytest.mark.parametrize("D,ns,dense,seed", SHAPES)
def test_posteriors_and_map_path_match_the_oracle(D, ns, dense, seed):
    from sapr_amd import _lib
    c = _case(D, ns, dense, seed)
    lengths = [X.shape[0] for X in c.utts]
    assert len(c.utts) == 68 and sorted(lengths)[:2] == [1, 2] and max(lengths) >= 100
    res, pack = _run(c)
    assert pack.topology == (_lib.TOPO_DENSE if dense else _lib.TOPO_BIDIAG)
    assert pack.S in (10, 18) and pack.D in (13, 39) and (pack.S_model, pack.D_model) == (ns + 2, D)
    _check_against_oracle(c, res)


@pytest.mark.parametrize("dense", [False, True])
def test_workgroup_and_tile_boundaries(dense):
    """330 utterances over 11 models: more than 256 slots, every tile partly filled, tiles ordered by model."""
    c = _case(13, 8, dense, 3, n_per_word=30)
    lengths = [X.shape[0] for X in c.utts]
    assert len(c.utts) == 330 and min(lengths) == 1 and max(lengths) == 109
    res, _ = _run(c)
    _check_against_oracle(c, res)


def test_each_utterance_is_a_function_of_its_own_pair():
    import torch
    from sapr_amd import _lib
    from sapr_amd.trellis import DiagModelPack, state_posteriors
    c = _case(13, 8)
    full, pack = _run(c)
    # reversed batch order: the same bits per utterance
    rev = state_posteriors(_batch(c.utts[::-1]), pack, c.utt_model[::-1].copy())
    assert torch.equal(rev.loglik.flip(0), full.loglik)
    roffs = np.r_[0, np.cumsum([X.shape[0] for X in c.utts[::-1]])]
    n = len(c.utts)
    for u in range(n):
        lo, hi = c.offs[u], c.offs[u + 1]
        rlo, rhi = roffs[n - 1 - u], roffs[n - u]
        assert torch.equal(rev.post[rlo:rhi], full.post[lo:hi]) and torch.equal(rev.path[rlo:rhi], full.path[lo:hi])
    # one output at a time: the other one keeps its bits
    only_path, _ = _run(c, want_post=False)
    assert only_path.post is None and torch.equal(only_path.path, full.path)
    assert torch.equal(only_path.loglik, full.loglik)
    only_post, _ = _run(c, want_path=False)
    assert only_post.path is None and torch.equal(only_post.post, full.post)
    with pytest.raises(ValueError):
        _run(c, want_post=False, want_path=False)
    # exact-kernel operands only
    lean = DiagModelPack.from_params(c.sp, c.A, c.mu, c.cv, exact_only=True)
    assert lean.flags & _lib.PACK_EXACT_ONLY
    got = state_posteriors(_batch(c.utts), lean, c.utt_model)
    assert torch.equal(got.loglik, full.loglik) and torch.equal(got.post, full.post)
    assert torch.equal(got.path, full.path)


@pytest.mark.parametrize("dense", [False, True])
def test_agreement_with_the_estep(dense):
    """sum_t gamma_t over a word's utterances = the E-step's stats['post'], the sum of the first rows = stats['start']."""
    from sapr_amd.trellis import DiagModelPack, EStep, state_posteriors
    c = _case(13, 8, dense, 3, n_per_word=30)
    batch = _batch(c.utts)
    pack = DiagModelPack.from_params(c.sp, c.A, c.mu, c.cv)
    es = EStep(batch, c.utt_model, 11, c.S)
    stats = es.run(pack).cpu().numpy()
    post = state_posteriors(batch, pack, c.utt_model, want_path=False).post.cpu().numpy()
    for w in range(11):
        st = es.split(stats[w])
        mine = [u for u in range(len(c.utts)) if c.utt_model[u] == w]
        occ = sum(post[c.offs[u]:c.offs[u + 1]].sum(axis=0) for u in mine)
        first = sum(post[c.offs[u]] for u in mine)
        np.testing.assert_allclose(occ, st["post"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(first, st["start"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("D,ns", [(13, 8), (39, 16)])
def test_one_forward_recursion_behind_three_entry_points(D, ns, dense):
    """The vocabulary scorer, the posteriors' first pass and the E-step's forward pass are one device body
    (diag_forward.h) on the same values: the log-likelihood of utterance u under model u % 11 is the same float64 from
    all three, bit for bit.  75 utterances (two wavefronts); the prefixes of 3 .. 9 frames, with the T = 1 and T = 2
    of the case, end the two- and the four-frame walk on every remainder."""
    from sapr_amd.trellis import DiagModelPack, EStep, forward_scores, state_posteriors
    c = _case(D, ns, dense)
    longest = max(c.utts, key=lambda a: a.shape[0])
    utts = list(c.utts) + [np.ascontiguousarray(longest[:n]) for n in range(3, 10)]
    assert len(utts) == 75 and {X.shape[0] for X in utts} >= set(range(1, 10))
    utt_model = np.arange(len(utts)) % 11
    batch = _batch(utts)
    pack = DiagModelPack.from_params(c.sp, c.A, c.mu, c.cv)
    vocab = forward_scores(batch, pack, want_post=False).loglik.cpu().numpy()[np.arange(len(utts)), utt_model]
    posteriors = state_posteriors(batch, pack, utt_model, want_post=False).loglik.cpu().numpy()
    es = EStep(batch, utt_model, 11, c.S)
    es.run(pack)
    estep = es.loglik.cpu().numpy()
    assert np.isfinite(vocab).all()
    assert np.array_equal(vocab, posteriors), f"{int((vocab != posteriors).sum())} of {len(utts)} utterances differ"
    assert np.array_equal(vocab, estep), f"{int((vocab != estep).sum())} of {len(utts)} utterances differ"


def _capi(batch, pack, layout, post, path, n_out=None, guard=0):
    """sapr_state_posteriors_diag on caller-owned buffers; ``guard`` elements in front of post / path are skipped."""
    import torch
    from sapr_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    _lib.check(lib.sapr_state_posteriors_workspace_bytes(layout.n_tiles, pack.S, batch.max_T, pack.topology,
                                                         ctypes.byref(nb)), "sapr_state_posteriors_workspace_bytes")
    ws = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device="cuda")
    loglik = torch.zeros(batch.n_utts, dtype=torch.float64, device="cuda")
    _lib.check(lib.sapr_state_posteriors_diag(
        _lib.ptr(batch.feats), _lib.ptr(batch.offsets), _lib.ptr(layout.slot_utt), _lib.ptr(layout.tile_model),
        layout.n_tiles, batch.D, batch.max_T, _lib.ptr(pack.blob), pack.W, pack.S, pack.topology,
        n_out or pack.S_model, _lib.ptr(ws), int(nb.value), _lib.ptr(loglik),
        ctypes.c_void_p(post.data_ptr() + 8 * guard), ctypes.c_void_p(path.data_ptr() + 4 * guard),
        _lib.current_stream()), "sapr_state_posteriors_diag")
    torch.cuda.synchronize()
    return loglik


def test_store_discipline_through_the_c_abi():
    import torch
    from sapr_amd.trellis import DiagModelPack, TileLayout, state_posteriors
    c = _case(13, 8)
    batch = _batch(c.utts)
    pack = DiagModelPack.from_params(c.sp, c.A, c.mu, c.cv)
    layout = TileLayout.build(batch.lengths, c.utt_model, pack.W, "cuda")
    G, total = 4096, batch.total_frames
    SENT64, SENT32 = 0x7FF8DEADBEEF1234, 0x5EA7BEEF
    post = torch.full((G + total * c.S + G,), SENT64, dtype=torch.int64, device="cuda")
    path = torch.full((G + total + G,), SENT32, dtype=torch.int32, device="cuda")
    loglik = _capi(batch, pack, layout, post, path, guard=G)
    for buf, sent, n in ((post, SENT64, total * c.S), (path, SENT32, total)):
        assert bool((buf[:G] == sent).all()) and bool((buf[G + n:] == sent).all())     # every sentinel intact
    ref = state_posteriors(batch, pack, c.utt_model)
    assert torch.equal(post[G:G + total * c.S].view(torch.float64).view(total, c.S), ref.post)
    assert torch.equal(path[G:G + total], ref.path) and torch.equal(loglik, ref.loglik)
    # fewer output states than the model has: the leading columns, rows packed at the narrower width
    post3 = torch.full((G + total * 3 + G,), SENT64, dtype=torch.int64, device="cuda")
    _capi(batch, pack, layout, post3, path, n_out=3, guard=G)
    assert bool((post3[:G] == SENT64).all()) and bool((post3[G + total * 3:] == SENT64).all())
    assert torch.equal(post3[G:G + total * 3].view(torch.float64).view(total, 3), ref.post[:, :3].contiguous())

    # an utterance without frames between two others: -inf, no rows, the neighbours' rows unchanged
    a, b = c.utts[3], c.utts[40]
    um = np.asarray([2, 2, 5])
    with_empty = state_posteriors(_batch([a, b], lengths=[a.shape[0], 0, b.shape[0]]), pack, um)
    without = state_posteriors(_batch([a, b]), pack, um[[0, 2]])
    ll = with_empty.loglik.cpu().numpy()
    assert ll[1] == -np.inf and np.isfinite(ll[[0, 2]]).all()
    assert torch.equal(with_empty.loglik[[0, 2]], without.loglik)
    assert with_empty.post.shape == (a.shape[0] + b.shape[0], c.S)
    assert torch.equal(with_empty.post, without.post) and torch.equal(with_empty.path, without.path)


def _hmm(c, w, **kw):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    m = GaussianHMM(n_components=c.S, covariance_type="diag", **kw)
    m.startprob_, m.transmat_, m.means_, m._covars_ = c.sp[w], c.A[w], c.mu[w], c.cv[w]
    return m


def test_gaussian_hmm_score_samples_predict_proba_and_map_decode():
    c = _case(13, 8)
    w = 4
    m = _hmm(c, w)
    seqs = [c.utts[u] for u in (4, 15, 66, 67, 26)]      # (T = 1 and T = 2 among them)
    for group in ([seqs[0]], seqs):
        X = np.ascontiguousarray(np.concatenate(group, axis=0))
        lengths = [s.shape[0] for s in group]
        ref_ll, ref_post = 0.0, []
        for s in group:
            logB = ho.log_density_diag(s, c.mu[w], c.cv[w])
            lp, fwd = ho.forward_log(c.sp[w], c.A[w], logB)
            ref_ll += lp
            ref_post.append(ho.posteriors(fwd, ho.backward_log(c.sp[w], c.A[w], logB)))
        ref_map = sum(float(np.max(p, axis=1).sum()) for p in ref_post)
        ref_post = np.concatenate(ref_post, axis=0)
        arg = None if len(group) == 1 else lengths
        lp, post = m.score_samples(X, arg)
        assert isinstance(lp, float) and post.shape == (X.shape[0], c.S) and post.dtype == np.float64
        np.testing.assert_allclose(lp, ref_ll, rtol=RTOL_LL)
        np.testing.assert_allclose(post, ref_post, rtol=TOL_POST, atol=TOL_POST)
        np.testing.assert_array_equal(m.predict_proba(X, arg), post)
        mlp, st = m.decode(X, arg, algorithm="map")
        np.testing.assert_array_equal(st, np.argmax(ref_post, axis=1))
        np.testing.assert_allclose(mlp, ref_map, rtol=1e-9)
        mm = _hmm(c, w, algorithm="map")
        np.testing.assert_array_equal(mm.predict(X, arg), np.argmax(ref_post, axis=1))
        got = mm.decode(X, arg)
        assert got[0] == mlp and np.array_equal(got[1], st)
        # Viterbi stays what it was: the oracle's bits, with the keyword and without
        vlp, vst = m.decode(X, arg)
        elp, est = m.decode(X, arg, algorithm="viterbi")
        assert vlp == elp and np.array_equal(vst, est)
        if len(group) == 1:
            rlp, rst = ho.decode(X, c.sp[w], c.A[w], c.mu[w], c.cv[w], tie="high")
            assert vlp == rlp and np.array_equal(vst, rst)
        got = mm.decode(X, arg, algorithm="viterbi")
        assert got[0] == vlp and np.array_equal(got[1], vst)
    m2 = pickle.loads(pickle.dumps(_hmm(c, w, algorithm="map")))
    assert m2.algorithm == "map"
    np.testing.assert_array_equal(m2.predict(seqs[1]), m.decode(seqs[1], algorithm="map")[1])
    with pytest.raises(ValueError):
        m.decode(seqs[1], algorithm="posterior")


def test_torch_op_is_the_same_launch():
    import torch
    import sapr_amd.torch_ops  # noqa: F401  (registers torch.ops.sapr.*)
    from sapr_amd.trellis import DiagModelPack, TileLayout, state_posteriors
    c = _case(13, 8)
    batch = _batch(c.utts)
    pack = DiagModelPack.from_params(c.sp, c.A, c.mu, c.cv)
    layout = TileLayout.build(batch.lengths, c.utt_model, pack.W, "cuda")
    ref = state_posteriors(batch, pack, layout=layout)
    ll, post, path = torch.ops.sapr.hmm_state_posteriors(batch.feats, batch.offsets, layout.slot_utt, layout.tile_model,
                                                         pack.blob, pack.W, pack.S, pack.D, batch.max_T, pack.topology,
                                                         pack.S_model)
    assert torch.equal(ll, ref.loglik) and torch.equal(post, ref.post) and torch.equal(path, ref.path)
    with pytest.raises((RuntimeError, NotImplementedError)):       # no CPU implementation
        torch.ops.sapr.hmm_state_posteriors(batch.feats.cpu(), batch.offsets.cpu(), layout.slot_utt.cpu(),
                                            layout.tile_model.cpu(), pack.blob.cpu(), pack.W, pack.S, pack.D,
                                            batch.max_T, pack.topology, pack.S_model)


def test_decoder_state_posteriors(tmp_path):
    from sapr_amd.decoder import Decoder
    from sapr_amd.trellis import DiagModelPack, FeatureBatch, state_posteriors
    c = _case(13, 8)
    d = tmp_path / "trained_models" / "hmmlearn"
    d.mkdir(parents=True)
    for w, word in enumerate(VOCAB):
        with open(d / f"{word}_hmmlearn_15.pkl", "wb") as f:
            pickle.dump(_hmm(c, w), f)
    dec = Decoder(models_dir=str(tmp_path / "trained_models"))
    order = [VOCAB.index(w) for w in dec.vocab]                # load order (glob) is the model index
    flat = [np.ascontiguousarray(X.T) for X in c.utts]         # (D, T) arrays, as mfcc_extract stores them
    pack = DiagModelPack.from_params(c.sp[order], c.A[order], c.mu[order], c.cv[order])
    batch = FeatureBatch.from_arrays(flat, layout="DT")

    def lattices(words):
        um = np.asarray([dec.vocab.index(w) for w in words])
        post = state_posteriors(batch, pack, um, want_path=False).post.cpu().numpy()
        return [post[c.offs[u]:c.offs[u + 1]] for u in range(len(flat))]

    best = [word for word, _, _ in dec.decode_batch(flat)]
    assert all(w is not None for w in best)
    got = dec.state_posteriors(flat)
    assert len(got) == len(flat)
    for u, (g, r) in enumerate(zip(got, lattices(best))):
        assert g.shape == (c.utts[u].shape[0], c.S) and g.dtype == np.float64
        np.testing.assert_array_equal(g, r)
    named = [VOCAB[u % 11] for u in range(len(flat))]
    for g, r in zip(dec.state_posteriors(flat, words=named), lattices(named)):
        np.testing.assert_array_equal(g, r)
    # ... which is the oracle's lattice under model u % 11
    np.testing.assert_allclose(np.concatenate(dec.state_posteriors(flat, words=named)), c.post, rtol=TOL_POST,
                               atol=TOL_POST)
    with pytest.raises(ValueError):
        dec.state_posteriors(flat, words=named[:-1])
    with pytest.raises(ValueError):
        dec.state_posteriors(flat[:1], words=["nosuchword"])


@pytest.mark.parametrize("D,S", [(40, 10), (13, 19)])
def test_unsupported_shapes_are_refused(D, S):
    import torch
    from sapr_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    _lib.check(lib.sapr_state_posteriors_workspace_bytes(1, S, 4, _lib.TOPO_BIDIAG, ctypes.byref(nb)), "workspace")
    buf = torch.zeros(max(int(nb.value), 1 << 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.SaprHipError, match=r"\{13,39\}x\{10,18\}"):
        _lib.check(lib.sapr_state_posteriors_diag(_lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 1, D, 4,
                                                  _lib.ptr(buf), 1, S, _lib.TOPO_BIDIAG, S, _lib.ptr(buf),
                                                  int(nb.value), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf),
                                                  _lib.current_stream()), "sapr_state_posteriors_diag")
    assert lib.sapr_state_posteriors_diag(_lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 1, D, 4,
                                          _lib.ptr(buf), 1, S, _lib.TOPO_BIDIAG, S, _lib.ptr(buf), int(nb.value),
                                          _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.current_stream()) == -2

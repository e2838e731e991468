"""CPU: the full-covariance vocabulary-scoring entry points (sapr_full_vocab, sapr_full_vocab_workspace_bytes) are
declared, bound and exported and report their argument errors before any HIP call; ``Decoder`` routes a vocabulary
with full / tied models to the full-covariance path; and the conditions under which tests/test_full_vocab_gpu.py may
compare EVERY utterance hold for the seeded cases, asserted from the numpy reference alone.  No compute call is made —
there is no GPU in the build container."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from sapr_amd import _lib
from tests import _full_vocab_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -2
P = ctypes.c_void_p(256)     # a dummy non-NULL pointer (never dereferenced on the paths exercised here)


# ---- the cases: no word and no path arg-max near a tie --------------------------------------------------------------
def _conditions(tag, utts, params, want):
    """Scores of utterances with frames are finite; the top-two word gap is above 1e-8 max|score| (rtol 1e-11 moves a
    score by 1e-11 max|score|: a thousand times less); no arg-max on the winner's Viterbi path is within 1e-9."""
    live = np.array([x.shape[0] > 0 for x in utts])
    for mode in vc.MODES:
        sc, bw = want[mode]
        assert sc.shape == (len(utts), len(params))
        assert np.all(np.isfinite(sc[live])) and np.all(np.isneginf(sc[~live])), (tag, mode)
        assert np.all(bw[live] >= 0) and np.all(bw[~live] == -1)
        gap, top = vc.top_two_gap(sc), np.abs(sc[live]).max()
        pgap = vc.winner_path_gap(utts, params, bw)
        print(f"{tag} {mode}: top-two word gap {gap:.3g}, max |score| {top:.3g}, winner-path arg-max gap {pgap:.3g}")
        assert gap > 1e-8 * top, (tag, mode, gap, top)
        assert pgap >= 1e-9, (tag, mode, pgap)


@pytest.mark.parametrize("name", list(vc.CASES))
def test_reference_conditions_of_the_cases(name):
    c = vc.case(name)
    D, S, _, n_words, n_per, _, _, extra, _ = vc.CASES[name]
    assert len(c["flat"]) == n_words * n_per + len(extra) and c["feats"].shape[1] == D
    assert c["feats"].dtype == np.float32 and all(p[3].shape == (S, D, D) for p in c["params"])
    _conditions(name, c["flat"], c["params"], vc.reference(name))


def test_reference_conditions_of_the_derived_vocabularies():
    c = vc.case("d5_s3_dense")
    params, want = vc.mixed_size()
    assert [p[2].shape[0] for p in params] == [3, 2, 3]
    for a in (params[1][0].sum(), *params[1][1].sum(axis=1)):
        assert abs(a - 1.0) < 1e-15
    _conditions("mixed sizes", c["flat"], params, want)
    params, want = vc.mixed_type()
    assert np.array_equal(params[0][3], c["params"][0][3])
    assert all(np.array_equal(cv, c["params"][1][3][0]) for cv in params[1][3])
    assert all(np.array_equal(cv, np.diag(np.diag(cv))) for cv in params[2][3])
    _conditions("mixed types", c["flat"], params, want)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def _call(lib, n_utts=4, total_frames=40, D=13, max_T=10, W=3, S=10, mode=_lib.FULL_VOCAB_FORWARD, feats=P, offsets=P,
          pack=P, score=P, best_word=None, word_post=None, workspace=None, workspace_bytes=0):
    return lib.sapr_full_vocab(feats, offsets, None, n_utts, total_frames, D, max_T, pack, W, S, mode, workspace,
                               workspace_bytes, score, best_word, word_post, None)


def _ws_bytes(lib, n_utts=4, total_frames=40, W=3, S=10, D=13):
    n = ctypes.c_size_t(12345)
    return lib.sapr_full_vocab_workspace_bytes(n_utts, total_frames, W, S, D, ctypes.byref(n)), int(n.value)


def test_symbols_are_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "sapr_hip.h")).read()
    assert re.search(r"#define\s+SAPR_FULL_VOCAB_FORWARD\s+0\b", txt) and re.search(
        r"#define\s+SAPR_FULL_VOCAB_VITERBI\s+1\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+sapr_full_vocab\s*\(", code)
    assert re.search(r"\bint\s+sapr_full_vocab_workspace_bytes\s*\(", code)
    res, args = _lib.SIGNATURES["sapr_full_vocab"]
    assert res is ctypes.c_int and len(args) == 17
    res, args = _lib.SIGNATURES["sapr_full_vocab_workspace_bytes"]
    assert res is ctypes.c_int and len(args) == 6
    assert (_lib.FULL_VOCAB_FORWARD, _lib.FULL_VOCAB_VITERBI) == (0, 1)
    lib = _lib.load()
    assert hasattr(lib, "sapr_full_vocab") and hasattr(lib, "sapr_full_vocab_workspace_bytes")
    assert lib.sapr_abi_version() == 2          # additive: the ABI version does not move


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    rc, need = _ws_bytes(lib)
    assert rc == 0 and need != 12345
    big = dict(workspace=P if need else None, workspace_bytes=need)
    assert _call(lib, feats=None, **big) == ERR_ARG
    assert b"NULL pointer" in lib.sapr_last_error()
    for name in ("offsets", "pack", "score"):
        assert _call(lib, **{name: None}, **big) == ERR_ARG, name
    assert _call(lib, mode=2, **big) == ERR_ARG
    assert b"bad mode" in lib.sapr_last_error()
    assert _call(lib, mode=-1, **big) == ERR_ARG
    assert _call(lib, mode=_lib.FULL_VOCAB_VITERBI, word_post=P, **big) == ERR_ARG
    assert b"word_post" in lib.sapr_last_error()
    for bad in (dict(W=0), dict(S=0), dict(D=0), dict(n_utts=-1), dict(total_frames=-1), dict(max_T=-1)):
        assert _call(lib, **bad, **big) == ERR_ARG, bad
        assert b"bad sizes" in lib.sapr_last_error()
    for bad in (dict(S=19), dict(D=40)):
        for mode in (_lib.FULL_VOCAB_FORWARD, _lib.FULL_VOCAB_VITERBI):
            assert _call(lib, mode=mode, **bad, **big) == ERR_UNSUPPORTED, bad
            assert b"S in 1..18" in lib.sapr_last_error()
        assert _ws_bytes(lib, **bad)[0] == ERR_UNSUPPORTED
    for bad in (dict(W=0), dict(S=0), dict(D=0), dict(n_utts=-1), dict(total_frames=-1)):
        assert _ws_bytes(lib, **bad)[0] == ERR_ARG, bad
    assert lib.sapr_full_vocab_workspace_bytes(4, 40, 3, 10, 13, None) == ERR_ARG
    if need:        # a staged instantiation: a workspace that is too small is refused before anything else happens
        assert _call(lib, workspace=P, workspace_bytes=need - 1) == ERR_ARG
        assert b"workspace too small" in lib.sapr_last_error()
        assert _call(lib, workspace=None, workspace_bytes=need) == ERR_ARG


def test_empty_batch_returns_after_the_checks():
    lib = _lib.load()
    none = dict(feats=None, offsets=None, pack=None, score=None)
    rc, need = _ws_bytes(lib, n_utts=0, total_frames=0)
    assert rc == 0
    ws = dict(workspace=P if need else None, workspace_bytes=need)
    for mode in (_lib.FULL_VOCAB_FORWARD, _lib.FULL_VOCAB_VITERBI):
        assert _call(lib, n_utts=0, total_frames=0, max_T=0, mode=mode, **none, **ws) == 0    # no pointer is touched
    # ... but sizes, shape, mode and the posterior rule are still checked
    assert _call(lib, n_utts=0, total_frames=0, W=0, **none, **ws) == ERR_ARG
    assert _call(lib, n_utts=0, total_frames=0, S=19, **none, **ws) == ERR_UNSUPPORTED
    assert _call(lib, n_utts=0, total_frames=0, mode=7, **none, **ws) == ERR_ARG
    assert _call(lib, n_utts=0, total_frames=0, mode=_lib.FULL_VOCAB_VITERBI, word_post=P, **none, **ws) == ERR_ARG


# ---- Python ---------------------------------------------------------------------------------------------------------
def test_full_vocab_scores_is_exported_and_validates_its_mode():
    import sapr_amd
    from sapr_amd import full_cov
    assert sapr_amd.full_vocab_scores is full_cov.vocab_scores
    with pytest.raises(ValueError, match="mode"):
        full_cov.vocab_scores(np.zeros((3, 5), np.float32), [3], [], mode="map")
    with pytest.raises(ValueError, match="want_post"):
        full_cov.vocab_scores(np.zeros((3, 5), np.float32), [3], [], mode="viterbi", want_post=True)


def _model(prm, ct):
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    m = GaussianHMM(n_components=prm[2].shape[0], covariance_type=ct, init_params="")
    m.startprob_, m.transmat_, m.means_ = (np.array(a) for a in prm[:3])
    m.covars_ = vc.typed_covars(prm, ct)
    return m


def test_pack_of_a_vocabulary_is_padded_to_its_largest_model():
    from sapr_amd import full_cov
    c = vc.case("d5_s3_dense")
    params, _ = vc.mixed_size()
    models = [_model(p, "full") for p in params]
    pack = full_cov.FullPack.from_models(models)
    assert (pack.W, pack.S, pack.D, pack.n_states) == (3, 3, 5, [3, 2, 3])
    assert np.array_equal(pack.data, full_cov.pack_models(params, 3))
    assert np.array_equal(pack.data, full_cov.FullPack.from_params(params).data)
    assert pack.data.shape == (3, full_cov.pack_layout(3, 5)[2])
    assert np.isneginf(pack.data[1, 2])                     # the two-state model's third log start probability
    SP = full_cov.pack_layout(3, 5)[0]
    assert np.isneginf(pack.data[1, SP + 2 * SP * SP + 2])  # ... and its emission constant
    with pytest.raises(ValueError):
        full_cov.FullPack.from_params(params + [vc.case("d14_s5_dense")["params"][0]])      # feature width differs
    with pytest.raises(ValueError):
        full_cov.FullPack.from_params([])
    # a vocabulary may mix the covariance types: every model is expanded to [S, D, D]
    typed, _ = vc.mixed_type()
    mixed = full_cov.FullPack.from_models([_model(p, ct) for p, ct in zip(c["params"], vc.MIXED_TYPES)])
    assert np.array_equal(mixed.data, full_cov.pack_models(typed, 3))
    sph = _model(c["params"][0], "diag")
    sph.covariance_type, sph._covars_ = "spherical", np.array([1.5, 2.0, 2.5])
    cv = sph._full_params()[3]
    assert cv.shape == (3, 5, 5) and all(np.array_equal(cv[s], np.eye(5) * v) for s, v in enumerate((1.5, 2.0, 2.5)))


def _write(root, word, model, n_iter=15):
    with open(root / "hmmlearn" / f"{word}_hmmlearn_{n_iter}.pkl", "wb") as f:
        pickle.dump(model, f)


def test_decoder_routes_full_and_tied_models_without_a_gpu(tmp_path, monkeypatch):
    from sapr_amd import full_cov
    from sapr_amd.decoder import Decoder
    from sapr_amd.trellis import DiagModelPack
    c = vc.case("d5_s3_dense")
    root = tmp_path / "trained_models"
    (root / "hmmlearn").mkdir(parents=True)
    for word, prm, ct in zip(("heed", "hid", "hood"), c["params"], vc.MIXED_TYPES):
        _write(root, word, _model(prm, ct))
    for scoring in ("viterbi", "forward"):
        dec = Decoder(models_dir=str(root), implementation="hmmlearn", scoring=scoring)
        assert sorted(dec.vocab) == ["heed", "hid", "hood"] and dec.vocab == list(dec.models)
        assert dec._is_full()
        pack = dec._vocab_pack()
        assert isinstance(pack, full_cov.FullPack) and dec._vocab_pack() is pack
        assert (pack.W, pack.S, pack.D, pack.n_states) == (3, 3, 5, [3, 3, 3])
        assert dec._pack is None                               # DiagModelPack.from_models was never called
    with pytest.raises(ValueError):
        DiagModelPack.from_models(dec._model_list())           # ... and keeps refusing such models
    with pytest.raises(ValueError, match="not in vocabulary"):
        dec._named_models(["who"], 1)
    # a vocabulary of diag models only keeps the single-Gaussian path
    diag = tmp_path / "diag_models"
    (diag / "hmmlearn").mkdir(parents=True)
    for word, prm in zip(("heed", "hid"), c["params"]):
        _write(diag, word, _model(prm, "diag"))
    dec = Decoder(models_dir=str(diag), implementation="hmmlearn")
    assert not dec._is_full() and dec._vocab is None

    class Reached(Exception):
        pass

    def from_models(models, *a, **kw):          # (the pack itself needs a device: stop where it would be built)
        assert models == dec._model_list()
        raise Reached

    monkeypatch.setattr(DiagModelPack, "from_models", staticmethod(from_models))
    x = np.ascontiguousarray(c["flat"][0].T)
    for call in (lambda: dec.score_batch([x]), lambda: dec.state_posteriors([x], words=["heed"])):
        with pytest.raises(Reached):
            call()

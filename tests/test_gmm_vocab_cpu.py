"""CPU: the mixture models' vocabulary-scoring entry point (sapr_gmm_vocab_diag) is declared, bound and exported and
reports its argument errors before any HIP call; ``Decoder(implementation="gmmhmm")`` loads a pickled vocabulary.  No
compute call is made — there is no GPU in the build container."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from sapr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -2
P = ctypes.c_void_p(256)     # a dummy non-NULL pointer (never dereferenced on the paths exercised here)


def _call(lib, n_utts=4, total_frames=40, D=13, max_T=10, W=3, S=10, M=2, mode=_lib.GMM_VOCAB_FORWARD, feats=P,
          offsets=P, pack=P, score=P, best_word=None, word_post=None):
    return lib.sapr_gmm_vocab_diag(feats, offsets, None, n_utts, total_frames, D, max_T, pack, W, S, M, mode, score,
                                   best_word, word_post, None)


def test_symbol_is_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "sapr_hip.h")).read()
    assert re.search(r"#define\s+SAPR_GMM_VOCAB_FORWARD\s+0\b", txt) and re.search(
        r"#define\s+SAPR_GMM_VOCAB_VITERBI\s+1\b", txt)
    assert re.search(r"\bint\s+sapr_gmm_vocab_diag\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    res, args = _lib.SIGNATURES["sapr_gmm_vocab_diag"]
    assert res is ctypes.c_int and len(args) == 16
    assert (_lib.GMM_VOCAB_FORWARD, _lib.GMM_VOCAB_VITERBI) == (0, 1)
    lib = _lib.load()
    assert hasattr(lib, "sapr_gmm_vocab_diag")
    assert lib.sapr_abi_version() == 2          # additive: the ABI version does not move


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    assert _call(lib, feats=None) == ERR_ARG
    assert b"NULL pointer" in lib.sapr_last_error()
    for name in ("offsets", "pack", "score"):
        assert _call(lib, **{name: None}) == ERR_ARG, name
    assert _call(lib, mode=2) == ERR_ARG
    assert b"bad mode" in lib.sapr_last_error()
    assert _call(lib, mode=-1) == ERR_ARG
    assert _call(lib, mode=_lib.GMM_VOCAB_VITERBI, word_post=P) == ERR_ARG
    assert b"word_post" in lib.sapr_last_error()
    for bad in (dict(W=0), dict(S=0), dict(M=0), dict(D=0), dict(n_utts=-1), dict(total_frames=-1), dict(max_T=-1)):
        assert _call(lib, **bad) == ERR_ARG, bad
        assert b"bad sizes" in lib.sapr_last_error()
    for bad in (dict(S=19), dict(M=9), dict(D=40)):
        for mode in (_lib.GMM_VOCAB_FORWARD, _lib.GMM_VOCAB_VITERBI):
            assert _call(lib, mode=mode, **bad) == ERR_UNSUPPORTED, bad
            assert b"S in 1..18" in lib.sapr_last_error()


def test_empty_batch_returns_after_the_checks():
    lib = _lib.load()
    none = dict(feats=None, offsets=None, pack=None, score=None)
    for mode in (_lib.GMM_VOCAB_FORWARD, _lib.GMM_VOCAB_VITERBI):
        assert _call(lib, n_utts=0, total_frames=0, max_T=0, mode=mode, **none) == 0    # no pointer is touched
    # ... but sizes, shape, mode and the posterior rule are still checked
    assert _call(lib, n_utts=0, total_frames=0, W=0, **none) == ERR_ARG
    assert _call(lib, n_utts=0, total_frames=0, S=19, **none) == ERR_UNSUPPORTED
    assert _call(lib, n_utts=0, total_frames=0, mode=7, **none) == ERR_ARG
    assert _call(lib, n_utts=0, total_frames=0, mode=_lib.GMM_VOCAB_VITERBI, word_post=P, **none) == ERR_ARG


def test_vocab_scores_is_exported_and_validates_its_mode():
    import sapr_amd
    from sapr_amd import gmm_hmm as gh
    assert sapr_amd.vocab_scores is gh.vocab_scores
    with pytest.raises(ValueError):
        gh.vocab_scores(np.zeros((3, 5), np.float32), [3], [], mode="map")
    with pytest.raises(ValueError):
        gh.vocab_scores(np.zeros((3, 5), np.float32), [3], [], mode="viterbi", want_post=True)


def _gmm(rng, S, M, D):
    from sapr_amd import GMMHMM
    m = GMMHMM(n_components=S, n_mix=M, init_params="")
    m.startprob_, m.transmat_ = rng.dirichlet(np.ones(S)), rng.dirichlet(np.ones(S), size=S)
    m.weights_, m.means_, m.covars_ = rng.dirichlet(np.ones(M), size=S), rng.normal(0, 1, (S, M, D)), np.ones((S, M, D))
    return m


def test_pack_of_a_vocabulary_is_padded_to_its_largest_model():
    from sapr_amd import gmm_hmm as gh
    rng = np.random.default_rng(0)
    models = [_gmm(rng, 3, 2, 5), _gmm(rng, 2, 2, 5), _gmm(rng, 3, 2, 5)]
    pack = gh.GmmPack.from_models(models)
    assert (pack.W, pack.S, pack.M, pack.D, pack.n_states) == (3, 3, 2, 5, [3, 2, 3])
    assert np.array_equal(pack.data, gh.pack_models([m._params() for m in models], 3))
    assert pack.data.shape == (3, gh.pack_layout(3, 2, 5)[3])
    assert np.isneginf(pack.data[1, 2])                     # the two-state model's third log start probability
    with pytest.raises(ValueError):
        gh.GmmPack.from_models(models + [_gmm(rng, 3, 3, 5)])      # n_mix differs: pack_models' ValueError
    with pytest.raises(ValueError):
        gh.GmmPack.from_models(models + [_gmm(rng, 3, 2, 6)])      # feature width differs


def test_decoder_loads_gmmhmm_models_without_a_gpu(tmp_path):
    from sapr_amd.decoder import Decoder
    root = tmp_path / "trained_models"
    (root / "gmmhmm").mkdir(parents=True)
    with pytest.raises(ValueError, match="No models found"):
        Decoder(models_dir=str(root), implementation="gmmhmm")
    rng = np.random.default_rng(1)
    for word in ("heed", "hid", "hood"):
        with open(root / "gmmhmm" / f"{word}_gmmhmm_15.pkl", "wb") as f:
            pickle.dump(_gmm(rng, 3, 2, 5), f)
    with open(root / "gmmhmm" / "head_gmmhmm_7.pkl", "wb") as f:       # another n_iter: not part of this vocabulary
        pickle.dump(_gmm(rng, 3, 2, 5), f)
    for scoring in ("viterbi", "forward"):
        dec = Decoder(models_dir=str(root), implementation="gmmhmm", scoring=scoring)
        want = [p.stem.split("_")[0] for p in (root / "gmmhmm").glob("*_gmmhmm_15.pkl")]     # glob order = load order
        assert dec.vocab == want == list(dec.models) and sorted(want) == ["heed", "hid", "hood"]
        assert all(type(m).__name__ == "GMMHMM" for m in dec.models.values())
    with pytest.raises(ValueError):
        Decoder(models_dir=str(root), implementation="gmmhmm", scoring="posterior")
    with pytest.raises(ValueError, match="not in vocabulary"):
        dec._named_models(["who"], 1)
    with pytest.raises(ValueError, match="one word per utterance"):
        dec._named_models(["heed"], 2)

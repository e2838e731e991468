"""CPU: the forward-scoring entry point (sapr_forward_vocab) is exported, bound and reports argument errors without
a device; the host side of ``Decoder.nbest`` orders a score matrix as documented; ``Decoder(scoring=...)`` is
validated.  No compute call is made — there is no GPU in the build container."""
import ctypes
import pickle
import types

import numpy as np
import pytest

from sapr_amd import _lib

ERR_ARG = -1


def _call(lib, n_utts, W, topology, loglik, D=13, S=10):
    """sapr_forward_vocab with dummy non-NULL pointers (never dereferenced on the paths exercised here)."""
    p = ctypes.c_void_p(256)
    return lib.sapr_forward_vocab(p, p, None, n_utts, D, 101, p, W, S, topology, loglik, None, None, None)


def test_symbol_is_exported_and_bound():
    assert "sapr_forward_vocab" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["sapr_forward_vocab"]
    assert res is ctypes.c_int and len(args) == 14
    lib = _lib.load()
    assert hasattr(lib, "sapr_forward_vocab")
    assert lib.sapr_abi_version() == 2          # additive: the ABI version does not move


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    out = ctypes.c_void_p(512)
    assert _call(lib, 4, 0, _lib.TOPO_BIDIAG, out) == ERR_ARG
    assert b"bad sizes" in lib.sapr_last_error()
    assert _call(lib, 4, -3, _lib.TOPO_BIDIAG, out) == ERR_ARG
    assert _call(lib, 4, 11, 7, out) == ERR_ARG
    assert b"bad topology" in lib.sapr_last_error()
    assert _call(lib, 4, 11, _lib.TOPO_BIDIAG, None) == ERR_ARG
    assert b"NULL" in lib.sapr_last_error()
    assert _call(lib, 4, 11, _lib.TOPO_DENSE, None) == ERR_ARG


def test_empty_batch_returns_at_once():
    lib = _lib.load()
    # n_utts == 0: success without touching any pointer, NULL ones included
    assert lib.sapr_forward_vocab(None, None, None, 0, 13, 0, None, 11, 10, _lib.TOPO_BIDIAG, None, None, None,
                                  None) == 0
    assert _call(lib, 0, 11, _lib.TOPO_DENSE, None) == 0
    # ... but the sizes and the topology are still checked
    assert _call(lib, 0, 0, _lib.TOPO_BIDIAG, None) == ERR_ARG
    assert _call(lib, 0, 11, 5, None) == ERR_ARG


def test_nbest_ordering_on_a_hand_made_matrix():
    from sapr_amd.decoder import Decoder
    vocab = ["a", "b", "c", "d", "e"]
    inf, nan = np.inf, np.nan
    ll = np.array([[-5.0, -2.0, -2.0, -9.0, -2.0],      # three-way tie for the lead: load order b, c, e
                   [nan, -1.0, nan, -inf, -3.0],        # NaN last (in load order), -inf before them
                   [-inf, -inf, -inf, -inf, -inf],      # nothing beats -inf: still load order
                   [-4.0, -3.0, -2.0, -1.0, 0.0]])      # plain descending
    post = np.arange(20, dtype=np.float64).reshape(4, 5) / 100.0
    rows = Decoder._nbest_rows(ll, post, vocab, 3)
    assert [[w for w, _, _ in r] for r in rows] == [["b", "c", "e"], ["b", "e", "d"], ["a", "b", "c"],
                                                      ["e", "d", "c"]]
    # every entry carries ITS score and ITS posterior
    assert rows[0][2] == ("e", -2.0, 0.04) and rows[3][0] == ("e", 0.0, 0.19) and rows[1][2] == ("d", -inf, 0.08)
    # n > W is clipped to W; NaN scores close the list
    full = Decoder._nbest_rows(ll, post, vocab, 99)
    assert all(len(r) == 5 for r in full)
    assert [w for w, _, _ in full[1]] == ["b", "e", "d", "a", "c"]
    assert np.isnan(full[1][3][1]) and np.isnan(full[1][4][1])
    assert [w for w, _, _ in full[0]] == ["b", "c", "e", "a", "d"]
    assert Decoder._nbest_rows(ll, post, vocab, 1) == [[("b", -2.0, 0.01)], [("b", -1.0, 0.06)], [("a", -inf, 0.10)],
                                                       [("e", 0.0, 0.19)]]
    assert Decoder._nbest_rows(ll, post, vocab, 0) == [[], [], [], []]


def _model_dir(tmp_path, implementation):
    d = tmp_path / "trained_models" / implementation
    d.mkdir(parents=True)
    for word in ("heed", "hid"):
        with open(d / f"{word}_{implementation}_15.pkl", "wb") as f:
            pickle.dump(types.SimpleNamespace(word=word), f)
    return str(tmp_path / "trained_models")


def test_scoring_keyword_is_validated(tmp_path):
    from sapr_amd.decoder import Decoder
    root = _model_dir(tmp_path, "hmmlearn")
    assert Decoder(models_dir=root).scoring == "viterbi"             # the default does not change
    assert Decoder(models_dir=root, scoring="viterbi").scoring == "viterbi"
    dec = Decoder(models_dir=root, scoring="forward")
    assert dec.scoring == "forward" and sorted(dec.vocab) == ["heed", "hid"]
    for bad in ("Forward", "posterior", "", None):
        with pytest.raises(ValueError):
            Decoder(models_dir=root, scoring=bad)


def test_custom_models_have_no_forward_scorer(tmp_path):
    from sapr_amd.decoder import Decoder
    root = _model_dir(tmp_path, "custom")
    with pytest.raises(ValueError):
        Decoder(models_dir=root, implementation="custom", scoring="forward")
    dec = Decoder(models_dir=root, implementation="custom")
    x = [np.zeros((13, 5), dtype=np.float32)]
    with pytest.raises(ValueError):
        dec.score_batch(x)
    with pytest.raises(ValueError):
        dec.nbest(x, n=2)

"""CPU: the state-posterior entry points (sapr_state_posteriors_workspace_bytes, sapr_state_posteriors_diag) are
exported, bound and report argument errors without a device; the workspace size follows the documented formula;
``GaussianHMM(algorithm=...)`` and ``Decoder.state_posteriors`` validate their arguments; the host side of MAP
decoding follows numpy's arg-max rules.  No compute call is made — there is no GPU in the build container."""
import ctypes
import pickle
import types

import numpy as np
import pytest

from sapr_amd import _lib

ERR_ARG = -1
P = ctypes.c_void_p(256)      # dummy non-NULL pointer (never dereferenced on the paths exercised here)
BIG = 1 << 40                 # a workspace size that is never too small


def _call(lib, n_tiles=2, D=13, max_T=101, W=11, S=10, topology=_lib.TOPO_BIDIAG, n_out=10, ws=P, ws_bytes=BIG,
          loglik=P, post=P, path=P):
    return lib.sapr_state_posteriors_diag(P, P, P, P, n_tiles, D, max_T, P, W, S, topology, n_out, ws, ws_bytes,
                                          loglik, post, path, None)


def test_symbols_are_exported_and_bound():
    for name, arity in (("sapr_state_posteriors_workspace_bytes", 5), ("sapr_state_posteriors_diag", 18)):
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == arity
        assert hasattr(_lib.load(), name)
    assert _lib.load().sapr_abi_version() == 2          # additive: the ABI version does not move


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    for bad in (dict(n_tiles=-1), dict(W=0), dict(S=0), dict(D=0), dict(max_T=-1)):
        assert _call(lib, **bad) == ERR_ARG, bad
        assert b"bad sizes" in lib.sapr_last_error()
    assert _call(lib, topology=7) == ERR_ARG
    assert b"bad topology" in lib.sapr_last_error()
    for n_out in (0, -2, 11):
        assert _call(lib, n_out=n_out) == ERR_ARG
        assert b"n_out_states" in lib.sapr_last_error()
    assert _call(lib, S=18, n_out=19) == ERR_ARG
    assert _call(lib, loglik=None) == ERR_ARG
    assert b"NULL" in lib.sapr_last_error()
    assert _call(lib, post=None, path=None) == ERR_ARG
    assert b"both NULL" in lib.sapr_last_error()
    for topology in (_lib.TOPO_BIDIAG, _lib.TOPO_DENSE):
        n = ctypes.c_size_t(0)
        assert lib.sapr_state_posteriors_workspace_bytes(2, 10, 101, topology, ctypes.byref(n)) == 0
        assert _call(lib, topology=topology, ws_bytes=n.value - 1) == ERR_ARG
        assert b"workspace too small" in lib.sapr_last_error()
    assert _call(lib, ws=None) == ERR_ARG


def test_no_tiles_returns_at_once():
    lib = _lib.load()
    # n_tiles == 0: success without touching any pointer, NULL ones included
    assert lib.sapr_state_posteriors_diag(None, None, None, None, 0, 13, 0, None, 11, 10, _lib.TOPO_BIDIAG, 10, None,
                                          0, None, None, None, None) == 0
    assert _call(lib, n_tiles=0, topology=_lib.TOPO_DENSE, loglik=None, post=None, path=None, ws_bytes=0) == 0
    # ... but the sizes, the topology and n_out_states are still checked
    assert _call(lib, n_tiles=0, W=0) == ERR_ARG
    assert _call(lib, n_tiles=0, topology=5) == ERR_ARG
    assert _call(lib, n_tiles=0, n_out=0) == ERR_ARG


def test_workspace_size_is_the_documented_formula():
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    for n_tiles, S, max_T in ((3, 10, 101), (7, 18, 57)):
        assert lib.sapr_state_posteriors_workspace_bytes(n_tiles, S, max_T, _lib.TOPO_BIDIAG, ctypes.byref(n)) == 0
        assert n.value == (max_T + 1) * S * n_tiles * 256 * 8        # stay shares + the last forward row
        assert lib.sapr_state_posteriors_workspace_bytes(n_tiles, S, max_T, _lib.TOPO_DENSE, ctypes.byref(n)) == 0
        assert n.value == 2 * max_T * S * n_tiles * 256 * 8          # forward lattice + log-densities
    assert lib.sapr_state_posteriors_workspace_bytes(2, 10, 0, _lib.TOPO_BIDIAG, ctypes.byref(n)) == 0
    assert n.value == 2 * 10 * 2 * 256 * 8                           # max_T = 0 is laid out as one frame
    assert lib.sapr_state_posteriors_workspace_bytes(0, 10, 101, _lib.TOPO_DENSE, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.sapr_state_posteriors_workspace_bytes(2, 10, 101, 3, ctypes.byref(n)) == ERR_ARG
    assert lib.sapr_state_posteriors_workspace_bytes(2, 0, 101, _lib.TOPO_DENSE, ctypes.byref(n)) == ERR_ARG
    assert lib.sapr_state_posteriors_workspace_bytes(2, 10, 101, _lib.TOPO_DENSE, None) == ERR_ARG


def test_gaussian_hmm_algorithm_keyword():
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    assert GaussianHMM(n_components=3).algorithm == "viterbi"       # the default does not change
    m = GaussianHMM(n_components=3, algorithm="map")
    assert m.algorithm == "map"
    assert pickle.loads(pickle.dumps(m)).algorithm == "map"
    assert pickle.loads(pickle.dumps(GaussianHMM(n_components=3))).algorithm == "viterbi"
    for bad in ("x", "MAP", "", None):
        with pytest.raises(ValueError):
            GaussianHMM(n_components=3, algorithm=bad)
    with pytest.raises(ValueError):                                  # refused before anything touches a device
        m.decode(np.zeros((4, 2), dtype=np.float32), algorithm="x")
    for name in ("score_samples", "predict_proba"):
        assert callable(getattr(m, name))


def test_custom_models_have_no_state_posteriors(tmp_path):
    from sapr_amd.decoder import Decoder
    d = tmp_path / "trained_models" / "custom"
    d.mkdir(parents=True)
    for word in ("heed", "hid"):
        with open(d / f"{word}_custom_15.pkl", "wb") as f:
            pickle.dump(types.SimpleNamespace(word=word), f)
    dec = Decoder(models_dir=str(tmp_path / "trained_models"), implementation="custom")
    x = [np.zeros((13, 5), dtype=np.float32)]
    with pytest.raises(ValueError):
        dec.state_posteriors(x)
    with pytest.raises(ValueError):
        dec.state_posteriors(x, words=["heed"])


def test_map_decoding_on_a_hand_made_lattice():
    """hmmlearn's _decode_map on the host: two sequences, one tie (lowest index wins) and one row holding NaN (its
    first NaN is the arg-max and the log_prob is NaN, as np.argmax / np.max give them)."""
    from sapr_amd.hmmlearn_hmm import map_decode_host
    nan = np.nan
    post = np.array([[0.1, 0.7, 0.2],
                     [0.4, 0.4, 0.2],       # tie between states 0 and 1
                     [0.0, 0.25, 0.75],
                     [0.5, 0.25, 0.25],     # second sequence
                     [0.2, 0.3, 0.5]])
    lp, st = map_decode_host(post, [3, 2])
    assert st.dtype == np.int64 and st.tolist() == [1, 0, 2, 0, 2]
    assert lp == (0.7 + 0.4 + 0.75) + (0.5 + 0.5)
    lp1, st1 = map_decode_host(post)                   # one sequence: the same states, one sum
    assert st1.tolist() == st.tolist() and lp1 == np.max(post, axis=1).sum()
    bad = post.copy()
    bad[3] = [0.9, nan, nan]
    lp, st = map_decode_host(bad, [3, 2])
    assert st.tolist() == [1, 0, 2, 1, 2] and np.isnan(lp)
    lp, st = map_decode_host(bad[:3], [3])             # the NaN row is outside: finite again
    assert lp == 0.7 + 0.4 + 0.75
    with pytest.raises(ValueError):
        map_decode_host(post, [3, 3])

"""CPU: the definition of the lattice posteriors (tests/_lattice_post_ref.py) against the enumeration of every lattice
path, the properties the device tests rely on, and the C ABI of ``sapr_connected_lattice_posteriors`` as far as it can
be checked without a device (symbols, the size function, the refusals before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _bigram_ref as bref
from tests import _lattice_cases as lc
from tests import _lattice_post_ref as pref
from tests import _lattice_ref as lref
from tests.test_lattice_cpu import _HostLattice, _tiny

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _path_scores(lat, tabs, kappa, keep=None):
    """Every complete lattice path under ``tabs`` with its score at the acoustic scale ``kappa``: the paths are
    ``lref.lattice_paths``'s, the score is rebuilt with ``kappa * ac`` per record."""
    lm, lm_start, lm_end = tabs
    ac = {(t, w): a for t, w, _, _, a in lref.records(lat["X"], lat["N"], lat["B"], lat["lm_start"])}
    out = {}
    for path, plain in lref.lattice_paths(lat, lm, lm_start, lm_end, keep=keep).items():
        v, prev = 0.0, None
        for w, _, b in path:
            v += (lm_start[w] if prev is None else lm[prev][w]) + np.float64(kappa) * ac[b - 1, w]
            prev = w
        out[path] = v + lm_end[prev]
        if kappa == 1.0:
            assert abs(out[path] - plain) <= 1e-12 * max(1.0, abs(plain))
    return out


def _against_paths(lat, tabs, kappa, keep, what):
    got = pref.posteriors(lat["X"], lat["N"], lat["B"], lat["lm_start"], *tabs, kappa=kappa, keep=keep)
    paths = _path_scores(lat, tabs, kappa, keep)
    T, W = lat["X"].shape
    assert not got["record_post"][lat["X"] == NEG].any()
    if not paths:
        assert got["loglik"] == NEG and got["loglik_backward"] == NEG, what
        assert not got["record_post"].any() and not got["word_post"].any(), what
        return 0, 0.0
    scores = np.array(list(paths.values()))
    ll = scores.max() + np.log(np.exp(scores - scores.max()).sum())
    worst = max(abs(got["loglik"] - ll), abs(got["loglik_backward"] - ll))
    share = np.zeros((T, W))
    inside = np.zeros((T, W))
    for path, v in paths.items():
        for w, a, b in path:
            share[b - 1, w] += np.exp(v - ll)
            inside[a:b, w] += np.exp(v - ll)
    worst = max(worst, np.abs(got["record_post"] - share).max(), np.abs(got["word_post"] - inside).max())
    assert worst <= 1e-12, (what, worst)
    assert np.abs(got["word_post"].sum(axis=1) - 1.0).max() <= 1e-12, what
    return len(paths), worst


def test_definition_against_the_enumeration_of_every_lattice_path():
    """W = 3, S = 2, T = 0 .. 6, random networks, 20 seeds, tables different from the forward pass's: ``loglik`` (both
    forms) is the log-sum of all complete lattice path scores and ``record_post`` the share of the paths through the
    record, within 1e-12 absolute — at kappa = 1, at kappa = 1/4 (the enumeration scales ``ac`` itself) and under a
    ``keep`` mask; ``word_post`` is the share of the paths on which the frame lies inside the word."""
    paths = masked = 0
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(500 + seed)
        T = seed % 7
        ls, lt, lx, lm, lm2, logb = _tiny(rng, T)
        lat = lref.lattice(logb, ls, lt, lx, *lm)
        keep = rng.random((T, 3)) < 0.7
        for tabs in (lm2, lm):
            for kappa in (1.0, 0.25):
                n, w = _against_paths(lat, tabs, kappa, None, (seed, kappa))
                paths, worst = paths + n, max(worst, w)
                n, w = _against_paths(lat, tabs, kappa, keep, (seed, kappa, "keep"))
                masked, worst = masked + n, max(worst, w)
        if T == 0:
            assert pref.posteriors(lat["X"], lat["N"], lat["B"], lm[1], *lm2)["loglik"] == NEG
    print(f"{paths} paths, {masked} under a mask; worst deviation {worst:.2e}")
    assert paths >= 200 and masked >= 40


@pytest.mark.parametrize("W,S", lc.SHAPES)
def test_device_cases_rows_sum_to_one_and_the_likelihood_dominates_the_best_path(W, S):
    """On the random cases of tests/test_lattice_posteriors_gpu.py: the ``word_post`` rows of every utterance with a
    finite ``loglik`` sum to 1, ``loglik`` is not below the best lattice path's score (``root`` of the max-semiring
    backward pass under the same tables, kappa = 1) by more than eps_u, the dead word carries nothing under ``lm`` and
    the empty utterance has ``loglik`` -inf."""
    for topology, exits in (("bidiag", "last"), ("dense", "any")):
        _, _, _, lm, lm2, _, dead = lc.random_case(W, S, topology, exits)
        per, tabs, per2, _ = lc.reference(W, S, topology, exits)
        for tables, roots in ((lm, per), (lm2, per2)):
            got, _ = pref.batch(tabs, lc.LENGTHS, lm[1], *tables)
            finite = 0
            for u, p in enumerate(got):
                if lc.LENGTHS[u] == 0:
                    assert p["loglik"] == NEG
                if np.isfinite(p["loglik"]):
                    finite += 1
                    assert np.abs(p["word_post"].sum(axis=1) - 1.0).max() <= 1e-9
                    assert np.abs(p["loglik"] - p["loglik_backward"]) <= 1e-11 * abs(p["loglik"])
                else:
                    assert p["loglik"] == NEG and not p["word_post"].any() and not p["record_post"].any()
                assert p["loglik"] >= roots[u]["root"] - per[u]["eps"] or roots[u]["root"] == NEG
                assert np.isfinite(p["loglik"]) == np.isfinite(roots[u]["root"])
                if W > 1 and tables is lm:
                    assert not p["word_post"][:, dead].any() and not p["record_post"][:, dead].any()
            assert finite >= 5


def test_host_side_of_the_posteriors():
    """``LatticePosteriors.segment_confidence`` and ``.slots`` over a table from the definition."""
    from sapr_amd.connected import LatticePath, LatticePosteriors
    rng = np.random.default_rng(77)
    done = 0
    for T in (4, 6, 9):
        ls, lt, lx, lm, _, logb = _tiny(rng, T)
        lat = lref.lattice(logb, ls, lt, lx, *lm)
        if not np.isfinite(lat["root"]):
            continue
        p = pref.posteriors(lat["X"], lat["N"], lat["B"], lm[1], *lm, kappa=0.25)
        offs = np.array([0, T], np.int64)
        post = LatticePosteriors(np.array([p["loglik"]]), p["record_post"], p["word_post"], offs)
        path = LatticePath(np.array([lat["root"]]), np.array([lat["n_words"]]), lat["path_word"], lat["path_entry"],
                           offs)
        conf, slots = post.segment_confidence(path, 0), post.slots(path, 0)
        assert len(conf) == len(slots) == lat["n_words"]
        for (w, a, b), c, slot in zip(path.segments(0), conf, slots):
            assert c == p["word_post"][a:b, w].mean() and dict(slot)[w] == c
            assert abs(sum(q for _, q in slot) - 1.0) <= 1e-12 and all(q > 0 for _, q in slot)
            assert [q for _, q in slot] == sorted((q for _, q in slot), reverse=True)
        assert [s[:1] for s in slots] == post.slots(path, 0, top=1)
        done += 1
    assert done >= 2


# ---- the C ABI, without a device ----------------------------------------------------------------------------------
NAMES = ("sapr_connected_lattice_posteriors_workspace_bytes", "sapr_connected_lattice_posteriors")


def test_symbols_are_declared_bound_and_exported():
    from sapr_amd import _lib
    with open(os.path.join(ROOT, "include", "sapr_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "tests/_lattice_post_ref.py" in header
    assert "4 * a16(8 * total_frames * W)" in header
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    import sapr_amd
    from sapr_amd import connected
    for name in ("LatticePosteriors", "lattice_posteriors_workspace_bytes"):
        assert getattr(sapr_amd, name) is getattr(connected, name)
    assert callable(connected.WordLattice.posteriors)


def _p(on):
    return C.cast((C.c_double * 1)(), C.c_void_p) if on else None


def _post(lib, n_utts=1, total=10, W=2, S=4, fwd=1, lm=1, lm_start=1, lm_end=1, scale=1.0, lat=None, lat_bytes=0,
          ws=None, ws_bytes=0):
    """``sapr_connected_lattice_posteriors`` with every pointer NULL except the four tables (a host address the checks
    never dereference) and the two workspaces."""
    return lib.sapr_connected_lattice_posteriors(None, n_utts, total, W, S, lat, lat_bytes, _p(fwd), _p(lm),
                                                 _p(lm_start), _p(lm_end), scale, None, ws, ws_bytes, None, None, None,
                                                 None)


def test_size_function_and_refusals_before_any_launch():
    from sapr_amd import _lib
    from sapr_amd.connected import lattice_posteriors_workspace_bytes
    lib = _lib.load()
    n = C.c_size_t(0)
    size = lib.sapr_connected_lattice_posteriors_workspace_bytes
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    assert size(1000, 7, 11, 10, C.byref(n)) == 0
    assert n.value == 4 * a16(8 * 1000 * 11) == 32 * 11 * 1000                          # 32 W bytes per frame
    assert lattice_posteriors_workspace_bytes(1000, 7, 11, 10) == n.value
    assert size(3, 1, 5, 7, C.byref(n)) == 0 and n.value == 4 * 128
    assert size(0, 0, 1, 1, C.byref(n)) == 0 and n.value == 0
    for W, S in ((2, 19), (26, 10), (65, 4)):       # unsupported: S = 19, W * SP = 260
        assert size(10, 1, W, S, C.byref(n)) == -2
        assert _post(lib, W=W, S=S) == -2
    assert b"W * SP" in lib.sapr_last_error()
    assert size(10, 1, 64, 4, C.byref(n)) == 0
    assert size(-1, 1, 2, 4, C.byref(n)) == -1 and b"bad sizes" in lib.sapr_last_error()
    assert size(10, -1, 2, 4, C.byref(n)) == -1 and size(10, 1, 0, 4, C.byref(n)) == -1
    assert size(10, 1, 2, 0, C.byref(n)) == -1 and size(10, 1, 2, 4, None) == -1
    for kw in (dict(n_utts=-1), dict(total=-1), dict(W=0), dict(S=-3)):
        assert _post(lib, **kw) == -1 and b"bad sizes" in lib.sapr_last_error()
    for kw in (dict(fwd=0), dict(lm=0), dict(lm_start=0), dict(lm_end=0)):      # a NULL table, each of them
        assert _post(lib, **kw) == -1 and b"NULL language model" in lib.sapr_last_error()
        assert _post(lib, n_utts=0, total=0, **kw) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert _post(lib, scale=bad) == -1 and b"acoustic_scale" in lib.sapr_last_error()
        assert _post(lib, n_utts=0, total=0, scale=bad) == -1
    # the workspaces, each one byte short (host memory: never touched before the refusal)
    assert lib.sapr_connected_lattice_workspace_bytes(10, 1, 2, 4, C.byref(n)) == 0
    lat = (C.c_uint8 * n.value)()
    lat_kw = dict(lat=C.cast(lat, C.c_void_p), lat_bytes=n.value)
    assert _post(lib, lat=lat_kw["lat"], lat_bytes=n.value - 1) == -1
    assert b"lattice workspace too small" in lib.sapr_last_error()
    assert size(10, 1, 2, 4, C.byref(n)) == 0
    buf = (C.c_uint8 * n.value)()
    assert _post(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value - 1, **lat_kw) == -1
    assert b"workspace too small" in lib.sapr_last_error() and b"lattice" not in lib.sapr_last_error()
    # full workspaces pass on to the next check: the other required pointers
    assert _post(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value, **lat_kw) == -1
    assert b"NULL pointer" in lib.sapr_last_error()
    assert _post(lib, n_utts=0, total=0) == 0               # nothing to do


def test_python_argument_refusals_come_before_a_device_is_asked_for(tmp_path):
    import pickle
    from sapr_amd.connected import WordBigram
    from sapr_amd.decoder import Decoder
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    rng = np.random.default_rng(5)
    ls, lt, lx, lm, _, logb = _tiny(rng, 5)
    host = _HostLattice(lref.lattice(logb, ls, lt, lx, *lm), lm)         # (no device behind it)
    for bad in ("bigram", WordBigram(*bref.random_lm(rng, 4))):
        with pytest.raises(ValueError, match="rescored under a WordBigram over 3 words"):
            host.posteriors(bad)
    for bad in (0.0, -2.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="acoustic_scale must be a finite number > 0"):
            host.posteriors(acoustic_scale=bad)
    for bad in (-1.0, float("nan"), "wide"):
        with pytest.raises(ValueError, match="beam must be a number >= 0"):
            host.posteriors(beam=bad)
    d = tmp_path / "trained_models" / "hmmlearn"
    d.mkdir(parents=True)
    for word in ("yes", "no"):
        m = GaussianHMM(n_components=2, covariance_type="diag")
        m.startprob_, m.transmat_ = np.r_[1.0, 0.0], np.array([[0.5, 0.5], [0.0, 1.0]])
        m.means_, m._covars_ = np.zeros((2, 3)), np.ones((2, 3))
        with open(d / f"{word}_hmmlearn_15.pkl", "wb") as f:
            pickle.dump(m, f)
    dec = Decoder(models_dir=str(tmp_path / "trained_models"), implementation="hmmlearn")
    x = [np.zeros((3, 6), np.float32)]
    for bad in ("nonsense", "Lattice", ""):
        with pytest.raises(ValueError, match="confidence must be True, False or 'lattice'"):
            dec.decode_connected(x, confidence=bad)
    for bad in (0.0, float("nan"), "2"):
        with pytest.raises(ValueError, match="acoustic_scale must be a finite number > 0"):
            dec.decode_connected(x, confidence="lattice", acoustic_scale=bad)

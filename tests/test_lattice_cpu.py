"""CPU: the definition of the connected-word lattice (tests/_lattice_ref.py) against an enumeration of every path, the
conditions the device tests rely on (tests/_lattice_cases.py), the SLF export read back, and the C ABI of
``sapr_connected_lattice`` / ``_backward`` / ``_walk`` as far as it can be checked without a device (symbols, the size
function, the refusals before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sapr_amd.connected import connected_lattice  # noqa: F401  (the feature under test)
from tests import _bigram_ref as bref
from tests import _lattice_cases as lc
from tests import _lattice_ref as lref

NEG = -np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(rng, T, W=3, S=2):
    ls = np.log(rng.uniform(0.05, 1.0, (W, S)))
    lt = np.log(rng.uniform(0.05, 1.0, (W, S, S)))
    lx = np.log(rng.uniform(0.05, 1.0, (W, S)))
    ls[rng.random((W, S)) < 0.2] = NEG
    lt[rng.random((W, S, S)) < 0.2] = NEG
    lx[rng.random((W, S)) < 0.2] = NEG
    return ls, lt, lx, bref.random_lm(rng, W), bref.random_lm(rng, W), rng.normal(-5.0, 3.0, (T, W, S))


def _path_records(path):
    return {(b - 1, w) for w, _, b in path}


# ---- the definition against the enumeration of every path ---------------------------------------------------------
def test_definition_against_the_enumeration_of_every_path():
    """W = 3, S = 2, T = 0 .. 6, dense random ``lm`` with a third of the pairs forbidden (and forbidden starts,
    transitions and exits).  (a) every complete lattice path scores, within eps_u, the best state path of the network
    with that word string and those boundaries; (b) ``root`` under the original tables is the bigram score within
    eps_u and the walk is the bigram back-trace's words and boundaries; (c) ``root`` under another random ``lm'`` never
    exceeds the full bigram decode under ``lm'`` by more than eps_u; (d) beam 0 keeps exactly the best path's records,
    the kept set grows with the beam and ``inf`` keeps exactly the records on complete paths."""
    rng = np.random.default_rng(11)
    paths = finite = reached = 0
    for case in range(28):
        T = case % 7
        ls, lt, lx, lm, lm2, logb = _tiny(rng, T)
        lat = lref.lattice(logb, ls, lt, lx, *lm)
        every = lref.enumerate_paths(logb, ls, lt, lx, *lm)
        eps = lat["eps"]
        want = bref.viterbi(logb, ls, lt, lx, *lm)
        assert lat["score"] == want[0]
        # (a)
        mine = lref.lattice_paths(lat, *lm)
        for p, v in mine.items():
            assert p in every and abs(v - every[p]) <= eps, (case, p)
        paths += len(mine)
        # (b)
        if not np.isfinite(want[0]):
            assert lat["root"] == NEG and not mine and not every and lat["n_words"] == 0
            assert (lat["path_word"] == -1).all() and not lat["path_entry"].any()
            assert not lref.kept(lat["margin"], np.inf, eps).any()
            continue
        finite += 1
        assert abs(lat["root"] - want[0]) <= eps and abs(max(every.values()) - want[0]) <= eps
        assert lat["n_words"] == want[1]
        assert np.array_equal(lat["path_word"], want[2]) and np.array_equal(lat["path_entry"], want[4])
        # (c)
        lat2 = lref.lattice(logb, ls, lt, lx, *lm, lm2=lm2)
        full2 = bref.viterbi(logb, ls, lt, lx, *lm2)[0]
        assert lat2["root"] <= full2 + eps, case
        mine2 = lref.lattice_paths(lat, *lm2)
        assert (abs(max(mine2.values()) - lat2["root"]) <= eps) if mine2 else lat2["root"] == NEG
        every2 = lref.enumerate_paths(logb, ls, lt, lx, *lm2)
        for p, v in mine2.items():   # the rescored paths are real paths under lm' too
            assert abs(v - every2[p]) <= eps, (case, p)
        reached += bool(mine2) and abs(lat2["root"] - full2) <= eps
        # (d)
        best = max(mine, key=mine.get)
        off = [v for p, v in mine.items() if p != best]
        assert not off or max(off) < mine[best] - 1e-9      # (the best string is unique far beyond eps_u)
        k0 = lref.kept(lat["margin"], 0.0, eps)
        assert {(int(t), int(w)) for t, w in zip(*np.nonzero(k0))} == _path_records(best)
        on_paths = set().union(*[_path_records(p) for p in mine])
        kinf = lref.kept(lat["margin"], np.inf, eps)
        assert {(int(t), int(w)) for t, w in zip(*np.nonzero(kinf))} == on_paths
        prev = k0
        for beam in (0.5, 2.0, 8.0, 50.0):
            k = lref.kept(lat["margin"], beam, eps)
            assert (k | prev).sum() == k.sum() and (k & ~kinf).sum() == 0
            # exactly the records of the paths within the beam
            within = set().union(*[_path_records(p) for p, v in mine.items() if v >= mine[best] - beam - eps])
            near = {(int(t), int(w)) for t, w in zip(*np.nonzero(k))}
            assert within <= near
            prev = k
    assert finite >= 18 and paths >= 100 and reached >= 6


def test_start_frames_by_carrying_equal_the_back_trace_and_the_tie_case():
    """(e) ``lref.forward`` asserts, for every live (t, w), that the carried ``B_t(w)`` is the frame the bigram
    back-trace from ``(t, w, xarg_t(w))`` reaches; here it runs over ties.  ``_bigram_ref.tie_case()`` by hand (its
    docstring has delta): t = 0: words 0 and 1 enter, B = 0, X = 1; word 2 cannot start, B = -1.  t = 1: word 2 is
    entered (N_0(2) = 1 from word 0, the WORD tie), B_1(2) = 1; words 0 and 1 stay, B = 0.  t = 2: d(2,0) has within =
    entry = 0, WITHIN keeps it, so b stays 1; d(2,1) = 1 comes from state 0, b = 1; X_2(2) = 1 in state 0 (the first
    maximum of 0 + 1 and 1 + 0): B_2(2) = 1.  t = 3: within again, X_3(2) = 0 in state 0 (the STATE tie): B_3(2) = 1.
    So the only complete path is word 0 over frame 0, word 2 over frames 1 .. 3; ac(0, t = 0) = X_0(0) - lm_start[0] =
    1, ac(2, t = 3) = X_3(2) - N_0(2) = 0 - 1 = -1, root = 0 + 1 + 0 + (-1) + 0 = 0 = score, and first = (0, 0): word 1
    ties with word 0 at the root and loses (the first maximum, w' ascending)."""
    logb, ls, lt, lx, lm, lm0, lm1, expected = bref.tie_case()
    lat = lref.lattice(logb, ls, lt, lx, lm, lm0, lm1)
    assert lat["B"].tolist() == [[0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 1]]
    assert lat["X"][:, 2].tolist() == [NEG, 2.0, 1.0, 0.0] and lat["X"][0].tolist() == [1.0, 1.0, NEG]
    assert lat["root"] == 0.0 == lat["score"] == expected[0] and lat["first"] == (0, 0)
    assert lat["next_end"][0].tolist() == [3, 3, -1] and lat["next_word"][0].tolist() == [2, 2, 255]
    assert lat["beta"][0].tolist() == [-1.0, -1.0, NEG] and lat["beta"][3].tolist() == [NEG, NEG, 0.0]
    assert lat["n_words"] == expected[1]
    assert np.array_equal(lat["path_word"], expected[2]) and np.array_equal(lat["path_entry"], expected[4])
    assert lat["margin"][0].tolist() == [0.0, 0.0, NEG] and lat["margin"][3].tolist() == [NEG, NEG, 0.0]
    rng = np.random.default_rng(3)
    for T in (1, 2, 5, 9):      # integer tables: ties everywhere, and the assertion inside forward() holds
        ls, lt, lx = (np.round(rng.normal(0, 1, s)) for s in ((3, 2), (3, 2, 2), (3, 2)))
        lm = tuple(np.round(a) for a in bref.random_lm(rng, 3))
        lat = lref.lattice(np.round(rng.normal(0, 1, (T, 3, 2))), ls, lt, lx, *lm)
        assert lat["root"] == lat["score"]      # (integers: no rounding at all)


# ---- what the device tests rely on --------------------------------------------------------------------------------
@pytest.mark.parametrize("W,S", lc.SHAPES)
def test_device_cases_have_a_unique_best_string(W, S):
    """On every random case of tests/test_lattice_gpu.py every record off the best path has a margin below -1e-6 (eps_u
    is about 1e-10 there), the walk is the bigram back-trace's string, and the dead word has no record on a complete
    path; both backward passes find paths."""
    for topology in lc.TOPOLOGIES:
        for exits in lc.EXITS:
            ls, lt, lx, lm, lm2, logb, dead = lc.random_case(W, S, topology, exits)
            per, tabs, per2, tabs2 = lc.reference(W, S, topology, exits)
            want = bref.viterbi_batch(logb, lc.LENGTHS, ls, lt, lx, *lm)
            assert np.array_equal(tabs["path_word"], want[2]) and np.array_equal(tabs["path_entry"], want[4])
            assert np.array_equal(tabs["n_words"], want[1]) and tabs["score"].tobytes() == want[0].tobytes()
            for u, lat in enumerate(per):
                assert lat["eps"] < 1e-9
                assert lc.off_path_margin(lat) < -lc.MARGIN, (W, S, topology, exits, u)
                assert abs(lat["root"] - lat["score"]) <= lat["eps"] or lat["root"] == lat["score"] == NEG
                if W > 1:
                    assert (lat["margin"][:, dead] == NEG).all()
                assert per2[u]["root"] <= bref.viterbi(
                    logb[sum(lc.LENGTHS[:u]):sum(lc.LENGTHS[:u + 1])], ls, lt, lx, *lm2)[0] + lat["eps"]
            assert sum(np.isfinite(lat["root"]) for lat in per) >= 5
            assert sum(np.isfinite(lat["root"]) for lat in per2) >= 5


@pytest.mark.parametrize("order", lc.E2E_ORDERS)
def test_end_to_end_case_has_reached_utterances_whose_strings_differ(order):
    """``_bigram_ref.E2E_CASE``: the free loop cannot tell words 2 and 3 apart (an exact tie: the lower position in the
    vocabulary wins); the lattice it leaves, rescored under the grammar, reaches the grammar decode's score on
    utterances whose free-loop string differs from the grammar's — with word 2 before word 3 in the vocabulary and with
    word 3 before word 2 (the decoder loads the words in directory order)."""
    rows = lc.e2e(order)
    assert all(r["root"] <= r["grammar_score"] + r["eps"] for r in rows)
    reach = [r for r in rows if r["reach"]]
    assert all(r["words"] == r["grammar_words"] for r in reach)
    assert sum(r["free_words"] != r["grammar_words"] for r in reach) >= 1
    assert all(r["grammar_words"] == r["truth"] for r in rows)


# ---- the SLF export, read back ------------------------------------------------------------------------------------
class _HostLattice:
    """``WordLattice``'s host side over the definition's tables: what ``to_slf`` and ``records`` read."""

    def __new__(cls, lat, lm):
        from sapr_amd.connected import LatticeBackward, WordLattice
        self = object.__new__(WordLattice)
        T, W = lat["X"].shape
        self.W, self.offsets, self.score = W, np.array([0, T], np.int64), np.array([lat["score"]])
        self._lm, self._host, self._eps = lm, (lat["X"], lat["N"], lat["B"]), None
        self._own = LatticeBackward(lat["beta"], lat["next_end"], lat["next_word"], np.array([lat["root"]]),
                                    np.array([lat["first"]], np.int32))
        return self


def _read_slf(text):
    nodes, links = {}, []
    for line in text.splitlines():
        f = dict(kv.split("=", 1) for kv in line.split())
        if "I" in f:
            nodes[int(f["I"])] = (float(f["t"]), f["W"])
        elif "J" in f:
            links.append((int(f["S"]), int(f["E"]), float(f["a"]), float(f["l"])))
        elif "N" in f:
            counts = (int(f["N"]), int(f["L"]))
    assert counts == (len(nodes), len(links))
    return nodes, links


def test_slf_round_trip():
    """A ten-line parser reads ``to_slf``'s text back; a best-path DP over its links reproduces ``root`` within eps_u,
    at ``beam=None`` and at beam 0 (the best path alone)."""
    rng = np.random.default_rng(23)
    names = ["one", "two", "three"]
    done = 0
    for T in (1, 4, 6, 9):
        ls, lt, lx, lm, _, logb = _tiny(rng, T)
        lat = lref.lattice(logb, ls, lt, lx, *lm)
        if not np.isfinite(lat["root"]):
            continue
        host = _HostLattice(lat, lm)
        for beam in (None, 0.0):
            nodes, links = _read_slf(host.to_slf(0, names, beam=beam))
            end = max(nodes)
            assert nodes[0] == (0.0, "!NULL") and nodes[end] == (pytest.approx(T * 0.01), "!NULL")
            best = {0: 0.0}
            for a, b, ac, l in sorted(links, key=lambda k: (nodes[k[0]][0], k[0])):   # (time order is topological)
                if a in best:
                    best[b] = max(best.get(b, NEG), best[a] + l + ac)
            assert abs(best[end] - lat["root"]) <= lat["eps"], (T, beam)
            recs = host.records(0, np.inf if beam is None else beam)
            assert len(nodes) == len(recs) + 2
            assert sorted(n[1] for k, n in nodes.items() if 0 < k < end) == sorted(names[r[0]] for r in recs)
            if beam == 0.0:
                segs = bref.segments(lat["path_word"], lat["path_entry"])
                assert [(w, a, b) for w, a, b, _, _ in recs] == segs and len(links) == len(segs) + 1
        every = host.records(0)
        assert [(r[2] - 1, r[0]) for r in every] == [(t, w) for t, w, *_ in lref.records(
            lat["X"], lat["N"], lat["B"], lm[1])]
        assert [r[3] for r in every] == [r[4] for r in lref.records(lat["X"], lat["N"], lat["B"], lm[1])]
        assert np.array_equal(host.prune(2.0), lref.kept(lat["margin"], 2.0, lat["eps"]))
        with pytest.raises(ValueError, match="beam must be a number >= 0"):
            host.prune(-1.0)
        with pytest.raises(ValueError, match="2 names for 3 words"):
            host.to_slf(0, names[:2])
        done += 1
    assert done >= 3


# ---- the C ABI, without a device ----------------------------------------------------------------------------------
NAMES = ("sapr_connected_lattice_workspace_bytes", "sapr_connected_lattice", "sapr_connected_lattice_backward",
         "sapr_connected_lattice_walk")


def test_symbols_are_declared_bound_and_exported():
    from sapr_amd import _lib
    with open(os.path.join(ROOT, "include", "sapr_hip.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert "tests/_lattice_ref.py" in header
    assert "2 * a16(8 * total_frames * W) + a16(4 * total_frames * W)" in header
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    import sapr_amd
    from sapr_amd import connected
    for name in ("WordLattice", "LatticePath", "LatticeBackward", "connected_lattice", "lattice_workspace_bytes"):
        assert getattr(sapr_amd, name) is getattr(connected, name)
    with open(os.path.join(ROOT, "sapr_amd", "build.py"), encoding="utf-8") as fh:
        assert '"connected_lattice.hip"' in fh.read()


def _p(on):
    return C.cast((C.c_double * 1)(), C.c_void_p) if on else None


def _run(lib, n_utts=1, total=10, W=2, S=4, lm=1, lm_start=1, lm_end=1, ws=None, ws_bytes=0):
    """``sapr_connected_lattice`` with every pointer NULL except the three language-model tables (a host address the
    checks never dereference) and the workspace."""
    return lib.sapr_connected_lattice(None, None, n_utts, total, None, None, None, _p(lm), _p(lm_start), _p(lm_end), W,
                                      S, ws, ws_bytes, None, None, None)


def _back(lib, n_utts=1, total=10, W=2, S=4, fwd=1, lm=1, lm_start=1, lm_end=1, ws=None, ws_bytes=0):
    return lib.sapr_connected_lattice_backward(None, n_utts, total, W, S, ws, ws_bytes, _p(fwd), _p(lm), _p(lm_start),
                                               _p(lm_end), None, None, None, None, None, None)


def _walk(lib, n_utts=1, total=10, W=2, S=4):
    return lib.sapr_connected_lattice_walk(None, n_utts, total, W, S, None, None, None, None, None, None, None, None)


def test_size_function_and_refusals_before_any_launch():
    from sapr_amd import _lib
    from sapr_amd.connected import lattice_workspace_bytes
    lib = _lib.load()
    n = C.c_size_t(0)
    size = lib.sapr_connected_lattice_workspace_bytes
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    assert size(1000, 7, 11, 10, C.byref(n)) == 0
    assert n.value == 2 * a16(8 * 1000 * 11) + a16(4 * 1000 * 11) == 20 * 11 * 1000     # 20 W bytes per frame
    assert lattice_workspace_bytes(1000, 7, 11, 10) == n.value
    assert size(3, 1, 5, 7, C.byref(n)) == 0 and n.value == 2 * 128 + 64
    assert size(0, 0, 1, 1, C.byref(n)) == 0 and n.value == 0
    # unsupported: S = 19, W * SP = 260 — from the size function and the three entry points
    for W, S in ((2, 19), (26, 10), (65, 4)):
        assert size(10, 1, W, S, C.byref(n)) == -2
        assert _run(lib, W=W, S=S) == -2 and _back(lib, W=W, S=S) == -2 and _walk(lib, W=W, S=S) == -2
    assert b"W * SP" in lib.sapr_last_error()
    assert size(10, 1, 64, 4, C.byref(n)) == 0
    # bad sizes
    assert size(-1, 1, 2, 4, C.byref(n)) == -1
    assert b"bad sizes" in lib.sapr_last_error()
    assert size(10, -1, 2, 4, C.byref(n)) == -1 and size(10, 1, 0, 4, C.byref(n)) == -1
    assert size(10, 1, 2, 0, C.byref(n)) == -1 and size(10, 1, 2, 4, None) == -1
    for kw in (dict(n_utts=-1), dict(total=-1), dict(W=0), dict(S=-3)):
        for call in (_run, _back, _walk):
            assert call(lib, **kw) == -1
            assert b"bad sizes" in lib.sapr_last_error()
    # a NULL table, each of them
    for kw in (dict(lm=0), dict(lm_start=0), dict(lm_end=0)):
        for call in (_run, _back):
            assert call(lib, **kw) == -1
            assert b"NULL language model" in lib.sapr_last_error()
            assert call(lib, n_utts=0, total=0, **kw) == -1
    assert _back(lib, fwd=0) == -1 and b"NULL language model" in lib.sapr_last_error()
    # a workspace one byte short (host memory: never touched before the refusal)
    assert size(10, 1, 2, 4, C.byref(n)) == 0
    buf = (C.c_uint8 * n.value)()
    for call in (_run, _back):
        assert call(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value - 1) == -1
        assert b"workspace too small" in lib.sapr_last_error()
        # a full workspace passes on to the next check: the other required pointers
        assert call(lib, ws=C.cast(buf, C.c_void_p), ws_bytes=n.value) == -1
        assert b"NULL pointer" in lib.sapr_last_error()
        assert call(lib, n_utts=0, total=0) == 0            # nothing to do
    assert _walk(lib) == -1 and b"NULL pointer" in lib.sapr_last_error()
    assert _walk(lib, n_utts=0, total=0) == 0


def test_python_argument_refusals_come_before_a_device_is_asked_for(tmp_path):
    import pickle
    from sapr_amd.connected import ConnectedResult
    from sapr_amd.decoder import Decoder
    from sapr_amd.hmmlearn_hmm import GaussianHMM
    assert ConnectedResult(*[None] * 5, offsets=None).lattice is None
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
    for bad in (-1.0, -0.5, float("nan"), "wide"):
        with pytest.raises(ValueError, match="beam must be a number >= 0"):
            dec.decode_connected(x, lattice=bad)

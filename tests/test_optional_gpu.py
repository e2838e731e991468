"""GPU: optional transcript slots in forced alignment and embedded Baum-Welch (the OPT instantiations of
csrc/connected_align.hip and csrc/connected_embed.hip) through the C ABI, the Python layer and the Decoder against the
CPU restatement tests/_optional_ref.py and against the kernels without flags.  Every comparison with the restatement's
alignment recursion is ``np.array_equal``; the embedded comparisons use the tolerances of tests/test_embedded_gpu.py,
tests/test_embedded_full_gpu.py and tests/test_embedded_gmm_gpu.py, imported from there.  tests/test_optional_cpu.py
checks that the cases step over slots, take optional ones and move both ends of the chain."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import _align_ref as aref
from tests import _connected_family_cases as cases
from tests import _optional_ref as oref
from tests.test_align_gpu import _diag_decoder_case, _pickle_models, _raw_align
from tests.test_embedded_full_gpu import _check_rows as _check_full_rows
from tests.test_embedded_gmm_gpu import _check_rows as _check_gmm_rows
from tests.test_embedded_gmm_gpu import _emitted, _network
from tests.test_embedded_gpu import STAT_KEYS, TOL, _check_loglik, _check_post, _check_stats, _raw_embed
from tests.test_embedded_gpu import _check_params, _raw_stats
from tests.test_optional_cpu import pause_family_case

pytestmark = pytest.mark.gpu

NEG = -np.inf
FIELDS = ("score", "path_word", "path_state", "path_entry", "word_start")
LENGTHS = aref.RECURSION_LENGTHS


def _assert_equal(res, want, what):
    for f, w in zip(FIELDS, want):
        assert np.array_equal(getattr(res, f), w), (f, what)     # (bit-equal: -inf == -inf, no NaN in these cases)


def _flag_bytes(optional):
    return None if optional is None else np.concatenate([np.asarray(o, np.uint8) for o in optional]).astype(np.uint8)


def _raw_align_opt(logb, lengths, transcripts, optional, ls, lt, lx, pen, max_words, small=False):
    """``sapr_connected_align_opt`` itself (``optional``: one sequence of bytes per utterance, whatever they hold, or
    ``None`` for NULL): ``(score, path_word, path_state, path_entry, word_start)`` on the host.  The workspace has the
    size of ``sapr_connected_align_opt_workspace_bytes`` (``small``: of ``sapr_connected_align_workspace_bytes``, which
    NULL flags make do with) and the bytes behind it must stay untouched."""
    import torch
    from sapr_amd import _lib
    from sapr_amd.connected import layout
    W, S = ls.shape
    SP = layout(W, S)[0]
    total = int(sum(lengths))
    wide = np.full((total, W, SP), NEG)
    wide[:, :, :S] = logb
    offs = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    woffs = np.r_[0, np.cumsum([len(t) for t in transcripts])].astype(np.int64)
    words = np.concatenate([np.asarray(t, np.int32) for t in transcripts]).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    lib = _lib.load()
    n, base = C.c_size_t(0), C.c_size_t(0)
    assert lib.sapr_connected_align_opt_workspace_bytes(total, len(lengths), max_words, S, C.byref(n)) == 0
    assert lib.sapr_connected_align_workspace_bytes(total, len(lengths), max_words, S, C.byref(base)) == 0
    assert n.value == base.value + (len(lengths) + 15) // 16 * 16
    size = base.value if small else n.value
    guard = 4096                                                 # the bytes behind the workspace must stay untouched
    ws = torch.full((size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    t_logb, t_offs, t_woffs, t_words, t_ls, t_lt, t_lx = (dev(a) for a in (wide, offs, woffs, words, ls, lt, lx))
    flags = _flag_bytes(optional)
    t_flags = None if flags is None else dev(flags)
    score = torch.empty(len(lengths), dtype=torch.float64, device="cuda")
    pw = torch.empty(total, dtype=torch.int32, device="cuda")
    ps = torch.empty(total, dtype=torch.int32, device="cuda")
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")
    start = torch.empty(len(words), dtype=torch.int32, device="cuda")
    _lib.check(lib.sapr_connected_align_opt(
        _lib.ptr(t_logb), _lib.ptr(t_offs), len(lengths), total, _lib.ptr(t_words), _lib.ptr(t_woffs),
        _lib.ptr(t_flags), len(words), max_words, _lib.ptr(t_ls), _lib.ptr(t_lt), _lib.ptr(t_lx), pen, W, S,
        _lib.ptr(ws), size, _lib.ptr(score), _lib.ptr(pw), _lib.ptr(ps), _lib.ptr(pe), _lib.ptr(start),
        _lib.current_stream()), "sapr_connected_align_opt")
    torch.cuda.synchronize()
    assert bool((ws[size:] == 0xA5).all())
    return tuple(a.cpu().numpy() for a in (score, pw, ps, pe, start))


def _raw_embed_opt(logb, lengths, transcripts, optional, ls, lt, lx, pen, max_words, feats=None):
    """``sapr_connected_embed_opt`` itself: ``(loglik, stats[W, width], post)``; the workspace is that of
    ``sapr_connected_embed_workspace_bytes`` and the bytes behind it must stay untouched."""
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
    D = 0 if feats is None else feats.shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    lib = _lib.load()
    n, width = C.c_size_t(0), C.c_int32(0)
    assert lib.sapr_connected_embed_workspace_bytes(total, len(lengths), len(words), max_words, S, D, C.byref(n)) == 0
    assert lib.sapr_connected_embed_stats_width(S, D, C.byref(width)) == 0
    guard = 4096
    ws = torch.full((n.value + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    t_logb, t_offs, t_woffs, t_words, t_ls, t_lt, t_lx = (dev(a) for a in (wide, offs, woffs, words, ls, lt, lx))
    t_feats = None if feats is None else dev(np.asarray(feats, np.float32))
    flags = _flag_bytes(optional)
    t_flags = None if flags is None else dev(flags)
    loglik = torch.empty(len(lengths), dtype=torch.float64, device="cuda")
    stats = torch.full((W, width.value), np.nan, dtype=torch.float64, device="cuda")
    post = torch.zeros((total, max_words * SP), dtype=torch.float64, device="cuda")
    _lib.check(lib.sapr_connected_embed_opt(
        _lib.ptr(t_logb), _lib.ptr(t_feats), D, _lib.ptr(t_offs), len(lengths), total, _lib.ptr(t_words),
        _lib.ptr(t_woffs), _lib.ptr(t_flags), len(words), max_words, _lib.ptr(t_ls), _lib.ptr(t_lt), _lib.ptr(t_lx),
        pen, W, S, _lib.ptr(ws), n.value, _lib.ptr(loglik), _lib.ptr(stats), _lib.ptr(post), _lib.current_stream()),
        "sapr_connected_embed_opt")
    torch.cuda.synchronize()
    assert bool((ws[n.value:] == 0xA5).all())
    return tuple(a.cpu().numpy() for a in (loglik, stats, post))


# ---- alignment: the recursion, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("exits", aref.EXITS)
@pytest.mark.parametrize("topology", aref.TOPOLOGIES)
@pytest.mark.parametrize("W,S,max_words", aref.RECURSION_SHAPES)
def test_recursion_equals_reference(W, S, max_words, topology, exits):
    """All nine (RL, SP) instantiations; the integer tables are where the near and the far slot tie."""
    from sapr_amd.connected import ConnectedNetwork, align_viterbi
    for integer in (False, True):
        ls, lt, lx, logb, transcripts, optional = oref.optional_case(W, S, max_words, topology, exits, integer)
        assert max(len(t) for t in transcripts) == max_words or max_words == 64
        for pen in oref.PENALTIES:
            res = align_viterbi(logb, LENGTHS, transcripts, ConnectedNetwork(ls, lt, lx, word_penalty=pen),
                                optional=optional)
            want = oref.align_batch(logb, LENGTHS, transcripts, optional, ls, lt, lx, pen)
            _assert_equal(res, want, (integer, pen))
            assert np.array_equal(res.optional, _flag_bytes(optional))
            woffs = res.word_offsets
            assert int(np.isfinite(res.score).sum()) >= 6
            # (the utterances of 1 and 2 frames carry T + 1 slots: without flags they have no path; with flags
            # the definition decides — stepping over slots may leave few enough — and the comparison above holds it)
            assert res.score[LENGTHS.index(0)] == NEG
            for u in np.flatnonzero(~np.isfinite(res.score)):
                assert res.score[u] == NEG and res.segments(u) == []
                lo, hi = res.offsets[u], res.offsets[u + 1]
                assert (res.path_word[lo:hi] == -1).all() and (res.path_state[lo:hi] == -1).all()
                assert not res.path_entry[lo:hi].any() and (res.word_start[woffs[u]:woffs[u + 1]] == -1).all()
            for u in np.flatnonzero(np.isfinite(res.score)):
                segs = res.segments(u)
                assert segs == oref.segments(transcripts[u], want[4][woffs[u]:woffs[u + 1]], LENGTHS[u])
                assert segs[0][1] == 0 and segs[-1][2] == LENGTHS[u]
                taken = [k for k in range(len(transcripts[u])) if want[4][woffs[u] + k] >= 0]
                assert [w for w, _, _ in segs] == [transcripts[u][k] for k in taken]
                assert all(optional[u][k] for k in range(len(transcripts[u])) if k not in taken)


@pytest.mark.parametrize("W,S,max_words", [(11, 10, 5), (11, 18, 5), (4, 10, 9), (3, 12, 3), (3, 4, 10)])
def test_alignment_is_the_best_expansion_under_the_kernel_without_flags(W, S, max_words):
    """Per utterance the best of ``align_viterbi`` WITHOUT flags over the explicit expansions (every subset of the
    optional slots deleted; at most 6 optional slots in these cases): ``==`` on the score, and equal rows where the
    best expansion is unique.  One call of the old kernel per rank of expansion, every utterance in it."""
    from sapr_amd.connected import ConnectedNetwork, align_viterbi
    ls, lt, lx, logb, transcripts, optional = oref.optional_case(W, S, max_words, "skip", "any", False)
    live = [u for u, t in enumerate(transcripts) if LENGTHS[u] > 2]
    offs = np.r_[0, np.cumsum(LENGTHS)]
    exps = {u: oref.expansions(transcripts[u], optional[u]) for u in live}
    assert max(sum(o) for o in optional) <= 6
    net = ConnectedNetwork(ls, lt, lx, word_penalty=-2.0)
    got = align_viterbi(logb, LENGTHS, transcripts, net, optional=optional)
    results = {u: [] for u in live}
    for rank in range(max(len(e) for e in exps.values())):
        us = [u for u in live if rank < len(exps[u])]
        res = align_viterbi(np.concatenate([logb[offs[u]:offs[u + 1]] for u in us]), [LENGTHS[u] for u in us],
                            [exps[u][rank][1] for u in us], net)
        for n, u in enumerate(us):
            lo, hi = res.offsets[n], res.offsets[n + 1]
            results[u].append((res.score[n], res.path_word[lo:hi], res.path_state[lo:hi], res.path_entry[lo:hi],
                               res.word_start[res.word_offsets[n]:res.word_offsets[n + 1]]))
    unique = 0
    for u in live:
        best = max(r[0] for r in results[u])
        assert got.score[u] == best, u
        winners = [n for n, r in enumerate(results[u]) if r[0] == best]
        if np.isfinite(best) and len(winners) == 1:
            unique += 1
            keep, r = exps[u][winners[0]][0], results[u][winners[0]]
            lo, hi = got.offsets[u], got.offsets[u + 1]
            for f, w in zip(FIELDS[1:4], r[1:4]):
                assert np.array_equal(getattr(got, f)[lo:hi], w), (u, f)
            start = np.full(len(transcripts[u]), -1, np.int32)
            start[keep] = r[4]
            assert np.array_equal(got.word_start[got.word_offsets[u]:got.word_offsets[u + 1]], start)
    assert unique >= 5


def test_zero_flags_and_null_return_the_bytes_of_the_entry_point_without_flags():
    W, S, max_words = 5, 7, 25
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, "skip", "any", False)
    old = _raw_align(logb, LENGTHS, transcripts, ls, lt, lx, -1.5, max_words)
    assert np.isfinite(old[0]).sum() >= 6
    zero = [[0] * len(t) for t in transcripts]
    for flags, small in ((zero, False), (None, False), (None, True)):
        got = _raw_align_opt(logb, LENGTHS, transcripts, flags, ls, lt, lx, -1.5, max_words, small)
        for a, b in zip(got, old):
            assert a.tobytes() == b.tobytes(), (flags is None, small)


def test_broken_flags_at_the_c_abi():
    """What the Python layer refuses earlier — two optional neighbours, every slot optional, a flag byte of 7 — makes
    its own utterance pathless and changes nothing else."""
    W, S, max_words = 5, 7, 4
    ls, lt, lx, logb, _ = aref.recursion_case(W, S, 25, "skip", "any", False)
    lengths = [40, 64, 30, 3, 50, 20]
    logb = logb[:sum(lengths)]
    words = [[1, 4, 4], [0, 2, 3, 1], [2], [3], [4, 0], [1, 1, 2]]
    good = [[1, 0, 0], [0, 1, 0, 1], [0], [0], [1, 0], [0, 1, 0]]
    bad = [[1, 0, 0], [0, 1, 1, 0], [1], [0], [1, 0], [0, 7, 0]]
    want = oref.align_batch(logb, lengths, words, good, ls, lt, lx, -1.5)
    assert np.isfinite(want[0]).all()
    offs = np.r_[0, np.cumsum(lengths)]
    woffs = np.r_[0, np.cumsum([len(t) for t in words])]
    got = _raw_align_opt(logb, lengths, words, bad, ls, lt, lx, -1.5, max_words)
    for a, b in zip(got, oref.align_batch(logb, lengths, words, bad, ls, lt, lx, -1.5)):
        assert np.array_equal(a, b)
    for u in (0, 3, 4):
        assert got[0][u] == want[0][u]
        for k in (1, 2, 3):
            assert np.array_equal(got[k][offs[u]:offs[u + 1]], want[k][offs[u]:offs[u + 1]])
        assert np.array_equal(got[4][woffs[u]:woffs[u + 1]], want[4][woffs[u]:woffs[u + 1]])
    for u in (1, 2, 5):
        assert got[0][u] == NEG
        assert (got[1][offs[u]:offs[u + 1]] == -1).all() and (got[2][offs[u]:offs[u + 1]] == -1).all()
        assert not got[3][offs[u]:offs[u + 1]].any() and (got[4][woffs[u]:woffs[u + 1]] == -1).all()
    for a, b in zip(_raw_align_opt(logb, lengths, words, good, ls, lt, lx, -1.5, max_words), want):
        assert np.array_equal(a, b)


def test_a_nan_frame_stays_inside_its_utterance():
    W, S, max_words = 14, 18, 14
    ls, lt, lx, logb, transcripts, optional = oref.optional_case(W, S, max_words, "dense", "any", False)
    offs = np.r_[0, np.cumsum(LENGTHS)]
    clean = _raw_align_opt(logb, LENGTHS, transcripts, optional, ls, lt, lx, -2.0, max_words)
    hit = LENGTHS.index(300)
    assert np.isfinite(clean[0][hit])
    dirty = logb.copy()
    dirty[offs[hit] + 150] = np.nan
    got = _raw_align_opt(dirty, LENGTHS, transcripts, optional, ls, lt, lx, -2.0, max_words)
    woffs = np.r_[0, np.cumsum([len(t) for t in transcripts])]
    for u in range(len(LENGTHS)):
        if u == hit:
            continue
        assert got[0][u:u + 1].tobytes() == clean[0][u:u + 1].tobytes()
        for k in (1, 2, 3):
            assert np.array_equal(got[k][offs[u]:offs[u + 1]], clean[k][offs[u]:offs[u + 1]])
        assert np.array_equal(got[4][woffs[u]:woffs[u + 1]], clean[4][woffs[u]:woffs[u + 1]])
    lo, hi = offs[hit], offs[hit + 1]
    assert not np.isfinite(got[0][hit])                          # nothing is repaired: the utterance has no path
    assert (got[1][lo:hi] == -1).all() and (got[2][lo:hi] == -1).all() and not got[3][lo:hi].any()
    assert (got[4][woffs[hit]:woffs[hit + 1]] == -1).all()


def test_alignment_is_deterministic_and_independent_of_the_batch():
    from sapr_amd.connected import ConnectedNetwork, align_viterbi
    W, S, max_words = 11, 18, 5
    ls, lt, lx, logb, transcripts, optional = oref.optional_case(W, S, max_words, "dense", "any", False)
    net = ConnectedNetwork(ls, lt, lx, word_penalty=-2.0)
    a, b = (align_viterbi(logb, LENGTHS, transcripts, net, optional=optional) for _ in range(2))
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for u in (1, 3, 9):
        lo, hi = a.offsets[u], a.offsets[u + 1]
        one = align_viterbi(logb[lo:hi], [LENGTHS[u]], [transcripts[u]], net, optional=[optional[u]])
        assert one.score.tobytes() == a.score[u:u + 1].tobytes()
        for f in ("path_word", "path_state", "path_entry"):
            assert np.array_equal(getattr(one, f), getattr(a, f)[lo:hi]), f
        assert np.array_equal(one.word_start, a.word_start[a.word_offsets[u]:a.word_offsets[u + 1]])


# ---- embedded Baum-Welch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,S,max_words", aref.RECURSION_SHAPES)
def test_embedded_recursion_equals_reference(W, S, max_words):
    """``loglik``, ``post`` and the statistics of the diagonal family over all nine (RL, SP) instantiations."""
    from sapr_amd.connected import ConnectedNetwork, embedded_forward_backward
    n = aref.RECURSION_SHAPES.index((W, S, max_words))
    topology, exits = aref.TOPOLOGIES[n % 3], aref.EXITS[n % 2]
    ls, lt, lx, logb, transcripts, optional = oref.optional_case(W, S, max_words, topology, exits, False)
    pen = aref.PENALTIES[n % 3]
    feats = np.random.default_rng(n).normal(0.0, 3.0, (sum(LENGTHS), 3)).astype(np.float32)
    res = embedded_forward_backward(logb, LENGTHS, transcripts, ConnectedNetwork(ls, lt, lx, word_penalty=pen),
                                    feats=feats, want_post=True, optional=optional)
    want = oref.estep_batch(logb, LENGTHS, transcripts, optional, ls, lt, lx, pen, feats)
    what = (W, S, topology, exits, pen)
    _check_loglik(res.loglik, want["loglik"], what)
    assert int(np.isfinite(res.loglik).sum()) >= 6
    assert res.loglik[LENGTHS.index(0)] == NEG                    # (1 and 2 frames: the definition decides, see above)
    _check_post(res, want["post"], S, LENGTHS, what)
    _check_stats(res, want, W, what=str(what))
    rows = res.post.sum(axis=1)
    offs = np.r_[0, np.cumsum(LENGTHS)]
    for u in np.flatnonzero(np.isfinite(res.loglik)):
        np.testing.assert_allclose(rows[offs[u]:offs[u + 1]], 1.0, rtol=0, atol=TOL["atol"])


def test_second_moments_with_optional_slots():
    """The batch of ``test_embedded_full_gpu.test_tile_geometry`` (repeated words: the slot collapse) at D = 13."""
    from sapr_amd.connected import ConnectedNetwork, embedded_forward_backward
    W, S, D = 4, 5, 13
    rng = np.random.default_rng(300)
    ls, lt, lx = aref.network(rng, W, S, "skip", "last", False)
    lengths = [33, 70, 12, 129, 2, 48]
    transcripts = [[2, 2, 2], [0, 1, 2, 3, 0], [3], [1, 1, 3, 3, 1, 1, 0], [0, 1, 2], [2, 0]]
    optional = [[0, 1, 0], [1, 0, 1, 0, 1], [0], [0, 1, 0, 1, 0, 0, 1], [1, 0, 1], [0, 1]]
    logb = rng.normal(-40.0, 15.0, (sum(lengths), W, S))
    feats = np.random.default_rng(300 + D).normal(0.0, 8.0, (sum(lengths), D)).astype(np.float32)
    want = oref.estep_batch(logb, lengths, transcripts, optional, ls, lt, lx, -4.0, feats, second_moments=True)
    assert np.isfinite(want["loglik"]).sum() == 5 and want["loglik"][4] == NEG
    net = ConnectedNetwork(ls, lt, lx, word_penalty=-4.0)
    res = embedded_forward_backward(logb, lengths, transcripts, net, feats=feats, want_post=True, second_moments=True,
                                    optional=optional)
    assert res.layout == "full"
    _check_loglik(res.loglik, want["loglik"], "full")
    _check_post(res, want["post"], S, lengths, "full")
    _check_full_rows(res.stats, want, S, D, what="optional")
    # all-zero flags: the bytes of the entry point without flags
    zero = [[0] * len(t) for t in transcripts]
    a = embedded_forward_backward(logb, lengths, transcripts, net, feats=feats, want_post=True, second_moments=True)
    b = embedded_forward_backward(logb, lengths, transcripts, net, feats=feats, want_post=True, second_moments=True,
                                  optional=zero)
    for key in ("loglik", "stats", "post"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key


def test_mixture_statistics_with_optional_slots():
    """The smallest committed mixture case through ``embedded_estep(..., mixtures=True, optional=)``; word 1 serves as
    the optional silence.  The restatement is fed the emitted ``logb`` read back from the device."""
    from sapr_amd.connected import embedded_estep, with_optional
    spec = cases.GMM_CASES[0]
    model, utts, truth, net = _network(spec, -3.0, "last")
    transcripts, optional = with_optional(truth, 1)
    x = np.concatenate(utts)
    lengths = [len(u) for u in utts]
    S, M, D = spec[2], spec[3], spec[4]
    want = oref.estep_batch(_emitted(net, x), lengths, transcripts, optional, net.log_start, net.log_trans,
                            net.log_exit, net.word_penalty, x,
                            mixtures=(model["weights"], model["means"], model["covars"]))
    assert np.isfinite(want["loglik"]).all()
    res = embedded_estep(utts, transcripts, net, want_post=True, mixtures=True, optional=optional)
    assert res.layout == "gmm" and res.M == M
    _check_loglik(res.loglik, want["loglik"], spec)
    np.testing.assert_allclose(res.post.reshape(len(x), -1, res.SP)[:, :, :S], want["post"], **TOL)
    _check_gmm_rows(res.stats, want, S, M, D, what=f"{spec} optional")
    zero = [[0] * len(t) for t in truth]
    a = embedded_estep(utts, truth, net, want_post=True, mixtures=True)
    b = embedded_estep(utts, truth, net, want_post=True, mixtures=True, optional=zero)
    for key in ("loglik", "stats", "post"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key


def test_embedded_zero_flags_null_broken_flags_and_two_calls():
    """At the C ABI: all-zero flags and NULL return the bytes of ``sapr_connected_embed``; broken flags make their own
    utterance pathless — -inf, zero posterior rows, exact zeros in the statistics: the other utterances keep their
    bytes and the statistics are those of the batch without it; two calls return the same bytes."""
    W, S, max_words, D = 5, 7, 4, 3
    ls, lt, lx, logb, _ = aref.recursion_case(W, S, 25, "skip", "any", False)
    lengths = [40, 64, 30, 3, 50, 20]
    logb = logb[:sum(lengths)]
    feats = np.random.default_rng(2).normal(0.0, 3.0, (sum(lengths), D)).astype(np.float32)
    words = [[1, 4, 4], [0, 2, 3, 1], [2], [3], [4, 0], [1, 1, 2]]
    good = [[1, 0, 0], [0, 1, 0, 1], [0], [0], [1, 0], [0, 1, 0]]
    bad = [[1, 0, 0], [0, 1, 1, 0], [1], [0], [1, 0], [0, 7, 0]]
    zero = [[0] * len(t) for t in words]
    old = _raw_embed(logb, lengths, words, ls, lt, lx, -1.5, max_words, feats)
    for flags in (zero, None):
        got = _raw_embed_opt(logb, lengths, words, flags, ls, lt, lx, -1.5, max_words, feats)
        for a, b in zip(got, old):
            assert a.tobytes() == b.tobytes(), flags is None
    clean = _raw_embed_opt(logb, lengths, words, good, ls, lt, lx, -1.5, max_words, feats)
    again = _raw_embed_opt(logb, lengths, words, good, ls, lt, lx, -1.5, max_words, feats)
    for a, b in zip(clean, again):
        assert a.tobytes() == b.tobytes()
    want = oref.estep_batch(logb, lengths, words, good, ls, lt, lx, -1.5, feats, max_words)
    assert np.isfinite(want["loglik"]).all()
    _check_loglik(clean[0], want["loglik"], "clean")
    got = _raw_embed_opt(logb, lengths, words, bad, ls, lt, lx, -1.5, max_words, feats)
    want = oref.estep_batch(logb, lengths, words, bad, ls, lt, lx, -1.5, feats, max_words)
    offs = np.r_[0, np.cumsum(lengths)]
    for u in range(len(lengths)):
        rows = slice(offs[u], offs[u + 1])
        if u in (1, 2, 5):
            assert got[0][u] == NEG and want["loglik"][u] == NEG and not got[2][rows].any(), u
        else:
            assert got[0][u:u + 1].tobytes() == clean[0][u:u + 1].tobytes(), u
            assert got[2][rows].tobytes() == clean[2][rows].tobytes(), u
    for w, st in enumerate(_raw_stats(got[1], S, D)):
        assert st["nobs"] == want["nobs"][w] and st["logprob"] == 0.0
        for k_ref, k_got in STAT_KEYS:
            np.testing.assert_allclose(st[k_got], want[k_ref][w], err_msg=f"{k_ref} {w}", **TOL)
    # a batch of pathless utterances only: every statistic is an exact zero
    none = _raw_embed_opt(logb, lengths, words, [[1] * len(t) for t in words], ls, lt, lx, -1.5, max_words, feats)
    assert (none[0] == NEG).all() and not none[1].any() and not none[2].any()


# ---- recordings with pauses nobody wrote down -------------------------------------------------------------------
def _family_network(family, model, pen):
    from sapr_amd.connected import ConnectedNetwork
    if family == "diag":
        return ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], pen, None, model["means"],
                                model["vars"], model["gconst"])
    return ConnectedNetwork.from_models(cases.models_of(family, model), word_penalty=pen)


def test_the_inserted_pauses_are_found_and_without_flags_they_are_pressed_into_words():
    from sapr_amd.connected import connected_align, with_optional
    model, utts, truth = pause_family_case("diag")
    recs, inserted, masks = oref.pause_case("diag", model, utts, truth)
    transcripts, optional = with_optional(truth, oref.PAUSE_WORD)
    lengths = [len(x) for x in recs]
    logb = oref._emission("diag", model, np.concatenate(recs))
    for pen in (0.0, -30.0):
        net = _family_network("diag", model, pen)
        res = connected_align(recs, transcripts, net, optional)
        want = oref.align_batch(logb, lengths, transcripts, optional, model["log_start"], model["log_trans"],
                                model["log_exit"], pen)
        assert np.isfinite(want[0]).all()
        for f, w in zip(FIELDS[1:], want[1:]):
            assert np.array_equal(getattr(res, f), w), f
        np.testing.assert_allclose(res.score, want[0], rtol=1e-12)
        for u in range(len(recs)):
            lo, hi = res.offsets[u], res.offsets[u + 1]
            assert (res.path_word[lo:hi][masks[u]] == oref.PAUSE_WORD).all()
            _, flags, took = oref.pause_slots(truth[u], inserted[u])
            start = res.word_start[res.word_offsets[u]:res.word_offsets[u + 1]]
            assert [k for k in range(len(flags)) if flags[k] and start[k] >= 0] == took
        # no silence in the transcript: every pause frame lands in a written word
        plain = connected_align(recs, truth, net)
        for u in range(len(recs)):
            if oref.PAUSE_WORD in truth[u] or not np.isfinite(plain.score[u]):
                continue
            lo, hi = plain.offsets[u], plain.offsets[u + 1]
            assert np.isin(plain.path_word[lo:hi][masks[u]], truth[u]).all()
            assert sum(b - a for _, a, b in plain.segments(u)) == lengths[u]
            assert plain.score[u] <= res.score[u]


@pytest.mark.parametrize("family,impl,rtol", [("diag", "hmmlearn", 1e-12), ("gmm", "gmmhmm", 1e-11),
                                              ("full", "hmmlearn", 1e-11)])
def test_decoder_align_with_optional_silence(tmp_path, family, impl, rtol):
    """``Decoder.align(optional_silence=)`` over pickled models against the restatement on the family's reference
    emission: the same segments by name, the silences among them, and the score within the family's bound of
    ``test_align_gpu.test_decoder_align``."""
    from sapr_amd.decoder import Decoder
    names = ["zero", "one", "two", "three"]
    model, utts, truth = pause_family_case(family)
    if family == "diag":
        models = _diag_decoder_case()[3]
    else:
        models = cases.models_of(family, model)
    recs, inserted, _ = oref.pause_case(family, model, utts, truth)
    dec = Decoder(models_dir=_pickle_models(tmp_path, impl, models, names), implementation=impl, n_iter=15)
    order = [names.index(w) for w in dec.vocab]                  # load order (glob) is the word order of the network
    rank = {w: k for k, w in enumerate(order)}
    sil = names[oref.PAUSE_WORD]
    said = [[names[w] for w in words] for words in truth]
    lengths = [len(x) for x in recs]
    offs = np.r_[0, np.cumsum(lengths)]
    logb = oref._emission(family, model, np.concatenate(recs))
    from sapr_amd.connected import with_optional
    slots, flags = with_optional([[rank[w] for w in words] for words in truth], rank[oref.PAUSE_WORD])
    woffs = np.r_[0, np.cumsum([len(t) for t in slots])]
    for pen in (0.0, -30.0):
        got = dec.align([x.T for x in recs], said, word_penalty=pen, optional_silence=sil)
        score, pw, ps, pe, start = oref.align_batch(logb[:, order], lengths, slots, flags, model["log_start"][order],
                                                    model["log_trans"][order], model["log_exit"][order], pen)
        assert np.isfinite(score).all()
        for u, row in enumerate(got):
            segs = oref.segments(slots[u], start[woffs[u]:woffs[u + 1]], lengths[u])
            assert row["words"] == said[u]
            assert row["segments"] == [(dec.vocab[w], a, b) for w, a, b in segs]
            assert len(row["segments"]) == len(said[u]) + len(inserted[u])
            assert sum(1 for w, _, _ in row["segments"] if w == sil) == len(inserted[u]) + said[u].count(sil)
            assert np.array_equal(row["state_sequence"], ps[offs[u]:offs[u + 1]])
            assert abs(row["log_likelihood"] - score[u]) / abs(score[u]) <= rtol
    with pytest.raises(ValueError, match="optional_silence names 'seven'"):
        dec.align([recs[0].T], [said[0]], optional_silence="seven")


# ---- training ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_case():
    """The recordings with pauses of the diagonal decoder case, its models perturbed, three iterations on the host."""
    from sapr_amd.connected import with_optional
    model, utts, truth = pause_family_case("diag")
    models = [copy.deepcopy(m) for m in _diag_decoder_case()[3]]
    rng = np.random.default_rng(9)
    for m in models:
        m.means_ = np.asarray(m.means_) + rng.normal(0.0, 1.5, np.shape(m.means_))
        m._covars_ = np.asarray(m._covars_) * 1.5
    recs, _, _ = oref.pause_case("diag", model, utts, truth)
    transcripts, optional = with_optional(truth, oref.PAUSE_WORD)
    ref_models, history = oref.fit(models, recs, transcripts, optional, n_iter=3, tol=0.0)
    return models, recs, truth, transcripts, optional, ref_models, history


def _rising(history):
    return all(b >= a - 1e-9 * abs(a) for a, b in zip(history, history[1:]))


def test_embedded_fit_with_optional_silence(fit_case):
    from sapr_amd.connected import embedded_fit
    models, recs, truth, transcripts, optional, ref_models, history = fit_case
    # (EM does not decrease the likelihood; once converged two entries agree to rounding, so "does not decrease" is
    # read at the 1e-9 relative bound the history itself is compared at)
    assert len(history) == 3 and history[-1] > history[0] and _rising(history)
    mine = [copy.deepcopy(m) for m in models]
    got = embedded_fit(mine, recs, transcripts, n_iter=3, tol=0.0, optional=optional)
    np.testing.assert_allclose(got, history, rtol=1e-9)
    assert _rising(got)
    for w in range(len(models)):
        _check_params(mine[w], ref_models[w], str(w))
        assert not np.array_equal(mine[w].means_, models[w].means_)


def test_decoder_train_embedded_with_optional_silence(tmp_path, fit_case):
    from sapr_amd.connected import with_optional
    from sapr_amd.decoder import Decoder
    names = ["zero", "one", "two", "three"]
    models, recs, truth, _, _, _, _ = fit_case
    dec = Decoder(models_dir=_pickle_models(tmp_path, "hmmlearn", models, names), implementation="hmmlearn", n_iter=15)
    order = [names.index(w) for w in dec.vocab]
    rank = {w: k for k, w in enumerate(order)}
    slots, flags = with_optional([[rank[w] for w in t] for t in truth], rank[oref.PAUSE_WORD])
    ref_models, history = oref.fit([models[w] for w in order], recs, slots, flags, n_iter=3, tol=0.0)
    said = [[names[w] for w in t] for t in truth]
    got = dec.train_embedded([x.T for x in recs], said, n_iter=3, tol=0.0, optional_silence=names[oref.PAUSE_WORD])
    np.testing.assert_allclose(got, history, rtol=1e-9)
    for k, word in enumerate(dec.vocab):
        _check_params(dec.models[word], ref_models[k], word)
    with pytest.raises(ValueError, match="optional_silence names 'seven'"):
        dec.train_embedded([recs[0].T], [said[0]], optional_silence="seven")

"""The restatement of online connected-word decoding (tests/_online_ref.py) against the offline restatement
(tests/_bigram_ref.py): the final answer equals offline, what was handed out is never revised, and the stable frame is
what an independent walk of every live state's back-trace finds.  The conditions on the shared inputs
(tests/_online_cases.py) are asserted here from the restatement alone, so that no test passes by committing nothing."""
import numpy as np
import pytest

from tests import _bigram_ref as bref
from tests import _online_cases as cases
from tests import _online_ref as oref

BIG = 4096      # a window nothing here fills


def _offline(tabs, lm, logb):
    return bref.viterbi(logb, *tabs, *lm)


def _assert_offline(got, want, what):
    score, n_words, pw, ps, pe, forced, _ = got
    assert forced == 0, what
    assert np.float64(score).tobytes() == np.float64(want[0]).tobytes(), what
    assert n_words == want[1], what
    for a, b in zip((pw, ps, pe), want[2:5]):
        assert a.dtype == b.dtype and np.array_equal(a, b), what


def _chunkings(T, seed):
    rng = np.random.default_rng(seed)
    return {"each": [1] * T, "seven": cases.fixed_chunks(T, 7), "ragged": cases.ragged_chunks(rng, T, 9)}


# ---- (a) equals offline ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exits", ["last", "any"])
@pytest.mark.parametrize("topology", ["bidiag", "dense"])
@pytest.mark.parametrize("W,S", [(3, 4), (5, 7), (11, 10)])
def test_equals_offline_on_random_logb(W, S, topology, exits):
    tabs, lm, logb = cases.random_case(W, S, topology, exits, 60)
    want = _offline(tabs, lm, logb)
    assert np.isfinite(want[0])
    for name, chunks in _chunkings(60, W + S).items():
        got = oref.decode(logb, chunks, *tabs, *lm, window=BIG, max_chunk=9)
        _assert_offline(got, want, (W, S, topology, exits, name))


@pytest.mark.parametrize("k", range(4))
def test_equals_offline_on_the_emitted_cases_and_commits_early(k):
    """Chunks of 7 frames under the word loop: offline's answer, and at least half of each of the two longest
    utterances' frames are final before the flush."""
    tabs, lm, logbs, _, _ = cases.e2e_case(k)
    longest = cases.two_longest(logbs)
    for u in sorted(set(longest) | {0, 1}):
        T = len(logbs[u])
        got = oref.decode(logbs[u], cases.fixed_chunks(T, 7), *tabs, *lm, window=BIG, max_chunk=7)
        _assert_offline(got, _offline(tabs, lm, logbs[u]), (k, u))
        before_flush = got[6][-1].first_frame
        latency = max(c.frames - c.stable_frames for c in got[6][:-1])
        print(f"case {k} utterance {u}: {before_flush}/{T} frames final before the flush, latency <= {latency}")
        if u in longest:
            assert 2 * before_flush >= T, (k, u, before_flush, T)


@pytest.mark.parametrize("W,S", [(11, 10), (25, 10)])
def test_dense_any_random_logb_settles_within_seven_frames(W, S):
    tabs, lm, logb = cases.random_case(W, S, "dense", "any", 65)
    got = oref.decode(logb, [1] * 65, *tabs, *lm, window=BIG, max_chunk=1)
    latency = max(c.frames - c.stable_frames for c in got[6][:-1])
    print(f"({W}, {S}) dense / any: latency <= {latency}")
    assert latency <= 7
    _assert_offline(got, _offline(tabs, lm, logb), (W, S))


# ---- (b) never revised -------------------------------------------------------------------------------------------
def _prefix_rows(tabs, lm, logb, n_prefix, chunk):
    ses = oref.Session(*tabs, *lm, 1, BIG, chunk)
    rows = [ses.push([logb[a:a + n]])[0] for a, n in zip(range(0, n_prefix, chunk), cases.fixed_chunks(n_prefix, chunk))]
    return [np.concatenate([getattr(c, f) for c in rows]) for f in ("path_word", "path_state", "path_entry")]


def test_committed_rows_are_never_revised_random():
    tabs, lm, logb = cases.random_case(11, 10, "dense", "any", 40)
    rows = _prefix_rows(tabs, lm, logb, 40, 5)
    assert len(rows[0]) >= 20
    for seed in range(5):
        tail = np.random.default_rng(900 + seed).normal(-40.0, 15.0, (25, 11, 10))
        want = _offline(tabs, lm, np.concatenate([logb, tail]))
        assert np.isfinite(want[0])
        for got, full in zip(rows, want[2:5]):
            assert np.array_equal(got, full[:len(got)]), seed


def test_committed_rows_are_never_revised_emitted():
    tabs, lm, logbs, _, _ = cases.e2e_case(3)
    u = cases.two_longest(logbs)[0]
    rows = _prefix_rows(tabs, lm, logbs[u], len(logbs[u]), 7)
    assert 2 * len(rows[0]) >= len(logbs[u])
    others = [v for v in range(len(logbs)) if v != u][:5]
    for v in others:                       # another utterance's frames follow without a pause
        want = _offline(tabs, lm, np.concatenate([logbs[u], logbs[v]]))
        assert np.isfinite(want[0])
        for got, full in zip(rows, want[2:5]):
            assert np.array_equal(got, full[:len(got)]), v


# ---- (c) the stable frame by brute force -------------------------------------------------------------------------
def _brute_stable(st):
    """Walk every live state's back-trace on its own, down to the oldest pending frame, then compare per frame."""
    _, back, xarg, warg, _ = st.lat
    t, c = st.frames - 1, st.committed
    live = np.argwhere(np.isfinite(st.lat[0][t]))
    if len(live) == 0 or c > t:
        return None
    traces = []
    for w, s in live.tolist():
        trace = {t: (w, s)}
        for tau in range(t, c, -1):
            b = back[tau, w, s]
            if b == oref.ENTRY:
                w = int(warg[tau - 1, w])
                s = int(xarg[tau - 1, w])
            else:
                s = int(b)
            trace[tau - 1] = (w, s)
        traces.append(trace)
    for tau in range(t, c - 1, -1):
        if len({tr[tau] for tr in traces}) == 1:
            return (tau,) + traces[0][tau]
    return None


@pytest.mark.parametrize("W,S,topology,exits", [(3, 4, "bidiag", "last"), (5, 7, "dense", "any"),
                                                (11, 10, "dense", "last"), (11, 10, "bidiag", "any")])
def test_stable_frame_equals_brute_force(W, S, topology, exits):
    tabs, lm, logb = cases.random_case(W, S, topology, exits, 40)
    ses = oref.Session(*tabs, *lm, 1, BIG, 3)
    st, found = ses.streams[0], 0
    for a in range(0, 40, 3):
        st.step(logb[a:a + 3])
        want = _brute_stable(st)
        assert st.stable() == want, a
        found += want is not None
        st.commit()
    assert found or (topology, exits) == ("bidiag", "last")


# ---- the forced rule ---------------------------------------------------------------------------------------------
def test_forcing_case_never_settles_and_a_small_window_forces():
    tabs, lm, logb = cases.forcing_case()
    want = _offline(tabs, lm, logb)
    assert np.isfinite(want[0])
    free = oref.decode(logb, cases.fixed_chunks(150, 7), *tabs, *lm, window=BIG, max_chunk=7)
    assert all(c.stable_frames == 0 for c in free[6][:-1])      # nothing becomes stable within 150 frames
    _assert_offline(free, want, "free")
    for window in (16, 64):
        got = oref.decode(logb, cases.fixed_chunks(150, 7), *tabs, *lm, window=window, max_chunk=7)
        assert got[5] > 0 and len(got[2]) == 150
        assert np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes()    # the score is never touched
        assert all(c.frames - c.stable_frames <= window - 7 for c in got[6][:-1])
        assert got[5] == sum(c.n_new for c in got[6][:-1])


def test_the_emitted_case_does_not_force_at_window_64():
    tabs, lm, logbs, _, _ = cases.e2e_case(2)       # (11, 18)
    for u in cases.two_longest(logbs):
        T = len(logbs[u])
        got = oref.decode(logbs[u], cases.fixed_chunks(T, 7), *tabs, *lm, window=64, max_chunk=7)
        assert max(c.frames - c.stable_frames for c in got[6][:-1]) <= 57
        _assert_offline(got, _offline(tabs, lm, logbs[u]), u)


# ---- edges -------------------------------------------------------------------------------------------------------
def test_tie_case_after_every_frame():
    logb, ls, lt, lx, lm, lm0, lm1, expected = bref.tie_case()
    got = oref.decode(logb, [1] * 4, ls, lt, lx, lm, lm0, lm1, window=8, max_chunk=1)
    assert got[0] == expected[0] and got[1] == expected[1] and got[5] == 0
    for a, b in zip(got[2:5], expected[2:5]):
        assert np.array_equal(a, b)


def test_flush_without_a_finite_score_keeps_what_was_handed_out():
    """A grammar whose ``lm_end`` allows only the dead word: every flush scores -inf."""
    tabs, lm, logb = cases.random_case(11, 10, "dense", "any", 30)
    end = np.full(11, -np.inf)
    end[11 // 2] = 0.0
    lm = (lm[0], lm[1], end)
    assert _offline(tabs, lm, logb)[0] == -np.inf
    got = oref.decode(logb, [5] * 6, *tabs, *lm, window=BIG, max_chunk=5)
    assert got[0] == -np.inf and got[1] == 0 and got[6][-1].n_new == 0
    assert 0 < len(got[2]) < 30 and (got[2] >= 0).all()
    # ... and they are the rows of the same frames under a grammar that lets the recording end
    free = _offline(tabs, (lm[0], lm[1], np.zeros(11)), logb)
    assert np.array_equal(got[2], free[2][:len(got[2])])


def test_a_stream_without_frames_and_zero_length_chunks():
    tabs, lm, logb = cases.random_case(5, 7, "dense", "any", 20)
    ses = oref.Session(*tabs, *lm, 2, 32, 8)
    empty = logb[:0]
    ups = ses.push([empty, None])
    assert [c.n_new for c in ups] == [0, 0] and [c.frames for c in ups] == [0, 0]
    rows = []
    for a in range(0, 20, 4):
        rows.append(ses.push([logb[a:a + 4], empty])[0])
        again = ses.push([empty, empty])[0]         # a commit without new frames hands out nothing
        assert again.n_new == 0 and again.stable_frames == rows[-1].stable_frames
    a, b = ses.finish()
    assert b.score == -np.inf and b.n_words == 0 and b.n_new == 0
    want = _offline(tabs, lm, logb)
    assert a.score == want[0] and a.n_words == want[1]
    assert np.array_equal(np.concatenate([c.path_word for c in rows + [a]]), want[2])
    assert ses.streams[0].frames == 0               # fresh again
    with pytest.raises(ValueError):
        ses.push([logb[:9], None])

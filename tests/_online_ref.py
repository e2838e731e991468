"""CPU restatement of online connected-word decoding (plain numpy, float64): THE DEFINITION of what
``sapr_connected_online_step`` and ``sapr_connected_online_commit`` compute (include/sapr_hip.h).  A recording arrives
in chunks; the trellis of ``tests/_bigram_ref.py`` is carried from chunk to chunk and the path is handed out as soon as
it can no longer change (partial traceback).

The recursion is not restated here: a stream keeps the ``logb`` rows it has consumed and a step IS
``_bigram_ref.viterbi(prefix, ..., want_lattice=True)`` — so ``delta``, ``X``, ``N`` and the rows ``back`` / ``xarg`` /
``warg`` after a step are, by construction, the values the offline recursion has at those frames (the device carries
``delta``, ``X`` and ``N`` instead and continues from them; the frame that takes the ``lm_start + log_start`` branch is
the stream's absolute frame 0).  What this file defines is what happens to the stored rows:

* ``stable(t, c)`` — the largest frame tau in [c, t] at which the back-traces of all live states (finite ``delta_t``)
  pass through one state; walking a back-trace uses the offline walk's rule (at an entry go to ``warg[tau - 1][w]``,
  then to ``xarg[tau - 1][that word]``);
* commit — after every step the rows c .. tau of the common back-trace become final and c <- tau + 1; if then
  ``frames - c > window - max_chunk`` the oldest ``k = frames - c - (window - max_chunk)`` pending frames are committed
  by force along the back-trace from the first maximum of ``delta_t`` over the live states in flat order (-1 / -1 / 0
  where nothing is live) and ``forced += k``; the score is never touched by that;
* flush — ``score = max_v (X(v) + lm_end[v])`` (the first maximum; -inf for a stream without frames); a finite score
  commits every pending row along the walk from ``(final word, xarg[t][final word])``; a score that is not finite
  commits nothing more and gives ``n_words = 0`` — the rows committed earlier stand, which is the one difference from
  offline (-1 rows for the whole utterance).  The stream is then fresh;
* hypothesis — the rows a flush would write now over the pending frames, empty where the score is not finite.
"""
import numpy as np

from . import _bigram_ref as bref

ENTRY = bref.ENTRY


class Commit:
    """What one commit (or flush) of one stream hands out: ``n_new`` rows from absolute frame ``first_frame`` on."""

    def __init__(self, first_frame, rows, frames, committed, forced):
        self.first_frame = int(first_frame)
        self.path_word = np.asarray([r[0] for r in rows], np.int32)
        self.path_state = np.asarray([r[1] for r in rows], np.int32)
        self.path_entry = np.asarray([r[2] for r in rows], np.uint8)
        self.n_new = len(rows)
        self.frames, self.stable_frames, self.forced = int(frames), int(committed), int(forced)
        self.score = self.n_words = None        # a flush fills these
        self.hyp = None                         # (path_word, path_state, path_entry) over the pending frames


class Stream:
    def __init__(self, session):
        self.net = session
        self.fresh()

    def fresh(self):
        W, S = self.net.W, self.net.S
        self.logb = np.zeros((0, W, S))
        self.frames = self.committed = self.forced = self.entries = 0
        self.lat = None                         # (deltas, back, xarg, warg, final) over [0, frames)
        self.score = float("-inf")

    # ---- the carried state, as the offline recursion has it at frame ``frames - 1`` --------------------------
    @property
    def delta(self):
        return self.lat[0][self.frames - 1]

    @property
    def X(self):
        t, words = self.frames - 1, np.arange(self.net.W)
        return self.delta[words, self.lat[2][t]] + self.net.tabs[2][words, self.lat[2][t]]

    @property
    def N(self):
        t, words = self.frames - 1, np.arange(self.net.W)
        with np.errstate(invalid="ignore"):
            return self.X[self.lat[3][t]] + self.net.lm[0][self.lat[3][t], words]

    def step(self, chunk):
        chunk = np.asarray(chunk, np.float64).reshape(-1, self.net.W, self.net.S)
        if len(chunk) > self.net.max_chunk:
            raise ValueError("chunk longer than max_chunk")
        if len(chunk) == 0:
            return
        self.logb = np.concatenate([self.logb, chunk])
        out = bref.viterbi(self.logb, *self.net.tabs, *self.net.lm, want_lattice=True)
        self.score, self.lat = out[0], out[5]
        self.frames = len(self.logb)

    # ---- walking the stored rows ---------------------------------------------------------------------------
    def live(self):
        """The live flat states ``(w, s)`` at the last frame, in flat order."""
        if self.frames == 0:
            return []
        return [(int(w), int(s)) for w, s in zip(*np.nonzero(np.isfinite(self.delta)))]

    def back_step(self, w, s, tau):
        """From ``(w, s)`` at frame ``tau > 0`` to the state at ``tau - 1``."""
        _, back, xarg, warg, _ = self.lat
        b = int(back[tau, w, s])
        if b == ENTRY:
            w = int(warg[tau - 1, w])
            return w, int(xarg[tau - 1, w])
        return w, b

    def rows(self, w, s, lo, hi):
        """The walk from ``(w, s)`` at frame ``frames - 1`` down to ``lo``: its rows ``(word, state, entry)`` at the
        frames ``lo .. hi - 1``, oldest first."""
        back = self.lat[1]
        out = []
        for tau in range(self.frames - 1, lo - 1, -1):
            if tau < hi:
                out.append((w, s, int(tau == 0 or back[tau, w, s] == ENTRY)))
            if tau > lo:
                w, s = self.back_step(w, s, tau)
        return out[::-1]

    def stable(self):
        """``(tau, w, s)``: the largest frame in [committed, frames - 1] at which every live state's back-trace holds
        the same state, and that state; ``None`` without one."""
        cur = set(self.live())      # (the distinct states the back-traces hold: traces that met stay together)
        if not cur:
            return None
        for tau in range(self.frames - 1, self.committed - 1, -1):
            if len(cur) == 1:
                return (tau,) + next(iter(cur))
            if tau > self.committed:
                cur = {self.back_step(w, s, tau) for w, s in cur}
        return None

    def best_live(self):
        """The first maximum of ``delta`` over the live states in flat order; ``None`` where nothing is live."""
        live = self.live()
        if not live:
            return None
        vals = [self.delta[w, s] for w, s in live]
        return live[int(np.argmax(vals))]

    def flush_rows(self):
        """The rows a flush would write now over the pending frames (``[]`` where the score is not finite)."""
        if self.frames == 0 or not np.isfinite(self.score):
            return []
        final = self.lat[4]
        return self.rows(final, int(self.lat[2][self.frames - 1, final]), self.committed, self.frames)

    def commit(self, want_hyp=False):
        c0, rows = self.committed, []
        st = self.stable()
        if st is not None:
            tau, w, s = st
            # the common back-trace: the walk from any live state passes through (w, s) at tau
            live = self.live()[0]
            rows = self.rows(live[0], live[1], c0, tau + 1)
            assert rows[-1][:2] == (w, s)
            self.committed = tau + 1
        over = self.frames - self.committed - (self.net.window - self.net.max_chunk)
        if over > 0:
            best = self.best_live()
            if best is None:
                rows += [(-1, -1, 0)] * over
            else:
                rows += self.rows(best[0], best[1], self.committed, self.committed + over)
            self.committed += over
            self.forced += over
        self.entries += sum(r[2] for r in rows)
        out = Commit(c0, rows, self.frames, self.committed, self.forced)
        if want_hyp:
            h = self.flush_rows()
            out.hyp = (np.asarray([r[0] for r in h], np.int32), np.asarray([r[1] for r in h], np.int32),
                       np.asarray([r[2] for r in h], np.uint8))
        return out

    def flush(self):
        c0 = self.committed
        rows = self.flush_rows()
        finite = self.frames > 0 and bool(np.isfinite(self.score))
        out = Commit(c0, rows, self.frames, c0 + len(rows), self.forced)
        out.score = float(self.score) if self.frames > 0 else float("-inf")
        out.n_words = self.entries + sum(r[2] for r in rows) if finite else 0
        self.fresh()
        return out


class Session:
    """B streams over one network: ``tabs = (log_start, log_trans, log_exit)``, ``lm = (lm, lm_start, lm_end)``."""

    def __init__(self, log_start, log_trans, log_exit, lm, lm_start, lm_end, n_streams, window=256, max_chunk=64):
        if not 1 <= max_chunk < window:
            raise ValueError("1 <= max_chunk < window")
        self.tabs = tuple(np.asarray(a, np.float64) for a in (log_start, log_trans, log_exit))
        self.lm = tuple(np.asarray(a, np.float64) for a in (lm, lm_start, lm_end))
        self.W, self.S = self.tabs[0].shape
        self.window, self.max_chunk = int(window), int(max_chunk)
        self.streams = [Stream(self) for _ in range(n_streams)]

    def push(self, chunks, want_hyp=False):
        """``chunks``: one ``logb[t, W, S]`` (or ``None``) per stream -> one :class:`Commit` per stream."""
        out = []
        for st, chunk in zip(self.streams, chunks):
            if chunk is not None:
                st.step(chunk)
            out.append(st.commit(want_hyp))
        return out

    def finish(self, streams=None):
        return [self.streams[u].flush() for u in (range(len(self.streams)) if streams is None else streams)]


def decode(logb, chunk_lengths, log_start, log_trans, log_exit, lm, lm_start, lm_end, window=256, max_chunk=64):
    """One utterance pushed in chunks of ``chunk_lengths`` (which sum to its frames) and flushed:
    ``(score, n_words, path_word, path_state, path_entry, forced, commits)`` — the rows are the concatenation of
    everything handed out, ``commits`` the list of :class:`Commit` (the last one is the flush)."""
    ses = Session(log_start, log_trans, log_exit, lm, lm_start, lm_end, 1, window, max_chunk)
    logb = np.asarray(logb, np.float64)
    commits, at = [], 0
    for n in chunk_lengths:
        commits.append(ses.push([logb[at:at + n]])[0])
        at += n
    assert at == len(logb)
    commits.append(ses.finish()[0])
    cat = lambda f, dt: np.concatenate([getattr(c, f) for c in commits]).astype(dt)  # noqa: E731
    fl = commits[-1]
    return (fl.score, fl.n_words, cat("path_word", np.int32), cat("path_state", np.int32),
            cat("path_entry", np.uint8), fl.forced, commits)

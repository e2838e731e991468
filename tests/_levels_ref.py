"""CPU restatement of connected-word recognition with a known or bounded number of words — level building over the
word loop (plain numpy, float64): THE DEFINITION of what ``sapr_connected_levels`` and
``sapr_connected_levels_backtrace`` compute (include/sapr_hip.h).  The conventions are those of
``tests/_bigram_ref.py``.

Levels are l = 0 .. L-1; level l holds the paths that are in their (l+1)-th word.  With ``b_t(w,s) = logb[t][w][s]``::

    delta_0(0,w,j) = (lm_start[w] + log_start[w][j]) + b_0(w,j)          delta_0(l>0,.,.) = -inf
    X_t(l,v)       = max_s (delta_t(l,v,s) + log_exit[v][s])             s ascending, the first maximum
    N_t(l,w)       = max_v (X_t(l-1,v) + lm[v][w])   for l >= 1          v ascending, the first maximum;  N_t(0,w) = -inf
    within         = max_i (delta_{t-1}(l,w,i) + log_trans[w][i][j])     i ascending, the first maximum
    entry          = N_{t-1}(l,w) + log_start[w][j]
    delta_t(l,w,j) = max(within, entry) + b_t(w,j)                       entry only where strictly greater
    level_score[k-1] = max_v (X_{T-1}(k-1,v) + lm_end[v])   k = 1..L     v ascending, the first maximum

The additions are made in exactly the order written, ``b_t`` last: float64 adds and compares only.  An utterance
without frames scores -inf on every level.

Count selection for a range lo <= k <= hi: lo > hi selects nothing; otherwise both are clamped into 1 .. L, the
selection starts from k = lo and takes a later k only where its score is strictly greater — on a tie the fewest words
win.  The back-trace for count k starts in level k-1 from the word that attained ``level_score[k-1]``, in the state
that attained its X; where ``entry`` won at frame t it steps to level l-1, to the word that attained ``N_{t-1}(l,.)``,
in the state that attained that word's ``X_{t-1}(l-1,.)``; it arrives at level 0 at frame 0.  Where the selected score
is not finite the path rows are -1, the entry flags 0 and ``n_words`` 0; otherwise ``n_words`` = k.

Three identities follow from the monotone rounding of add and max.  Loop: where ``_bigram_ref.viterbi`` on the same
``logb`` and tables decodes n <= L words, ``level_score[n-1]`` is its score bit for bit and no level scores higher.
L = 1: ``level_score[0]`` is the bigram score with every pair forbidden.  Chain: under ``_bigram_ref.chain_lm`` of a
transcript of K distinct words, ``level_score[K-1]`` and its path are ``_align_ref.align``'s outputs and every other
level is -inf.
"""
import numpy as np

from . import _bigram_ref as bref

ENTRY = 255


def levels(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, L):
    """One utterance: ``logb[T, W, S]`` -> ``(level_score[L], lattice)`` with ``lattice = (back[T, L, W, S],
    xarg[T, L, W], warg[T, L, W], final[L])``; ``warg[t, l]`` is the word that attained ``N_t(l, .)``."""
    logb = np.asarray(logb, dtype=np.float64)
    ls = np.asarray(log_start, dtype=np.float64)
    lt = np.asarray(log_trans, dtype=np.float64)
    lx = np.asarray(log_exit, dtype=np.float64)
    lm = np.asarray(lm, dtype=np.float64)
    lm0 = np.asarray(lm_start, dtype=np.float64)
    lm1 = np.asarray(lm_end, dtype=np.float64)
    W, S = ls.shape
    L = int(L)
    if L < 1:
        raise ValueError("L must be >= 1")
    if lm.shape != (W, W) or lm0.shape != (W,) or lm1.shape != (W,):
        raise ValueError("lm must be [W, W], lm_start and lm_end [W]")
    T = logb.shape[0]
    back = np.zeros((T, L, W, S), np.int64)
    xarg = np.zeros((T, L, W), np.int64)
    warg = np.zeros((T, L, W), np.int64)
    final = np.zeros(L, np.int64)
    score = np.full(L, -np.inf)
    words = np.arange(W)
    delta = np.full((L, W, S), -np.inf)
    X = np.full((L, W), -np.inf)
    N = np.full((L, W), -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            if t == 0:
                delta[0] = (lm0[:, None] + ls) + logb[0]
                back[0] = ENTRY
            else:
                for l in range(L):
                    cand = delta[l][:, :, None] + lt             # [w][i][j]
                    arg = cand.argmax(axis=1)                    # first maximum: the lowest i
                    within = np.take_along_axis(cand, arg[:, None, :], axis=1)[:, 0, :]
                    entry = N[l][:, None] + ls
                    take = entry > within
                    delta[l] = np.where(take, entry, within) + logb[t]
                    back[t, l] = np.where(take, ENTRY, arg)
            for l in range(L):
                e = delta[l] + lx
                xarg[t, l] = e.argmax(axis=1)                    # the lowest state among equals
                X[l] = e[words, xarg[t, l]]
            for l in range(1, L):
                n = X[l - 1][:, None] + lm                       # [v][w]
                warg[t, l] = n.argmax(axis=0)                    # the lowest predecessor word among equals
                N[l] = n[warg[t, l], words]
        if T > 0:
            for l in range(L):
                f = X[l] + lm1
                final[l] = int(np.argmax(f))
                score[l] = f[final[l]]
    return score, (back, xarg, warg, final)


def select(level_score, lo=None, hi=None):
    """The count the range selects, 0 for an empty range: from k = lo a later k only where strictly greater."""
    L = len(level_score)
    lo = 1 if lo is None else int(lo)
    hi = L if hi is None else int(hi)
    if lo > hi:
        return 0
    lo, hi = min(max(lo, 1), L), min(max(hi, 1), L)
    k = lo
    for c in range(lo + 1, hi + 1):
        if level_score[c - 1] > level_score[k - 1]:
            k = c
    return k


def backtrace(T, level_score, lattice, lo=None, hi=None):
    """``(score, n_words, path_word[T], path_state[T], path_entry[T])`` of the count the range selects."""
    back, xarg, warg, final = lattice
    pw = np.full(T, -1, np.int32)
    ps = np.full(T, -1, np.int32)
    pe = np.zeros(T, np.uint8)
    k = select(level_score, lo, hi)
    score = float(level_score[k - 1]) if k > 0 and T > 0 else float("-inf")
    if not np.isfinite(score):
        return score, 0, pw, ps, pe
    l = k - 1
    w = int(final[l])
    s = int(xarg[T - 1, l, w])
    for t in range(T - 1, -1, -1):
        pw[t], ps[t] = w, s
        b = int(back[t, l, w, s])
        if t == 0 or b == ENTRY:
            pe[t] = 1
            if t > 0:
                w = int(warg[t - 1, l, w])
                l -= 1
                s = int(xarg[t - 1, l, w])
        else:
            s = b
    assert l == 0, "a finite path arrives at level 0 at frame 0"
    return score, k, pw, ps, pe


def decode(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, L, lo=None, hi=None):
    """One utterance: ``(level_score[L], (score, n_words, path_word, path_state, path_entry))``."""
    score, lattice = levels(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, L)
    return score, backtrace(np.asarray(logb).shape[0], score, lattice, lo, hi)


class Batch:
    """A packed batch ``logb[total_frames, W, S]`` run once: ``level_score[N, L]`` and, by :meth:`select`, the five
    outputs of a back-trace — ``lo`` / ``hi``: ``None``, an int or one per utterance."""

    def __init__(self, logb, lengths, log_start, log_trans, log_exit, lm, lm_start, lm_end, L):
        self.L = int(L)
        self.offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
        runs = [levels(logb[a:b], log_start, log_trans, log_exit, lm, lm_start, lm_end, L)
                for a, b in zip(self.offs[:-1], self.offs[1:])]
        self.lattices = [r[1] for r in runs]
        self.level_score = np.asarray([r[0] for r in runs], np.float64).reshape(len(runs), self.L)

    def select(self, lo=None, hi=None):
        n = len(self.lattices)
        per = lambda a: [a] * n if a is None or np.ndim(a) == 0 else list(a)  # noqa: E731
        res = [backtrace(int(self.offs[u + 1] - self.offs[u]), self.level_score[u], self.lattices[u], a, b)
               for u, (a, b) in enumerate(zip(per(lo), per(hi)))]
        cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.zeros(0, dt)  # noqa: E731
        return (np.asarray([r[0] for r in res], np.float64), np.asarray([r[1] for r in res], np.int32),
                cat(2, np.int32), cat(3, np.int32), cat(4, np.uint8))


segments = bref.segments


def enumerate_best(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, L):
    """The best score of every path of exactly k words, k = 1 .. L, by enumeration of every path through the loop
    (small W, S, T only).  A path's score is accumulated in the order the recursion adds, so the maximum over the
    paths is the recursion's value bit for bit (rounding is monotone)."""
    logb = np.asarray(logb, dtype=np.float64)
    T, W, S = logb.shape
    best = np.full(L, -np.inf)
    if T == 0:
        return best

    def walk(t, w, s, k, acc):
        if acc == -np.inf:
            return
        if t == T - 1:
            f = (acc + log_exit[w][s]) + lm_end[w]
            if f > best[k - 1]:
                best[k - 1] = f
            return
        for j in range(S):                                   # stay in the word
            walk(t + 1, w, j, k, (acc + log_trans[w][s][j]) + logb[t + 1][w][j])
        if k < L:                                            # leave it and enter a word
            x = acc + log_exit[w][s]
            for v in range(W):
                n = x + lm[w][v]
                for j in range(S):
                    walk(t + 1, v, j, k + 1, (n + log_start[v][j]) + logb[t + 1][v][j])

    for w in range(W):
        for s in range(S):
            walk(0, w, s, 1, (lm_start[w] + log_start[w][s]) + logb[0][w][s])
    return best


def tie_case():
    """``_bigram_ref.tie_case`` with word 2 allowed to follow itself at -2.0: every tie of that case and, on top, an
    exact tie BETWEEN COUNTS, which the fewer words win.  W = 3 words of S = 2 states, T = 4 frames, every ``logb``
    0.0; words 0 and 1 are the same model and may start, word 2 follows either at 0.0 and is the only word that may
    end.  A word is entered in state 0; 0 -> 0 costs -1.0, 0 -> 1 is free, state 1 cannot be held; leaving from state
    0 earns +1.0, from state 1 0.0 — so a word held for n frames earns 2 - n whichever state it leaves from.  By hand
    (d = delta, level first)::

        level 0   t = 0  d(0,w,0) = 0                        X_0(0,w) = 1 (state 0)        w = 0, 1; word 2 is dead
                  t = 1  d(0,w,0) = -1, d(0,w,1) = 0         X_1(0,w) = max(0, 0) = 0      state 0
                  t = 2  d(0,w,0) = -2, d(0,w,1) = -1        X_2(0,w) = -1                 state 0
        level 1   N_t(1,2) = X_t(0,0) + 0: 1, 0, -1          the WORD tie: word 0
                  t = 1  d(1,2,0) = 1 (entry)                X_1(1,2) = 2
                  t = 2  d(1,2,0): within 0, entry 0 -> within; d(1,2,1) = 1       X_2(1,2) = max(1, 1) = 1, state 0
                  t = 3  d(1,2,0): within -1, entry -1 -> within; d(1,2,1) = 0     X_3(1,2) = max(0, 0) = 0, state 0
                  level_score[1] = 0        path 0 2 2 2, entries 1 1 0 0          (``_bigram_ref.tie_case``'s)
        level 2   N_t(2,2) = X_t(1,2) - 2: N_1 = 0, N_2 = -1
                  t = 2  d(2,2,0) = 0 (entry)                X_2(2,2) = 1
                  t = 3  d(2,2,0): within -1, entry -1 -> within; d(2,2,1) = 0     X_3(2,2) = max(0, 0) = 0, state 0
                  level_score[2] = 0        path 0 2 2 2, entries 1 1 1 0
        level 3   N_2(3,2) = X_2(2,2) - 2 = -1
                  t = 3  d(3,2,0) = -1 (entry)               X_3(3,2) = 0
                  level_score[3] = 0        path 0 2 2 2, entries 1 1 1 1
        level 0 cannot end (only word 2 may): level_score[0] = -inf; a fifth word has no frame: level_score[4] = -inf

    Two, three and four words tie at 0.0: the selection over 1 .. L returns two.  Returns ``(logb, log_start,
    log_trans, log_exit, lm, lm_start, lm_end, L, level_score, expected)`` with ``expected[k] = (score, n_words,
    path_word, path_state, path_entry)`` for k = 1 .. 5 and ``expected[None]`` the default selection's."""
    logb, ls, lt, lx, lm, lm0, lm1, _ = bref.tie_case()
    lm = lm.copy()
    lm[2, 2] = -2.0
    NEG = -np.inf
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
    u8 = lambda *a: np.array(a, np.uint8)  # noqa: E731
    none = (NEG, 0, i32(-1, -1, -1, -1), i32(-1, -1, -1, -1), u8(0, 0, 0, 0))
    expected = {1: none, 5: none,
                2: (0.0, 2, i32(0, 2, 2, 2), i32(0, 0, 0, 0), u8(1, 1, 0, 0)),
                3: (0.0, 3, i32(0, 2, 2, 2), i32(0, 0, 0, 0), u8(1, 1, 1, 0)),
                4: (0.0, 4, i32(0, 2, 2, 2), i32(0, 0, 0, 0), u8(1, 1, 1, 1))}
    expected[None] = expected[2]
    return logb, ls, lt, lx, lm, lm0, lm1, 5, np.array([NEG, 0.0, 0.0, 0.0, NEG]), expected

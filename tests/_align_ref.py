"""CPU restatement of forced alignment (plain numpy, float64): THE DEFINITION of what ``sapr_connected_align``
computes (include/sapr_hip.h).  The conventions are those of ``tests/_connected_ref.py``.

Utterance u has frames ``0..T-1`` and a transcript ``w_0..w_{K-1}`` of vocabulary indices (the same word may follow
itself); its network is the left-to-right chain of these K words: word slot k is entered only from the exit of slot
k - 1 and the score is read only at the exit of the last slot.  With ``b_t(k,s) = logb[t][w_k][s]``::

    delta_0(0,j)   = log_start[w_0][j] + b_0(0,j)          delta_0(k>0,j) = -inf
    X_{t-1}(k)     = max_s (delta_{t-1}(k,s) + log_exit[w_k][s])            s ascending, the first maximum
    within         = max_i (delta_{t-1}(k,i) + log_trans[w_k][i][j])        i ascending, the first maximum
    entry (k >= 1) = (X_{t-1}(k-1) + word_penalty) + log_start[w_k][j]      (k = 0: -inf)
    delta_t(k,j)   = max(within, entry) + b_t(k,j)                          entry only where strictly greater
    score          = X_{T-1}(K-1)

The additions are made in exactly the order written, ``b_t`` last: float64 adds and compares only.  The back-trace
starts from the arg-max of the last slot's exit at ``T - 1``; where ``entry`` won it steps to slot k - 1 in the state
that attained ``X_{t-1}(k-1)``.  Without a path (``T == 0``, ``K == 0``, a score that is not finite) the score is -inf
(or the NaN that propagated), the path rows are -1, the entry flags 0 and ``word_start`` -1.  ``path_word`` holds
vocabulary indices, ``path_entry`` is 1 at frame 0 and wherever a word begins, ``word_start[k]`` is the frame (counted
from the utterance's start) at which transcript word k begins.
"""
import numpy as np

ENTRY = 255


def align(logb, words, log_start, log_trans, log_exit, word_penalty=0.0):
    """One utterance: ``logb[T, W, S]`` and its transcript -> ``(score, path_word[T], path_state[T], path_entry[T],
    word_start[K])``."""
    logb = np.asarray(logb, dtype=np.float64)
    words = [int(w) for w in words]
    pen = np.float64(word_penalty)
    T, K = logb.shape[0], len(words)
    pw = np.full(T, -1, np.int32)
    ps = np.full(T, -1, np.int32)
    pe = np.zeros(T, np.uint8)
    start = np.full(K, -1, np.int32)
    if T == 0 or K == 0:
        return float("-inf"), pw, ps, pe, start
    ls = np.asarray(log_start, dtype=np.float64)[words]      # [K][S]
    lt = np.asarray(log_trans, dtype=np.float64)[words]      # [K][S][S]
    lx = np.asarray(log_exit, dtype=np.float64)[words]
    S = ls.shape[1]
    back = np.zeros((T, K, S), np.int64)
    xarg = np.zeros((T, K), np.int64)
    X = np.full(K, -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            b = logb[t][words]                               # [K][S]
            if t == 0:
                delta = np.full((K, S), -np.inf)
                delta[0] = ls[0] + b[0]
                back[0] = ENTRY
            else:
                cand = delta[:, :, None] + lt                # [k][i][j]
                arg = cand.argmax(axis=1)                    # first maximum: the lowest i
                within = np.take_along_axis(cand, arg[:, None, :], axis=1)[:, 0, :]
                entry = np.full((K, S), -np.inf)
                entry[1:] = (X[:-1, None] + pen) + ls[1:]
                take = entry > within
                delta = np.where(take, entry, within) + b
                back[t] = np.where(take, ENTRY, arg)
            e = delta + lx
            xarg[t] = e.argmax(axis=1)                       # the lowest state among equals
            X = e[np.arange(K), xarg[t]]
    score = float(X[K - 1])
    if np.isfinite(score):
        k, s = K - 1, int(xarg[T - 1, K - 1])
        for t in range(T - 1, -1, -1):
            pw[t], ps[t] = words[k], s
            bk = int(back[t, k, s])
            if t == 0 or bk == ENTRY:
                pe[t] = 1
                start[k] = t
                if t > 0:
                    k -= 1
                    s = int(xarg[t - 1, k])
            else:
                s = bk
    return score, pw, ps, pe, start


def align_batch(logb, lengths, transcripts, log_start, log_trans, log_exit, word_penalty=0.0, max_words=None):
    """A packed batch ``logb[total_frames, W, S]``: ``(score[N], path_word, path_state, path_entry, word_start)`` with
    ``word_start`` packed like the transcripts.  ``max_words``: transcripts longer than this have no path (what a call
    sized for fewer words answers)."""
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    res = []
    for a, b, words in zip(offs[:-1], offs[1:], transcripts):
        if max_words is not None and len(words) > max_words:
            res.append((float("-inf"), np.full(b - a, -1, np.int32), np.full(b - a, -1, np.int32),
                        np.zeros(b - a, np.uint8), np.full(len(words), -1, np.int32)))
        else:
            res.append(align(logb[a:b], words, log_start, log_trans, log_exit, word_penalty))
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.zeros(0, dt)  # noqa: E731
    return (np.asarray([r[0] for r in res], np.float64), cat(1, np.int32), cat(2, np.int32), cat(3, np.uint8),
            cat(4, np.int32))


def segments(words, word_start, T):
    """``[(word, start, end_exclusive), ...]`` of one utterance: K entries, or ``[]`` where there is no path."""
    if len(words) == 0 or word_start[0] < 0:
        return []
    starts = [int(a) for a in word_start]
    return [(int(w), a, b) for w, a, b in zip(words, starts, starts[1:] + [int(T)])]


def brute(logb, words, ls, lt, lx, pen):
    """The best total over EVERY path of the chain by depth-first enumeration (tiny cases only)."""
    T, K, S = logb.shape[0], len(words), ls.shape[1]
    best = [-np.inf]

    def walk(t, k, s, acc):
        if acc == -np.inf:
            return
        w = words[k]
        if t == T - 1:
            if k == K - 1:
                best[0] = max(best[0], acc + lx[w, s])
            return
        for s2 in range(S):
            walk(t + 1, k, s2, (acc + lt[w, s, s2]) + logb[t + 1, w, s2])
            if k + 1 < K:
                w2 = words[k + 1]
                walk(t + 1, k + 1, s2, (((acc + lx[w, s]) + pen) + ls[w2, s2]) + logb[t + 1, w2, s2])

    for s in range(S):
        walk(0, 0, s, ls[words[0], s] + logb[0, words[0], s])
    return best[0]


# ---- the recursion test's generator (tests/test_align_gpu.py; tests/test_align_cpu.py checks its condition) --------
# (W, S, max_words); RL follows max_words * SP.  The second row: (RL, SP) = (1, 4), (2, 4), (2, 10), (1, 18) — with the
# first row's (4, 4), (1, 10), (2, 18), (4, 18), (4, 10), all nine
RECURSION_SHAPES = [(3, 4, 64), (11, 10, 5), (11, 18, 5), (14, 18, 14), (5, 7, 25), (2, 1, 64),
                    (3, 4, 10), (3, 4, 20), (4, 10, 9), (3, 12, 3)]
RECURSION_LENGTHS = [3, 64, 1, 300, 0, 65, 2, 63, 40, 129]
TOPOLOGIES = ("bidiag", "skip", "dense")
EXITS = ("last", "any")
PENALTIES = (0.0, -20.0, 3.0)


def network(rng, W, S, topology, exits, integer):
    """The tables of ``tests/test_connected_gpu.py::_network`` with one change: in the integer tables -inf is sprinkled
    only on transitions other than i -> i and i -> i + 1, so that a bidiagonal word keeps a way to its last state."""
    width = {"bidiag": 1, "skip": 2, "dense": S}[topology]
    lt = np.full((W, S, S), -np.inf)
    ls = np.full((W, S), -np.inf)
    for i in range(S):
        lo = 0 if topology == "dense" else i
        for j in range(lo, min(S, i + width + 1)):
            lt[:, i, j] = -rng.integers(0, 2, W) if integer else np.log(rng.uniform(0.05, 1.0, W))
            if integer and j != i and j != i + 1:
                lt[rng.random(W) < 0.2, i, j] = -np.inf
    n_start = S if topology == "dense" else min(S, 2)
    ls[:, :n_start] = -rng.integers(0, 2, (W, n_start)) if integer else np.log(rng.uniform(0.05, 1.0, (W, n_start)))
    lx = np.full((W, S), -np.inf)
    if exits == "last":
        lx[:, S - 1] = 0.0
    else:
        lx[:] = 0.0
    return ls, lt, lx


def recursion_transcripts(rng, W, S, max_words):
    """Transcript length ``min(max_words, max(1, T // (S + 1)))``; three deliberately pathless utterances: K = T + 1
    at the 1- and 2-frame utterances, and the empty utterance."""
    out = []
    for T in RECURSION_LENGTHS:
        K = T + 1 if T in (1, 2) else min(max_words, max(1, T // (S + 1)))
        out.append(rng.integers(0, W, K).tolist())
    return out


def recursion_case(W, S, max_words, topology, exits, integer):
    """``(ls, lt, lx, logb[total, W, S], transcripts)`` of one parametrised case (the same on the CPU and the GPU)."""
    rng = np.random.default_rng(1000 * W + 10 * S + TOPOLOGIES.index(topology) * 3 + EXITS.index(exits) + 7 * integer)
    ls, lt, lx = network(rng, W, S, topology, exits, integer)
    total = sum(RECURSION_LENGTHS)
    logb = (-rng.integers(0, 4, (total, W, S)).astype(np.float64) if integer
            else rng.normal(-40.0, 15.0, (total, W, S)))
    return ls, lt, lx, logb, recursion_transcripts(rng, W, S, max_words)

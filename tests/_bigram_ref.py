"""CPU restatement of connected-word recognition under a word-pair language model (plain numpy, float64): THE
DEFINITION of what ``sapr_connected_bigram`` computes (include/sapr_hip.h).  The conventions are those of
``tests/_connected_ref.py``.

W word models with S states each; ``lm[v][w]`` is added when word ``w`` follows word ``v`` (the same word may follow
itself), ``lm_start[w]`` when an utterance begins with ``w``, ``lm_end[v]`` when it ends with ``v``.  With
``b_t(w,s) = logb[t][w][s]``::

    delta_0(w,j)  = (lm_start[w] + log_start[w][j]) + b_0(w,j)
    X_{t-1}(v)    = max_s (delta_{t-1}(v,s) + log_exit[v][s])        s ascending, the first maximum
    N_{t-1}(w)    = max_v (X_{t-1}(v) + lm[v][w])                    v ascending, the first maximum
    within        = max_i (delta_{t-1}(w,i) + log_trans[w][i][j])    i ascending, the first maximum
    entry         = N_{t-1}(w) + log_start[w][j]
    delta_t(w,j)  = max(within, entry) + b_t(w,j)                    entry only where strictly greater
    score         = max_v (X_{T-1}(v) + lm_end[v])                   v ascending, the first maximum

The additions are made in exactly the order written, ``b_t`` last: float64 adds and compares only.  ``-inf`` in ``lm``,
``lm_start`` or ``lm_end`` forbids a pair, a first word or a last word: a finite-state word-pair grammar is a table of
0.0 and ``-inf``.  There is no separate ``word_penalty``; the host folds it into ``lm``.  The back-trace starts from
the word that attained the score, in the state that attained its ``X_{T-1}``; where ``entry`` won at frame t it steps
to the word that attained ``N_{t-1}`` in the state that attained that word's ``X_{t-1}``.  An utterance without frames
scores -inf; where the score is not finite the path rows are -1, the entry flags 0 and ``n_words`` 0.

Two identities follow.  Word loop: ``lm == p``, ``lm_start == 0``, ``lm_end == 0`` gives the score of
``_connected_ref.viterbi(..., word_penalty=p)`` bit for bit (rounding is monotone: ``max_v fl(X(v) + p) =
fl(max_v X(v) + p)``), and with ``p = 0.0`` every output.  Chain: ``lm = -inf`` except ``lm[w_k][w_{k+1}] = p`` along
a transcript of distinct words, ``lm_start = -inf`` except 0.0 at ``w_0``, ``lm_end = -inf`` except 0.0 at
``w_{K-1}`` gives every output of ``_align_ref.align(..., word_penalty=p)``.
"""
import numpy as np

from . import _connected_ref as cref

ENTRY = 255


def viterbi(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, want_lattice=False):
    """One utterance: ``logb[T, W, S]`` -> ``(score, n_words, path_word[T], path_state[T], path_entry[T])``
    (+ ``(delta[T, W, S], back[T, W, S], xarg[T, W], warg[T, W], final_word)`` with ``want_lattice``; ``warg[t]`` is
    the word that attained ``N_t``)."""
    logb = np.asarray(logb, dtype=np.float64)
    ls = np.asarray(log_start, dtype=np.float64)
    lt = np.asarray(log_trans, dtype=np.float64)
    lx = np.asarray(log_exit, dtype=np.float64)
    lm = np.asarray(lm, dtype=np.float64)
    lm0 = np.asarray(lm_start, dtype=np.float64)
    lm1 = np.asarray(lm_end, dtype=np.float64)
    W, S = ls.shape
    if lm.shape != (W, W) or lm0.shape != (W,) or lm1.shape != (W,):
        raise ValueError("lm must be [W, W], lm_start and lm_end [W]")
    T = logb.shape[0]
    pw = np.full(T, -1, np.int32)
    ps = np.full(T, -1, np.int32)
    pe = np.zeros(T, np.uint8)
    deltas = np.full((T, W, S), -np.inf)
    back = np.zeros((T, W, S), np.int64)
    xarg = np.zeros((T, W), np.int64)
    warg = np.zeros((T, W), np.int64)
    words = np.arange(W)
    X = np.full(W, -np.inf)
    N = np.full(W, -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            if t == 0:
                delta = (lm0[:, None] + ls) + logb[0]
                back[0] = ENTRY
            else:
                cand = delta[:, :, None] + lt            # [w][i][j]
                arg = cand.argmax(axis=1)                # first maximum: the lowest i
                within = np.take_along_axis(cand, arg[:, None, :], axis=1)[:, 0, :]
                entry = N[:, None] + ls
                take = entry > within
                delta = np.where(take, entry, within) + logb[t]
                back[t] = np.where(take, ENTRY, arg)
            deltas[t] = delta
            e = delta + lx
            xarg[t] = e.argmax(axis=1)                   # the lowest state among equals
            X = e[words, xarg[t]]
            n = X[:, None] + lm                          # [v][w]
            warg[t] = n.argmax(axis=0)                   # the lowest predecessor word among equals
            N = n[warg[t], words]
        final = 0
        score = float("-inf")
        if T > 0:
            f = X + lm1
            final = int(np.argmax(f))
            score = float(f[final])
    n_words = 0
    if T > 0 and np.isfinite(score):
        w, s = final, int(xarg[T - 1, final])
        for t in range(T - 1, -1, -1):
            pw[t], ps[t] = w, s
            b = int(back[t, w, s])
            if t == 0 or b == ENTRY:
                pe[t] = 1
                n_words += 1
                if t > 0:
                    w = int(warg[t - 1, w])
                    s = int(xarg[t - 1, w])
            else:
                s = b
    out = (score, n_words, pw, ps, pe)
    return out + ((deltas, back, xarg, warg, final),) if want_lattice else out


def viterbi_batch(logb, lengths, log_start, log_trans, log_exit, lm, lm_start, lm_end):
    """A packed batch ``logb[total_frames, W, S]``: ``(score[N], n_words[N], path_word, path_state, path_entry)``."""
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    res = [viterbi(logb[a:b], log_start, log_trans, log_exit, lm, lm_start, lm_end)
           for a, b in zip(offs[:-1], offs[1:])]
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.zeros(0, dt)  # noqa: E731
    return (np.asarray([r[0] for r in res], np.float64), np.asarray([r[1] for r in res], np.int32),
            cat(2, np.int32), cat(3, np.int32), cat(4, np.uint8))


segments = cref.segments


def word_loop_lm(W, p=0.0):
    """The language model of the word-loop identity: ``lm == p``, ``lm_start == 0``, ``lm_end == 0``."""
    return np.full((W, W), np.float64(p)), np.zeros(W), np.zeros(W)


def chain_lm(W, words, p=0.0):
    """The language model of the chain identity over a transcript of DISTINCT words."""
    words = [int(w) for w in words]
    if len(set(words)) != len(words):
        raise ValueError("the chain identity needs distinct words")
    lm = np.full((W, W), -np.inf)
    for a, b in zip(words[:-1], words[1:]):
        lm[a, b] = np.float64(p)
    lm0 = np.full(W, -np.inf)
    lm1 = np.full(W, -np.inf)
    lm0[words[0]] = 0.0
    lm1[words[-1]] = 0.0
    return lm, lm0, lm1


def grammar_lm(W, pairs, starts=None, ends=None):
    """0.0 where allowed, -inf elsewhere (what ``WordBigram.from_grammar`` builds)."""
    lm = np.full((W, W), -np.inf)
    for a, b in pairs:
        lm[a, b] = 0.0
    lm0 = np.zeros(W) if starts is None else np.full(W, -np.inf)
    lm1 = np.zeros(W) if ends is None else np.full(W, -np.inf)
    if starts is not None:
        lm0[list(starts)] = 0.0
    if ends is not None:
        lm1[list(ends)] = 0.0
    return lm, lm0, lm1


def random_lm(rng, W, forbidden=1.0 / 3.0, dead_word=None):
    """Dense random ``(lm, lm_start, lm_end)`` of log-probability size with about ``forbidden`` of the pairs -inf;
    ``dead_word``: a word with an all -inf column and -inf in ``lm_start`` — nothing reaches it."""
    lm = np.log(rng.uniform(0.02, 1.0, (W, W)))
    lm[rng.random((W, W)) < forbidden] = -np.inf
    lm0 = np.log(rng.uniform(0.02, 1.0, W))
    lm1 = np.log(rng.uniform(0.02, 1.0, W))
    if dead_word is not None:
        lm[:, dead_word] = -np.inf
        lm0[dead_word] = -np.inf
    return lm, lm0, lm1


def tie_case():
    """Integer-valued tables in which two predecessor words, two exit states and ``within`` / ``entry`` tie exactly;
    the lowest index (and ``within``) wins.  W = 3 words of S = 2 states, T = 4 frames, every ``logb`` 0.0.  Words 0
    and 1 are the same model and may start an utterance; word 2 may follow either at 0.0 and is the only word that may
    end.  A word is entered in state 0; 0 -> 0 costs -1.0, 0 -> 1 is free, state 1 cannot be held; leaving from state 0
    earns +1.0, from state 1 0.0.  By hand (d = delta)::

        t = 0   d(0,0) = d(1,0) = 0            X(0) = X(1) = 0 + 1 = 1 (state 0)
                N(2) = max(1 + 0, 1 + 0, -inf) = 1                         the WORD tie: word 0
        t = 1   d(2,0) = 1 (entry), d(0,0) = -1, d(0,1) = 0
                X(0) = max(-1 + 1, 0 + 0) = 0, X(2) = 1 + 1 = 2, N(2) = 0
        t = 2   d(2,0): within 1 - 1 = 0, entry 0 + 0 = 0                  the WITHIN / ENTRY tie: within
                d(2,1) = 1 + 0 = 1          X(2) = max(0 + 1, 1 + 0) = 1, N(2) = X(0) = -1
        t = 3   d(2,0): within -1, entry -1 -> within; d(2,1) = 0 + 0 = 0
                X(2) = max(-1 + 1, 0 + 0) = 0                              the STATE tie: state 0
        score = X(2) + lm_end[2] = 0.0

    The walk: word 2 state 0 at t = 3, from state 0 at t = 2, from state 0 at t = 1, entered there from word 0, which
    left from state 0 at t = 0.  Returns ``(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, expected)``
    with ``expected = (score, n_words, path_word, path_state, path_entry)``."""
    W, S, T = 3, 2, 4
    logb = np.zeros((T, W, S))
    ls = np.full((W, S), -np.inf)
    ls[:, 0] = 0.0
    lt = np.full((W, S, S), -np.inf)
    lt[:, 0, 0] = -1.0
    lt[:, 0, 1] = 0.0
    lx = np.zeros((W, S))
    lx[:, 0] = 1.0
    lm = np.full((W, W), -np.inf)
    lm[0, 2] = lm[1, 2] = 0.0
    lm0 = np.array([0.0, 0.0, -np.inf])
    lm1 = np.array([-np.inf, -np.inf, 0.0])
    expected = (0.0, 2, np.array([0, 2, 2, 2], np.int32), np.array([0, 0, 0, 0], np.int32),
                np.array([1, 1, 0, 0], np.uint8))
    return logb, ls, lt, lx, lm, lm0, lm1, expected


def sample_bigram(rng, W, density=0.6):
    """A sampled word bigram as probabilities: ``(P[W, W + 1], start[W])`` — row v holds the successors of v and, last,
    the end of the string; about ``1 - density`` of the word pairs are impossible."""
    P = rng.uniform(0.1, 1.0, (W, W + 1)) * np.c_[rng.random((W, W)) < density, np.ones(W, bool)]
    P /= P.sum(axis=1, keepdims=True)
    start = rng.uniform(0.1, 1.0, W)
    return P, start / start.sum()


def sample_bigram_case(seed, W, S, D, n_utts, exit_states="last", spherical=False, bigram=None, max_words=5,
                       shared=()):
    """``_connected_ref.sample_case`` with the word strings drawn from a bigram: ``bigram = (P[W, W + 1], start[W])``
    in probabilities (``sample_bigram`` by default), strings of at most ``max_words`` words.  ``shared``: pairs
    ``(a, b)`` of words that share their Gaussians (b takes a's means and variances), so that the acoustics cannot
    tell them apart.  Returns ``(model, utterances, truth, (lm, lm_start, lm_end))`` with the log-probabilities the
    strings were drawn from."""
    model, _, _ = cref.sample_case(seed, W, S, D, 0, exit_states, spherical)
    rng = np.random.default_rng(seed + 7919)
    for a, b in shared:
        model["means"][b] = model["means"][a]
        model["vars"][b] = model["vars"][a]
        model["gconst"][b] = model["gconst"][a]
        model["transmat"][b] = model["transmat"][a]
        model["log_trans"][b] = model["log_trans"][a]
    P, start = sample_bigram(rng, W) if bigram is None else (np.asarray(bigram[0], float), np.asarray(bigram[1], float))
    utts, truth = [], []
    for _ in range(n_utts):
        words = [int(rng.choice(W, p=start))]
        while len(words) < max_words:
            nxt = int(rng.choice(W + 1, p=P[words[-1]]))
            if nxt == W:
                break
            words.append(nxt)
        rows = []
        for w in words:
            for s in range(S):
                n = int(rng.integers(1, 5))
                rows.append(rng.normal(model["means"][w, s], np.sqrt(model["vars"][w, s]), (n, D)))
        utts.append(np.concatenate(rows).astype(np.float32))
        truth.append(words)
    with np.errstate(divide="ignore"):
        lms = (np.log(P[:, :W]), np.log(start), np.log(P[:, W]))
    return model, utts, truth, lms


# the committed case of the end-to-end test (tests/test_bigram_gpu.py) and of the CPU test that guards it
# (tests/test_bigram_cpu.py): (seed, W, S, D, utterances).  Word 2 occurs only after word 0, word 3 only after word 1;
# words 2 and 3 share their Gaussians.
E2E_CASE = (211, 4, 5, 13, 12)
E2E_SHARED = ((2, 3),)
E2E_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 3), (2, 0), (2, 1), (3, 0), (3, 1))
E2E_STARTS = (0, 1)


def e2e_bigram():
    """The sampling distribution of the end-to-end case: uniform over the grammar's allowed successors and the end."""
    W = E2E_CASE[1]
    P = np.zeros((W, W + 1))
    for a, b in E2E_PAIRS:
        P[a, b] = 1.0
    P[:, W] = 1.0
    P /= P.sum(axis=1, keepdims=True)
    start = np.zeros(W)
    start[list(E2E_STARTS)] = 1.0 / len(E2E_STARTS)
    return P, start

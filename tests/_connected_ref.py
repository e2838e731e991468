"""CPU restatement of connected-word recognition (plain numpy, float64): THE DEFINITION of what
``sapr_connected_viterbi`` / ``sapr_connected_emit_diag`` compute (include/sapr_hip.h).

W word models with S states each (a padded state has -inf in log_start, log_exit and its rows and columns of
log_trans), ``log_exit[w][s] = -inf``: a word may not end in state s, one scalar ``word_penalty`` per word boundary.
With ``b_t(w,s) = logb[t][w][s]``::

    delta_0(w,j) = log_start[w][j] + b_0(w,j)
    E_{t-1}      = max over (w,s) in flat order of (delta_{t-1}(w,s) + log_exit[w][s])
    within       = max_i (delta_{t-1}(w,i) + log_trans[w][i][j])          i ascending
    entry        = (E_{t-1} + word_penalty) + log_start[w][j]
    delta_t(w,j) = max(within, entry) + b_t(w,j)
    score        = max over (w,s) of (delta_{T-1}(w,s) + log_exit[w][s])

The first maximum wins everywhere (``np.argmax``); ``entry`` wins only when strictly greater than ``within``; the
additions are made in exactly the order written, ``b_t`` last, so the recursion is float64 adds and compares only.  An
utterance without frames scores -inf; where the score is not finite the path rows are -1, the entry flags 0 and
``n_words`` 0.  ``path_entry`` is 1 at frame 0 and wherever ``entry`` won (the same word may follow itself).
"""
import numpy as np

ENTRY = 255


def viterbi(logb, log_start, log_trans, log_exit, word_penalty=0.0, want_lattice=False):
    """One utterance: ``logb[T, W, S]`` -> ``(score, n_words, path_word[T], path_state[T], path_entry[T])``
    (+ ``(delta[T, W, S], back[T, W, S], exit_idx[T])`` with ``want_lattice``)."""
    logb = np.asarray(logb, dtype=np.float64)
    ls = np.asarray(log_start, dtype=np.float64)
    lt = np.asarray(log_trans, dtype=np.float64)
    lx = np.asarray(log_exit, dtype=np.float64)
    pen = np.float64(word_penalty)
    W, S = ls.shape
    T = logb.shape[0]
    pw = np.full(T, -1, np.int32)
    ps = np.full(T, -1, np.int32)
    pe = np.zeros(T, np.uint8)
    deltas = np.full((T, W, S), -np.inf)
    back = np.zeros((T, W, S), np.int64)
    ex = np.zeros(T, np.int64)
    E = -np.inf
    with np.errstate(invalid="ignore"):
        for t in range(T):
            if t == 0:
                delta = ls + logb[0]
                back[0] = ENTRY
            else:
                cand = delta[:, :, None] + lt            # [w][i][j]
                arg = cand.argmax(axis=1)                # first maximum: the lowest i
                within = np.take_along_axis(cand, arg[:, None, :], axis=1)[:, 0, :]
                entry = (E + pen) + ls
                take = entry > within
                delta = np.where(take, entry, within) + logb[t]
                back[t] = np.where(take, ENTRY, arg)
            deltas[t] = delta
            e = (delta + lx).ravel()
            ex[t] = int(np.argmax(e))                    # the lowest flat index w * S + s
            E = e[ex[t]]
    score = float(E) if T > 0 else float("-inf")
    n_words = 0
    if T > 0 and np.isfinite(score):
        r = int(ex[T - 1])
        for t in range(T - 1, -1, -1):
            w, s = divmod(r, S)
            pw[t], ps[t] = w, s
            b = int(back[t, w, s])
            if t == 0 or b == ENTRY:
                pe[t] = 1
                n_words += 1
                if t > 0:
                    r = int(ex[t - 1])
            else:
                r = w * S + b
    out = (score, n_words, pw, ps, pe)
    return out + ((deltas, back, ex),) if want_lattice else out


def viterbi_batch(logb, lengths, log_start, log_trans, log_exit, word_penalty=0.0):
    """A packed batch ``logb[total_frames, W, S]``: ``(score[N], n_words[N], path_word, path_state, path_entry)``."""
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    res = [viterbi(logb[a:b], log_start, log_trans, log_exit, word_penalty) for a, b in zip(offs[:-1], offs[1:])]
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.zeros(0, dt)  # noqa: E731
    return (np.asarray([r[0] for r in res], np.float64), np.asarray([r[1] for r in res], np.int32),
            cat(2, np.int32), cat(3, np.int32), cat(4, np.uint8))


def segments(path_word, path_entry):
    """``[(word, start, end_exclusive), ...]`` of one utterance's path rows (cut at the entry flags)."""
    if len(path_word) == 0 or path_word[0] < 0:
        return []
    starts = np.flatnonzero(path_entry).tolist()
    return [(int(path_word[a]), a, b) for a, b in zip(starts, starts[1:] + [len(path_word)])]


def emit_diag(feats, means, vars_, gconst):
    """``logb[T, W, S] = -0.5 * (gconst + sum_d (x_d - mean_d)^2 / var_d)`` in float64 (features promoted exactly)."""
    x = np.asarray(feats, dtype=np.float64)[:, None, None, :]
    return -0.5 * (gconst[None] + ((x - means[None]) ** 2 / vars_[None]).sum(axis=-1))


def margins(logb, log_start, log_trans, log_exit, word_penalty=0.0):
    """The decisions along the optimal path — within versus entry (and among the within candidates), the arg-max of E
    where a word was entered, the final arg-max — each as ``winner - best other candidate``: 0.0 is an exact tie,
    +inf a decision without a finite rival.  ``[]`` where the score is not finite."""
    ls, lt, lx = (np.asarray(a, dtype=np.float64) for a in (log_start, log_trans, log_exit))
    score, _, pw, ps, pe, (deltas, _, ex) = viterbi(logb, ls, lt, lx, word_penalty, want_lattice=True)
    if not np.isfinite(score):
        return []
    T = len(pw)

    def gap(vals, k):
        rest = np.delete(np.asarray(vals, dtype=np.float64), k)
        rest = rest[~np.isnan(rest)]
        return float("inf") if rest.size == 0 or rest.max() == -np.inf else float(vals[k] - rest.max())

    with np.errstate(invalid="ignore"):
        out = [gap((deltas[T - 1] + lx).ravel(), int(ex[T - 1]))]
        for t in range(T - 1, 0, -1):
            w, j = int(pw[t]), int(ps[t])
            e = (deltas[t - 1] + lx).ravel()
            cands = list(deltas[t - 1, w, :] + lt[w, :, j]) + [(e[ex[t - 1]] + word_penalty) + ls[w, j]]
            if pe[t]:
                out.append(gap(cands, len(cands) - 1))
                out.append(gap(e, int(ex[t - 1])))
            else:
                out.append(gap(cands, int(ps[t - 1])))
    return out


def sample_case(seed, W, S, D, n_utts, exit_states="last", spherical=False):
    """Sampled concatenations: left-to-right word models with means N(0, 20^2) and variances U(4, 36); utterances of
    1-5 words, every state of a word held for 1-4 frames and drawn from its Gaussian (float32 features).  Returns
    ``(model, utterances, truth)``: ``model`` a dict of startprob[W,S], transmat[W,S,S], means, vars (float64) with
    log_start / log_trans / log_exit / gconst, ``utterances`` frame-major (T, D) float32 arrays, ``truth`` the
    sampled word strings.  ``spherical``: the odd words have one variance per state (a "spherical" model)."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, 20.0, (W, S, D))
    vars_ = rng.uniform(4.0, 36.0, (W, S, D))
    if spherical:
        vars_[1::2] = vars_[1::2, :, :1]
    stay = rng.uniform(0.3, 0.7, (W, S))
    transmat = np.zeros((W, S, S))
    for s in range(S):
        if s + 1 < S:
            transmat[:, s, s], transmat[:, s, s + 1] = stay[:, s], 1.0 - stay[:, s]
        else:
            transmat[:, s, s] = 1.0
    startprob = np.zeros((W, S))
    startprob[:, 0] = 1.0
    with np.errstate(divide="ignore"):
        log_start, log_trans = np.log(startprob), np.log(transmat)
    log_exit = np.full((W, S), -np.inf)
    if exit_states == "last":
        log_exit[:, S - 1] = 0.0
    else:
        log_exit[:] = 0.0
    gconst = D * np.log(2 * np.pi) + np.log(vars_).sum(axis=-1)
    utts, truth = [], []
    for _ in range(n_utts):
        words = rng.integers(0, W, int(rng.integers(1, 6))).tolist()
        rows = []
        for w in words:
            for s in range(S):
                n = int(rng.integers(1, 5))
                rows.append(rng.normal(means[w, s], np.sqrt(vars_[w, s]), (n, D)))
        utts.append(np.concatenate(rows).astype(np.float32))
        truth.append(words)
    model = dict(startprob=startprob, transmat=transmat, means=means, vars=vars_, gconst=gconst,
                 log_start=log_start, log_trans=log_trans, log_exit=log_exit)
    return model, utts, truth


# the committed cases of the end-to-end test (tests/test_connected_gpu.py) and of the margin test that guards it
# (tests/test_connected_cpu.py): (seed, W, S, D, utterances)
DECODER_CASE = (105, 4, 5, 13, 12)   # Decoder.decode_connected: diag and (odd words) spherical models
E2E_CASES = [(101, 11, 10, 13, 24), (102, 5, 7, 26, 16), (103, 11, 18, 39, 12), (104, 3, 4, 5, 16)]

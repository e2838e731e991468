"""CPU restatement of the connected-word N-best list — the ``n_best`` best DISTINCT word strings of an utterance with
their Viterbi scores, in one pass over the word loop (plain numpy, float64 / uint64): THE DEFINITION of what
``sapr_connected_nbest`` computes (include/sapr_hip.h).  The conventions are those of ``tests/_bigram_ref.py``:
``logb[T, W, S]``, ``log_start``, ``log_trans``, ``log_exit``, ``lm``, ``lm_start``, ``lm_end``.

A hypothesis is a pair ``(score: float64, code: uint64)``.  ``code`` is the word string so far, the current word
included: the string ``w_0 .. w_{k-1}`` has ``code = sum (w_i + 1) * B**(k-1-i)`` with ``B = W + 1``; appending ``w``
is ``code * B + (w + 1)``.  ``cap(W)`` is the largest K with ``B**K <= 2**64``: the longest string a code holds.

``merge_n(cands)`` is a function of the candidates' values alone:

    1. drop every candidate whose score is not ``> -inf`` (this drops ``-inf`` and NaN);
    2. among candidates with equal ``code`` keep the largest score;
    3. order by score descending, then ``code`` ascending;
    4. keep the first ``n = n_best``.

With ``b_t(w,j) = logb[t][w][j]``; every ``+`` applies to each hypothesis's score and leaves its code alone unless
said otherwise::

    cell_0(w,j) = merge_n{ ((lm_start[w] + log_start[w][j]), w + 1) }                       then + b_0(w,j)
    X_t(v)      = merge_n{ h + log_exit[v][s]        : s, h in cell_t(v,s) }
    N_t(w)      = merge_n{ (h + lm[v][w], code * B + (w+1)) : v, h in X_t(v), code < B**(cap-1) }      t < T-1
    cell_t(w,j) = merge_n( { h + log_trans[w][i][j] : i, h in cell_{t-1}(w,i) }
                           | { h + log_start[w][j]  : h in N_{t-1}(w) } )                   then + b_t(w,j)
    result      = merge_n{ h + lm_end[v]             : v, h in X_{T-1}(v) }

A cell is the set AFTER ``b_t`` was added, with no re-sort and no drop: the next merge drops what became ``-inf``, and
nothing relies on a cell being sorted across the ``+ b_t`` (rounding can make two scores equal).  ``overflow`` is 1 iff
some candidate of an ``N_t`` had ``h + lm[v][w] > -inf`` and ``code >= B**(cap-1)``: that string would not fit and the
candidate was dropped.  T = 0 gives an empty list.

Every addition is made in the bigram definition's order, ``((delta + log_exit) + lm) + log_start``, then ``+ b``, and
adding a constant is monotone under rounding: a hypothesis's score is its best path's sum in ``_bigram_ref``'s order,
rank 1 has ``_bigram_ref.viterbi``'s score bit for bit, and with ``n_best = 1`` the recursion is the bigram recursion.
Where no two of the top ``n + 1`` string scores are equal and ``overflow == 0`` the list is exactly the ``n`` best
strings of an enumeration of every path; with exact ties or overflow the recursion above is still the definition.

The arrays below hold a list of ``n`` hypotheses along their last axis; an empty slot is ``(-inf, 0)``.
"""
import numpy as np

NEG = -np.inf
MAX_NBEST = 8


def cap(W):
    """The largest K with ``(W + 1)**K <= 2**64``."""
    B, K = int(W) + 1, 0
    while B ** (K + 1) <= 2 ** 64:
        K += 1
    return K


def encode(words, W):
    code = 0
    for w in words:
        code = code * (int(W) + 1) + int(w) + 1
    return code


def decode(code, W):
    """The word string of a code, first word first; ``[]`` for 0."""
    code, B, out = int(code), int(W) + 1, []
    while code:
        out.append(code % B - 1)
        code //= B
    return out[::-1]


def merge_n(score, code, n):
    """``merge_n`` over the last axis: ``score[..., C]`` float64, ``code[..., C]`` uint64 -> ``(score[..., n],
    code[..., n])``, empty slots ``(-inf, 0)``."""
    score = np.array(score, dtype=np.float64)
    code = np.array(code, dtype=np.uint64)
    score, code = np.broadcast_arrays(score, code)
    score, code = score.copy(), code.copy()
    with np.errstate(invalid="ignore"):
        dead = ~(score > NEG)                                  # 1. -inf and NaN
    score[dead], code[dead] = NEG, 0
    order = np.lexsort((-score, code), axis=-1)                # 2. by code, the largest score of a code first
    score, code = np.take_along_axis(score, order, -1), np.take_along_axis(code, order, -1)
    dup = np.zeros(score.shape, bool)
    dup[..., 1:] = code[..., 1:] == code[..., :-1]
    score[dup], code[dup] = NEG, 0
    order = np.lexsort((code, -score), axis=-1)                # 3. score descending, then code ascending
    score, code = np.take_along_axis(score, order, -1), np.take_along_axis(code, order, -1)
    out_s = np.full(score.shape[:-1] + (n,), NEG)              # 4. the first n
    out_c = np.zeros(score.shape[:-1] + (n,), np.uint64)
    m = min(n, score.shape[-1])
    out_s[..., :m], out_c[..., :m] = score[..., :m], code[..., :m]
    return out_s, out_c


def nbest(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, n_best):
    """One utterance: ``logb[T, W, S]`` -> ``(score[n], code[n], n_found, overflow)``, best first, ``(-inf, 0)``
    padded."""
    logb = np.asarray(logb, dtype=np.float64)
    ls = np.asarray(log_start, dtype=np.float64)
    lt = np.asarray(log_trans, dtype=np.float64)
    lx = np.asarray(log_exit, dtype=np.float64)
    lm = np.asarray(lm, dtype=np.float64)
    lm0 = np.asarray(lm_start, dtype=np.float64)
    lm1 = np.asarray(lm_end, dtype=np.float64)
    W, S = ls.shape
    n = int(n_best)
    if not 1 <= n <= MAX_NBEST:
        raise ValueError("n_best must be inside 1..8")
    if lm.shape != (W, W) or lm0.shape != (W,) or lm1.shape != (W,):
        raise ValueError("lm must be [W, W], lm_start and lm_end [W]")
    T = logb.shape[0]
    B = np.uint64(W + 1)
    limit = np.uint64((W + 1) ** (cap(W) - 1))
    own = (np.arange(W) + 1).astype(np.uint64)                 # w + 1
    overflow = False
    if T == 0:
        return np.full(n, NEG), np.zeros(n, np.uint64), 0, 0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            if t == 0:
                cs, cc = merge_n((lm0[:, None] + ls)[:, :, None], own[:, None, None], n)       # [W, S, n]
            else:
                # within: [w][j][(i, r)] = cell(w,i)[r] + log_trans[w][i][j]
                ws_ = (cell_s[:, :, None, :] + lt[:, :, :, None]).transpose(0, 2, 1, 3).reshape(W, S, S * n)
                wc_ = np.broadcast_to(cell_c[:, :, None, :], (W, S, S, n)).transpose(0, 2, 1, 3).reshape(W, S, S * n)
                es_ = N_s[:, None, :] + ls[:, :, None]                                          # [w][j][r]
                ec_ = np.broadcast_to(N_c[:, None, :], (W, S, n))
                cs, cc = merge_n(np.concatenate([ws_, es_], -1), np.concatenate([wc_, ec_], -1), n)
            cell_s, cell_c = cs + logb[t][:, :, None], cc      # the cell: after + b_t, as it is
            X_s, X_c = merge_n((cell_s + lx[:, :, None]).reshape(W, S * n), cell_c.reshape(W, S * n), n)  # [v][r]
            if t < T - 1:
                sc = (X_s[:, :, None] + lm[:, None, :]).transpose(2, 0, 1)                      # [w][v][r]
                fits = np.broadcast_to((X_c < limit)[None], sc.shape)
                overflow |= bool(((sc > NEG) & ~fits).any())
                code = np.where(fits, X_c[None], np.uint64(0)) * B + own[:, None, None]
                N_s, N_c = merge_n(np.where(fits, sc, NEG).reshape(W, W * n), code.reshape(W, W * n), n)
        out_s, out_c = merge_n((X_s + lm1[:, None]).reshape(W * n), X_c.reshape(W * n), n)
    return out_s, out_c, int((out_c != 0).sum()), int(overflow)


def nbest_batch(logb, lengths, log_start, log_trans, log_exit, lm, lm_start, lm_end, n_best):
    """A packed batch ``logb[total_frames, W, S]``: ``(score[N, n], code[N, n], n_found[N] i32, overflow[N] u8)``."""
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    res = [nbest(logb[a:b], log_start, log_trans, log_exit, lm, lm_start, lm_end, n_best)
           for a, b in zip(offs[:-1], offs[1:])]
    n = int(n_best)
    return (np.asarray([r[0] for r in res], np.float64).reshape(len(res), n),
            np.asarray([r[1] for r in res], np.uint64).reshape(len(res), n),
            np.asarray([r[2] for r in res], np.int32), np.asarray([r[3] for r in res], np.uint8))


def strings(score, code, W):
    """``[(score, words), ...]`` of one utterance's list, best first, empty slots left out."""
    return [(float(s), decode(c, W)) for s, c in zip(score, code) if int(c) != 0]


def enumerate_strings(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end):
    """Every word string with a path, by enumeration of every path through the loop (small W, S, T only): ``[(score,
    code), ...]`` ordered by score descending, then code ascending.  A path's score is accumulated in the order the
    recursion adds and a string's score is the largest over its paths."""
    logb = np.asarray(logb, dtype=np.float64)
    T, W, S = logb.shape
    B = W + 1
    best = {}
    if T == 0:
        return []

    def walk(t, w, s, code, acc):
        if not acc > NEG:
            return
        if t == T - 1:
            f = (acc + log_exit[w][s]) + lm_end[w]
            if f > NEG and f > best.get(code, NEG):
                best[code] = f
            return
        for j in range(S):                                   # stay in the word
            walk(t + 1, w, j, code, (acc + log_trans[w][s][j]) + logb[t + 1][w][j])
        x = acc + log_exit[w][s]                             # leave it and enter a word
        for v in range(W):
            e = x + lm[w][v]
            for j in range(S):
                walk(t + 1, v, j, code * B + v + 1, (e + log_start[v][j]) + logb[t + 1][v][j])

    for w in range(W):
        for s in range(S):
            walk(0, w, s, w + 1, (lm_start[w] + log_start[w][s]) + logb[0][w][s])
    return sorted(((float(f), c) for c, f in best.items()), key=lambda p: (-p[0], p[1]))

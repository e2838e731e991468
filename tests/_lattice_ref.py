"""CPU restatement of the connected-word lattice (plain numpy, float64): THE DEFINITION of what
``sapr_connected_lattice``, ``sapr_connected_lattice_backward`` and ``sapr_connected_lattice_walk`` compute
(include/sapr_hip.h).  The conventions and the recursion are those of ``tests/_bigram_ref.py`` — delta, X_t(w), N_t(w),
the order of the additions, first maxima, "entry only where strictly greater" — and are taken from it, not restated.

Forward tables, per utterance of T frames, for every t < T and w < W::

    wend_score[t][w] = X_t(w)
    wend_entry[t][w] = N_t(w)
    wend_start[t][w] = B_t(w)     the utterance-relative frame at which the path that attains X_t(w) entered word w

``B`` is carried beside delta: ``b_0(w,j) = 0``; ``b_t(w,j) = t`` where entry won, else ``b_{t-1}(w,i*)`` with i* the
within-word predecessor that won; ``B_t(w) = b_t(w, xarg_t(w))``, and -1 where ``X_t(w)`` is not greater than -inf.
It is the frame the bigram back-trace from ``(t, w, xarg_t(w))`` reaches; :func:`forward` computes it both ways and
asserts that they agree.

A record is a pair (w, t) with ``X_t(w) > -inf``; tau = ``B_t(w)``; ``in = lm_start[w]`` if tau = 0, else
``N_{tau-1}(w)``; ``ac = X_t(w) - in`` (one subtraction).  Under the time-conditioned boundary the record may follow any
word v that ends at tau - 1; a record with tau = 0 starts the utterance.

Backward pass under any tables ``(lm', lm_start', lm_end')``: ``beta_{T-1}(w) = lm_end'[w]``, every other beta -inf,
``next = (-1, 255)``, ``root = -inf``, ``first = (-1, 255)``.  Records are visited with t' from T - 1 down to 0 and,
inside a frame, w' ascending::

    g = ac + beta_{t'}(w')
    tau > 0:   for every v:  c = lm'[v][w'] + g;   where c > beta_{tau-1}(v):  beta_{tau-1}(v) = c, next_{tau-1}(v) = (t', w')
    tau = 0:                 c = lm_start'[w'] + g; where c > root:            root = c, first = (t', w')

float64 adds, one subtract and strict compares only.  The walk goes from ``first`` along ``next`` until a record ends
at T - 1.  ``margin[t][w] = (X_t(w) + beta_t(w)) - score`` under the original tables, -inf for a record on no complete
path; a record is kept at beam B when ``margin >= -(B + eps_u)``, ``eps_u = 4 T_u 2^-52 M_u`` with M_u the largest
finite ``|X|`` or ``|N|`` of the utterance (DESIGN 4.3t derives it).
"""
import numpy as np

from . import _bigram_ref as bref

ENTRY = bref.ENTRY
NO_WORD = 255


def forward(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end):
    """One utterance ``logb[T, W, S]`` -> ``(X[T, W] f64, N[T, W] f64, B[T, W] i32, score, final_word)``."""
    logb = np.asarray(logb, dtype=np.float64)
    lx = np.asarray(log_exit, dtype=np.float64)
    lm = np.asarray(lm, dtype=np.float64)
    T = logb.shape[0]
    W, S = lx.shape
    score, _, _, _, _, (deltas, back, xarg, warg, final) = bref.viterbi(
        logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, want_lattice=True)
    words = np.arange(W)
    X = np.full((T, W), -np.inf)
    N = np.full((T, W), -np.inf)
    B = np.full((T, W), -1, np.int32)
    b = np.zeros((W, S), np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            X[t] = (deltas[t] + lx)[words, xarg[t]]
            N[t] = (X[t][:, None] + lm)[warg[t], words]
            if t > 0:   # carried: the frame number where entry won, the winning predecessor's otherwise
                prev = np.take_along_axis(b, np.where(back[t] == ENTRY, 0, back[t]), axis=1)
                b = np.where(back[t] == ENTRY, t, prev)
            live = X[t] > -np.inf
            B[t] = np.where(live, b[words, xarg[t]], -1)
            for w in np.flatnonzero(live):   # ... and by the bigram back-trace from (t, w, xarg_t(w))
                s, u = int(xarg[t, w]), t
                while u > 0 and back[u, w, s] != ENTRY:
                    s = int(back[u, w, s])
                    u -= 1
                assert u == B[t, w], (t, w, u, B[t, w])
    return X, N, B, float(score), int(final)


def eps(X, N):
    """``eps_u = 4 T 2^-52 M`` with M the largest finite ``|X|`` or ``|N|`` (0.0 for an utterance without any)."""
    v = np.abs(np.concatenate([np.ravel(X), np.ravel(N)]))
    v = v[np.isfinite(v)]
    return 4.0 * X.shape[0] * 2.0 ** -52 * (float(v.max()) if v.size else 0.0)


def records(X, N, B, lm_start):
    """``[(t, w, tau, in, ac), ...]`` with t ascending and, inside a frame, w ascending.  ``in`` and ``ac`` are read
    under the tables the forward pass ran under."""
    out = []
    T, W = X.shape
    for t in range(T):
        for w in range(W):
            if not X[t, w] > -np.inf:
                continue
            tau = int(B[t, w])
            if tau < 0 or tau > t:
                continue
            inc = float(lm_start[w]) if tau == 0 else float(N[tau - 1, w])
            with np.errstate(invalid="ignore"):
                out.append((t, w, tau, inc, float(np.float64(X[t, w]) - np.float64(inc))))
    return out


def backward(X, N, B, lm_start, lm2, lm_start2, lm_end2):
    """``lm_start``: the table the forward pass ran under (it defines ``ac``); ``(lm2, lm_start2, lm_end2)``: the
    tables of this pass.  Returns ``(beta[T, W] f64, next_end[T, W] i32, next_word[T, W] u8, root, first)`` with
    ``first = (end, word)``."""
    T, W = X.shape
    lm2 = np.asarray(lm2, dtype=np.float64)
    beta = np.full((T, W), -np.inf)
    nend = np.full((T, W), -1, np.int32)
    nword = np.full((T, W), NO_WORD, np.uint8)
    root, first = -np.inf, (-1, NO_WORD)
    if T == 0:
        return beta, nend, nword, root, first
    beta[T - 1] = np.asarray(lm_end2, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for t, w, tau, _, ac in sorted(records(X, N, B, lm_start), key=lambda r: (-r[0], r[1])):
            g = np.float64(ac) + beta[t, w]
            if tau > 0:
                c = lm2[:, w] + g
                take = c > beta[tau - 1]
                beta[tau - 1] = np.where(take, c, beta[tau - 1])
                nend[tau - 1] = np.where(take, t, nend[tau - 1])
                nword[tau - 1] = np.where(take, w, nword[tau - 1])
            else:
                c = np.float64(lm_start2[w]) + g
                if c > root:
                    root, first = float(c), (t, w)
    return beta, nend, nword, float(root), first


def walk(T, W, nend, nword, root, first):
    """``(n_words, path_word[T] i32, path_entry[T] u8)``: from ``first`` along ``next`` until a record ends at T - 1;
    -1 / 0 / 0 where ``root`` is not finite.  ``next_end`` is clamped into (t, T - 1] and ``next_word`` below W."""
    pw = np.full(T, -1, np.int32)
    pe = np.zeros(T, np.uint8)
    if T == 0 or not np.isfinite(root):
        return 0, pw, pe
    clamp = lambda e, lo: min(max(int(e), lo), T - 1)   # noqa: E731
    word = lambda w: int(w) if int(w) < W else 0        # noqa: E731
    e, w, a, n = clamp(first[0], 0), word(first[1]), 0, 0
    while True:
        pw[a:e + 1] = w
        pe[a] = 1
        n += 1
        if e >= T - 1:
            return n, pw, pe
        a = e + 1
        e, w = clamp(nend[a - 1, w], a), word(nword[a - 1, w])


def margins(X, beta, score):
    """``(X + beta) - score``; -inf where ``X + beta`` is not greater than -inf."""
    with np.errstate(invalid="ignore"):
        m = X + beta
        return np.where(m > -np.inf, m - np.float64(score), -np.inf)


def kept(margin, beam, eps_u):
    """The records kept at ``beam``: on a complete path and ``margin >= -(beam + eps_u)``."""
    return (margin > -np.inf) & (margin >= -(np.float64(beam) + eps_u))


def lattice(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end, lm2=None):
    """One utterance, everything: a dict of the forward tables, the backward pass under the original tables (or under
    ``lm2 = (lm', lm_start', lm_end')``), the walk and, under the original tables, the margins."""
    X, N, B, score, final = forward(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end)
    tabs = (lm, lm_start, lm_end) if lm2 is None else lm2
    beta, nend, nword, root, first = backward(X, N, B, lm_start, *tabs)
    n, pw, pe = walk(X.shape[0], X.shape[1], nend, nword, root, first)
    out = dict(X=X, N=N, B=B, score=score, final=final, beta=beta, next_end=nend, next_word=nword, root=root,
               first=first, n_words=n, path_word=pw, path_entry=pe, eps=eps(X, N),
               lm_start=np.asarray(lm_start, dtype=np.float64))
    if lm2 is None:
        out["margin"] = margins(X, beta, score)
    return out


def batch(logb, lengths, log_start, log_trans, log_exit, lm, lm_start, lm_end, lm2=None):
    """A packed batch: the per-utterance dicts of :func:`lattice` and the concatenated tables the device returns:
    ``(per_utt, dict(X, N, B, beta, next_end, next_word, path_word, path_entry, score, final, root, first[N, 2],
    n_words))``."""
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    W = np.asarray(log_exit).shape[0]
    per = [lattice(logb[a:b], log_start, log_trans, log_exit, lm, lm_start, lm_end, lm2)
           for a, b in zip(offs[:-1], offs[1:])]
    cat = lambda k, dt, tail: (np.concatenate([r[k] for r in per]).astype(dt) if per  # noqa: E731
                               else np.zeros((0,) + tail, dt))
    out = dict(X=cat("X", np.float64, (W,)), N=cat("N", np.float64, (W,)), B=cat("B", np.int32, (W,)),
               beta=cat("beta", np.float64, (W,)), next_end=cat("next_end", np.int32, (W,)),
               next_word=cat("next_word", np.uint8, (W,)), path_word=cat("path_word", np.int32, ()),
               path_entry=cat("path_entry", np.uint8, ()),
               score=np.asarray([r["score"] for r in per], np.float64),
               final=np.asarray([r["final"] for r in per], np.int32),
               root=np.asarray([r["root"] for r in per], np.float64),
               first=np.asarray([r["first"] for r in per], np.int32).reshape(len(per), 2),
               n_words=np.asarray([r["n_words"] for r in per], np.int32))
    return per, out


# ---- the enumeration of every path (tiny shapes) ---------------------------------------------------------------
def enumerate_paths(logb, log_start, log_trans, log_exit, lm, lm_start, lm_end):
    """Every word string with its boundaries, each with the score of its best state path (every state sequence of every
    segment is enumerated; plain float64 sums — the comparison allows ``eps_u``):
    ``{((w_0, a_0, b_0), (w_1, a_1, b_1), ...): score}``; strings whose score is -inf are left out."""
    import itertools
    logb = np.asarray(logb, dtype=np.float64)
    T, W, S = logb.shape
    seg = {}
    for w in range(W):
        for a in range(T):
            for b in range(a + 1, T + 1):
                best = -np.inf
                for states in itertools.product(range(S), repeat=b - a):
                    v = log_start[w][states[0]] + logb[a, w, states[0]]
                    for k in range(1, b - a):
                        v += log_trans[w][states[k - 1]][states[k]] + logb[a + k, w, states[k]]
                    best = max(best, v + log_exit[w][states[-1]])
                seg[w, a, b] = best
    out = {}
    for k in range(1, T + 1):
        for cuts in itertools.combinations(range(1, T), k - 1):
            bounds = (0,) + cuts + (T,)
            for ws in itertools.product(range(W), repeat=k):
                v = lm_start[ws[0]] + lm_end[ws[-1]]
                for q in range(k):
                    v += seg[ws[q], bounds[q], bounds[q + 1]]
                    if q:
                        v += lm[ws[q - 1]][ws[q]]
                if v > -np.inf:
                    out[tuple((ws[q], bounds[q], bounds[q + 1]) for q in range(k))] = float(v)
    return out


def lattice_paths(lat, lm, lm_start, lm_end, keep=None):
    """Every complete path of the lattice ``lat`` (:func:`lattice`'s dict; ``keep``: a mask [T, W] of the records that
    may be used) under the given tables (``ac`` stays the forward pass's): ``{((w, a, b), ...): score}``,
    ``score = lm_start[w_0] + ac_0 + lm[w_0][w_1] + ac_1 + ... + lm_end[w_last]``."""
    X, N, B = lat["X"], lat["N"], lat["B"]
    T = X.shape[0]
    by_start = {}
    for t, w, tau, _, ac in records(X, N, B, lat["lm_start"]):
        if keep is None or keep[t, w]:
            by_start.setdefault(tau, []).append((t, w, ac))
    out = {}

    def grow(path, acc, prev, a):
        for t, w, ac in by_start.get(a, []):
            step = lm_start[w] if prev is None else lm[prev][w]
            if not step > -np.inf:
                continue
            v, p = acc + step + ac, path + ((w, a, t + 1),)
            if t == T - 1:
                if lm_end[w] > -np.inf:
                    out[p] = float(v + lm_end[w])
            else:
                grow(p, v, w, t + 1)

    if T:
        grow((), 0.0, None, 0)
    return out

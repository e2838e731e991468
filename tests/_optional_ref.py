"""CPU restatement of the chain units with OPTIONAL transcript slots (plain numpy, float64): THE DEFINITION of what
``sapr_connected_align_opt`` and ``sapr_connected_embed[_full | _gmm]_opt`` compute (include/sapr_hip.h).  The
conventions are those of ``tests/_align_ref.py`` and ``tests/_embedded_ref.py``.

Utterance u has a transcript ``w_0..w_{K-1}`` and flags ``opt_0..opt_{K-1}`` in {0, 1}: an optional slot may be walked
through or stepped over.  No two neighbouring slots are optional and at least one slot is mandatory (anything else, or a
flag other than 0 / 1, has no path), so a slot has at most two predecessor slots; ``far(k)`` holds for k >= 2 with
``opt_{k-1} = 1``.  Alignment::

    delta_0(0,j) = log_start[w_0][j] + b_0(0,j)
    delta_0(1,j) = log_start[w_1][j] + b_0(1,j)   where opt_0 = 1 and K > 1;   every other slot -inf
    X_{t-1}(k)   as in _align_ref (s ascending, the first maximum)
    enter(k)     = X_{t-1}(k-1);  where far(k) and X_{t-1}(k-2) is STRICTLY greater: X_{t-1}(k-2), a "skip entry"
    entry        = (enter(k) + word_penalty) + log_start[w_k][j]        (k = 0: -inf)
    delta_t(k,j) = max(within, entry) + b_t(k,j)                        entry only where strictly greater
    score        = X_{T-1}(K-1);  where opt_{K-1} = 1, K >= 2 and X_{T-1}(K-2) is STRICTLY greater: X_{T-1}(K-2), and the
                   path ends in slot K-2

The nearer slot wins every tie; ``word_penalty`` is paid for every slot entered and never for a slot stepped over; the
back-trace steps two slots back over a skip entry; ``word_start[k] = -1`` for a slot the path stepped over.  With all
flags 0 this is ``_align_ref.align`` word for word.  Forward-backward is the same chain with ``lse`` in place of
``max``::

    alpha_0                         the two start slots above
    alpha_t(k,j) entry term         (lse(X_{t-1}(k-1), X_{t-1}(k-2) where far(k)) + word_penalty) + log_start[w_k][j]
    loglik                          lse(X_{T-1}(K-1), X_{T-1}(K-2) where opt_{K-1} = 1 and K >= 2)
    beta_{T-1}(k,s)                 log_exit  for k = K-1, and for k = K-2 where opt_{K-1} = 1;   else -inf
    beta_t(k,i) exit term           log_exit[w_k][i] + lse(E_{t+1}(k+1), E_{t+1}(k+2) where far(k+2))
    start[k]                        sum_t exp((lse(X_{t-1}(k-1), X_{t-1}(k-2) where far(k)) + word_penalty) + log_start
                                    + b_t + beta_t - loglik), plus gamma_0 of the start slots

``gamma``, ``trans`` and every observation sum are per slot as in ``_embedded_ref``; ``nobs`` counts the slots of
utterances with a path, whether or not mass went through them.
"""
import copy
import itertools

import numpy as np

from tests import _align_ref as aref
from tests import _embedded_ref as eref
from tests._align_ref import RECURSION_LENGTHS, RECURSION_SHAPES, network, recursion_case  # noqa: F401

NEG = -np.inf
ENTRY = 255
SKIP = 254
PENALTIES = aref.PENALTIES


def flags_ok(opt, K):
    """The two rules (and 0 / 1 values, one flag per slot)."""
    o = [int(v) for v in opt]
    if len(o) != K or any(v not in (0, 1) for v in o):
        return False
    return not any(a and b for a, b in zip(o, o[1:])) and not all(o)


def _far(opt, K):
    return np.array([k >= 2 and opt[k - 1] == 1 for k in range(K)], dtype=bool)


def align(logb, words, optional, log_start, log_trans, log_exit, word_penalty=0.0):
    """One utterance: ``logb[T, W, S]``, its transcript and its flags -> ``(score, path_word[T], path_state[T],
    path_entry[T], word_start[K])``."""
    logb = np.asarray(logb, dtype=np.float64)
    words = [int(w) for w in words]
    pen = np.float64(word_penalty)
    T, K = logb.shape[0], len(words)
    pw = np.full(T, -1, np.int32)
    ps = np.full(T, -1, np.int32)
    pe = np.zeros(T, np.uint8)
    start = np.full(K, -1, np.int32)
    if T == 0 or K == 0 or not flags_ok(optional, K):
        return float("-inf"), pw, ps, pe, start
    opt = [int(v) for v in optional]
    far = _far(opt, K)
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
                if opt[0] == 1 and K > 1:
                    delta[1] = ls[1] + b[1]
                back[0] = ENTRY
            else:
                cand = delta[:, :, None] + lt                # [k][i][j]
                arg = cand.argmax(axis=1)                    # first maximum: the lowest i
                within = np.take_along_axis(cand, arg[:, None, :], axis=1)[:, 0, :]
                near = np.r_[-np.inf, X[:-1]]
                over = np.where(far, np.r_[-np.inf, -np.inf, X[:-2]][:K], -np.inf)
                skip = far & (over > near)
                enter = np.where(skip, over, near)
                entry = (enter[:, None] + pen) + ls
                entry[0] = -np.inf
                take = entry > within
                delta = np.where(take, entry, within) + b
                back[t] = np.where(take, np.where(skip[:, None], SKIP, ENTRY), arg)
            e = delta + lx
            xarg[t] = e.argmax(axis=1)                       # the lowest state among equals
            X = e[np.arange(K), xarg[t]]
    k = K - 1
    if opt[K - 1] == 1 and K >= 2 and X[K - 2] > X[K - 1]:
        k = K - 2
    score = float(X[k])
    if np.isfinite(score):
        s = int(xarg[T - 1, k])
        for t in range(T - 1, -1, -1):
            pw[t], ps[t] = words[k], s
            bk = int(back[t, k, s])
            if t == 0 or bk in (ENTRY, SKIP):
                pe[t] = 1
                start[k] = t
                if t > 0:
                    k -= 2 if bk == SKIP else 1
                    s = int(xarg[t - 1, k])
            else:
                s = bk
    return score, pw, ps, pe, start


def align_batch(logb, lengths, transcripts, optional, log_start, log_trans, log_exit, word_penalty=0.0,
                max_words=None):
    """A packed batch, as ``_align_ref.align_batch``."""
    offs = np.r_[0, np.cumsum(np.asarray(lengths, dtype=np.int64))]
    res = []
    for a, b, words, opt in zip(offs[:-1], offs[1:], transcripts, optional):
        if max_words is not None and len(words) > max_words:
            res.append((float("-inf"), np.full(b - a, -1, np.int32), np.full(b - a, -1, np.int32),
                        np.zeros(b - a, np.uint8), np.full(len(words), -1, np.int32)))
        else:
            res.append(align(logb[a:b], words, opt, log_start, log_trans, log_exit, word_penalty))
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.zeros(0, dt)  # noqa: E731
    return (np.asarray([r[0] for r in res], np.float64), cat(1, np.int32), cat(2, np.int32), cat(3, np.uint8),
            cat(4, np.int32))


def segments(words, word_start, T):
    """``[(word, start, end_exclusive), ...]`` over the slots the path took; ``[]`` where there is no path."""
    taken = [(int(w), int(a)) for w, a in zip(words, word_start) if int(a) >= 0]
    ends = [a for _, a in taken[1:]] + [int(T)]
    return [(w, a, b) for (w, a), b in zip(taken, ends)]


def _lse(a, axis):
    return np.logaddexp.reduce(a, axis=axis)


def forward_backward(logb, words, optional, ls, lt, lx, pen=0.0):
    """One utterance -> a dict with ``loglik``, ``gamma[T, K, S]`` and the per-slot ``start[K, S]``,
    ``trans[K, S, S]`` (zeros, and the likelihood that is not finite, without a path)."""
    logb = np.asarray(logb, dtype=np.float64)
    ls, lt, lx = (np.asarray(a, dtype=np.float64) for a in (ls, lt, lx))
    words = [int(w) for w in words]
    pen = np.float64(pen)
    T, K = logb.shape[0], len(words)
    W, S = ls.shape
    out = {"loglik": NEG, "gamma": np.zeros((T, K, S)), "start": np.zeros((K, S)), "trans": np.zeros((K, S, S))}
    if T == 0 or K == 0 or any(w < 0 or w >= W for w in words) or not flags_ok(optional, K):
        return out
    opt = [int(v) for v in optional]
    far = _far(opt, K)
    firsts = [0] + ([1] if opt[0] == 1 and K > 1 else [])
    lasts = [K - 1] + ([K - 2] if opt[K - 1] == 1 and K >= 2 else [])
    LS, LT, LX = ls[words], lt[words], lx[words]
    B = logb[:, words, :]                                        # [T][K][S]

    def joined(x):                                               # lse(x(k-1), x(k-2) where far(k)), -inf for k = 0
        near = np.r_[NEG, x[:-1]]
        over = np.where(far, np.r_[NEG, NEG, x[:-2]][:K], NEG)
        return np.logaddexp(near, over)

    with np.errstate(invalid="ignore", over="ignore"):
        alpha = np.full((T, K, S), NEG)
        X = np.full((T, K), NEG)
        Xin = np.full((T, K), NEG)                               # Xin[t]: what enters slot k at frame t + 1
        for k in firsts:
            alpha[0, k] = LS[k] + B[0, k]
        X[0] = _lse(alpha[0] + LX, 1)
        Xin[0] = joined(X[0])
        for t in range(1, T):
            within = _lse(alpha[t - 1][:, :, None] + LT, 1)      # [k][j]
            entry = (Xin[t - 1][:, None] + pen) + LS
            entry[0] = NEG
            alpha[t] = np.logaddexp(within, entry) + B[t]
            X[t] = _lse(alpha[t] + LX, 1)
            Xin[t] = joined(X[t])
        ll = _lse(np.array([X[T - 1, k] for k in lasts]), 0)
        out["loglik"] = float(ll)
        if not np.isfinite(ll):
            return out
        beta = np.full((T, K, S), NEG)
        for k in lasts:
            beta[T - 1, k] = LX[k]
        for t in range(T - 2, -1, -1):
            c = B[t + 1] + beta[t + 1]
            E = np.full(K + 2, NEG)
            E[1:K] = pen + _lse(LS[1:] + c[1:], 1)
            nxt = np.array([np.logaddexp(E[k + 1], E[k + 2] if (k + 2 < K and far[k + 2]) else NEG) for k in range(K)])
            beta[t] = np.logaddexp(_lse(LT + c[:, None, :], 2), LX + nxt[:, None])
        out["gamma"] = np.exp(alpha + beta - ll)
        c = B[1:] + beta[1:]                                     # [T-1][K][S]
        out["trans"] = np.exp(alpha[:-1, :, :, None] + LT[None] + c[:, :, None, :] - ll).sum(axis=0)
        start = np.zeros((K, S))
        for k in firsts:
            start[k] = out["gamma"][0, k]
        start[1:] += np.exp((Xin[:-1, 1:, None] + pen) + LS[None, 1:] + c[:, 1:] - ll).sum(axis=0)
        out["start"] = start
    return out


def estep_batch(logb, lengths, transcripts, optional, ls, lt, lx, pen=0.0, feats=None, max_words=None,
                second_moments=False, mixtures=None):
    """``_embedded_ref.estep_batch`` over :func:`forward_backward`.  ``second_moments``: also ``oo[W, S, D, D]`` (the
    sums of ``_embedded_full_ref``); ``mixtures = (weights, means, covars)``: ``post_mix``, and ``obs`` / ``obs2`` per
    component in place of the single-Gaussian ones (the sums of ``_embedded_gmm_ref``)."""
    ls = np.asarray(ls, dtype=np.float64)
    W, S = ls.shape
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.r_[0, np.cumsum(lengths)]
    if max_words is None:
        max_words = max([len(t) for t in transcripts] + [1])
    D = 0 if feats is None else int(np.shape(feats)[1])
    x32 = np.zeros((int(offs[-1]), 0), np.float32) if feats is None else np.asarray(feats, dtype=np.float32)
    x, x2 = x32.astype(np.float64), (x32 * x32).astype(np.float64)   # (the float32 square, as hmmlearn evaluates X**2)
    res = {"loglik": np.full(len(lengths), NEG), "post": np.zeros((int(offs[-1]), max_words, S)),
           "nobs": np.zeros(W), "start": np.zeros((W, S)), "trans": np.zeros((W, S, S)), "post_sum": np.zeros((W, S)),
           "obs": np.zeros((W, S, D)), "obs2": np.zeros((W, S, D))}
    if second_moments:
        res["oo"] = np.zeros((W, S, D, D))
    if mixtures is not None:
        from tests._embedded_gmm_ref import _mix_sums
        weights, means, covars = (np.asarray(a, dtype=np.float64) for a in mixtures)
        M = means.shape[2]
        res.update(post_mix=np.zeros((W, S, M)), obs=np.zeros((W, S, M, D)), obs2=np.zeros((W, S, M, D)))
    for u, (a, b, words, opt) in enumerate(zip(offs[:-1], offs[1:], transcripts, optional)):
        if len(words) > max_words:
            continue
        r = forward_backward(logb[a:b], words, opt, ls, lt, lx, pen)
        res["loglik"][u] = r["loglik"]
        if not np.isfinite(r["loglik"]):
            continue
        g = r["gamma"]
        res["post"][a:b, :len(words)] = g
        for k, w in enumerate(words):
            res["nobs"][w] += 1
            res["start"][w] += r["start"][k]
            res["trans"][w] += r["trans"][k]
            res["post_sum"][w] += g[:, k].sum(axis=0)
            if mixtures is None:
                res["obs"][w] += g[:, k].T @ x[a:b]
                res["obs2"][w] += g[:, k].T @ x2[a:b]
            if second_moments:
                res["oo"][w] += np.einsum("ts,tab->sab", g[:, k], x[a:b, :, None] * x[a:b, None, :])
        if mixtures is not None:
            for w in sorted(set(int(v) for v in words)):
                gw = np.zeros((b - a, S))
                for k, wk in enumerate(words):                    # (k ascending)
                    if wk == w:
                        gw += g[:, k]
                pm, o1, o2 = _mix_sums(gw, x[a:b], x2[a:b], weights[w], means[w], covars[w])
                res["post_mix"][w] += pm
                res["obs"][w] += o1
                res["obs2"][w] += o2
    return res


def fit(models, features, transcripts, optional, n_iter=10, tol=1e-2, exit_states="last", word_penalty=0.0):
    """``_embedded_ref.fit`` over :func:`estep_batch`: the host EM loop for "diag" / "spherical" ``GaussianHMM``
    objects.  Returns ``(models, history)``."""
    from sapr_amd.hmmlearn_hmm import ConvergenceMonitor, m_step_typed
    models = [copy.deepcopy(m) for m in models]
    feats = [np.asarray(f, dtype=np.float32) for f in features]
    lengths = [len(f) for f in feats]
    x = np.concatenate(feats)
    monitor = ConvergenceMonitor(tol, n_iter)
    for _ in range(n_iter):
        ls, lt, lx, means, vars_, gconst = eref.tables(models, exit_states)
        logb = eref.emit_diag(x.astype(np.float64), means, vars_, gconst)
        r = estep_batch(logb, lengths, transcripts, optional, ls, lt, lx, word_penalty, feats=x)
        for w, m in enumerate(models):
            if r["nobs"][w] == 0:
                continue
            st = {"nobs": r["nobs"][w], "start": r["start"][w], "trans": r["trans"][w], "post": r["post_sum"][w],
                  "obs": r["obs"][w], "obs**2": r["obs2"][w]}
            m.startprob_, m.transmat_, m.means_, m._covars_ = m_step_typed(
                st, m.covariance_type, m.startprob_, m.transmat_, m.params, m.startprob_prior, m.transmat_prior,
                m.means_prior, m.means_weight, m.covars_prior, m.covars_weight, np.asarray(m.means_, dtype=np.float64),
                np.asarray(m._covars_, dtype=np.float64))
        ll = r["loglik"]
        monitor.report(float(ll[np.isfinite(ll)].sum()))
        if monitor.converged:
            break
    return models, list(monitor.history)


# ---- every path, and every explicit transcript -------------------------------------------------------------------
def _paths(logb, words, optional, ls, lt, lx, pen):
    """``[(log score, [(k, s)] * T), ...]`` over EVERY path of the chain (tiny cases only); the additions of a path are
    made in the order of the recursion."""
    T, K, S = logb.shape[0], len(words), ls.shape[1]
    paths = []
    if not (T and K) or not flags_ok(optional, K):
        return paths
    opt = [int(v) for v in optional]

    def walk(t, k, s, acc, trail):
        if acc == NEG:
            return
        w = words[k]
        if t == T - 1:
            if (k == K - 1 or (k == K - 2 and opt[K - 1] == 1)) and lx[w, s] > NEG:
                paths.append((acc + lx[w, s], trail))
            return
        for s2 in range(S):
            walk(t + 1, k, s2, (acc + lt[w, s, s2]) + logb[t + 1, w, s2], trail + [(k, s2)])
            for k2 in (k + 1, k + 2):
                if k2 < K and (k2 == k + 1 or opt[k + 1] == 1):
                    w2 = words[k2]
                    walk(t + 1, k2, s2, (((acc + lx[w, s]) + pen) + ls[w2, s2]) + logb[t + 1, w2, s2],
                         trail + [(k2, s2)])

    for k in [0] + ([1] if opt[0] == 1 and K > 1 else []):
        for s in range(S):
            walk(0, k, s, ls[words[k], s] + logb[0, words[k], s], [(k, s)])
    return paths


def brute(logb, words, optional, ls, lt, lx, pen=0.0):
    """``best`` (the alignment score), ``loglik``, ``gamma``, ``start`` and ``trans`` of one utterance by enumerating
    every path: each complete path adds its probability to what it passes through."""
    logb = np.asarray(logb, dtype=np.float64)
    words = [int(w) for w in words]
    T, K, S = logb.shape[0], len(words), ls.shape[1]
    paths = _paths(logb, words, optional, ls, lt, lx, pen)
    out = {"best": NEG, "loglik": NEG, "gamma": np.zeros((T, K, S)), "start": np.zeros((K, S)),
           "trans": np.zeros((K, S, S)), "paths": len(paths)}
    if not paths:
        return out
    scores = np.array([p[0] for p in paths])
    out["best"] = float(scores.max())
    ll = scores.max() + np.log(np.exp(scores - scores.max()).sum())
    out["loglik"] = float(ll)
    for sc, trail in paths:
        p = np.exp(sc - ll)
        for t, (k, s) in enumerate(trail):
            out["gamma"][t, k, s] += p
            if t == 0 or trail[t - 1][0] != k:
                out["start"][k, s] += p
            else:
                out["trans"][k, trail[t - 1][1], s] += p
    return out


def expansions(words, optional):
    """Every explicit transcript the optional one stands for: ``[(kept slot indices, their words), ...]``, each subset
    of the optional slots deleted; the subsets in the order that keeps the NEARER slot first wherever two expansions
    tie (all kept first)."""
    K = len(words)
    where = [k for k in range(K) if int(optional[k]) == 1]
    out = []
    for drop in itertools.product((0, 1), repeat=len(where)):
        gone = {k for k, d in zip(where, drop) if d}
        keep = [k for k in range(K) if k not in gone]
        out.append((keep, [int(words[k]) for k in keep]))
    return out


# ---- the recursion cases (tests/test_optional_gpu.py; tests/test_optional_cpu.py checks their conditions) ----------
def silence_flags(K):
    """Even slots optional (``sil? w sil? w ...``); a lone slot is mandatory."""
    return [0] if K == 1 else [1 - k % 2 for k in range(K)]


def random_flags(rng, K):
    """A random pattern with no two neighbours optional; slot 0 mandatory when everything else came out optional."""
    o = [0] * K
    for k in range(K):
        if (k == 0 or o[k - 1] == 0) and rng.random() < 0.5:
            o[k] = 1
    if all(o):
        o[0] = 0
    return o


def recursion_flags(W, S, max_words, topology, exits, integer, transcripts):
    """The flags of one parametrised case: utterances alternate between the silence pattern and a random one."""
    rng = np.random.default_rng(77 + 1000 * W + 10 * S + aref.TOPOLOGIES.index(topology) * 3
                                + aref.EXITS.index(exits) + 7 * integer)
    return [silence_flags(len(t)) if u % 2 == 0 else random_flags(rng, len(t)) for u, t in enumerate(transcripts)]


def optional_case(W, S, max_words, topology, exits, integer):
    """``(ls, lt, lx, logb[total, W, S], transcripts, optional)``: ``_align_ref.recursion_case`` with flags."""
    ls, lt, lx, logb, transcripts = aref.recursion_case(W, S, max_words, topology, exits, integer)
    return ls, lt, lx, logb, transcripts, recursion_flags(W, S, max_words, topology, exits, integer, transcripts)


def tiny_case(seed):
    """A random tiny chain for the enumeration: 2 to 4 slots of 2 states over 3 words, 3 to 6 frames."""
    rng = np.random.default_rng(seed)
    W, S = 3, 2
    K, T = int(rng.integers(1, 5)), int(rng.integers(3, 7))
    ls, lt, lx = aref.network(rng, W, S, ("bidiag", "dense")[seed % 2], ("last", "any")[(seed // 2) % 2], False)
    logb = rng.normal(-3.0, 2.0, (T, W, S))
    words = rng.integers(0, W, K).tolist()
    opt = silence_flags(K) if seed % 3 == 0 else random_flags(rng, K)
    return ls, lt, lx, logb, words, opt, float(rng.choice([0.0, -2.0, 1.5]))


def path_facts(words, optional, word_start, T, score):
    """Of one aligned utterance: ``(has a path, steps over a slot, takes an optional slot, starts in slot 1, ends in
    slot K - 2)``."""
    if not np.isfinite(score):
        return False, False, False, False, False
    taken = [int(a) >= 0 for a in word_start]
    opt = [int(v) == 1 for v in optional]
    return (True, any(o and not t for o, t in zip(opt, taken)), any(o and t for o, t in zip(opt, taken)),
            not taken[0], not taken[-1])


# ---- recordings with pauses nobody wrote down (the end-to-end tests) ----------------------------------------------
PAUSE_SEED = 31
PAUSE_WORD = 1            # the vocabulary word that serves as silence


def _emission(family, model, x):
    from tests import _connected_family_cases as cases
    from tests import _connected_ref as cref
    if family == "diag":
        return cref.emit_diag(x, model["means"], model["vars"], model["gconst"])
    return cases.emission(family, model, x)


def pause_case(family, model, utts, truth, sil=PAUSE_WORD, seed=PAUSE_SEED):
    """A committed-style case with pauses: ``(recordings, inserted, pause_frames)``.  The word boundaries of every
    utterance come from ``_align_ref.align`` to its truth on the family's reference emission; into each gap (in front
    of word g, g = K: behind the last) that touches no written ``sil``, with probability 1/2, goes a pause: every state
    of ``sil`` held for 1 to 3 frames, drawn around the state's mean (of its first component) with unit variance —
    inside every family's state distribution.  ``inserted[u]``: the gaps that got one; ``pause_frames[u]``: a mask."""
    rng = np.random.default_rng(seed)
    mu = np.asarray(model["means"], dtype=np.float64)[sil]
    mu = mu[:, 0] if mu.ndim == 3 else mu                        # [S][D]
    S = model["log_start"].shape[1]
    from tests._connected_family_cases import log_exit
    lx = model.get("log_exit", log_exit(model["log_start"].shape[0], S))
    recs, inserted, masks = [], [], []
    for x, words in zip(utts, truth):
        logb = _emission(family, model, x)
        score, _, _, _, start = aref.align(logb, words, model["log_start"], model["log_trans"], lx, 0.0)
        assert np.isfinite(score)
        cuts = [int(a) for a in start] + [len(x)]
        K = len(words)
        rows, mask, gaps = [], [], []
        for g in range(K + 1):
            free = (g == 0 or words[g - 1] != sil) and (g == K or words[g] != sil)
            if free and rng.random() < 0.5:
                p = np.concatenate([mu[s] + rng.normal(size=(int(rng.integers(1, 4)), mu.shape[1])) for s in range(S)])
                rows.append(p.astype(np.float32))
                mask += [True] * len(p)
                gaps.append(g)
            if g < K:
                rows.append(x[cuts[g]:cuts[g + 1]])
                mask += [False] * (cuts[g + 1] - cuts[g])
        recs.append(np.concatenate(rows).astype(np.float32))
        inserted.append(gaps)
        masks.append(np.asarray(mask, dtype=bool))
    return recs, inserted, masks


def pause_slots(words, inserted, sil=PAUSE_WORD):
    """The flags ``with_optional`` gives ``words``, and the optional slots that stand for the gaps in ``inserted``."""
    slots, flags, want = [], [], []
    for k, w in enumerate(words):
        if w != sil and (k == 0 or words[k - 1] != sil):
            if k in inserted:
                want.append(len(slots))
            slots.append(sil)
            flags.append(1)
        slots.append(int(w))
        flags.append(0)
    if words and words[-1] != sil:
        if len(words) in inserted:
            want.append(len(slots))
        slots.append(sil)
        flags.append(1)
    return slots, flags, want

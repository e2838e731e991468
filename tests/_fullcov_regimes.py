"""Seeded inputs and the np.longdouble reference of tests/test_fullcov_regimes_*.py: full-covariance word models whose
states differ in their covariance matrices and overlap with the data they are scored on.

tests/_fullcov_cases.py and tests/_full_vocab_cases.py start every state of every model from ONE matrix and score
tests/_synth.py's data, whose posteriors are one-hot: a kernel that reads Winv or c of the wrong state, or weights a
Gram product with the wrong state's posterior, computes the same numbers there.  Here (``word_model``):

    B       = Q diag(lam) Q^T       Q from the QR of a standard normal matrix, lam log-uniform in [1, kappa] with
                                    lam[0] = 1 and lam[-1] = kappa;  L0 = chol(B)                  (one per word)
    Sigma_s = L0 (I + a E_s) L0^T   E_s symmetric with entries N(0, 1) / sqrt(D), symmetrised      (one per STATE)
    mu_s    = mu_{s-1} + sep * L0 g / sqrt(D),  g ~ N(0, I);  mu_0 ~ N(0, 5^2) with mu_0[0] = -300
    bidiag: stay probability U(0.5, 0.8), start in state 0;  dense: Dirichlet(2) rows and start vector

and every utterance is SAMPLED from its own word model (a state path, then x_t = mu_q + chol(Sigma_q) N(0, I), cast to
float32).  The models' random numbers come from seed 100 * D + S (+ 1000 per seed skipped, see SEED_SKIPS), the data's
from that seed + 7.

Regimes (``check_conditions`` asserts each one's conditions from the longdouble reference alone; the CPU test and the GPU
tests run it before they compare anything):
    soft    kappa 1e4, a 0.3, sep 0.7, three words with the lengths SOFT_LENGTHS each, at SOFT_SHAPES.  At least 10 % of
            the frames have a largest posterior below 0.9 (where S > 1: the single state of (15, 1) has posterior 1 by
            definition, its case is about the one-state group of the accumulate pass), no two states of a word share a
            covariance matrix, the largest cond(Sigma_s) is at most 2e4.
    ill     kappa 1e6 at ILL_SHAPES, otherwise the same recipe: the largest cond(Sigma_s) is at least 1e5.
    tied    a = 0 (one matrix per word) at TIED_SHAPES: the states of a word share their matrix bit for bit.
    ragged  (17, 5) dense, five words: word 0's utterances, in batch order, put the running frame total on 63, 64, 65
            (a 0-frame utterance keeps it there), 255, 256 and 257; word 1 has one utterance of one frame (a tile with
            fewer chunks than partial rows), word 2 none, word 3 has 300 utterances of 12 or 13 frames (two tiles), word
            4 the lengths 63, 1, 1.  (A tile's slots are sorted by falling length, so word 0's tile runs 190, 253, 254,
            255, 256, 257 and ends one frame into its fifth chunk; word 4's runs 63, 64, 65 and ends one frame into its
            second.)
In every regime the MAP path and the Viterbi path are compared on every frame, so every case must have a smallest gap
between the two largest posteriors of a frame above 1e-6 and a smallest relative Viterbi arg-max gap above 1e-9.

The reference: ``log_density`` is a Cholesky factorisation and a forward substitution written out in np.longdouble
(x87 80-bit, eps 1.08e-19); the recursions, the soft-max and the log-sum-exp are those of tests/_fb_ref.py; start, trans,
post, obs and oo are accumulated in longdouble; Viterbi is restated over the longdouble logb (first maximum, the gap
measure of tests/_fullcov_ref.viterbi).  ``e_ref`` is the deviation of the float64 restatement tests/_fullcov_ref.py
from it on the same inputs, in the measures the GPU test uses (``rel_err``, ``mixed_err``, ``normwise_err``).

MEASURED on the CPU from the reference ("soft" = frames whose largest posterior is below 0.9, "top-two" = smallest gap
between the two largest posteriors of a frame, "vit gap" = smallest relative arg-max gap of a Viterbi pass, "cond" =
largest cond(Sigma_s); then E_ref per quantity: logb and the scores relative, gamma / trans / obs as
|x - ref| / (1e-3 + |ref|), oo norm-wise per state):
    case           frames      soft    top-two    vit gap       cond       logb     loglik    viterbi      gamma      trans        obs         oo
    soft-5-3          846    98.9 %    2.4e-04    1.4e-06    1.5e+04    4.1e-13    5.4e-15    8.0e-15    1.9e-12    1.3e-13    3.0e-13    2.9e-14
    soft-13-10        846    40.0 %    1.9e-03    6.5e-06    1.5e+04    3.3e-13    3.9e-15    3.8e-15    1.6e-12    4.5e-13    1.0e-11    1.2e-13
    soft-12-4         846    96.3 %    7.3e-05    2.0e-06    1.4e+04    4.2e-13    2.7e-15    3.5e-15    3.0e-12    7.5e-13    1.8e-12    5.3e-14
    soft-16-4         846    91.4 %    9.2e-04    1.4e-06    1.5e+04    2.2e-13    1.0e-15    1.9e-15    1.5e-12    4.1e-13    1.9e-11    5.0e-14
    soft-17-5         846    94.9 %    1.7e-05    4.6e-09    1.5e+04    3.6e-13    1.6e-15    2.5e-15    1.9e-12    1.1e-12    1.4e-11    6.2e-14
    soft-15-1         846     0.0 %        inf        inf    1.2e+04    1.2e-13    1.9e-15    1.9e-15    0.0e+00    7.5e-13    0.0e+00    1.4e-16
    soft-32-8         846    13.6 %    2.2e-02    2.0e-05    1.5e+04    1.9e-13    4.1e-15    4.1e-15    2.5e-12    3.6e-12    1.6e-10    2.1e-13
    soft-33-17        846    30.9 %    2.4e-03    2.2e-06    1.5e+04    2.0e-13    4.3e-15    4.3e-15    5.9e-12    2.4e-12    8.2e-11    4.2e-13
    soft-39-18        846    27.1 %    1.0e-05    2.7e-06    1.7e+04    1.5e-13    7.1e-16    7.1e-16    3.5e-12    2.7e-12    8.4e-11    2.2e-13
    ill-13-10         846    40.0 %    1.9e-03    5.1e-06    1.5e+06    3.2e-11    2.5e-13    2.5e-13    1.1e-10    4.8e-12    3.2e-10    6.2e-12
    ill-17-5          846    94.9 %    1.7e-05    4.3e-09    1.5e+06    2.5e-11    1.5e-13    1.8e-13    1.3e-10    3.7e-12    2.6e-09    2.4e-12
    ill-39-18         846    27.1 %    5.6e-06    2.0e-06    1.7e+06    1.7e-11    7.3e-14    7.3e-14    9.6e-11    9.6e-12    2.3e-09    4.1e-12
    tied-16-4         846   100.0 %    2.4e-04    2.3e-06    1.0e+04    1.3e-13    3.5e-15    3.6e-15    1.1e-12    6.6e-13    3.3e-11    3.2e-14
    tied-33-17        846    77.8 %    1.2e-04    5.2e-06    1.0e+04    1.8e-13    2.8e-15    2.8e-15    5.0e-12    2.6e-12    1.5e-09    5.4e-13
    ragged-17-5      4073    95.0 %    1.3e-04    2.6e-07    1.6e+04       -       1.0e-15    2.3e-15    3.1e-12    6.5e-12    6.4e-11    5.1e-13
Every condition holds at the first seed (SEED_SKIPS is empty).  The largest cond(Sigma_s) of the soft regime is 1.7e4:
I + a E_s adds a factor of up to 1.7 to kappa.  "logb" is the largest relative error of any single density, the scores'
errors are those of sums of hundreds of them.  The obs column is large where an entry of obs[s] is a sum of terms of
both signs that nearly cancel (every feature but the first is centred near zero): the float64 sums hold an absolute
error of about 1e-11 there, which the measure divides by the entry's own size.  The vit gap of soft-17-5 / ill-17-5
(4e-9) is relative to the score, whose own relative error is 1e-15 on both sides: six orders of room.
"""
import functools

import numpy as np

from tests import _fb_ref as F
from tests import _fullcov_ref as ref64
from tests import _full_vocab_cases as vc

LD = F.LD

A_SOFT, SEP = 0.3, 0.7
KAPPA_SOFT, KAPPA_ILL = 1e4, 1e6
SOFT_LENGTHS = (1, 2, 63, 64, 65, 40, 30, 17)
# (D, S, topology)
SOFT_SHAPES = [(5, 3, "dense"),       # padded D and S
               (13, 10, "bidiag"),    # unpadded
               (12, 4, "dense"),      # the ones column next to the last feature; a full state group
               (16, 4, "dense"),      # tile edge inside DP 26
               (17, 5, "dense"),      # tile edge inside DP 26
               (15, 1, "dense"),      # one state
               (32, 8, "bidiag"),     # tile edge inside DP 39
               (33, 17, "bidiag"),    # tile edge inside DP 39; S not a multiple of four
               (39, 18, "bidiag")]    # largest
ILL_SHAPES = [(13, 10, "bidiag"), (17, 5, "dense"), (39, 18, "bidiag")]
TIED_SHAPES = [(16, 4, "dense"), (33, 17, "bidiag")]
# (regime, D, S) -> seeds skipped because a condition failed at them, with what failed (never a loosened condition)
SEED_SKIPS = {}
RAGGED_WORD0 = (63, 1, 1, 0, 190, 1, 1)          # running total 63, 64, 65, 65, 255, 256, 257
RAGGED_WORD4 = (63, 1, 1)
RAGGED_TILES = 300


class Case:
    """name, regime, D, S, W, topology, kappa, params (per word: startprob, transmat, means, covars[S, D, D]), utts (in
    batch order: [T, D] float32), utt_model, feats, lengths, offs, vocab (scored under every word too)."""

    def __repr__(self):
        return f"<{self.name}>"


def word_model(rng, D, S, topology, kappa, a, sep=SEP):
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    lam = np.exp(rng.uniform(0.0, np.log(kappa), D))
    lam[0], lam[-1] = 1.0, kappa
    B = (Q * lam) @ Q.T
    L0 = np.linalg.cholesky((B + B.T) / 2)
    covars = np.empty((S, D, D))
    for s in range(S):
        G = rng.normal(size=(D, D)) / np.sqrt(D)
        E = np.triu(G) + np.triu(G, 1).T
        cv = L0 @ (np.eye(D) + a * E) @ L0.T
        covars[s] = (cv + cv.T) / 2
    means = np.empty((S, D))
    means[0] = rng.normal(0.0, 5.0, D)
    means[0, 0] = -300.0
    for s in range(1, S):
        means[s] = means[s - 1] + sep * (L0 @ rng.normal(size=D)) / np.sqrt(D)
    if topology == "bidiag":
        sp = np.zeros(S)
        sp[0] = 1.0
        A = np.zeros((S, S))
        stay = rng.uniform(0.5, 0.8, S)
        for i in range(S - 1):
            A[i, i], A[i, i + 1] = stay[i], 1 - stay[i]
        A[S - 1, S - 1] = 1.0
    else:
        sp = rng.dirichlet(np.full(S, 2.0))
        A = rng.dirichlet(np.full(S, 2.0), size=S)
    return sp, A, means, covars


def sample(rng, sp, A, means, chols, T):
    S, D = means.shape
    q = np.empty(T, dtype=np.int64)
    if T:
        q[0] = rng.choice(S, p=sp)
    for t in range(1, T):
        q[t] = rng.choice(S, p=A[q[t - 1]])
    z = rng.normal(size=(T, D))
    return (means[q] + np.einsum("tab,tb->ta", chols[q], z)).astype(np.float32).reshape(T, D)


def make_case(name, regime, D, S, topology, kappa, a, lengths_per_word, vocab):
    c = Case()
    c.name, c.regime, c.D, c.S, c.topology, c.kappa, c.vocab = name, regime, D, S, topology, kappa, vocab
    c.W = len(lengths_per_word)
    c.seed = 100 * D + S + 1000 * len(SEED_SKIPS.get((regime, D, S), ()))
    rng = np.random.default_rng(c.seed)
    c.params = [word_model(rng, D, S, topology, kappa, a) for _ in range(c.W)]
    rng = np.random.default_rng(c.seed + 7)
    c.utts, um = [], []
    for w, lens in enumerate(lengths_per_word):
        sp, A, mu, cv = c.params[w]
        chols = np.linalg.cholesky(cv)
        for T in lens:
            c.utts.append(sample(rng, sp, A, mu, chols, int(T)))
            um.append(w)
    c.utt_model = np.asarray(um, dtype=np.int64)
    c.feats = np.concatenate(c.utts, axis=0)
    c.lengths = np.asarray([x.shape[0] for x in c.utts], dtype=np.int64)
    c.offs = np.r_[0, np.cumsum(c.lengths)]
    for arr in (c.utt_model, c.feats, c.lengths, c.offs, *c.utts, *(p for prm in c.params for p in prm)):
        arr.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def soft(D, S, topology):
    return make_case(f"soft-{D}-{S}", "soft", D, S, topology, KAPPA_SOFT, A_SOFT, [SOFT_LENGTHS] * 3, True)


@functools.lru_cache(maxsize=None)
def ill(D, S, topology):
    return make_case(f"ill-{D}-{S}", "ill", D, S, topology, KAPPA_ILL, A_SOFT, [SOFT_LENGTHS] * 3, True)


@functools.lru_cache(maxsize=None)
def tied(D, S, topology):
    return make_case(f"tied-{D}-{S}", "tied", D, S, topology, KAPPA_SOFT, 0.0, [SOFT_LENGTHS] * 3, True)


@functools.lru_cache(maxsize=None)
def ragged():
    many = [12 + (i % 2) for i in range(RAGGED_TILES)]
    return make_case("ragged-17-5", "ragged", 17, 5, "dense", KAPPA_SOFT, A_SOFT,
                     [RAGGED_WORD0, (1,), (), many, RAGGED_WORD4], False)


def all_cases():
    """(constructor, arguments) of every case, in test order."""
    return ([(soft, s) for s in SOFT_SHAPES] + [(ill, s) for s in ILL_SHAPES] + [(tied, s) for s in TIED_SHAPES]
            + [(ragged, ())])


def vocab_cases():
    return [fa for fa in all_cases() if fa[0] is not ragged]


def emit_cases():
    return [fa for fa in all_cases() if fa[0] in (soft, ill)]


def case_id(fn_args):
    fn, args = fn_args
    return "-".join([fn.__name__] + [str(a) for a in args])


# ------------------------------------------------------------------------------------------
# the longdouble reference
# ------------------------------------------------------------------------------------------
def cholesky_ld(cov):
    """Lower L with cov = L L^T, column by column (Cholesky-Banachiewicz), in longdouble."""
    a = np.asarray(cov, dtype=LD)
    D = a.shape[0]
    L = np.zeros((D, D), dtype=LD)
    for j in range(D):
        d = a[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert d > 0, "not positive-definite"
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (a[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def log_density(X, means, covars):
    """logb[T, S] longdouble of the frames X[T, D]: -(D log 2 pi + log|Sigma_s| + |L_s^-1 (x - mu_s)|^2) / 2 by forward
    substitution."""
    X = np.asarray(X, dtype=LD)
    T, D = X.shape
    out = np.empty((T, len(means)), dtype=LD)
    for s, (mu, cv) in enumerate(zip(means, covars)):
        L = cholesky_ld(cv)
        diff = X - np.asarray(mu, dtype=LD)[None]
        y = np.empty((T, D), dtype=LD)
        for i in range(D):
            y[:, i] = (diff[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
        out[:, s] = LD(-0.5) * (D * np.log(2 * F.PI) + LD(2) * np.log(np.diag(L)).sum() + (y * y).sum(axis=1))
    return out


def viterbi(sp, A, logb):
    """tests/_fullcov_ref.viterbi over a given logb[T, S] (any float type) -> (logprob, path, gap)."""
    ls, lA = F._log(sp).astype(logb.dtype), F._log(A).astype(logb.dtype)
    T, S = logb.shape
    d = np.empty((T, S), dtype=logb.dtype)
    d[0] = ls + logb[0]
    for t in range(1, T):
        d[t] = np.max(d[t - 1][:, None] + lA, axis=0) + logb[t]
    gap = np.inf

    def take(v):
        nonlocal gap
        k = int(np.argmax(v))
        fin = np.sort(v[np.isfinite(v)])
        if fin.size >= 2:
            gap = min(gap, float((fin[-1] - fin[-2]) / abs(fin[-1])))
        return k
    path = np.empty(T, dtype=np.int64)
    path[T - 1] = take(d[T - 1])
    logprob = d[T - 1, path[T - 1]]
    for t in range(T - 2, -1, -1):
        path[t] = take(d[t] + lA[:, path[t + 1]])
    return logprob, path, gap


def utterance(X, sp, A, logb):
    """Every E-step quantity of one utterance of T >= 1 frames under one model, longdouble."""
    ll, fwd = F.forward(sp, A, logb)
    bwd = F.backward(A, logb)
    with np.errstate(invalid="ignore"):
        gamma = F._softmax(fwd + bwd, 1)
    S = logb.shape[1]
    if X.shape[0] > 1:
        with np.errstate(invalid="ignore"):
            lx = fwd[:-1, :, None] + F._log(A)[None] + (logb[1:] + bwd[1:])[:, None, :]
        trans = F._softmax(lx, (1, 2)).sum(axis=0)
    else:
        trans = np.zeros((S, S), dtype=LD)
    x = np.asarray(X, dtype=np.float32).astype(LD)
    oo = np.stack([(x * gamma[:, s:s + 1]).T @ x for s in range(S)])
    return {"ll": ll, "gamma": gamma, "start": gamma[0], "trans": trans, "post": gamma.sum(axis=0),
            "obs": gamma.T @ x, "oo": oo}


STAT_KEYS = ("start", "trans", "post", "obs", "oo")


class Result:
    """ll[N] (own model), gamma[total, S], path (MAP), top, top_gap, vit_score[N], vit_path[total], vit_gap, per-word
    stats (STAT_KEYS, logprob, nobs), and for a vocabulary case logb[W][total, S] and scores[mode][N, W]."""


def _finish(r, case, per_utt, vit, dtype):
    S, D = case.S, case.D
    r.ll = np.asarray([p["ll"] for p in per_utt], dtype=dtype)
    r.gamma = np.concatenate([p["gamma"] for p in per_utt], axis=0).reshape(-1, S)
    r.path = np.argmax(r.gamma, axis=1)
    top = np.sort(r.gamma, axis=1)
    r.top = top[:, -1]
    r.top_gap = top[:, -1] - top[:, -2] if S > 1 else np.full(r.top.shape, np.inf)
    r.vit_score = np.asarray([v[0] for v in vit], dtype=dtype)
    r.vit_path = np.concatenate([v[1] for v in vit]).astype(np.int64)
    r.vit_gap = min([v[2] for v in vit], default=np.inf)
    zero = {"start": (S,), "trans": (S, S), "post": (S,), "obs": (S, D), "oo": (S, D, D)}
    r.stats = []
    for w in range(case.W):
        mine = [p for u, p in enumerate(per_utt) if case.utt_model[u] == w and case.lengths[u]]
        st = {k: sum((p[k] for p in mine), np.zeros(zero[k], dtype=dtype)) for k in STAT_KEYS}
        st["logprob"] = sum((p["ll"] for p in mine), dtype(0))
        st["nobs"] = len(mine)
        r.stats.append(st)
    return F._freeze(r)


def _empty(S, dtype):
    return ({"ll": dtype(-np.inf), "gamma": np.zeros((0, S), dtype=dtype)},
            (dtype(-np.inf), np.zeros(0, np.int64), np.inf))


@functools.lru_cache(maxsize=None)
def reference(case):
    """The longdouble reference of a case: every utterance under its own model (all quantities) and, for a vocabulary
    case, under every other word's model (forward and Viterbi scores, and logb of every frame)."""
    r = Result()
    N, W = len(case.utts), case.W
    if case.vocab:
        r.logb = [log_density(case.feats, prm[2], prm[3]) for prm in case.params]
        r.scores = {m: np.full((N, W), -np.inf, dtype=LD) for m in vc.MODES}
    per_utt, vit = [], []
    own = {}
    if not case.vocab:
        for w in range(W):
            rows = np.concatenate([np.arange(case.offs[u], case.offs[u + 1]) for u in range(N)
                                   if case.utt_model[u] == w] + [np.zeros(0, np.int64)]).astype(np.int64)
            lb = np.empty((case.feats.shape[0], case.S), dtype=LD)
            lb[rows] = log_density(case.feats[rows], case.params[w][2], case.params[w][3])
            own[w] = lb
    for u, X in enumerate(case.utts):
        w = int(case.utt_model[u])
        lo, hi = case.offs[u], case.offs[u + 1]
        if hi == lo:
            p, v = _empty(case.S, LD)
        else:
            sp, A = case.params[w][:2]
            lb = (r.logb[w] if case.vocab else own[w])[lo:hi]
            p, v = utterance(X, sp, A, lb), viterbi(sp, A, lb)
            if case.vocab:
                for k in range(W):
                    if k == w:
                        r.scores["forward"][u, k], r.scores["viterbi"][u, k] = p["ll"], v[0]
                    else:
                        r.scores["forward"][u, k] = F.forward(*case.params[k][:2], r.logb[k][lo:hi])[0]
                        r.scores["viterbi"][u, k] = viterbi(*case.params[k][:2], r.logb[k][lo:hi])[0]
        per_utt.append(p)
        vit.append(v)
    return _finish(r, case, per_utt, vit, LD)


@functools.lru_cache(maxsize=None)
def float64_oracle(case):
    """The same quantities from tests/_fullcov_ref.py (and tests/_full_vocab_cases.ref_pair for the other words): what
    the existing GPU tests compare the kernels with.  Its deviation from reference() is E_ref."""
    r = Result()
    N, W = len(case.utts), case.W
    if case.vocab:
        x64 = case.feats.astype(np.float64)
        r.logb = [ref64.log_density(x64, prm[2], prm[3]) for prm in case.params]
        r.scores = {m: np.full((N, W), -np.inf) for m in vc.MODES}
    per_utt, vit = [], []
    for u, X in enumerate(case.utts):
        w = int(case.utt_model[u])
        prm = case.params[w]
        if X.shape[0] == 0:
            p, v = _empty(case.S, np.float64)
        else:
            e = ref64.estep_utt(X, *prm)
            p = {"ll": e["loglik"], **{k: e[k] for k in ("gamma",) + STAT_KEYS}}
            v = ref64.viterbi(X, *prm)
            if case.vocab:
                for k in range(W):
                    for m in vc.MODES:
                        r.scores[m][u, k] = (p["ll"] if m == "forward" else v[0]) if k == w else \
                            vc.ref_pair(X, case.params[k], m)
        per_utt.append(p)
        vit.append(v)
    return _finish(r, case, per_utt, vit, np.float64)


# ------------------------------------------------------------------------------------------
# the measures of the comparisons
# ------------------------------------------------------------------------------------------
def rel_err(x, want):
    """max |x - want| / |want| over the finite entries of ``want``: the measure of the rtol 1e-11 pin on log scores.
    Where ``want`` is not finite, x must equal it (else inf)."""
    x, want = np.asarray(x, dtype=LD), np.asarray(want, dtype=LD)
    fin = np.isfinite(want)
    if not np.array_equal(x[~fin], want[~fin]):
        return np.inf
    return float(np.max(np.abs(x[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0


def mixed_err(x, want):
    """max |x - want| / (1e-3 + |want|): at most 1e-9 exactly when |x - want| <= 1e-12 + 1e-9 |want| everywhere, the
    pin on posteriors and statistics (rtol 1e-9 with atol 1e-12)."""
    x, want = np.asarray(x, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.max(np.abs(x - want) / (LD(1e-3) + np.abs(want)))) if want.size else 0.0


def normwise_err(x, want):
    """max |x - want| / max |want| (0 where ``want`` is all zero and x too): the pin on every oo[s]."""
    x, want = np.asarray(x, dtype=LD), np.asarray(want, dtype=LD)
    top = np.max(np.abs(want)) if want.size else LD(0)
    if top == 0:
        return 0.0 if not np.any(x) else np.inf
    return float(np.max(np.abs(x - want)) / top)


def stat_errs(case, stats_of, want):
    """{key: error} of per-word statistics ``stats_of(w)`` (a dict with STAT_KEYS and logprob) against the reference's,
    the largest over the words (and, for oo, over the states)."""
    e = {}
    for k in ("start", "trans", "post", "obs"):
        e[k] = max(mixed_err(stats_of(w)[k], want.stats[w][k]) for w in range(case.W))
    e["oo"] = max(normwise_err(stats_of(w)["oo"][s], want.stats[w]["oo"][s])
                  for w in range(case.W) for s in range(case.S))
    e["logprob"] = max([rel_err(stats_of(w)["logprob"], want.stats[w]["logprob"]) for w in range(case.W)
                        if want.stats[w]["nobs"]], default=0.0)
    return e


@functools.lru_cache(maxsize=None)
def e_ref(case):
    """Deviation of the float64 restatement from the longdouble reference on the case's inputs, per compared quantity."""
    want, o64 = reference(case), float64_oracle(case)
    e = {"ll": rel_err(o64.ll, want.ll), "vit": rel_err(o64.vit_score, want.vit_score),
         "gamma": mixed_err(o64.gamma, want.gamma), **stat_errs(case, lambda w: o64.stats[w], want)}
    if case.vocab:
        e["logb"] = max(rel_err(a, b) for a, b in zip(o64.logb, want.logb))
        for m in vc.MODES:
            e[m] = rel_err(o64.scores[m], want.scores[m])
    return e


# ------------------------------------------------------------------------------------------
# the conditions
# ------------------------------------------------------------------------------------------
def measure(case, want):
    """The figures the conditions are about, from the longdouble reference alone."""
    conds = [float(np.linalg.cond(cv)) for prm in case.params for cv in prm[3]]
    distinct = all(not np.array_equal(prm[3][i], prm[3][j]) for prm in case.params
                   for i in range(case.S) for j in range(i))
    return {"frames": int(want.gamma.shape[0]), "soft_frames": float(np.mean(want.top < 0.9)),
            "top_gap": float(want.top_gap.min()), "vit_gap": float(want.vit_gap), "cond_max": max(conds),
            "cond_min": min(conds), "distinct": distinct,
            "ll_finite": bool(np.isfinite(want.ll[case.lengths > 0]).all())}


def check_conditions(case, want):
    """Asserted before any comparison; returns the measured figures."""
    m = measure(case, want)
    assert m["ll_finite"], (case, m)
    assert m["frames"] <= (3000 if case.regime != "ragged" else 4100), (case, m)   # (two tiles of 12-13 frames: 3750)
    assert m["top_gap"] > 1e-6, (case, m)        # the MAP path is compared on every frame
    assert m["vit_gap"] > 1e-9, (case, m)        # ... and the Viterbi path
    if case.regime in ("soft", "ragged"):
        assert m["cond_max"] <= 2e4, (case, m)
    if case.regime in ("soft", "ill", "ragged"):
        assert m["distinct"] or case.S == 1, (case, m)
    if case.regime == "soft" and case.S > 1:
        assert m["soft_frames"] >= 0.10, (case, m)
    if case.regime == "ill":
        assert m["cond_max"] >= 1e5, (case, m)
    if case.regime == "tied":
        assert all(np.array_equal(cv, prm[3][0]) for prm in case.params for cv in prm[3])
    if case.regime == "ragged":
        lens = [case.lengths[case.utt_model == w].tolist() for w in range(case.W)]
        assert np.cumsum(lens[0]).tolist() == [63, 64, 65, 65, 255, 256, 257] and lens[1] == [1] and lens[2] == []
        assert len(lens[3]) == RAGGED_TILES and set(lens[3]) == {12, 13} and np.cumsum(lens[4]).tolist() == [63, 64, 65]
        assert want.stats[2]["nobs"] == 0 and not any(np.any(want.stats[2][k]) for k in STAT_KEYS)
    return m


def table_row(case, m, e):
    cols = [f"{case.name:13s}", f"{m['frames']:6d}", f"{100 * m['soft_frames']:6.1f} %", f"{m['top_gap']:9.1e}",
            f"{m['vit_gap']:9.1e}", f"{m['cond_max']:9.1e}"]
    cols += [f"{e[k]:9.1e}" if k in e else "     -   " for k in ("logb", "ll", "vit", "gamma", "trans", "obs", "oo")]
    return "  ".join(cols)


TABLE_HEAD = "  ".join([f"{'case':13s}", "frames", "    soft", "  top-two", "  vit gap", "     cond", "     logb",
                        "   loglik", "  viterbi", "    gamma", "    trans", "      obs", "       oo"])

"""Seeded inputs of tests/test_fb_regimes_*.py: models whose states overlap with the data they are scored on.

tests/_synth.py draws the state means (trained_like_models) independently of the prototypes the utterances are built
from (synth_feature_set), so nearly every posterior is one-hot and nearly every two-candidate log-sum-exp of a
bidiagonal recursion has a gap |a - b| in the hundreds.  Here every utterance is SAMPLED from its own word model: a
state path from (startprob, transmat), then x_t = mu[q_t] + sqrt(var[q_t]) * N(0, I), cast to float32; the means form
a chain  mu[s] = mu[s-1] + sep * sqrt((var[s] + var[s-1]) / 2) * g / sqrt(D),  g ~ N(0, I),  so ``sep`` is the
distance of neighbouring states in standard deviations.  Topology and variances come from trained_like_models.

Every case has W = 3 word models and, unless stated, 16 utterances per word with T uniform in 1..109.  The conditions
each regime has to meet are computed from the longdouble reference alone (tests/_fb_ref.py) by ``check_conditions``,
which tests/test_fb_regimes_cpu.py runs for every case and the GPU tests run before they compare anything.

Measured on the CPU from the reference (models seed 5, data seed 12; "soft" = frames whose largest posterior is
below 0.9, gaps = |a - b| of the two candidates of a bidiagonal forward step with both finite, "top-two" = smallest gap
between the two largest posteriors of a frame, last column = smallest log-likelihood):
    case                           frames     soft     gaps < 2   [700, 800]    > 745     top-two    min loglik
    soft-13-8                        2748    27.7 %    27.0 %     0.0 %     0.0 %    1.1e-03   -4.44e+03
    soft-39-16                       2748    12.7 %    19.2 %     0.0 %     0.0 %    2.4e-03   -1.34e+04
    soft-13-16                       2748    41.6 %    30.0 %     0.0 %     0.0 %    9.5e-06   -4.46e+03
    soft-39-8                        2748    10.2 %    18.0 %     0.0 %     0.0 %    1.1e-02   -1.34e+04
    soft-26-5                        2748    10.3 %    17.6 %     0.0 %     0.0 %    8.7e-03   -8.89e+03
    separated-13-8                   2748     0.0 %     0.0 %     0.1 %    99.8 %    1.0e+00   -4.45e+03
    separated-39-16                  2748     0.0 %     0.0 %     0.0 %    99.8 %    1.0e+00   -1.34e+04
    clamp-13-8                       2748     0.0 %     0.0 %     2.9 %    75.8 %    1.0e+00   -4.45e+03
    clamp-39-16                      2748     0.0 %     0.0 %     2.7 %    85.5 %    1.0e+00   -1.34e+04
    far-13-8                         2748     0.0 %     0.0 %     0.0 %   100.0 %    1.0e+00   -1.92e+09
    far-39-16                        2748     0.0 %     0.0 %     0.0 %   100.0 %    1.0e+00   -5.81e+09
    long-13-8                       12454     3.4 %    12.6 %     2.0 %    26.8 %    4.9e-04   -1.70e+05
    long-39-16                       4256     5.0 %    12.9 %     0.5 %     2.9 %    2.2e-04   -1.28e+05
    structure-13-8-start_spread      2748    29.0 %    27.1 %     0.0 %     0.0 %    5.3e-04   -4.44e+03
    structure-13-8-start_state3      2748    23.6 %    27.5 %     0.0 %     0.0 %    1.0e-03   -4.46e+03
    structure-13-8-no_self_loop      2748    24.0 %    20.7 %     0.0 %     0.0 %    3.9e-03   -4.46e+03
    structure-13-8-absorbing         2748    16.8 %    21.4 %     0.0 %     0.0 %    3.6e-03   -4.50e+03
    structure-13-8-sparse            2748    88.1 %      -        -        -      3.0e-04   -4.50e+03
    structure-13-8-skips             2748    11.2 %      -        -        -      3.9e-03   -4.46e+03
    structure-13-8-no_way_in         2748    94.7 %      -        -        -      3.4e-04   -4.52e+03
    structure-39-16-start_spread     2748    13.0 %    19.2 %     0.0 %     0.0 %    2.4e-03   -1.34e+04
    structure-39-16-start_state3     2748    11.8 %    19.3 %     0.0 %     0.0 %    8.2e-03   -1.34e+04
    structure-39-16-no_self_loop     2748    10.6 %    18.4 %     0.0 %     0.0 %    2.4e-03   -1.34e+04
    structure-39-16-absorbing        2748     5.6 %    14.0 %     0.0 %     0.0 %    2.4e-03   -1.34e+04
    structure-39-16-sparse           2748    73.9 %      -        -        -      2.1e-04   -1.35e+04
    structure-39-16-skips            2748     9.3 %      -        -        -      1.6e-02   -1.34e+04
    structure-39-16-no_way_in        2748    84.1 %      -        -        -      4.4e-05   -1.35e+04
Data seed 9 gives 9.4 % soft frames at (39, 8) and 8.5 % at (26, 5) with this module's order of draws (seeds 9 .. 14:
8.9 .. 10.9 % and 8.5 .. 10.3 %), below the 10 % the soft regime asks for; seed 12 meets it at all five shapes.  The
clamp range was tuned on the CPU: 36 .. 41 gives 1.4 % of the gaps in [700, 800], 24 .. 32 gives 3.4 % / 1.7 %,
20 .. 30 gives 2.9 % / 2.7 %.  sep = 1.5 instead of 0.7 is not soft enough (tests/test_fb_regimes_cpu.py).
"""
import functools

import numpy as np

from tests._synth import trained_like_models

W = 3
N_PER_WORD = 16
MODEL_SEED, DATA_SEED = 5, 12
SEP_SOFT, SEP_SEPARATED = 0.7, 60.0
SEP_CLAMP = (20.0, 30.0)       # per state pair, uniform: tuned on the CPU so that >= 2 % of the gaps lie in [700, 800]
LONG_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 15, 16, 17, 18, 19, 63, 64, 65, 255, 256, 257, 1023, 4099]
SHIFT_FAR = np.float32(1e4)

BIDIAG_KINDS = ("start_spread", "start_state3", "no_self_loop", "absorbing")
DENSE_KINDS = ("sparse", "skips", "no_way_in")


class Case:
    """name, D, ns, S, W, bidiag, sp[W,S], A[W,S,S], mu[W,S,D], cv[W,S,D], utts (list of (T, D) float32), utt_model."""

    def __repr__(self):
        return f"<{self.name} ({self.D}, {self.ns})>"


def chain_means(mu, cv, sep, rng):
    """mu[w, 0] kept; sep a scalar or one value per (word, state pair)."""
    Wn, S, D = mu.shape
    sep = np.broadcast_to(np.asarray(sep, dtype=np.float64), (Wn, S - 1)) if np.ndim(sep) else np.full((Wn, S - 1), sep)
    out = mu.copy()
    for w in range(Wn):
        for s in range(1, S):
            g = rng.normal(0.0, 1.0, D)
            out[w, s] = out[w, s - 1] + sep[w, s - 1] * np.sqrt((cv[w, s] + cv[w, s - 1]) / 2) * g / np.sqrt(D)
    return out


def sample(rng, sp, A, mu, cv, T):
    S, D = mu.shape
    q = np.empty(T, dtype=np.int64)
    q[0] = rng.choice(S, p=sp)
    for t in range(1, T):
        q[t] = rng.choice(S, p=A[q[t - 1]])
    return (mu[q] + np.sqrt(cv[q]) * rng.normal(0.0, 1.0, (T, D))).astype(np.float32)


def soft_models(D, ns, sep, seed=MODEL_SEED):
    sp, A, mu, cv = trained_like_models(W, ns, D, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    if isinstance(sep, tuple):
        sep = rng.uniform(sep[0], sep[1], (W, ns + 1))
    return sp, A, chain_means(mu, cv, sep, rng), cv


def is_bidiagonal(A):
    """Only A[i, i] and A[i, i + 1] are non-zero (what trellis.is_bidiagonal decides the kernel route by)."""
    S = A.shape[-1]
    band = np.eye(S, dtype=bool) | np.eye(S, k=1, dtype=bool)
    return bool(np.all(A[..., ~band] == 0))


def make_case(name, D, ns, params, lengths_per_word=None, seed=DATA_SEED, shift=None):
    c = Case()
    c.name, c.D, c.ns, c.S, c.W = name, D, ns, ns + 2, W
    c.sp, c.A, c.mu, c.cv = params
    c.bidiag = is_bidiagonal(c.A)
    rng = np.random.default_rng(seed)
    if lengths_per_word is None:
        lengths_per_word = [rng.integers(1, 110, N_PER_WORD) for _ in range(W)]
    c.utts, um = [], []
    for w, lens in enumerate(lengths_per_word):
        for T in lens:
            x = sample(rng, c.sp[w], c.A[w], c.mu[w], c.cv[w], int(T))
            c.utts.append(x if shift is None else (x + shift).astype(np.float32))
            um.append(w)
    c.utt_model = np.asarray(um, dtype=np.int64)
    for a in (c.sp, c.A, c.mu, c.cv, c.utt_model, *c.utts):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def soft(D, ns, sep=SEP_SOFT):
    return make_case("soft" if sep == SEP_SOFT else f"sep{sep}", D, ns, soft_models(D, ns, sep))


@functools.lru_cache(maxsize=None)
def separated(D, ns):
    return make_case("separated", D, ns, soft_models(D, ns, SEP_SEPARATED))


@functools.lru_cache(maxsize=None)
def clamp(D, ns):
    return make_case("clamp", D, ns, soft_models(D, ns, SEP_CLAMP))


@functools.lru_cache(maxsize=None)
def far(D, ns):
    return make_case("far", D, ns, soft_models(D, ns, SEP_SOFT), shift=SHIFT_FAR)


@functools.lru_cache(maxsize=None)
def long(D, ns):
    """Words 0 and 1, each with every length of the list in that order: T = 1 and the longest share a wavefront."""
    lens = LONG_LENGTHS if (D, ns) == (13, 8) else LONG_LENGTHS[:-1]
    return make_case("long", D, ns, soft_models(D, ns, SEP_SOFT), lengths_per_word=[lens, lens, []])


def _renorm(M):
    return M / M.sum(axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def structure(D, ns, kind):
    sp, A, mu, cv = soft_models(D, ns, SEP_SOFT)
    S = ns + 2
    rng = np.random.default_rng(77)
    sp, A = sp.copy(), A.copy()
    if kind == "start_spread":
        sp[:, :3] = [0.5, 0.3, 0.2]
    elif kind == "start_state3":
        sp[:] = 0.0
        sp[:, 3] = 1.0
    elif kind == "no_self_loop":
        for s in (4, 7):
            A[:, s, s], A[:, s, s + 1] = 0.0, 1.0
    elif kind == "absorbing":
        A[:, 5, 5], A[:, 5, 6] = 1.0, 0.0
    elif kind == "sparse":            # Dirichlet rows, about 40 % of the entries zeroed (never a row's largest)
        A = rng.dirichlet(np.ones(S), (W, S))
        sp = rng.dirichlet(np.ones(S), W)
        for M in (A, sp):
            keep = M == M.max(axis=-1, keepdims=True)
            M[(rng.random(M.shape) < 0.4) & ~keep] = 0.0
        A, sp = _renorm(A), _renorm(sp)
    elif kind == "skips":             # left to right: i -> i, i + 1, i + 2
        A = np.zeros((W, S, S))
        for w in range(W):
            for i in range(S):
                n = min(3, S - i)
                A[w, i, i:i + n] = rng.dirichlet(np.ones(n))
    elif kind == "no_way_in":         # state 4: not a start state, no transition into it (its own row stays a distribution)
        A = rng.dirichlet(np.ones(S), (W, S))
        sp = rng.dirichlet(np.ones(S), W)
        A[:, :, 4] = 0.0
        sp[:, 4] = 0.0
        A, sp = _renorm(A), _renorm(sp)
    else:
        raise ValueError(kind)
    c = make_case(kind, D, ns, (sp, A, mu, cv))
    assert c.bidiag == (kind in BIDIAG_KINDS)
    return c


def reachable(sp, A):
    """States with a path from a start state (boolean [S])."""
    r = sp > 0
    while True:
        nxt = r | ((A > 0) & r[:, None]).any(axis=0)
        if (nxt == r).all():
            return r
        r = nxt


CONTAINED_COUNTS = (300, 40, 40)


@functools.lru_cache(maxsize=None)
def contained(D, ns):
    """(B, B', touched): B' is B with non-finite values in four utterances.  ``touched`` maps the utterance index to
    what was done: three utterances of word 1 (a NaN in one frame, a +inf, a -inf in the last frame) and one of word 2
    (a whole NaN frame).  The first utterances of the word with three frames or more are taken."""
    rng = np.random.default_rng(DATA_SEED + 1)
    lens = [rng.integers(1, 110, n) for n in CONTAINED_COUNTS]
    b = make_case("contained", D, ns, soft_models(D, ns, SEP_SOFT), lengths_per_word=lens)
    um = b.utt_model
    w1 = [u for u in range(len(b.utts)) if um[u] == 1 and b.utts[u].shape[0] >= 3][:3]
    w2 = [u for u in range(len(b.utts)) if um[u] == 2 and b.utts[u].shape[0] >= 3][:1]
    touched = dict(zip(w1 + w2, ("nan", "+inf", "-inf last", "nan frame")))
    bp = Case()
    vars(bp).update(vars(b))
    bp.name = "contained'"
    bp.utts = [x.copy() if u in touched else x for u, x in enumerate(b.utts)]
    for u, what in touched.items():
        x = bp.utts[u]
        T = x.shape[0]
        if what == "nan":
            x[T // 2, 3] = np.nan
        elif what == "+inf":
            x[1, D - 1] = np.inf
        elif what == "-inf last":
            x[T - 1, 0] = -np.inf
        else:
            x[T // 3, :] = np.nan
        x.setflags(write=False)
    return b, bp, touched


SOFT_SHAPES = [(13, 8), (39, 16), (13, 16), (39, 8), (26, 5)]
SHAPES = [(13, 8), (39, 16)]


def all_cases():
    """(constructor, arguments) of every case that is compared with the reference, in test order."""
    out = [(soft, s) for s in SOFT_SHAPES]
    for fn in (separated, clamp, far, long):
        out += [(fn, s) for s in SHAPES]
    out += [(structure, s + (k,)) for s in SHAPES for k in BIDIAG_KINDS + DENSE_KINDS]
    return out


def case_id(fn_args):
    fn, args = fn_args
    return "-".join([fn.__name__] + [str(a) for a in args])


def measure(case, ref):
    """The figures the conditions are about, from the longdouble reference alone."""
    g = ref.gaps
    frac = (lambda m: float(np.mean(m))) if g.size else (lambda m: float("nan"))
    return {"frames": int(ref.gamma.shape[0]), "soft_frames": float(np.mean(ref.top < 0.9)),
            "gaps_lt2": frac(g < 2), "gaps_700_800": frac((g >= 700) & (g <= 800)), "gaps_gt745": frac(g > 745),
            "top_gap": float(ref.top_gap.min()), "ll_finite": bool(np.isfinite(ref.scores).all()),
            "ll_min": float(ref.ll.min()), "one_hot": bool((ref.top == 1).all())}


def check_conditions(case, ref):
    """Asserted before any comparison; returns the measured figures."""
    m = measure(case, ref)
    assert m["ll_finite"], (case, m)
    assert m["top_gap"] > 1e-6, (case, m)            # the MAP path is compared on every frame, no exclusion rule
    if case.name == "soft":
        assert m["soft_frames"] >= 0.10 and m["gaps_lt2"] >= 0.15, (case, m)
    elif case.name == "separated":
        assert m["gaps_gt745"] >= 0.90, (case, m)
    elif case.name == "clamp":
        assert m["gaps_700_800"] >= 0.02, (case, m)
    elif case.name == "far":
        assert m["one_hot"] and m["ll_min"] < -1e8, (case, m)
    elif case.name == "long":
        lens = [X.shape[0] for X in case.utts]
        want = LONG_LENGTHS if (case.D, case.ns) == (13, 8) else LONG_LENGTHS[:-1]
        assert lens == want + want, (case, lens)
    elif case.name in BIDIAG_KINDS:
        assert is_bidiagonal(case.A)
    elif case.name in DENSE_KINDS:
        assert not is_bidiagonal(case.A)
    if case.name == "sparse":
        z = float(np.mean(case.A == 0))
        assert 0.3 <= z <= 0.5 and (case.sp == 0).any(), z
    if case.name in ("absorbing", "start_state3", "no_way_in"):
        for w in range(case.W):
            dead = ~reachable(case.sp[w], case.A[w])
            assert dead.any()
            rows = np.concatenate([np.arange(ref.offs[u], ref.offs[u + 1]) for u in range(len(case.utts))
                                   if case.utt_model[u] == w])
            assert (ref.gamma[np.ix_(rows, np.nonzero(dead)[0])] == 0).all()
    return m

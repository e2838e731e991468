"""References and case builders for the training units custom_estep.hip and custom_update.hip (numpy only; no GPU, no torch).

Parts 1-4 (folds, M-step accumulators, moments, flat-start statistics): plain ``np.longdouble`` accumulations of the
definitions in the comments above each entry point.  Features are float32 and posteriors float64, both promoted
exactly; every value comes with the sum of the absolute values of its terms, so an error is measured as
``|got - ref| / sum|terms|`` (a backward-error measure that does not blow up where a sum cancels).

Part 5 (E-step): the ground truth is ``oracle/custom_hmm_oracle.py`` in float64 — in the band
``-750 <= c0 < -678`` the reference's behaviour is DEFINED by float64 underflow, so a higher-precision reference
would describe a different function.  ``c0 = log rho - s`` (s = max alpha of the utterance, rho = the exit state's
share of the last forward row) is what custom_estep_fast_kernel classifies an utterance by.

Everything here is deterministic (fixed seeds) and cached, so the CPU test (conditions on the inputs) and the GPU test
(kernels against these references) see the same cases and build each once.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import custom_hmm_oracle as co

LD = np.longdouble
U64 = 2.0 ** -53

# ---------------------------------------------------------------------------------------------------------------
# tolerances of parts 2-4: allowance = max(pin, 4 E_64) on |got - ref| / sum|terms|
PIN_OCC = 1e-12      # occupancies, global covariance (test_g1_flat_start_on_gpu)
PIN_MOMENT = 1e-10   # first and second moments (test_stage_features_and_weighted_moments_through_the_c_abi)


def measure(got, ref, mag):
    """max over entries of |got - ref| / sum|terms| (entries without terms must be exactly zero)."""
    got = np.asarray(got, dtype=LD)
    err = np.abs(got - ref)
    live = mag > 0
    assert not np.any(err[~live]), "an entry with no terms is not exactly zero"
    return float(np.max(err[live] / mag[live])) if live.any() else 0.0


def allowance(pin, e64, n_terms=0):
    """max(pin, 4 E_64); where the project has no pin: 4 E_64 floored at n_terms 2^-53."""
    return max(pin, 4.0 * e64) if pin is not None else max(4.0 * e64, n_terms * U64)


# ---------------------------------------------------------------------------------------------------------------
# 1. fold kernels
FOLD_ROWS = (0, 1, 31, 32, 33, 127, 128, 129, 8191, 8192, 8193, 20011)
FOLD_COLS = (1, 7, 8, 9, 13, 64, 65, 112, 504, 512)
FOLD_RUNS = 128            # runs of the two-level tree (launch_fold)
FOLD_TWO_LEVEL_ROWS = 8192


def fold_branch(n_rows, K):
    """which branch of launch_fold a (n_rows, K) single-model fold takes in the default (tree) mode"""
    return "two-level" if n_rows >= FOLD_TWO_LEVEL_ROWS and (K + 7) // 8 < 64 else "single"


def fold_columns(n_rows, K):
    """(cancelling column, NaN column) of a fold case, or None where the shape has no room for it"""
    cancel = 1 if (K >= 3 and n_rows >= 2) else None
    nan = K - 1 if (K >= 2 and n_rows >= 1) else None
    return cancel, nan


def fold_case(n_rows, K):
    """part[n_rows][K]: magnitudes 1e-6 .. 1e4, both signs; one column that cancels to exactly 0 in exact arithmetic
    (pairs v, -v in shuffled rows); one column (the last: it sits in the column tail of its workgroup) with a single
    NaN row.  Returns (part, nan_row)."""
    rng = np.random.default_rng(1000003 * n_rows + K)
    part = rng.standard_normal((n_rows, K)) * 10.0 ** rng.uniform(-6, 4, (n_rows, K))
    cancel, nan = fold_columns(n_rows, K)
    nan_row = None
    if cancel is not None:
        half = n_rows // 2
        v = part[:half, cancel].copy()
        col = np.zeros(n_rows)
        col[:half], col[half:2 * half] = v, -v
        part[:, cancel] = col[rng.permutation(n_rows)]
    if nan is not None:
        nan_row = int(rng.integers(n_rows))
        part[nan_row, nan] = np.nan
    return part, nan_row


def fold_ref(part):
    """(sum, sum|x|) per column in long double.  The column is contiguous after the transpose, so numpy adds it
    pair-wise: the reference's own error is below (log2 n + 1) 2^-64 sum|x|, inside the slack u sum|x| between the
    (n - 1) u of the summation bound and the n u the test allows."""
    n_rows, K = part.shape
    ref, mag = np.zeros(K, LD), np.zeros(K, LD)
    for k0 in range(0, K, 64):
        blk = np.ascontiguousarray(part[:, k0:k0 + 64].T).astype(LD)
        ref[k0:k0 + 64] = blk.sum(axis=1)
        mag[k0:k0 + 64] = np.abs(blk).sum(axis=1)
    return ref, mag


def fold_chain(part):
    """the float64 chain acc += part[r][k] in row order (np.cumsum is one sequential chain per column whatever the
    strides; np.add.reduce turns pair-wise where a column is contiguous, as at K = 1)"""
    n_rows, K = part.shape
    acc = np.zeros(K)
    for r0 in range(0, n_rows, 4096):  # (row blocks only bound the temporary; the chain carries on through acc)
        acc = np.cumsum(np.concatenate([acc[None], part[r0:r0 + 4096]]), axis=0)[-1]
    return acc


# ---------------------------------------------------------------------------------------------------------------
# 2. / 3. M-step accumulators
class MstepCase:
    """One ragged batch: x[total][D] float32 (mean about 100, spread about 5), offsets, gamma[total][S] (rows of random
    weights normalised over the emitting states; one emitting state zero everywhere when there is more than one),
    utt_model (or None), W.  Holds one utterance of 0 frames and one of 1 frame when it has at least two."""

    def __init__(self, n_utts, S, D, W=1, empty_model=None, max_T=4, seed=0):
        rng = np.random.default_rng([n_utts, S, D, W, seed])
        lens = rng.integers(1, max_T + 1, n_utts)
        if n_utts >= 2:
            lens[n_utts // 2] = 0
            lens[n_utts - 1] = 1
        else:
            lens[0] = 1
        self.n_utts, self.S, self.D, self.W = n_utts, S, D, W
        self.lens = lens.astype(np.int64)
        self.offs = np.r_[0, np.cumsum(self.lens)].astype(np.int64)
        total = int(self.offs[-1])
        self.x = (rng.standard_normal((total, D)) * 5 + 100).astype(np.float32)
        g = rng.random((total, S)) + 0.05
        g[:, 0] = g[:, -1] = 0.0
        self.zero_state = 1 + (S - 2) // 2 if S > 3 else None
        if self.zero_state is not None:
            g[:, self.zero_state] = 0.0
        self.gamma = g / g.sum(axis=1, keepdims=True)
        self.empty_model = empty_model
        if W > 1:
            owners = [w for w in range(W) if w != empty_model]
            self.utt_model = np.array([owners[u % len(owners)] for u in range(n_utts)], dtype=np.int32)
        else:
            self.utt_model = None
        self.frame_utt = np.repeat(np.arange(n_utts), self.lens)
        self.frame_model = self.utt_model[self.frame_utt] if W > 1 else np.zeros(total, np.int64)
        self.slots = ((n_utts + 63) // 64) * 64
        self.max_T = int(self.lens.max())

    def gamma_slots(self):
        """the slot layout [max_T][S][slots]; NaN wherever no (utterance, frame) lives, so that a read past an
        utterance's end or into an empty slot poisons the result"""
        out = np.full((self.max_T, self.S, self.slots), np.nan)
        t = np.arange(len(self.frame_utt)) - self.offs[self.frame_utt]
        out[t, :, self.frame_utt] = self.gamma
        return out


def _weighted(G, Y, frame_model, W):
    """sum_f [model(f) == w] G[f][s] Y[f][k] and the same of absolute values, in long double: (W, S, K) each"""
    S, K = G.shape[1], Y.shape[1]
    val, mag = np.zeros((W, S, K), LD), np.zeros((W, S, K), LD)
    aG, aY = np.abs(G), np.abs(Y)
    for w in range(W):
        m = frame_model == w
        if m.any():
            val[w] = np.einsum("fs,fk->sk", G[m], Y[m])
            mag[w] = np.einsum("fs,fk->sk", aG[m], aY[m])
    return val, mag


def _weighted64(G, Y, frame_model, W):
    """the same in plain float64, the frames added one after another (E_64's evaluation)"""
    S, K = G.shape[1], Y.shape[1]
    val = np.zeros((W, S, K))
    for w in range(W):
        m = frame_model == w
        for s in range(S):
            if m.any() and G[m, s].any():
                val[w, s] = np.add.reduce(G[m, s, None] * Y[m], axis=0)
    return val


def sums_ref(c, f64=False):
    """sapr_custom_update_b_sums: occ[W][S], sum_x[W][S][D] (unnormalised) -> ((occ, |occ|), (sum_x, |sum_x|));
    ``f64``: the float64 frame-order evaluation instead (values only)"""
    if f64:
        v = _weighted64(c.gamma, np.c_[c.x.astype(np.float64), np.ones(len(c.x))], c.frame_model, c.W)
        return v[:, :, -1], v[:, :, :-1]
    v, m = _weighted(c.gamma.astype(LD), np.c_[c.x.astype(LD), np.ones(len(c.x), LD)], c.frame_model, c.W)
    return (v[:, :, -1], m[:, :, -1]), (v[:, :, :-1], m[:, :, :-1])


def scatter_ref(c, means, f64=False):
    """sapr_custom_update_b_scatter: scatter[W][S][D][D] = sum gamma outer(x - means[w][s], x - means[w][s])"""
    W, S, D = c.W, c.S, c.D
    T = LD if not f64 else np.float64
    val, mag = np.zeros((W, S, D, D), T), np.zeros((W, S, D, D), T)
    G, X = c.gamma.astype(T), c.x.astype(T)
    for w in range(W):
        m = c.frame_model == w
        if not m.any():
            continue
        for s in range(1, S - 1):
            g = G[m, s]
            if not g.any():
                continue
            d = X[m] - means[w, s].astype(T)
            if f64:
                val[w, s] = np.add.reduce(g[:, None, None] * (d[:, :, None] * d[:, None, :]), axis=0)
            else:
                val[w, s] = np.einsum("f,fa,fb->ab", g, d, d)
                mag[w, s] = np.einsum("f,fa,fb->ab", g, np.abs(d), np.abs(d))
    return val if f64 else (val, mag)


def means_of(c):
    """the float64 means pass 2 centres on: the long-double sums normalised and rounded once"""
    (occ, _), (sx, _) = sums_ref(c)
    out = np.zeros((c.W, c.S, c.D))
    live = occ > 0
    out[live] = (sx[live] / occ[live][:, None]).astype(np.float64)
    return out


MOM_COLS = 112


def moments_ref(c, centre, f64=False):
    """sapr_custom_update_b_moments: out[16][112]; row s (emitting states): columns 0..90 the upper triangle of
    sum g x'x'^T row by row, 91..103 sum g x', 104 sum g; x' = x - centre."""
    assert c.W == 1 and c.D == 13
    T = np.float64 if f64 else LD
    xc = c.x.astype(T) - centre.astype(T)
    iu = np.triu_indices(13)
    Y = np.concatenate([xc[:, iu[0]] * xc[:, iu[1]], xc, np.ones((len(xc), 1), T)], axis=1)
    G = c.gamma.astype(T)
    val, mag = np.zeros((16, MOM_COLS), T), np.zeros((16, MOM_COLS), T)
    aY = np.abs(Y)
    for s in range(1, c.S - 1):
        g = G[:, s]
        if not g.any():
            continue
        if f64:
            val[s, :105] = np.add.reduce(g[:, None] * Y, axis=0)
        else:
            val[s, :105] = g @ Y
            mag[s, :105] = g @ aY
    return val if f64 else (val, mag)


MOM_PARTS = (("second", slice(0, 91), PIN_MOMENT), ("first", slice(91, 104), PIN_MOMENT),
             ("occ", slice(104, 105), PIN_OCC))


@functools.lru_cache(maxsize=4)
def moments_reference(n_utts, S):
    """(case, centre, ref, mag, {part: E_64}) of one moments case, shared by the two posterior layouts"""
    c = mstep_case(n_utts, S, 13)
    centre = c.x.astype(np.float64).mean(axis=0)
    ref, mag = moments_ref(c, centre)
    f64 = moments_ref(c, centre, f64=True)
    e64 = {name: measure(f64[:, cols], ref[:, cols], mag[:, cols]) for name, cols, _ in MOM_PARTS}
    return c, centre, ref, mag, e64


# ---------------------------------------------------------------------------------------------------------------
# 4. flat-start statistics
def flat_features(total_frames, D, seed=0):
    rng = np.random.default_rng([total_frames, D, seed])
    return (rng.standard_normal((total_frames, D)) * 5 + 100).astype(np.float32)


def global_cov_ref(x, mean, f64=False):
    """sapr_custom_global_cov: the UNNORMALISED sum over frames of outer(x - mean, x - mean) (custom_hmm.py:82-92
    divides by the frame count afterwards: oracle.global_covariance)"""
    T = np.float64 if f64 else LD
    n, D = x.shape
    val, mag = np.zeros((D, D), T), np.zeros((D, D), T)
    for f0 in range(0, n, 2048):
        d = x[f0:f0 + 2048].astype(T) - mean.astype(T)
        if f64:
            val = np.add.reduce(np.concatenate([val[None], d[:, :, None] * d[:, None, :]]), axis=0)
        else:
            val += np.einsum("fa,fb->ab", d, d)
            mag += np.einsum("fa,fb->ab", np.abs(d), np.abs(d))
    return val if f64 else (val, mag)


def global_sum_chain(feats_dt):
    """custom_hmm.py:70-80 as the oracle states it: float32 pair-wise row sums, added in list order in float64"""
    acc = np.zeros(feats_dt[0].shape[0])
    for f in feats_dt:
        acc += np.sum(f, axis=1)
    return acc


# ---------------------------------------------------------------------------------------------------------------
# 5. E-step
C0_HI, C0_LO = -678.0, -750.0
XI_FRAME_CAP = 1e-3


def model_arrays(A, means, covs):
    """(means, inv, cterm, A, logA) stacked over models, as custom_hmm.py computes them per call: inverse and
    log-determinant of cov + 1e-6 I per emitting state"""
    W, S, D = means.shape
    inv, cterm = np.zeros((W, S, D, D)), np.zeros((W, S))
    cov = covs[:, 1:S - 1] + 1e-6 * np.eye(D)
    inv[:, 1:S - 1] = np.linalg.inv(cov)
    cterm[:, 1:S - 1] = D * np.log(2 * np.pi) + np.linalg.slogdet(cov)[1]
    with np.errstate(divide="ignore"):
        logA = np.log(A)
    return means.copy(), inv, cterm, A.copy(), logA


def make_models(ns, D, W, sigma, seed, zero_self_loop=True):
    """left-right models whose states sit close together (a fraction of sigma apart) with small full covariances:
    densities far above 1, so the forward scale s grows with the length of an utterance"""
    rng = np.random.default_rng([ns, D, W, seed])
    S = ns + 2
    A, means, covs = np.zeros((W, S, S)), np.zeros((W, S, D)), np.zeros((W, S, D, D))
    for w in range(W):
        A[w, 0, 1] = A[w, -1, -1] = 1.0
        for j in range(1, S - 1):
            aii = rng.uniform(0.5, 0.9)
            A[w, j, j], A[w, j, j + 1] = aii, 1.0 - aii
            means[w, j] = rng.normal(0.0, 0.3 * sigma, D)
            a = rng.normal(0.0, 0.3 * sigma, (D, D)) / np.sqrt(D)
            covs[w, j] = sigma ** 2 * (0.8 + 0.4 * rng.random()) * np.eye(D) + a @ a.T
    if zero_self_loop and S > 4:
        A[W - 1, 2, 2], A[W - 1, 2, 3] = 0.0, 1.0   # a state that is always left at once: its xi self term is skipped
    return A, means, covs


def _emission_fast(x_dt, means, inv, cterm):
    """the row-sum form with the inverses at hand: the bisection's cheap stand-in for oracle.emission"""
    S = means.shape[0]
    T = x_dt.shape[1]
    E = np.full((T, S), -np.inf)
    for j in range(1, S - 1):
        d = x_dt.astype(np.float64) - means[j, :, None]
        E[:, j] = -0.5 * (cterm[j] + d.T @ (inv[j] @ d.sum(axis=1)))
    return E


def c0_of(al, sc):
    """log rho - s from the oracle's shifted alpha and scale, in the kernel's order of operations"""
    with np.errstate(invalid="ignore"):
        ll = np.logaddexp.reduce(al[-1])
        return (al[-1, -1] + sc - (ll + sc)) - sc


def xi_totals(al, be, E, A):
    """s_t: the unnormalised total of the xi terms of every step, as oracle.xi computes it (same additions in the
    same order, np.sum pair-wise over the flattened (S, S) matrix); also returns the normalised xi so that the CPU
    test can pin this restatement to oracle.xi bit for bit"""
    T, S = al.shape
    lgA = co._log(A)
    out = np.zeros((max(T - 1, 0), S, S))
    if T < 2:
        return np.zeros(0), out
    with np.errstate(invalid="ignore", over="ignore"):
        ll = np.logaddexp.reduce(al[-1])
        a, e, b = al[:-1], E[1:], be[1:]
        out[:, 0, 1] = np.exp(a[:, 0] + lgA[0, 1] + e[:, 1] + b[:, 1] - ll)
        for i in range(1, S - 1):
            if A[i, i] > 0:
                out[:, i, i] = np.exp(a[:, i] + lgA[i, i] + e[:, i] + b[:, i] - ll)
            if i < S - 2:
                out[:, i, i + 1] = np.exp(a[:, i] + lgA[i, i + 1] + e[:, i + 1] + b[:, i + 1] - ll)
        out[:, -2, -1] = np.exp(a[:, -2] + lgA[-2, -1] + e[:, -1] + b[:, -1] - ll)
        out[:, -1, -1] = np.exp(a[:, -1] + lgA[-1, -1] + e[:, -1] + b[:, -1] - ll)
        s = np.array([np.sum(out[t]) for t in range(T - 1)])
        for t in range(T - 1):
            if s[t] > 0:
                out[t] /= s[t]
    return s, out


class Utt:
    __slots__ = ("x", "T", "w", "kind", "c0", "E", "al", "sc", "be", "gamma", "xi_sum", "ll", "s_t", "xi_allow",
                 "xi_in_oracle")


def oracle_utt(x_dt, A, means, covs):
    """the oracle's E-step of one (D, T) utterance, piece by piece (= oracle.e_step), with c0 and s_t"""
    u = Utt()
    u.x, u.T = x_dt, x_dt.shape[1]
    S = A.shape[0]
    with np.errstate(all="ignore"):
        u.E = co.emission(x_dt, means, covs)
        u.al, u.sc = co.forward(u.E, A)
        u.be = co.backward(u.E, A, u.sc)
        u.gamma = co.gamma(u.al, u.be)
        u.ll = np.logaddexp.reduce(u.al[-1])
        u.c0 = c0_of(u.al, u.sc)
        u.xi_sum = co.xi(u.al, u.be, u.E, A).sum(axis=0) if u.T > 1 else np.zeros((S, S))
        u.s_t, _ = xi_totals(u.al, u.be, u.E, A)
    # per-frame allowance on the normalised xi: each of the 2S - 2 terms is a denormal quantised to 2^-1074, the
    # device's exp may land one step off, and so may the total: 4 (2S - 2) 2^-1074 / s_t.  A step whose total is
    # exactly 0 where it need not be (every term under 2^-1075) is outside the comparison; the last step's total is
    # 0 by structure (the exit state emits -inf) on both sides.
    allow = np.full(len(u.s_t), 1e-9)
    pos = u.s_t > 0
    allow[pos] = np.maximum(1e-9, 4 * (2 * S - 2) * 2.0 ** -1074 / u.s_t[pos])
    if len(allow) > 1:
        allow[:-1][~pos[:-1]] = np.inf
    u.xi_allow = allow
    u.xi_in_oracle = bool(np.all(allow <= XI_FRAME_CAP))
    return u


def classify(c0):
    if np.isnan(c0):
        return "nan"
    if c0 == -np.inf:
        return "unreachable"
    return "smooth" if c0 >= C0_HI else ("band" if c0 >= C0_LO else "zero")


def _place(rng, T, D, A, means, inv, cterm, target, sigma):
    """an utterance of T frames whose c0 lands within 0.2 of `target`: frames drawn about the states of an even
    walk through the model, the scale nu of their noise bisected (c0 is continuous in nu: about -T log-density-peak
    at nu = 0, near 0 for large nu)"""
    S = A.shape[0]
    seg = np.minimum(np.arange(T) * (S - 2) // T, S - 3) + 1
    z = rng.standard_normal((T, D))

    def build(nu):
        return np.ascontiguousarray((means[seg] + nu * sigma * z).T.astype(np.float32))

    def c0(nu):
        with np.errstate(all="ignore"):
            al, sc = co.forward(_emission_fast(build(nu), means, inv, cterm), A)
            return c0_of(al, sc)

    # c0 need not be monotone in nu (the row-sum emission can push the last frames far down): bracket on a grid
    grid = np.linspace(0.0, 4.0, 9)
    vals = np.array([c0(nu) for nu in grid])
    below = vals < target
    ok = np.isfinite(vals)
    hit = np.flatnonzero((below[:-1] != below[1:]) & ok[:-1] & ok[1:])
    if len(hit) == 0:
        return None
    lo, hi, up = grid[hit[0]], grid[hit[0] + 1], bool(below[hit[0]])
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        v = c0(mid)
        if abs(v - target) < 0.2:
            return build(mid)
        lo, hi = (mid, hi) if (v < target) == up else (lo, mid)
    return None


class EstepBatch:
    """utterances (each against model utt_model[u]) with the oracle's results"""

    def __init__(self, ns, D, A, means, covs, utts, sigma):
        self.ns, self.S, self.D, self.W = ns, ns + 2, D, A.shape[0]
        self.A, self.means, self.covs, self.sigma = A, means, covs, sigma
        self.utts = utts
        self.n_utts = len(utts)
        self.utt_model = np.array([u.w for u in utts], dtype=np.int32)
        self.lens = np.array([u.T for u in utts], dtype=np.int64)
        self.offs = np.r_[0, np.cumsum(self.lens)].astype(np.int64)
        self.x = np.ascontiguousarray(np.concatenate([u.x.T for u in utts], axis=0), dtype=np.float32)
        self.kinds = np.array([u.kind for u in utts])
        self.c0 = np.array([u.c0 for u in utts])

    def arrays(self):
        return model_arrays(self.A, self.means, self.covs)

    def count(self, kind):
        return int(np.sum(self.kinds == kind))

    def band_frame_share_outside_oracle(self):
        band = [u for u in self.utts if u.kind == "band"]
        total = sum(len(u.xi_allow) for u in band)
        out = sum(len(u.xi_allow) for u in band if not u.xi_in_oracle)
        return out / max(total, 1)


FAST_SHAPES = ((8, 13), (16, 13), (8, 39), (16, 39))
SIGMA = 0.05


def _targets(which):
    """(lowest, highest) admissible c0 of every placed utterance of a batch; a point target has both ends equal"""
    def span(lo, hi, n):
        return [(lo, hi)] * n

    def at(v, n):
        return [(v, v)] * n
    if which == "smooth":    # every utterance in the first class: redo_count = 0
        return span(-670.0, -300.0, 124) + at(-677.5, 6)
    if which == "band":      # every utterance in the band: redo_count = n_utts
        return span(-731.0, -679.0, 118) + at(-678.5, 6) + at(-749.4, 6)
    smooth = span(-670.0, -300.0, 50) + at(-677.5, 5) + at(-677.2, 2)
    band = (span(-731.0, -680.0, 56) + at(-678.5, 5) + at(-678.8, 2) + at(-732.5, 3) + span(-748.0, -735.0, 6)
            + at(-749.4, 5) + at(-749.7, 2))
    zero = span(-1100.0, -760.0, 48) + at(-750.5, 5) + at(-751.0, 2)
    return smooth + band + zero


@functools.lru_cache(maxsize=None)
def estep_batch(ns, D, which="mixed"):
    """`mixed`: all three classes of c0 (at least 40 / 70 / 40), utterances that cannot reach the exit state, a NaN
    and an infinite feature, T = 0, 1, 2, two interleaved models one of which has a state with A[i][i] = 0, shuffled
    so that every workgroup of 64 holds every class.  `smooth` / `band`: one class only."""
    S = ns + 2
    rng = np.random.default_rng([ns, D, {"mixed": 0, "smooth": 1, "band": 2}[which]])
    A, means, covs = make_models(ns, D, 2, SIGMA, seed=5)
    _, inv, cterm, _, _ = model_arrays(A, means, covs)
    peak = [float(np.min(-0.5 * cterm[w, 1:S - 1])) for w in range(2)]   # smallest log-density peak per frame
    specs = []
    for k, (t_lo, t_hi) in enumerate(_targets(which)):
        w = k % 2
        x = None
        for _ in range(16):   # (a draw that offers no bracket for its target is drawn again)
            target = rng.uniform(t_lo, t_hi)
            # long enough for the densities to carry c0 below the target with room to spare, and to reach the exit
            T = max(S - 1 + int(rng.integers(0, 8)), int(np.ceil(-target / peak[w] * rng.uniform(1.3, 1.8))) + 2)
            x = _place(rng, T, D, A[w], means[w], inv[w], cterm[w], target, SIGMA)
            if x is not None:
                break
        assert x is not None, (ns, D, which, k, t_lo, t_hi)
        specs.append((x, w))
    if which == "mixed":
        def plain(T, w):
            seg = np.minimum(np.arange(max(T, 1)) * (S - 2) // max(T, 1), S - 3)[:T] + 1
            return np.ascontiguousarray((means[w][seg] + SIGMA * rng.standard_normal((T, D))).T.astype(np.float32))
        for T in (3, S - 3, S - 2, 5):                     # too short to reach the exit state
            specs.append((plain(min(T, S - 2), len(specs) % 2), len(specs) % 2))
        for T in (1, 2, 0):
            specs.append((plain(T, len(specs) % 2), len(specs) % 2))
        for bad in (np.nan, np.inf):
            w = len(specs) % 2
            x = plain(S + 7, w)
            x[D // 2, (S + 7) // 2] = bad
            specs.append((x, w))
    # shuffled within each model, then the two models interleaved utterance by utterance
    by_model = [rng.permutation([k for k, (_, w) in enumerate(specs) if w == m]) for m in (0, 1)]
    order = [by_model[i % 2][i // 2] for i in range(2 * min(map(len, by_model)))]
    order += [k for m in (0, 1) for k in by_model[m][len(order) // 2:]]
    utts = []
    for k in order:
        x, w = specs[k]
        if x.shape[1] == 0:
            u = Utt()
            u.x, u.T, u.c0, u.kind = x, 0, np.nan, "empty"
            u.xi_allow, u.xi_in_oracle = np.zeros(0), False
        else:
            u = oracle_utt(x, A[w], means[w], covs[w])
            u.kind = classify(u.c0)
        u.w = w
        utts.append(u)
    return EstepBatch(ns, D, A, means, covs, utts, SIGMA)


GENERIC_SHAPES = ((3, 1), (5, 12), (12, 26), (20, 40))   # (S, D)


@functools.lru_cache(maxsize=None)
def generic_batch(S, D, dense):
    """the run-time-shaped kernel alone: 70 ragged utterances of two models; `dense` = small variances (densities far
    above 1), otherwise unit-scale data"""
    ns = S - 2
    sigma = 0.05 if dense else 1.0
    rng = np.random.default_rng([S, D, int(dense)])
    A, means, covs = make_models(ns, D, 2, sigma, seed=9)
    utts = []
    for k in range(70):
        w = k % 2
        T = [0, 1, 2][k] if k < 3 else int(rng.integers(max(2, ns - 2), ns + 14))
        seg = np.minimum(np.arange(max(T, 1)) * ns // max(T, 1), ns - 1)[:T] + 1
        x = np.ascontiguousarray((means[w][seg] + rng.uniform(0.5, 2.0) * sigma * rng.standard_normal((T, D))).T
                                 .astype(np.float32))
        if T == 0:
            u = Utt()
            u.x, u.T, u.c0, u.kind = x, 0, np.nan, "empty"
            u.xi_allow, u.xi_in_oracle = np.zeros(0), False
        else:
            u = oracle_utt(x, A[w], means[w], covs[w])
            u.kind = classify(u.c0)
        u.w = w
        utts.append(u)
    return EstepBatch(ns, D, A, means, covs, utts, sigma)


# ---------------------------------------------------------------------------------------------------------------
# case lists of parts 2-4 (shared by the CPU and the GPU test)
LANE_CASES = [(n, S) for n in (1, 255, 256, 257, 700) for S in (3, 10, 18, 20)]            # one model, D = 13
GENERIC_D_CASES = [(70, 10, D) for D in (1, 12, 26, 39, 40)] + [(70, 18, 39)]              # one model, any D
MULTI_CASES = [(n, D, W) for n in (33, 64, 65, 97) for D in (13, 39) for W in (3, 4)]      # utt_model; W = 4: model 2 empty
MOM_UTTS = (1, 15, 16, 17, 63, 64, 65, 65553)
MOM_STATES = (3, 10, 16)
COV_MFMA_FRAMES = (1, 2, 3, 4, 5, 255, 32767, 32768, 32769, 32773, 100003)
COV_FALLBACK_FRAMES = (4095, 4096, 4097, 12289)
COV_FALLBACK_D = (1, 39, 40)


@functools.lru_cache(maxsize=None)
def mstep_case(n_utts, S, D, W=1):
    # (frames per utterance stay tiny where the count is large or the scatter matrix is)
    max_T = 3 if n_utts > 1000 else (4 if D <= 13 else 3)
    return MstepCase(n_utts, S, D, W, empty_model=2 if W == 4 else None, max_T=max_T)

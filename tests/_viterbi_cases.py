"""Seeded inputs of tests/test_viterbi_cases_*.py: the Viterbi decoders (sapr_viterbi_diag_scores + sapr_viterbi_backtrace,
sapr_viterbi_decode_pruned) on every kernel shape, chain structure, tie rule, summation order and division variant.

The bar of the GPU file is the project's own: float64 scores equal bit for bit, best words and state paths equal to
oracle/c_oracle.decode_batch with the same ``tie`` and ``sum_order``; no tolerance anywhere.  tests/test_viterbi_cases_cpu.py
checks, from the two CPU oracles alone, that every case is what it claims to be.

Cases (W = 3 word models; the utterances of tests/_fb_regimes.py are SAMPLED from their word model, so neighbouring states
overlap with the data and the lattice's candidates are close):

  dense-<D>-<ns>-<kind>       _fb_regimes.structure(D, ns, kind), kind in sparse / skips / no_way_in, at the four kernel
                              shapes (D, ns) = (13, 8), (39, 16), (13, 16), (39, 8); 48 utterances of 1 .. 109 frames.
  dense-13-3-no_way_in,       padded dense models: S = 5 runs in the 10-state kernel, S = 12 in the 18-state one
  dense-13-10-sparse          (at ns = 3 the state without a way in, 4, is the last real state in front of the padding).
  dense_ties-<D>-<ns>         per word every state has the same Gaussian, startprob and every transmat entry are 1 / S:
                              all S candidates of every lattice cell tie exactly.  Word w's means are shifted by w.  One
                              utterance of each length 1, 2, 3, 5, 17, 40, 64, 65 (197 frames).  TIE_LOW walks state 0,
                              TIE_HIGH state S - 1 up to the last frame (first maximum: state 0): 189 of 197 frames differ.
  bidiag-<D>-<ns>-<kind>      the four BIDIAG_KINDS of _fb_regimes (start_spread, start_state3, no_self_loop = states 4 and 7,
                              absorbing = state 5) and three more built the same way:
                                no_self_loop_48  states 4 and 8 without a self-loop (chain positions the matrix-core bounding
                                                 pass serves: PACK_GEMM_OK stays set);
                                two_chains       A[5,5] = 1, A[5,6] = 0, startprob 0.6 on state 0 and 0.4 on state 6: the
                                                 second half of the chain is reachable from the start distribution only;
                                head_and_tail    start in state 3 and A[6,6] = 1, A[6,7] = 0: states 0 .. 2 and 7 .. S - 1
                                                 are unreachable.
  bidiag_ties-<D>-<ns>        states 0 .. S - 2 of a word share one Gaussian, the last state has its own; A[i,i] = A[i,i+1]
                              = 0.5, A[S-1,S-1] = 1, start in state 0.  Utterance k (word k % 3) is T - 3 frames from the
                              shared Gaussian and then 3 from the last state's; one utterance of each length 1, 2, 3, 5, 17,
                              S, S + 1, 2 S, 40, 64, 65, 100.  Every path that reaches the same state at the same frame
                              has the same score bits up to rounding order, so the two candidates of a cell tie wherever
                              both exist: TIE_HIGH advances at once, TIE_LOW stays in state 0 until it must leave.  The four
                              shapes and a padded (13, ns = 3).
  long-<D>-<ns>               _fb_regimes.long: (13, 8) up to 4099 frames, (39, 16) up to 1023, T = 1 in the same wavefront
  long_dense-<D>-<ns>         as the longest; the dense twin has the same models and data with "skips" transition matrices.
  contained(D, ns, dense)     _fb_regimes.contained: batch B, and B' with NaN / +inf / -inf in four utterances.

MEASURED on the CPU from the C oracle (tests/test_viterbi_cases_cpu.py prints them): frames on which the best word's
TIE_HIGH and TIE_LOW paths differ — dense ties 189 of 197 at every shape; bidiagonal ties 276 of 338 at S = 10, 280 of
370 at S = 18, 266 of 318 at S = 5 (every utterance of S frames or more ends in the last state; between its first frame
and its entry into state S - 2 the two rules' paths differ).  The condition asserted is "at least half".
"""
import functools

import numpy as np

from tests import _fb_regimes as R
from tests._synth import trained_like_models

SHAPES = [(13, 8), (39, 16), (13, 16), (39, 8)]
NEW_BIDIAG_KINDS = ("no_self_loop_48", "two_chains", "head_and_tail")
BIDIAG_KINDS = R.BIDIAG_KINDS + NEW_BIDIAG_KINDS
DENSE_KINDS = R.DENSE_KINDS
PADDED_DENSE = [(13, 3, "no_way_in"), (13, 10, "sparse")]
DENSE_TIE_LENGTHS = [1, 2, 3, 5, 17, 40, 64, 65]
TIE_SEED = 31

# states no path from the start distribution reaches, per structure kind (checked with _fb_regimes.reachable)
DEAD_STATES = {
    "start_state3": lambda S: [0, 1, 2],
    "absorbing": lambda S: list(range(6, S)),
    "head_and_tail": lambda S: [0, 1, 2] + list(range(7, S)),
    "no_way_in": lambda S: [4],
}


def bidiag_tie_lengths(S):
    return [1, 2, 3, 5, 17, S, S + 1, 2 * S, 40, 64, 65, 100]


@functools.lru_cache(maxsize=None)
def structure(D, ns, kind):
    """_fb_regimes.structure, and the three bidiagonal kinds added here (same models, same data seed)."""
    if kind not in NEW_BIDIAG_KINDS:
        return R.structure(D, ns, kind)
    sp, A, mu, cv = R.soft_models(D, ns, R.SEP_SOFT)
    sp, A = sp.copy(), A.copy()
    if kind == "no_self_loop_48":
        for s in (4, 8):
            A[:, s, s], A[:, s, s + 1] = 0.0, 1.0
    elif kind == "two_chains":
        A[:, 5, 5], A[:, 5, 6] = 1.0, 0.0
        sp[:] = 0.0
        sp[:, 0], sp[:, 6] = 0.6, 0.4
    else:
        sp[:] = 0.0
        sp[:, 3] = 1.0
        A[:, 6, 6], A[:, 6, 7] = 1.0, 0.0
    c = R.make_case(kind, D, ns, (sp, A, mu, cv))
    assert c.bidiag
    return c


def _with_transmat(case, name, A):
    """The same models and utterances under other transition matrices."""
    c = R.Case()
    vars(c).update(vars(case))
    c.name, c.A, c.bidiag = name, A, R.is_bidiagonal(A)
    return c


@functools.lru_cache(maxsize=None)
def long(D, ns, dense=False):
    c = R.long(D, ns)
    return _with_transmat(c, "long_dense", structure(D, ns, "skips").A) if dense else c


@functools.lru_cache(maxsize=None)
def contained(D, ns, dense=False):
    """(B, B', touched) of _fb_regimes.contained; ``dense``: under the "skips" transition matrices."""
    b, bp, touched = R.contained(D, ns)
    if dense:
        A = structure(D, ns, "skips").A
        b, bp = _with_transmat(b, "contained_dense", A), _with_transmat(bp, "contained_dense'", A)
    return b, bp, touched


def _finish(name, D, ns, sp, A, mu, cv, utts, um):
    c = R.Case()
    c.name, c.D, c.ns, c.S, c.W = name, D, ns, ns + 2, R.W
    c.sp, c.A, c.mu, c.cv = sp, A, mu, cv
    c.bidiag = R.is_bidiagonal(A)
    c.utts, c.utt_model = utts, np.asarray(um, dtype=np.int64)
    for a in (c.sp, c.A, c.mu, c.cv, c.utt_model, *c.utts):
        a.setflags(write=False)
    return c


def _draw(rng, mu, cv, T):
    return mu + np.sqrt(cv) * rng.normal(0.0, 1.0, (T, mu.shape[0]))


@functools.lru_cache(maxsize=None)
def dense_ties(D, ns):
    S = ns + 2
    _, _, mu, cv = trained_like_models(R.W, ns, D, seed=TIE_SEED)
    mu = np.repeat(mu[0, 1][None, None, :], R.W, 0).repeat(S, 1) + np.arange(R.W, dtype=np.float64)[:, None, None]
    cv = np.repeat(cv[0, 1][None, None, :], R.W, 0).repeat(S, 1)
    sp = np.full((R.W, S), 1.0 / S)
    A = np.full((R.W, S, S), 1.0 / S)
    rng = np.random.default_rng(TIE_SEED + 1)
    utts, um = [], []
    for k, T in enumerate(DENSE_TIE_LENGTHS):
        w = k % R.W
        utts.append(_draw(rng, mu[w, 0], cv[w, 0], T).astype(np.float32))
        um.append(w)
    return _finish("dense_ties", D, ns, sp, A, mu, cv, utts, um)


@functools.lru_cache(maxsize=None)
def bidiag_ties(D, ns):
    S = ns + 2
    _, _, m0, c0 = trained_like_models(R.W, ns, D, seed=TIE_SEED)
    mu, cv = m0.copy(), c0.copy()
    mu[:, :S - 1], cv[:, :S - 1] = m0[:, 1:2], c0[:, 1:2]          # states 0 .. S-2 share state 1's Gaussian
    # the last state two standard deviations away per dimension: the closing three frames pull the path into it
    mu[:, S - 1] = m0[:, 1] + 2.0 * np.sqrt(c0[:, 1]) * np.sign(m0[:, S - 1] - m0[:, 1])
    sp = np.zeros((R.W, S))
    sp[:, 0] = 1.0
    A = np.zeros((R.W, S, S))
    for i in range(S - 1):
        A[:, i, i] = A[:, i, i + 1] = 0.5
    A[:, S - 1, S - 1] = 1.0
    rng = np.random.default_rng(TIE_SEED + 2)
    utts, um = [], []
    for k, T in enumerate(bidiag_tie_lengths(S)):
        w = k % R.W
        head = _draw(rng, mu[w, 0], cv[w, 0], max(T - 3, 0))
        tail = _draw(rng, mu[w, S - 1], cv[w, S - 1], min(T, 3))
        utts.append(np.concatenate([head, tail], axis=0).astype(np.float32))
        um.append(w)
    return _finish("bidiag_ties", D, ns, sp, A, mu, cv, utts, um)


def dense_cases():
    """(constructor, arguments) of every case of the dense route, in test order."""
    out = [(structure, s + (k,)) for s in SHAPES for k in DENSE_KINDS]
    out += [(structure, p) for p in PADDED_DENSE]
    out += [(dense_ties, s) for s in SHAPES]
    out += [(long, s + (True,)) for s in R.SHAPES]
    return out


def bidiag_cases():
    out = [(structure, s + (k,)) for s in SHAPES for k in BIDIAG_KINDS]
    out += [(bidiag_ties, s) for s in SHAPES + [(13, 3)]]
    out += [(long, s) for s in R.SHAPES]
    return out


def case_id(fn_args):
    fn, args = fn_args
    if fn is structure:
        return f"{'dense' if args[2] in DENSE_KINDS else 'bidiag'}-{args[0]}-{args[1]}-{args[2]}"
    if fn is long:
        return f"long{'_dense' if len(args) > 2 and args[2] else ''}-{args[0]}-{args[1]}"
    return f"{fn.__name__}-{args[0]}-{args[1]}"


def make(fn_args):
    fn, args = fn_args
    return fn(*args)


def is_tie_case(case):
    return case.name in ("dense_ties", "bidiag_ties")


def packed(case):
    feats = np.concatenate(case.utts, axis=0)
    offs = np.r_[0, np.cumsum([u.shape[0] for u in case.utts])].astype(np.int64)
    return feats, offs


_ORACLE = {}


def oracle(case, tie, sum_order=1):
    """c_oracle.decode_batch of the whole case: (scores [N, W], best_word [N], path [frames]); computed once, read-only."""
    key = (id(case), tie, sum_order)
    if key not in _ORACLE:
        from oracle import c_oracle
        feats, offs = packed(case)
        out = c_oracle.decode_batch(feats, offs, case.sp, case.A, case.mu, case.cv, tie=1 if tie == "high" else 0,
                                    sum_order=sum_order)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = (case, out)          # (the case is kept alive: its id stays its own)
    return _ORACLE[key][1]


def numpy_viterbi(X, sp, A, mu, cv, ties=("high", "low")):
    """hmmlearn_oracle.decode with the lattice rows evaluated as whole-array numpy operations (the same individually
    rounded additions and exact maxima as its per-state loop; tests/test_viterbi_cases_cpu.py compares the two) →
    (log_prob, {tie: states}).  ``X`` in the layout whose summation order is wanted (hmmlearn_oracle.log_density_diag)."""
    from oracle import hmmlearn_oracle as ho
    logB = ho.log_density_diag(X, mu, cv)
    with np.errstate(divide="ignore"):
        ls, lA = np.log(sp), np.log(A)
    T, S = logB.shape
    d = np.empty((T, S))
    d[0] = ls + logB[0]
    for t in range(1, T):
        d[t] = (d[t - 1][:, None] + lA).max(axis=0) + logB[t]
    last = int(np.argmax(d[T - 1]))
    out = {}
    for tie in ties:
        st = np.empty(T, dtype=np.int64)
        st[T - 1] = prev = last
        for t in range(T - 2, -1, -1):
            v = d[t] + lA[:, prev]
            prev = int(np.argmax(v)) if tie == "low" else S - 1 - int(np.argmax(v[::-1]))   # first / last maximum
            st[t] = prev
        out[tie] = st
    return float(d[T - 1, last]), out

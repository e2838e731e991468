"""float64 numpy restatement of the initialisation ``GaussianHMM.fit`` and ``GMMHMM.fit`` run from scratch (never imported
by ``sapr_amd``), and the cases of tests/test_init_*.py.

hmmlearn is not installed where these tests run: THIS RESTATEMENT IS THE REFERENCE.  It is written from the rules the
class docstrings of ``sapr_amd.hmmlearn_hmm.GaussianHMM`` and ``sapr_amd.gmm_hmm.GMMHMM`` and DESIGN.md §8 state
(hmmlearn 0.3.x ``_init`` with this project's k-means in place of scikit-learn's), not from the code under test:

``GaussianHMM``, ``rs = RandomState(random_state)``, S = ``n_components``:
  * ``startprob_ = rs.dirichlet(full(S, 1/S))``, ``transmat_ = rs.dirichlet(full(S, 1/S), size=S)``, then ONE integer
    ``rs.randint(2^31 - 1)`` seeds the k-means
  * ``means_``: ``_kmeans_ref.kmeans_seeded(X, S, n_init=10, seed)``, the centres of the best restart
  * ``cv = np.cov(X64.T) + min_covar I``: diag ``tile(var(X, ddof=1) + min_covar)``, tied ``cv``, full ``tile(cv)``,
    spherical ``tile(cv.mean())`` — the mean over all D x D entries
``GMMHMM``, M = ``n_mix``: the same ``s`` / ``t`` draws, then one integer for stage 1 and S more, one per state, for stage
  2; ``weights_ = 1/M``; ``covars_ = tile(var(X, ddof=1) + min_covar, (S, M, 1))``; stage 1 = the k-means above with K =
  S; every frame gets the label of its nearest final centre; stage 2 = per state a k-means with K = M over that state's
  frames in frame order.

Best-restart ties.  With ten restarts two may reach the same optimum; which of them wins, and with it the order of the
states, then hangs on the last bits of the inertias.  :func:`search_random_state` looks among the first 50
``random_state`` values for one whose best restart wins by a relative margin above 1e-9 at every stage; the value found
is committed in GAUSSIAN_RANDOM_STATE / GMM_RANDOM_STATE.  Cases for which none exists carry ``None`` there and a fixed value in
FALLBACK_RANDOM_STATE: the GPU test then accepts equality with the restatement continued from ANY ONE of the tied restarts
(:func:`gaussian_candidates`, :func:`gmm_candidates`).  Cases that needed that, as measured on the CPU
(tests/test_init_cpu.py prints the margins):
  * the Gaussian cases found a value: d13 ``random_state=1`` (margin 5.6e-2; 0 and 2..7 tie), d5 ``random_state=0``
    (3.5e-4)
  * gmm-3-2 and gmm-4-1 NEEDED THE TIE RULE: none of the 50 values gives a clear margin at every stage.  On the recipe's
    words (eight well-separated segments) several of the ten restarts reach the same optimum at stage 1 with K = 3 or 4
    (margins 0 or about 1e-16), and stage 2 — two clusters over 82 to 122 frames, or ONE cluster at ``n_mix=1``, where
    all ten restarts reach the state's mean by construction — ties at every state.  The tied restarts hold the same
    centres in another order (the same centres at ``n_mix=1``), and every inertia outside the tied set is more than
    1e-6 away from it (:func:`tie_set_is_clear`), so the rule admits a permutation of states or mixtures, nothing else.
"""
import functools

import numpy as np

from tests import _kmeans_ref as ref

N_INIT = 10
MARGIN = 1e-9
MIN_COVAR = 1e-3

# (name, word of the recipe, D, n_components) x covariance type -> random_state (None: the tie rule, see the docstring)
COVARIANCE_TYPES = ("diag", "tied", "full", "spherical")
GAUSSIAN_WORDS = {"d13": (1, 13, 5), "d5": (4, 5, 3)}
GAUSSIAN_RANDOM_STATE = {"d13": 1, "d5": 0}
# name -> (word, D, n_components, n_mix)
GMM_CASES = {"gmm-3-2": (2, 13, 3, 2), "gmm-4-1": (5, 13, 4, 1)}
GMM_RANDOM_STATE = {"gmm-3-2": None, "gmm-4-1": None}
FALLBACK_RANDOM_STATE = 0


def word(g, D):
    """(X float32 [n, D], utterance lengths) of word g of the k-means recipe."""
    return ref.recipe_groups(D)[g], list(ref.recipe_lengths(D)[g])


def draws(random_state, S, n_seeds):
    """-> (startprob, transmat, [n_seeds k-means seeds]) in the order the initialisers draw them."""
    rs = np.random.RandomState(random_state)
    sp = rs.dirichlet(np.full(S, 1.0 / S))
    tm = rs.dirichlet(np.full(S, 1.0 / S), size=S)
    return sp, tm, [int(rs.randint(np.iinfo(np.int32).max)) for _ in range(n_seeds)]


def seed_of_preset_topology(random_state):
    """The k-means seed of a model whose ``startprob_`` and ``transmat_`` are preset and not in ``init_params``: the
    stream's FIRST integer (the ``s`` / ``t`` draws that would precede it are not made)."""
    return int(np.random.RandomState(random_state).randint(np.iinfo(np.int32).max))


def data_cov(X, min_covar=MIN_COVAR):
    X64 = np.asarray(X, dtype=np.float64)
    return np.cov(X64.T).reshape(X64.shape[1], X64.shape[1]) + min_covar * np.eye(X64.shape[1])


def covars(X, S, covariance_type, min_covar=MIN_COVAR):
    """``_covars_`` in hmmlearn's shape for the type."""
    X64 = np.asarray(X, dtype=np.float64)
    if covariance_type == "diag":
        return np.tile(np.var(X64, axis=0, ddof=1) + min_covar, (S, 1))
    cv = data_cov(X64, min_covar)
    if covariance_type == "tied":
        return cv
    if covariance_type == "full":
        return np.tile(cv, (S, 1, 1))
    if covariance_type == "spherical":
        return np.tile(cv.mean(), S)
    raise ValueError(covariance_type)


def gaussian_init(X, S, covariance_type, random_state, min_covar=MIN_COVAR):
    """-> dict(startprob, transmat, covars, km: the ``kmeans_seeded`` dict behind ``means_``)."""
    sp, tm, (seed,) = draws(random_state, S, 1)
    return dict(startprob=sp, transmat=tm, covars=covars(X, S, covariance_type, min_covar),
                km=ref.kmeans_seeded(X, S, N_INIT, seed))


def gaussian_candidates(init):
    """The ``means_`` the tie rule admits: the centres of every restart within 1e-9 of the best inertia."""
    return [init["km"]["runs"][r]["centers"] for r in init["km"]["tied"]]


def final_labels(X, centres):
    """-> (labels under the final centres, the smallest non-zero relative gap of that assignment)."""
    labels, _, dist = ref.step(np.asarray(X, dtype=np.float64), centres)
    gaps = ref.relative_gaps(dist)
    return labels, (gaps[gaps > 0].min() if (gaps > 0).any() else np.inf)


def gmm_stage2(X, labels, S, M, seeds):
    """-> one ``kmeans_seeded`` dict per state over the state's frames in frame order."""
    X = np.asarray(X)
    return [ref.kmeans_seeded(X[labels == s], M, N_INIT, seeds[s]) for s in range(S)]


def gmm_init(X, S, M, random_state, min_covar=MIN_COVAR):
    """-> dict(startprob, transmat, weights, covars, stage1 (``kmeans_seeded``), labels, label_gap, stage2 (list over
    the states), means [S, M, D] from the best restarts, margins (stage 1 first), seeds)."""
    sp, tm, seeds = draws(random_state, S, 1 + S)
    X64 = np.asarray(X, dtype=np.float64)
    s1 = ref.kmeans_seeded(X, S, N_INIT, seeds[0])
    labels, gap = final_labels(X, s1["runs"][s1["best"]]["centers"])
    if np.bincount(labels, minlength=S).min() < max(M, 2):
        raise ValueError("a label group holds fewer frames than the second stage needs")
    s2 = gmm_stage2(X, labels, S, M, seeds[1:])
    return dict(startprob=sp, transmat=tm, weights=np.full((S, M), 1.0 / M),
                covars=np.tile(np.var(X64, axis=0, ddof=1) + min_covar, (S, M, 1)), stage1=s1, labels=labels,
                label_gap=gap, stage2=s2, means=np.stack([k["runs"][k["best"]]["centers"] for k in s2]),
                margins=[s1["margin"]] + [k["margin"] for k in s2], seeds=seeds)


def gmm_candidates(X, init):
    """The tie rule for ``means_[S, M, D]``: for every tied stage-1 restart, per state the centres of every tied stage-2
    restart -> list over the stage-1 restarts of list over the states of list of [M, D] arrays."""
    S, M = init["weights"].shape
    out = []
    for r in init["stage1"]["tied"]:
        if r == init["stage1"]["best"]:
            s2 = init["stage2"]
        else:
            labels, _ = final_labels(X, init["stage1"]["runs"][r]["centers"])
            s2 = gmm_stage2(X, labels, S, M, init["seeds"][1:])
        out.append([[k["runs"][t]["centers"] for t in k["tied"]] for k in s2])
    return out


def runs_are_clear(km):
    """What the comparison of a k-means result rests on: gaps above 1e-8 and no centre shift near the threshold, in
    every restart."""
    return all(r["min_gap"] > 1e-8 and all(s == 0.0 or s >= 2 * r["threshold"] for s in r["shifts"])
               for r in km["runs"])


def tie_set_is_clear(km):
    """Every restart is either within 1e-9 of the best inertia or more than 1e-6 away from it."""
    ri = np.array([r["inertia"] for r in km["runs"]])
    rel = (ri - ri.min()) / ri.min()
    return bool(((rel <= MARGIN) | (rel > 1e-6)).all())


def search_random_state(margins_of, limit=50):
    """The first ``random_state`` below ``limit`` for which ``margins_of(random_state)`` (None: unusable) all exceed
    1e-9; None when there is none."""
    for rs in range(limit):
        m = margins_of(rs)
        if m is not None and min(m) > MARGIN:
            return rs
    return None


@functools.lru_cache(maxsize=None)
def gaussian_case(name, covariance_type):
    g, D, S = GAUSSIAN_WORDS[name]
    X, lengths = word(g, D)
    rs = GAUSSIAN_RANDOM_STATE[name]
    return X, lengths, S, gaussian_init(X, S, covariance_type, FALLBACK_RANDOM_STATE if rs is None else rs)


@functools.lru_cache(maxsize=None)
def gmm_case(name):
    g, D, S, M = GMM_CASES[name]
    X, lengths = word(g, D)
    rs = GMM_RANDOM_STATE[name]
    return X, lengths, S, M, gmm_init(X, S, M, FALLBACK_RANDOM_STATE if rs is None else rs)


# ---- mixed batches -----------------------------------------------------------------------------------------------------
MIXED_WORDS = (0, 3, 6, 9)
MIXED_S = 5
MIXED_SCALE = 10000   # model 1's data is this much wider: a threshold from the wrong model's moments shows
MIXED_RANDOM_STATE = (10, 11, 12, 13)
GMM_MIXED = ((7, 3), (8, 4), (10, 3))     # (word, n_components); n_mix = 2


def mixed_data(D=13):
    """``data[w] = (X_w, lengths_w)`` of the four-model batch: model 0 fully preset, 1 needs ``c`` only, 2 ``m`` only,
    3 everything."""
    out = []
    for i, g in enumerate(MIXED_WORDS):
        X, lengths = word(g, D)
        X = X.copy()
        if i == 1:
            X = (X * np.float32(MIXED_SCALE)).astype(np.float32)
        out.append((X, lengths))
    return out

"""hmmlearn-shaped Gaussian-mixture HMM (``hmmlearn.hmm.GMMHMM``, diagonal covariances) over the HIP kernels of
``csrc/gmm_hmm.hip``: S states, M components per state, D features.

hmmlearn is not a dependency (it is not installed where this is built): the class below restates hmmlearn 0.3.x's
``GMMHMM`` from knowledge of it, like :class:`sapr_amd.hmmlearn_hmm.GaussianHMM`.  The E-step, the
posteriors and both decoders run in ``libsapr_hip.so`` (``sapr_gmm_estep_diag``, ``sapr_gmm_viterbi_diag``); the M-step
(:func:`gmm_m_step`, numpy float64), the convergence monitor and the bookkeeping of hmmlearn's initialisation run on the
host, its two k-means stages on the device (:mod:`sapr_amd.kmeans`).

Two deliberate rules sit on top of hmmlearn's M-step formulas:

* EMPTY COMPONENT: a component whose mean denominator ``means_weight + post_mix`` is exactly 0 keeps its previous mean
  and covariance (its weight becomes 0 through the weights rule) — the k-means rule "an empty cluster keeps its
  centre" again; the plain formula is 0 / 0;
* VARIANCE FLOOR: after the formula ``covars_ = max(covars_, min_covar)`` — a component that owns one frame would
  otherwise collapse to a zero variance.

Anything else non-finite propagates; nothing is repaired.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np

from . import _lib
from .hmmlearn_hmm import (DECODER_ALGORITHMS, ConvergenceMonitor, check_random_state, kmeans_seed, m_step,
                           map_decode_host)
from .tile_family import (VOCAB_MODES, TileBatch, VocabPack, VocabScores, _features_f32,  # noqa: F401  (re-exported)
                          _vocab_scores, baum_welch, pack_head, stats_head, vocab_features)

MAX_STATES, MAX_MIX, MAX_DIMS = 18, 8, 39


def _torch():
    import torch
    return torch


# ------------------------------------------------------------------------------------------
# the C ABI: sizes, pack, launches
# ------------------------------------------------------------------------------------------
def stats_width(S, M, D) -> int:
    n = C.c_int32(0)
    _lib.check(_lib.load().sapr_gmm_stats_width(S, M, D, C.byref(n)), "sapr_gmm_stats_width")
    return int(n.value)


def pack_layout(S, M, D):
    """(SP, MP, DP, doubles per model): the padded shape the kernels run (S, M, D) at."""
    sp, mp, dp, n = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_size_t(0)
    _lib.check(_lib.load().sapr_gmm_pack_layout(S, M, D, C.byref(sp), C.byref(mp), C.byref(dp), C.byref(n)),
               "sapr_gmm_pack_layout")
    return int(sp.value), int(mp.value), int(dp.value), int(n.value)


def pack_models(params, S=None) -> np.ndarray:
    """``params``: W tuples ``(startprob[S_w], transmat[S_w, S_w], weights[S_w, M], means[S_w, M, D], covars[S_w, M,
    D])`` that share M and D -> the kernels' operand block ``[W, doubles_per_model]`` float64 for ``S >= max S_w``
    kernel states (include/sapr_hip.h).  States beyond a model's own are unreachable (log start and log transitions
    -inf) and emit nothing (every component switched off)."""
    W = len(params)
    M, D = np.asarray(params[0][3]).shape[1:]
    S = max(int(np.asarray(p[0]).shape[0]) for p in params) if S is None else int(S)
    SP, MP, DP, n = pack_layout(S, M, D)
    out = np.zeros((W, n))
    with np.errstate(divide="ignore"):
        for w, (sp, tm, wt, mu, cv) in enumerate(params):
            sp, tm, wt, mu, cv = (np.asarray(a, dtype=np.float64) for a in (sp, tm, wt, mu, cv))
            s = sp.shape[0]
            if tm.shape != (s, s) or wt.shape != (s, M) or mu.shape != (s, M, D) or cv.shape != (s, M, D) or s > S:
                raise ValueError("pack_models: the models must share n_mix and the feature width")
            cc = np.full((SP, MP), -np.inf)
            cc[:s, :M] = np.log(wt) - 0.5 * (D * np.log(2 * np.pi) + np.log(cv).sum(axis=-1))
            prm = np.zeros((SP, DP, MP, 2))
            prm[:s, :D, :M, 0] = mu.transpose(0, 2, 1)
            prm[:s, :D, :M, 1] = (-0.5 / cv).transpose(0, 2, 1)
            out[w] = np.concatenate([pack_head(sp, tm, SP), cc.ravel(), prm.ravel()])
    return out


def split_stats(row, S, M, D, S_model=None):
    """One model's row of ``sapr_gmm_estep_diag``'s statistics (kernel state count S) -> a dict for the model's own
    ``S_model <= S`` states (the padding states carry exact zeros)."""
    row = np.asarray(row, dtype=np.float64)
    m = S if S_model is None else S_model
    st, o = stats_head(row, S, m)
    post_mix = row[o:o + S * M].reshape(S, M)[:m].copy()
    o += S * M
    obs = row[o:o + S * M * D].reshape(S, M, D)[:m].copy()
    o += S * M * D
    obs2 = row[o:o + S * M * D].reshape(S, M, D)[:m].copy()
    return {**st, "post_mix": post_mix, "obs": obs, "obs**2": obs2}


class GmmBatch(TileBatch):
    """The :class:`sapr_amd.tile_family.TileBatch` of the mixtures: the utterances under the model ``utt_model[u]`` of W
    models of S kernel states and M components (``sapr_gmm_estep_diag``, ``sapr_gmm_viterbi_diag``)."""
    STATS_WIDTH, WORKSPACE_BYTES = "sapr_gmm_stats_width", "sapr_gmm_workspace_bytes"
    ESTEP, VITERBI = "sapr_gmm_estep_diag", "sapr_gmm_viterbi_diag"
    pack_layout = staticmethod(pack_layout)

    def __init__(self, feats, lengths, utt_model, W, S, M):
        self.M = int(M)
        super().__init__(feats, lengths, utt_model, W, S)

    @staticmethod
    def dims(o):
        return o.W, o.S, o.M, o.D


# ------------------------------------------------------------------------------------------
# scoring over the vocabulary: every utterance under every word model in one launch
# ------------------------------------------------------------------------------------------
class GmmPack(VocabPack):
    """A vocabulary's operand block ready for the kernels: ``data`` float64 ``[W, doubles_per_model]``
    (:func:`pack_models`) with the shape it was packed for (W models, S kernel states = the largest model's, M
    components, D features) and each model's own state count ``n_states``; the device copy is made once."""

    def __init__(self, data, S, M, D, n_states=None):
        self.M = int(M)
        super().__init__(data, S, D, pack_layout(int(S), self.M, int(D))[3], n_states)

    @staticmethod
    def from_params(params) -> "GmmPack":
        """``params``: W tuples as :func:`pack_models` takes them; padded to the largest S of the vocabulary."""
        if len(params) == 0:
            raise ValueError("empty vocabulary")
        n_states = [int(np.asarray(p[0]).shape[0]) for p in params]
        M, D = (int(k) for k in np.asarray(params[0][3]).shape[1:])
        return GmmPack(pack_models(params, max(n_states)), max(n_states), M, D, n_states)

    @staticmethod
    def from_models(models) -> "GmmPack":
        """A list of fitted :class:`GMMHMM` objects that share ``n_mix`` and the feature width."""
        for m in models:
            m._check()
        return GmmPack.from_params([m._params() for m in models])

    def batch(self, feats, lengths, utt_model) -> GmmBatch:
        """The utterances under ONE model each (``utt_model[u]``) of this vocabulary."""
        return GmmBatch(feats, lengths, utt_model, self.W, self.S, self.M)

    def launch(self, feats, offsets, order, N, max_T, mode, score, best_word, word_post):
        _lib.check(_lib.load().sapr_gmm_vocab_diag(
            _lib.ptr(feats), _lib.ptr(offsets), _lib.ptr(order), N, int(feats.shape[0]), self.D, max_T,
            _lib.ptr(self.device(feats.device)), self.W, self.S, self.M, VOCAB_MODES[mode], _lib.ptr(score),
            _lib.ptr(best_word), _lib.ptr(word_post), _lib.current_stream()), "sapr_gmm_vocab_diag")

    def vocab_scores(self, batch_or_feats, lengths=None, mode="forward", want_post=False) -> "VocabScores":
        return vocab_scores(batch_or_feats, lengths, self, mode=mode, want_post=want_post)


def vocab_scores(batch_or_feats, lengths, pack_or_models, mode="forward", want_post=False) -> VocabScores:
    """Every utterance under EVERY word model in one launch of ``sapr_gmm_vocab_diag``: ``mode="forward"`` gives the
    forward log-likelihoods (``GMMHMM.score`` per sequence), ``mode="viterbi"`` the Viterbi log-probabilities
    (``GMMHMM.decode``'s), bit for bit what :class:`GmmBatch` returns for each (utterance, model) pair.  Device tensors;
    no workspace.  ``batch_or_feats``: a ``trellis.FeatureBatch`` (``lengths`` is ignored) or host / device ``feats``
    with host ``lengths``.  ``pack_or_models``: a :class:`GmmPack` or a list of :class:`GMMHMM` objects (padded to the
    largest S of the vocabulary; M and D must match).  ``want_post`` (forward mode only): the posterior over the
    words."""
    return _vocab_scores(GmmPack, batch_or_feats, lengths, pack_or_models, mode, want_post)


# ------------------------------------------------------------------------------------------
# M-step (host, float64)
# ------------------------------------------------------------------------------------------
def gmm_m_step(stats, startprob, transmat, weights, means, covars, params="stmcw", startprob_prior=1.0,
               transmat_prior=1.0, weights_prior=1.0, means_prior=0.0, means_weight=0.0, covars_prior=-1.5,
               covars_weight=0.0, min_covar=1e-3):
    """hmmlearn 0.3.x ``GMMHMM._do_mstep`` (diag), restated, plus the two rules of the module docstring.  ``stats``: a
    :func:`split_stats` dict.  Returns ``(startprob, transmat, weights, means, covars)``.

    * ``s`` / ``t``: :func:`sapr_amd.hmmlearn_hmm.m_step`'s rules
    * ``w``: ``(post_mix + weights_prior - 1) / (post + sum_m (weights_prior - 1))``; a state whose denominator is
      exactly 0 keeps its weights
    * ``m``: ``(means_weight * means_prior + obs) / (means_weight + post_mix)``
    * ``c``: ``(obs2 - 2 mu obs + mu^2 post_mix + means_weight (mu - means_prior)^2 + 2 covars_weight) /
      (post_mix + 1 + 2 (covars_prior + 1))`` with the NEW mean, then ``max(., min_covar)``"""
    weights, means, covars = (np.asarray(a, dtype=np.float64) for a in (weights, means, covars))
    st_letters = "".join(ch for ch in params if ch in "st")
    startprob, transmat, _, _ = m_step(stats, np.asarray(startprob, dtype=np.float64),
                                       np.asarray(transmat, dtype=np.float64), st_letters, startprob_prior,
                                       transmat_prior)
    S, M = weights.shape
    post_mix = stats["post_mix"]
    with np.errstate(divide="ignore", invalid="ignore"):
        if "w" in params:
            wp = np.broadcast_to(np.asarray(weights_prior, dtype=np.float64), (S, M))
            den = stats["post"] + (wp - 1).sum(axis=1)
            weights = np.where(den[:, None] == 0, weights, (post_mix + wp - 1) / den[:, None])
        m_den = (means_weight + post_mix)[:, :, None]
        empty = m_den == 0
        if "m" in params:
            means = np.where(empty, means, (means_weight * means_prior + stats["obs"]) / m_den)
        if "c" in params:
            c_n = (stats["obs**2"] - 2 * means * stats["obs"] + means ** 2 * post_mix[:, :, None]
                   + means_weight * (means - means_prior) ** 2 + 2 * covars_weight)
            c_d = post_mix[:, :, None] + 1 + 2 * (covars_prior + 1)
            covars = np.where(empty, covars, np.maximum(c_n / c_d, min_covar))
    return startprob, transmat, weights, means, covars


# ------------------------------------------------------------------------------------------
# the model class
# ------------------------------------------------------------------------------------------
class GMMHMM:
    """``hmmlearn.hmm.GMMHMM`` with diagonal covariances: ``startprob_[S]``, ``transmat_[S, S]``, ``weights_[S, M]``,
    ``means_[S, M, D]``, ``covars_[S, M, D]``.

    ``fit`` first initialises what ``init_params`` names — or what is not set yet — as hmmlearn's ``_init`` does
    (restated from knowledge of hmmlearn 0.3.x), with ``rs = check_random_state(random_state)``:

    * ``s`` / ``t``  the Dirichlet draws of :class:`sapr_amd.hmmlearn_hmm.GaussianHMM`
    * ``m``  two stages of k-means on the device (:func:`sapr_amd.kmeans.kmeans`, ``n_init=10``): S clusters over the
      model's frames, then M clusters inside each of the S label groups (gathered by label on the device, the groups
      of all models in one batched call); a label group with fewer than M frames raises ``ValueError``.  Seeds: one
      integer from ``rs`` for the first stage, then one per state for the second
    * ``c``  ``diag(np.cov(X.T)) + min_covar``, tiled to ``(S, M, D)``
    * ``w``  ``1 / M``

    The k-means deviations of ``GaussianHMM`` carry over (``kmeans.py``)."""

    _INIT_ATTRS = (("s", "startprob_"), ("t", "transmat_"), ("m", "means_"), ("c", "covars_"), ("w", "weights_"))

    def __init__(self, n_components=1, n_mix=1, covariance_type="diag", min_covar=1e-3, startprob_prior=1.0,
                 transmat_prior=1.0, weights_prior=1.0, means_prior=0.0, means_weight=0.0, covars_prior=None,
                 covars_weight=None, algorithm="viterbi", random_state=None, n_iter=10, tol=1e-2, verbose=False,
                 params="stmcw", init_params="stmcw"):
        if covariance_type != "diag":
            raise NotImplementedError(f"covariance_type={covariance_type!r}: only 'diag' is implemented")
        if algorithm not in DECODER_ALGORITHMS:
            raise ValueError(f"algorithm must be one of {DECODER_ALGORITHMS}, got {algorithm!r}")
        if not 1 <= int(n_components) <= MAX_STATES or not 1 <= int(n_mix) <= MAX_MIX:
            raise ValueError(f"n_components must lie in 1..{MAX_STATES} and n_mix in 1..{MAX_MIX}")
        self.n_components, self.n_mix, self.covariance_type = int(n_components), int(n_mix), covariance_type
        self.min_covar, self.startprob_prior, self.transmat_prior = min_covar, startprob_prior, transmat_prior
        self.weights_prior, self.means_prior, self.means_weight = weights_prior, means_prior, means_weight
        # hmmlearn's defaults for 'diag': covars_prior = -1.5, covars_weight = 0 (the ML estimate)
        self.covars_prior = -1.5 if covars_prior is None else covars_prior
        self.covars_weight = 0.0 if covars_weight is None else covars_weight
        self.algorithm, self.random_state, self.n_iter, self.tol, self.verbose = \
            algorithm, random_state, n_iter, tol, verbose
        self.params, self.init_params = params, init_params
        self.monitor_ = ConvergenceMonitor(self.tol, self.n_iter, self.verbose)

    # ---- initialisation / validation ------------------------------------------------------
    def _needs_init(self, code, name):
        if code in self.init_params:
            return True
        return not hasattr(self, name)

    def _check(self):
        S, M = self.n_components, self.n_mix
        self.startprob_ = np.asarray(self.startprob_, dtype=np.float64)
        self.transmat_ = np.asarray(self.transmat_, dtype=np.float64)
        self.weights_ = np.asarray(self.weights_, dtype=np.float64)
        self.means_ = np.asarray(self.means_, dtype=np.float64)
        self.covars_ = np.asarray(self.covars_, dtype=np.float64)
        if self.startprob_.shape != (S,) or not np.allclose(self.startprob_.sum(), 1.0):
            raise ValueError("startprob_ must have length n_components and sum to 1.0")
        if self.transmat_.shape != (S, S) or not np.allclose(self.transmat_.sum(axis=1), 1.0):
            raise ValueError("rows of transmat_ must sum to 1.0")
        if self.weights_.shape != (S, M) or not np.allclose(self.weights_.sum(axis=1), 1.0):
            raise ValueError("weights_ must be (n_components, n_mix) with rows that sum to 1.0")
        if self.means_.ndim != 3 or self.means_.shape[:2] != (S, M) or self.covars_.shape != self.means_.shape:
            raise ValueError("means_ / covars_ must be (n_components, n_mix, n_features)")
        if np.any(self.covars_ <= 0):
            raise ValueError("'diag' covars must be positive")
        self.n_features = int(self.means_.shape[2])
        if self.n_features > MAX_DIMS:
            raise ValueError(f"at most {MAX_DIMS} features are served")

    def _params(self):
        return (self.startprob_, self.transmat_, self.weights_, self.means_, self.covars_)

    @staticmethod
    def _split(X, lengths):
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("X must be 2-D (n_samples, n_features)")
        lengths = [X.shape[0]] if lengths is None else [int(n) for n in lengths]
        if sum(lengths) != X.shape[0]:
            raise ValueError("lengths do not sum to n_samples")
        return X, lengths

    def _batch(self, X, lengths):
        self._check()
        X, lengths = self._split(X, lengths)
        if X.shape[1] != self.n_features:
            raise ValueError(f"X has {X.shape[1]} features, the model {self.n_features}")
        batch = GmmBatch(_features_f32(X), lengths, np.zeros(len(lengths), dtype=np.int64), 1, self.n_components,
                         self.n_mix)
        return batch, pack_models([self._params()]), lengths

    # ---- inference ------------------------------------------------------------------------
    def score(self, X, lengths=None):
        batch, pack, _ = self._batch(X, lengths)
        ll, = _lib.to_host(batch.estep(pack, want_stats=False)[0])
        return float(ll.sum())

    def score_samples(self, X, lengths=None):
        """``(log_prob, posteriors)``: the forward log-likelihood summed over the sequences and the state posteriors
        ``(n_samples, n_components)`` float64."""
        batch, pack, lengths = self._batch(X, lengths)
        ll, _, post, _ = batch.estep(pack, want_stats=False, want_post=True)
        ll, post = _lib.to_host(ll, post)
        return (float(ll.sum()) if len(lengths) > 1 else float(ll[0])), post.copy()

    def predict_proba(self, X, lengths=None):
        return self.score_samples(X, lengths)[1]

    def decode(self, X, lengths=None, algorithm=None):
        """``(log_prob, state_sequence)`` by ``algorithm or self.algorithm``: ``"viterbi"`` (hmmlearn's ``viterbi``, the
        log-probabilities of the sequences summed) or ``"map"`` (``_decode_map``: the per-frame arg-max of the state
        posteriors and ``max(posteriors, axis=1).sum()``)."""
        algorithm = algorithm or self.algorithm
        if algorithm not in DECODER_ALGORITHMS:
            raise ValueError(f"algorithm must be one of {DECODER_ALGORITHMS}, got {algorithm!r}")
        batch, pack, lengths = self._batch(X, lengths)
        if algorithm == "map":
            post, = _lib.to_host(batch.estep(pack, want_stats=False, want_post=True)[2])
            return map_decode_host(post, lengths)
        lp, path = _lib.to_host(*batch.viterbi(pack))
        return (float(lp.sum()) if len(lengths) > 1 else float(lp[0])), path.astype(np.int64)

    def predict(self, X, lengths=None):
        return self.decode(X, lengths)[1]

    # ---- training -------------------------------------------------------------------------
    def fit(self, X, lengths=None):
        """Baum-Welch: per iteration one batched E-step on the GPU, the M-step on the host, ``monitor_.report`` and
        the convergence test."""
        fit_gmm_models([self], [self._split(X, lengths)])
        return self

    # pickling: plain attributes only (no device handles are ever stored on the object)


def fit_gmm_models(models: List[GMMHMM], data) -> None:
    """Train several word models together: ``data[w] = (X_w, lengths_w)``.  One E-step launch set per iteration covers
    every model's utterances; converged models stop updating.  Models may differ in ``n_components`` (the kernels run
    at the largest); they share ``n_mix`` and the feature width.  Models that need it are initialised first, the
    k-means stages batched over all of them."""
    torch = _torch()
    if len({m.n_mix for m in models}) != 1:
        raise ValueError("models trained together must share n_mix")
    dev = _lib.require_gpu()
    W, M = len(models), models[0].n_mix
    needs = [[code for code, name in GMMHMM._INIT_ATTRS if m._needs_init(code, name)] for m in models]
    feats, lengths, utt_model, frames = [], [], [], []
    for w, (X, ln) in enumerate(data):
        X = _features_f32(X)
        if X.ndim != 2:
            raise ValueError("X must be 2-D (n_samples, n_features)")
        if X.shape[0]:
            feats.append(X)
        frames.append(X.shape[0])
        lengths += [int(n) for n in ln]
        utt_model += [w] * len(ln)
    D = int(np.asarray(data[0][0]).shape[1])
    if any(int(np.asarray(X).shape[1]) != D for X, _ in data):
        raise ValueError("models trained together must share the feature width")
    packed = np.concatenate(feats, axis=0) if feats else np.zeros((0, D), np.float32)
    dfeats = torch.from_numpy(packed).to(dev)
    if any(needs):
        _init_gmm_models(models, needs, dfeats, frames)
    for m in models:
        m._check()
        if m.n_features != D:
            raise ValueError(f"X has {D} features, the model {m.n_features}")
        m.monitor_ = ConvergenceMonitor(m.tol, m.n_iter, m.verbose)
    S = max(m.n_components for m in models)
    batch = GmmBatch(dfeats, lengths, utt_model, W, S, M)

    def update(m, st):
        m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_ = gmm_m_step(
            st, *m._params(), m.params, m.startprob_prior, m.transmat_prior, m.weights_prior, m.means_prior,
            m.means_weight, m.covars_prior, m.covars_weight, m.min_covar)
    baum_welch(models, batch, lambda ms: pack_models([m._params() for m in ms], S),
               lambda row, m: split_stats(row, S, M, D, m.n_components), update)


def _init_gmm_models(models, needs, dfeats, frames) -> None:
    """hmmlearn's ``GMMHMM._init`` for the models whose ``needs[w]`` is not empty (see :class:`GMMHMM`).  ``dfeats``:
    the packed device features of ALL models, model after model, ``frames[w]`` of them per model."""
    torch = _torch()
    from . import kmeans as km
    D = int(dfeats.shape[1])
    seeds = {}
    for w, m in enumerate(models):
        if not needs[w]:
            continue
        S, M = m.n_components, m.n_mix
        rs = check_random_state(m.random_state)
        if "s" in needs[w]:
            m.startprob_ = rs.dirichlet(np.full(S, 1.0 / S))
        if "t" in needs[w]:
            m.transmat_ = rs.dirichlet(np.full(S, 1.0 / S), size=S)
        if "w" in needs[w]:
            m.weights_ = np.full((S, M), 1.0 / M)
        if "m" in needs[w]:
            seeds[w] = (kmeans_seed(rs), [kmeans_seed(rs) for _ in range(S)])
    sel = [w for w, n in enumerate(needs) if "m" in n or "c" in n]
    if not sel:
        return
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)

    def gather(ws):
        if len(ws) == len(models):
            return dfeats
        return torch.cat([dfeats[off[w]:off[w + 1]] for w in ws], dim=0) if ws else dfeats[:0]
    feats_sel = gather(sel)
    count, mean, sqdev = km.column_moments(km.Stepper(feats_sel, km.FrameTiles.build([frames[w] for w in sel],
                                                                                      dfeats.device)))
    for g, w in enumerate(sel):
        m = models[w]
        if "c" in needs[w]:
            if count[g] < 2:
                raise ValueError(f"covariance initialisation needs at least 2 frames, model {w} has {int(count[g])}")
            m.covars_ = np.tile(sqdev[g] / (count[g] - 1) + m.min_covar, (m.n_components, m.n_mix, 1))
    # the two k-means stages, the models of one n_components together
    for S in sorted({models[w].n_components for w in sel if "m" in needs[w]}):
        msel = [w for w in sel if "m" in needs[w] and models[w].n_components == S]
        M = models[msel[0]].n_mix
        at = [sel.index(w) for w in msel]
        fm = gather(msel)
        glen = [frames[w] for w in msel]
        centres, _, _, _ = km.kmeans(fm, glen, S, n_init=10, seeds=[seeds[w][0] for w in msel],
                                     moments=(count[at], mean[at], sqdev[at]))
        # the frames' labels under the final centres, then the frames gathered by (model, label) on the device
        stepper = km.Stepper(fm, km.FrameTiles.build(glen, dfeats.device))
        _, labels = stepper.step(centres[:, None], want_labels=True)
        group = torch.repeat_interleave(torch.arange(len(msel), device=dfeats.device),
                                        torch.from_numpy(np.asarray(glen, dtype=np.int64)).to(dfeats.device))
        key = group * S + labels[0].to(torch.int64)
        order = torch.sort(key, stable=True)[1]
        sizes = torch.bincount(key, minlength=len(msel) * S).cpu().numpy()
        small = np.nonzero(sizes < M)[0]
        if small.size:
            raise ValueError(f"GMMHMM initialisation: label group(s) {[(msel[i // S], int(i % S)) for i in small]} "
                             f"(model, state) hold {[int(sizes[i]) for i in small]} frames, fewer than n_mix={M}")
        sub, _, _, _ = km.kmeans(fm[order].contiguous(), sizes, M, n_init=10,
                                 seeds=[s for w in msel for s in seeds[w][1]])
        for g, w in enumerate(msel):
            models[w].means_ = sub[g * S:(g + 1) * S].copy()

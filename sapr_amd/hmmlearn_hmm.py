"""Host-side mirror of ``assignment2/hmmlearn_hmm.py`` over the HIP trellis kernels.

The reference wraps ``hmmlearn.hmm.GaussianHMM`` (``hmmlearn_hmm.py:27-43``) and what it pickles
and later decodes with is that GaussianHMM object (``hmmlearn_hmm.py:106``, ``train.py:116-120``,
``decoder.py:26-27,43``).  hmmlearn is not a dependency here: :class:`GaussianHMM` below is a
picklable object with the same attribute names and ``fit / score / decode`` methods whose
arithmetic runs in ``libsapr_hip.so`` (sapr_estep_diag, sapr_forward_diag, sapr_viterbi_*).
Only the tiny M-step (hmmlearn ``base.py _do_mstep`` / ``hmm.py GaussianHMM._do_mstep``) and the
convergence monitor run on the host.

Known, documented deviation: the reference's flat-start ``means_`` / ``covars_`` are
float32 (``np.mean`` / ``np.var`` of float32 frames), so under numpy 1.26 its FIRST E-step evaluates
log-densities in float32; here the flat-start values are the same float32 numbers promoted to
float64 and every E-step is float64.
"""
from __future__ import annotations

import logging
from collections import deque
from typing import List

import numpy as np

from . import _lib
from .mfcc_extract import load_mfccs, load_mfccs_by_word  # noqa: F401  (same import surface as the reference)
from .tile_family import VocabPack, _features_f32, baum_welch  # noqa: F401  (VocabPack: imported from here too)

logging.getLogger("matplotlib").setLevel(logging.WARNING)


class ConvergenceMonitor:
    """hmmlearn ``base.py ConvergenceMonitor``: ``history`` keeps every reported log-prob
    (``train.py:117`` and ``visualize.py:124`` read ``monitor_.history``)."""

    def __init__(self, tol, n_iter, verbose=False):
        self.tol, self.n_iter, self.verbose = tol, n_iter, verbose
        self.history = deque()
        self.iter = 0

    def _reset(self):
        self.iter = 0
        self.history.clear()

    def report(self, log_prob):
        precision = np.finfo(float).eps ** (1 / 2)
        if self.history and (log_prob - self.history[-1]) < -precision:
            logging.warning("Model is not converging.  Current: %s is not greater than %s. Delta is %s",
                            log_prob, self.history[-1], log_prob - self.history[-1])
        self.history.append(log_prob)
        self.iter += 1

    @property
    def converged(self):
        return (self.iter == self.n_iter
                or (len(self.history) >= 2 and self.history[-1] - self.history[-2] < self.tol))


def m_step(stats, startprob, transmat, params="stmc", startprob_prior=1.0, transmat_prior=1.0,
           means_prior=0.0, means_weight=0.0, covars_prior=1e-2, covars_weight=1.0, means=None, covars=None):
    """hmmlearn base.py ``_do_mstep`` + hmm.py ``GaussianHMM._do_mstep`` (diag).  Structural zeros of
    startprob / transmat stay zero; σ² = (covars_prior + obs² − 2μ·obs + μ²·post) / max(post, 1e-5)."""
    if "s" in params:
        sp = np.maximum(startprob_prior - 1 + stats["start"], 0)
        sp = np.where(startprob == 0, 0, sp)
        tot = sp.sum()
        startprob = sp / (tot if tot != 0 else 1.0)  # hmmlearn.utils.normalize: a zero sum divides by 1
    if "t" in params:
        tm = np.maximum(transmat_prior - 1 + stats["trans"], 0)
        tm = np.where(transmat == 0, 0, tm)
        rs = tm.sum(axis=1)
        rs[rs == 0] = 1
        transmat = tm / rs[:, None]
    denom = stats["post"][:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        if "m" in params:
            means = (means_weight * means_prior + stats["obs"]) / (means_weight + denom)
        if "c" in params:
            meandiff = means - means_prior
            c_n = (means_weight * meandiff ** 2 + stats["obs**2"] - 2 * means * stats["obs"] + means ** 2 * denom)
            c_d = max(covars_weight - 1, 0) + denom
            covars = (covars_prior + c_n) / np.maximum(c_d, 1e-5)
    return startprob, transmat, means, covars


COVARIANCE_TYPES = ("diag", "spherical", "tied", "full")


def m_step_typed(stats, covariance_type, startprob, transmat, params="stmc", startprob_prior=1.0, transmat_prior=1.0,
                 means_prior=0.0, means_weight=0.0, covars_prior=1e-2, covars_weight=1.0, means=None, covars=None):
    """:func:`m_step` for every ``covariance_type`` (hmm.py ``GaussianHMM._do_mstep``, restated from knowledge of
    hmmlearn 0.3.x); ``covars`` comes and goes in the shape of ``_covars_``.  ``stats`` carries ``obs**2`` for "diag"
    and "spherical" and ``obs*obs.T`` for "tied" and "full".

    * spherical: the diag formula, then the mean over the features of each state;
    * full / tied, with mu the new means: ``c_n[s] = means_weight outer(mu_s - means_prior, mu_s - means_prior) +
      oo[s] - (outer(obs_s, mu_s) + outer(obs_s, mu_s)^T) + outer(mu_s, mu_s) post_s`` (the two cross terms are added
      to each other first, so that every matrix is exactly symmetric), ``cvweight = max(covars_weight - D, 0)``, full:
      ``(covars_prior + c_n[s]) / (cvweight + post_s)``, tied: ``(covars_prior + sum_s c_n[s]) / (cvweight + sum_s
      post_s)``.  No floor and no repair: a result that is not positive-definite is refused when it is next packed."""
    if covariance_type == "diag":
        return m_step(stats, startprob, transmat, params, startprob_prior, transmat_prior, means_prior, means_weight,
                      covars_prior, covars_weight, means, covars)
    if covariance_type == "spherical":
        wide = None if covars is None else np.broadcast_to(np.asarray(covars)[:, None], np.shape(means))
        startprob, transmat, means, wide = m_step(stats, startprob, transmat, params, startprob_prior, transmat_prior,
                                                  means_prior, means_weight, covars_prior, covars_weight, means, wide)
        return startprob, transmat, means, (wide.mean(axis=1) if "c" in params else covars)
    startprob, transmat, means, _ = m_step(stats, startprob, transmat, params.replace("c", ""), startprob_prior,
                                           transmat_prior, means_prior, means_weight, covars_prior, covars_weight,
                                           means, None)
    if "c" in params:
        S, D = means.shape
        post = stats["post"]
        c_n = np.empty((S, D, D))
        for s in range(S):
            md = means[s] - means_prior
            om = np.outer(stats["obs"][s], means[s])
            c_n[s] = (means_weight * np.outer(md, md) + stats["obs*obs.T"][s] - (om + om.T)
                      + np.outer(means[s], means[s]) * post[s])
        cvweight = max(covars_weight - D, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            if covariance_type == "tied":
                covars = (covars_prior + c_n.sum(axis=0)) / (cvweight + post.sum())
            else:
                covars = (covars_prior + c_n) / (cvweight + post[:, None, None])
    return startprob, transmat, means, covars


def m_step_batch(rows, S, D, startprob, transmat, means, covars, params="stmc", startprob_prior=1.0,
                 transmat_prior=1.0, means_prior=0.0, means_weight=0.0, covars_prior=1e-2, covars_weight=1.0,
                 S_model=None, D_model=None):
    """:func:`m_step` for W models at once: ``rows[W, width]`` are sapr_estep_diag's statistics rows (kernel state
    count S, kernel feature width D), the model arrays carry a leading word axis.  Every operation is the per-model one
    applied along the trailing axes — the same elementwise arithmetic and the same row reductions, hence the same bits
    as W calls — in a tenth of the interpreter time.  Returns (startprob, transmat, means, covars, logprob[W])."""
    rows = np.asarray(rows, dtype=np.float64)
    W = rows.shape[0]
    m = S if S_model is None else S_model
    dm = D if D_model is None else D_model
    o = 2
    start = rows[:, o:o + S][:, :m]
    o += S
    trans = rows[:, o:o + S * S].reshape(W, S, S)[:, :m, :m]
    o += S * S
    post = rows[:, o:o + S][:, :m]
    o += S
    obs = rows[:, o:o + S * D].reshape(W, S, D)[:, :m, :dm]
    o += S * D
    obs2 = rows[:, o:o + S * D].reshape(W, S, D)[:, :m, :dm]
    logprob = rows[:, 1].copy()
    if "s" in params:
        sp = np.maximum(startprob_prior - 1 + start, 0)
        sp = np.where(startprob == 0, 0, sp)
        tot = sp.sum(axis=1)
        startprob = sp / np.where(tot != 0, tot, 1.0)[:, None]
    if "t" in params:
        tm = np.maximum(transmat_prior - 1 + trans, 0)
        tm = np.where(transmat == 0, 0, tm)
        rs = tm.sum(axis=2)
        rs[rs == 0] = 1
        transmat = tm / rs[:, :, None]
    denom = post[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        if "m" in params:
            means = (means_weight * means_prior + obs) / (means_weight + denom)
        if "c" in params:
            meandiff = means - means_prior
            c_n = (means_weight * meandiff ** 2 + obs2 - 2 * means * obs + means ** 2 * denom)
            c_d = max(covars_weight - 1, 0) + denom
            covars = (covars_prior + c_n) / np.maximum(c_d, 1e-5)
    return startprob, transmat, means, covars, logprob


DECODER_ALGORITHMS = ("viterbi", "map")


def map_decode_host(posteriors, lengths=None):
    """hmmlearn ``base.py _decode_map`` on a posterior lattice ``(n_samples, n_components)`` (restated from knowledge of
    hmmlearn 0.3.x): per sequence ``state_sequence = argmax(posteriors, axis=1)`` and ``log_prob =
    max(posteriors, axis=1).sum()``, the log_probs summed over the sequences → ``(log_prob, state_sequence)``.  numpy's
    rules: equal values give the lowest state, a row holding NaN gives its first NaN and makes ``log_prob`` NaN."""
    post = np.asarray(posteriors, dtype=np.float64)
    if post.ndim != 2:
        raise ValueError("posteriors must be 2-D (n_samples, n_components)")
    lengths = [post.shape[0]] if lengths is None else [int(n) for n in lengths]
    if sum(lengths) != post.shape[0]:
        raise ValueError("lengths do not sum to n_samples")
    log_prob, at = 0.0, 0
    for n in lengths:
        log_prob += float(np.max(post[at:at + n], axis=1).sum()) if n else 0.0
        at += n
    states = np.argmax(post, axis=1).astype(np.int64) if post.shape[0] else np.zeros(0, np.int64)
    return log_prob, states


def check_random_state(seed):
    """sklearn.utils.check_random_state: None -> numpy's global RandomState, an int -> a fresh ``RandomState(seed)``,
    a ``RandomState`` -> itself (and its stream is consumed)."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        return np.random.RandomState(int(seed))
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def kmeans_seed(rs) -> int:
    """The one integer a model's ``random_state`` contributes to its k-means (drawn after the ``s`` / ``t`` draws)."""
    return int(rs.randint(np.iinfo(np.int32).max))


class GaussianHMM:
    """hmmlearn-shaped Gaussian HMM (every state emits) on the HIP kernels, ``covariance_type`` "diag", "spherical",
    "tied" or "full".  "diag" and "spherical" (one variance per state, broadcast over the features) run on the diagonal
    kernels; "full" and "tied" on the full-covariance kernels (:mod:`sapr_amd.full_cov`), where Viterbi ties go to the
    first maximum and ``tie_break`` does not apply.  ``_covars_`` has hmmlearn's shapes — ``(S,)`` spherical, ``(D, D)``
    tied, ``(S, D, D)`` full, ``(S, D)`` diag — and ``covars_`` always returns ``(S, D, D)``.

    ``fit`` first initialises what ``init_params`` names — or what is not set yet — the way hmmlearn's ``_init`` does
    (restated from knowledge of hmmlearn 0.3.x, the reference's pinned version, like SURVEY §9.3), with
    ``rs = check_random_state(random_state)`` and S = ``n_components``:

    * ``s``  ``startprob_ = rs.dirichlet(np.full(S, 1/S))``
    * ``t``  ``transmat_ = rs.dirichlet(np.full(S, 1/S), size=S)``  (hmmlearn <= 0.2.7 set both to the uniform value)
    * ``m``  ``means_`` = the centres of a k-means with S clusters and ``n_init=10`` over all frames of the model, on the
      device (:func:`sapr_amd.kmeans.kmeans`), seeded by ONE integer drawn from ``rs`` after the ``s`` / ``t`` draws —
      a model's initialisation depends only on its own ``random_state`` and data, not on what else is trained with it
    * ``c``  ``covars_ = tile(diag(np.cov(X.T)) + min_covar, (S, 1))``: the ddof = 1 column variance about the column
      mean, two K = 1 steps of the same kernel ("diag"); the other types start from ``cv = np.cov(X.T) + min_covar I``
      (float64, on the device): "tied" ``cv``, "full" ``tile(cv)``, "spherical" ``tile(cv.mean())`` over all D x D entries

    Not scikit-learn's random stream or seeding, and an empty cluster keeps its centre (``kmeans.py``);
    hmmlearn's warning about fewer data points than free parameters is not reproduced.  A preset attribute whose
    letter is in ``init_params`` is overwritten, with a warning; ``init_params=""`` trains from the preset values."""

    def __init__(self, n_components=1, covariance_type="diag", min_covar=1e-3, startprob_prior=1.0,
                 transmat_prior=1.0, means_prior=0, means_weight=0, covars_prior=1e-2, covars_weight=1,
                 algorithm="viterbi", random_state=None, n_iter=10, tol=1e-2, verbose=False, params="stmc",
                 init_params="stmc", implementation="log"):
        if covariance_type not in COVARIANCE_TYPES:
            raise ValueError(f"covariance_type must be one of {COVARIANCE_TYPES}, got {covariance_type!r}")
        if implementation != "log":
            raise ValueError("only implementation='log' is implemented (hmmlearn_hmm.py:32)")
        if algorithm not in DECODER_ALGORITHMS:
            raise ValueError(f"algorithm must be one of {DECODER_ALGORITHMS}, got {algorithm!r}")
        self.n_components, self.covariance_type, self.min_covar = n_components, covariance_type, min_covar
        self.startprob_prior, self.transmat_prior = startprob_prior, transmat_prior
        self.means_prior, self.means_weight = means_prior, means_weight
        self.covars_prior, self.covars_weight = covars_prior, covars_weight
        self.algorithm, self.random_state, self.n_iter, self.tol, self.verbose = \
            algorithm, random_state, n_iter, tol, verbose
        self.params, self.init_params, self.implementation = params, init_params, implementation
        self.monitor_ = ConvergenceMonitor(self.tol, self.n_iter, self.verbose)
        # which back-trace tie-break GaussianHMM.decode uses (oracle/hmmlearn_oracle.py docstring)
        self.tie_break = "high"

    # hmmlearn exposes full matrices through covars_ and keeps the type's own array in _covars_
    @property
    def covars_(self):
        ct = self.covariance_type
        if ct == "full":
            return np.array(self._covars_, copy=True)
        if ct == "tied":
            return np.tile(self._covars_, (self.n_components, 1, 1))
        if ct == "spherical":
            D = int(self.n_features if hasattr(self, "n_features") else np.shape(self.means_)[1])
            return np.array([np.eye(D) * c for c in self._covars_])
        return np.array([np.diag(c) for c in self._covars_])

    @covars_.setter
    def covars_(self, covars):
        covars = np.array(covars, copy=True)
        ct, S = self.covariance_type, self.n_components
        if ct == "diag":
            if covars.ndim != 2 or np.any(covars <= 0):
                raise ValueError("'diag' covars must be a positive (n_components, n_features) array")
        elif ct == "spherical":
            if covars.ndim != 1 or len(covars) != S or np.any(covars <= 0):
                raise ValueError("'spherical' covars must be a positive array of length n_components")
        else:
            from .full_cov import cholesky_lower
            if ct == "tied":
                if covars.ndim != 2 or covars.shape[0] != covars.shape[1]:
                    raise ValueError("'tied' covars must have shape (n_features, n_features)")
                cholesky_lower(covars, "tied")
            else:
                if covars.ndim != 3 or covars.shape[0] != S or covars.shape[1] != covars.shape[2]:
                    raise ValueError("'full' covars must have shape (n_components, n_features, n_features)")
                for cv in covars:
                    cholesky_lower(cv, "full")
        self._covars_ = covars

    def _is_full(self):
        return self.covariance_type in ("full", "tied")

    def _full_params(self):
        """``(startprob, transmat, means[S, D], covars[S, D, D])`` as :func:`sapr_amd.full_cov.pack_models` takes it.
        A "diag" or "spherical" model is expanded to diagonal matrices, so that a vocabulary may mix the types
        (``full_cov.FullPack.from_models``)."""
        cv = np.asarray(self._covars_, dtype=np.float64)
        if self.covariance_type == "tied":
            cv = np.broadcast_to(cv, (self.n_components,) + cv.shape)
        elif self.covariance_type == "spherical":
            D = int(np.shape(self.means_)[1])
            cv = cv[:, None, None] * np.eye(D)
        elif self.covariance_type == "diag":
            cv = np.array([np.diag(c) for c in cv])
        return (np.asarray(self.startprob_, dtype=np.float64), np.asarray(self.transmat_, dtype=np.float64),
                np.asarray(self.means_, dtype=np.float64), cv)

    def _full_batch(self, X, lengths):
        """(batch, pack, lengths) of one model over its sequences on the full-covariance kernels."""
        from . import full_cov
        self._check()
        Xa, lengths = self._split(X, lengths)
        batch = full_cov.FullCovBatch(_features_f32(Xa), lengths, np.zeros(len(lengths), np.int64), 1,
                                      self.n_components)
        return batch, full_cov.pack_models([self._full_params()], name=self.covariance_type), lengths

    # ---- initialisation (hmmlearn _needs_init / _init) ---------------------------------------
    _INIT_ATTRS = (("s", "startprob_"), ("t", "transmat_"), ("m", "means_"), ("c", "covars_"))

    def _needs_init(self, code, name):
        if code in self.init_params:
            if hasattr(self, name):
                logging.getLogger(__name__).warning(
                    "Even though the %r attribute is set, it will be overwritten during initialization because "
                    "'init_params' contains %r", name, code)
            return True
        return not hasattr(self, name)

    # ---- validation (hmmlearn _check) -----------------------------------------------------
    def _check(self):
        self.startprob_ = np.asarray(self.startprob_)
        self.transmat_ = np.asarray(self.transmat_)
        self.means_ = np.asarray(self.means_)
        S = self.n_components
        if len(self.startprob_) != S or not np.allclose(self.startprob_.sum(), 1.0):
            raise ValueError("startprob_ must have length n_components and sum to 1.0")
        if self.transmat_.shape != (S, S) or not np.allclose(self.transmat_.sum(axis=1), 1.0):
            raise ValueError("rows of transmat_ must sum to 1.0")
        self._covars_ = np.asarray(self._covars_)
        D = self.means_.shape[1] if self.means_.ndim == 2 else -1
        want = {"diag": (S, D), "spherical": (S,), "tied": (D, D), "full": (S, D, D)}[self.covariance_type]
        if self.means_.ndim != 2 or self.means_.shape[0] != S or self._covars_.shape != want:
            raise ValueError("means_ / covars_ shape mismatch")
        self.n_features = D

    def _pack(self):
        from .trellis import DiagModelPack
        # one model, scored or decoded on its own (decode / score below): the exact kernels' operands only
        cv = np.asarray(self._covars_, dtype=np.float64)
        if self.covariance_type == "spherical":
            cv = np.broadcast_to(cv[:, None], np.shape(self.means_))
        return DiagModelPack.from_params(self.startprob_[None], self.transmat_[None],
                                         np.asarray(self.means_, dtype=np.float64)[None], cv[None], exact_only=True)

    @staticmethod
    def _split(X, lengths):
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("X must be 2-D (n_samples, n_features)")
        if lengths is None:
            lengths = [X.shape[0]]
        lengths = [int(n) for n in lengths]
        if sum(lengths) != X.shape[0]:
            raise ValueError("lengths do not sum to n_samples")
        return X, lengths

    # ---- GaussianHMM.decode (decoder.py:43) -----------------------------------------------
    def decode(self, X, lengths=None, algorithm=None):
        """``(log_prob, state_sequence)`` by ``algorithm or self.algorithm``.

        ``"viterbi"``: the order of numpy's sum inside the log-density
        depends on X's memory layout (oracle/hmmlearn_oracle.py): a C-contiguous X reduces pair-wise,
        the ``feat.T`` view decoder.py:59 passes reduces left to right — both reproduced.

        ``"map"``: hmmlearn's ``_decode_map`` (restated from knowledge of hmmlearn 0.3.x, like SURVEY §9.3): the
        per-frame arg-max of the state posteriors, ``log_prob = max(posteriors, axis=1).sum()`` per sequence, summed
        over the sequences — computed on the host from the lattice the device returns (:func:`map_decode_host`)."""
        from .trellis import FeatureBatch, viterbi_decode
        algorithm = algorithm or getattr(self, "algorithm", "viterbi")
        if algorithm not in DECODER_ALGORITHMS:
            raise ValueError(f"algorithm must be one of {DECODER_ALGORITHMS}, got {algorithm!r}")
        if algorithm == "map":
            Xa, lengths = self._split(X, lengths)
            return map_decode_host(self._state_posteriors(Xa, lengths)[1], lengths)
        if self._is_full():
            batch, pack, lengths = self._full_batch(X, lengths)
            lp, path = batch.viterbi(pack)
            lp = lp.cpu().numpy()
            return (float(lp.sum()) if len(lengths) > 1 else float(lp[0])), path.cpu().numpy().astype(np.int64)
        self._check()
        Xa = np.asarray(X)
        sum_order = _lib.SUM_PAIRWISE if Xa.flags.c_contiguous else _lib.SUM_TVIEW
        Xa, lengths = self._split(Xa, lengths)
        if len(lengths) > 1 and sum_order == _lib.SUM_TVIEW:
            sum_order = _lib.SUM_PAIRWISE  # row slices of a transposed view: treat as contiguous copies
        feats = _features_f32(Xa)
        import torch
        dev = _lib.require_gpu()
        batch = FeatureBatch.from_packed(torch.from_numpy(feats).to(dev), np.asarray(lengths))
        tie = _lib.TIE_HIGH if self.tie_break == "high" else _lib.TIE_LOW
        res = viterbi_decode(batch, self._pack(), tie=tie, sum_order=sum_order, word_sel=np.zeros(len(lengths)))
        log_prob = float(res.best_score.sum().item()) if len(lengths) > 1 else float(res.best_score[0].item())
        return log_prob, res.path.cpu().numpy().astype(np.int64)

    def predict(self, X, lengths=None):
        return self.decode(X, lengths)[1]

    # ---- GaussianHMM.score_samples / predict_proba (hmmlearn base.py) -----------------------
    def _state_posteriors(self, Xa, lengths):
        """(per-sequence log-likelihoods, posterior lattice) as host arrays."""
        from .trellis import FeatureBatch, state_posteriors
        if self._is_full():
            batch, pack, _ = self._full_batch(Xa, lengths)
            ll, _, post, _ = batch.estep(pack, want_stats=False, want_post=True)
            return ll.cpu().numpy(), post.cpu().numpy()
        self._check()
        import torch
        dev = _lib.require_gpu()
        feats = _features_f32(Xa)
        batch = FeatureBatch.from_packed(torch.from_numpy(feats).to(dev), np.asarray(lengths))
        res = state_posteriors(batch, self._pack(), want_path=False)
        ll, post = _lib.to_host(res.loglik, res.post)
        return ll, post.copy()  # (out of the pinned buffer)

    def score_samples(self, X, lengths=None):
        """``(log_prob, posteriors)``: the forward log-likelihood summed over the sequences and the state posteriors
        ``(n_samples, n_components)`` float64 (hmmlearn ``score_samples``)."""
        Xa, lengths = self._split(X, lengths)
        ll, post = self._state_posteriors(Xa, lengths)
        return float(ll.sum()) if len(lengths) > 1 else float(ll[0]), post

    def predict_proba(self, X, lengths=None):
        return self.score_samples(X, lengths)[1]

    # ---- GaussianHMM.score (hmmlearn_hmm.py:104) ------------------------------------------
    def score(self, X, lengths=None):
        from .trellis import FeatureBatch, forward_loglik
        if self._is_full():
            batch, pack, _ = self._full_batch(X, lengths)
            return float(batch.estep(pack, want_stats=False)[0].cpu().numpy().sum())
        self._check()
        Xa, lengths = self._split(X, lengths)
        import torch
        dev = _lib.require_gpu()
        feats = _features_f32(Xa)
        batch = FeatureBatch.from_packed(torch.from_numpy(feats).to(dev), np.asarray(lengths))
        ll = forward_loglik(batch, self._pack(), np.zeros(len(lengths), dtype=np.int64))
        return float(ll.sum().item())

    # ---- GaussianHMM.fit (hmmlearn_hmm.py:103) --------------------------------------------
    def fit(self, X, lengths=None):
        """Baum-Welch: per iteration one batched E-step on the GPU (all sequences at once), one
        all-reduce of the statistics when torch.distributed is initialised (each rank passes its own
        shard of sequences), M-step, ``monitor_.report`` and the convergence test."""
        fit_models([self], [self._split(X, lengths)])
        return self

    # pickling: plain attributes only (no device handles are ever stored on the object)


def fit_models(models: List[GaussianHMM], data) -> None:
    """Train several word models together: ``data[w] = (X_w, lengths_w)`` (this rank's shard).
    One E-step launch sequence covers every word's utterances; converged models stop updating.  Models that need it
    (``GaussianHMM._needs_init``) are initialised first, all of them in one batched k-means on the device."""
    import torch
    from . import dist as sdist
    from .trellis import DiagModelPack, EStep, FeatureBatch
    # the models are grouped by the kernels that serve them: "diag" / "spherical" and "full" / "tied"
    families = [m._is_full() for m in models]
    if any(families) and not all(families):
        for fam in (False, True):
            idx = [w for w, f in enumerate(families) if f == fam]
            fit_models([models[w] for w in idx], [data[w] for w in idx])
        return
    if any(m.covariance_type != "diag" for m in models) and sdist.world()[1] > 1:
        raise NotImplementedError("training a model whose covariance_type is not 'diag' over several ranks is not "
                                  "implemented")
    dev = _lib.require_gpu()
    W = len(models)
    needs = [[code for code, name in GaussianHMM._INIT_ATTRS if m._needs_init(code, name)] for m in models]
    if not any(needs):
        for m in models:
            m._check()
    feats, lengths, utt_model, frames = [], [], [], []
    for w, (X, ln) in enumerate(data):
        X = _features_f32(X)
        if X.shape[0]:
            feats.append(X)
        frames.append(X.shape[0])
        lengths += list(ln)
        utt_model += [w] * len(ln)
    D = models[0].n_features if not any(needs) else int(np.asarray(data[0][0]).shape[1])
    packed = np.concatenate(feats, axis=0) if feats else np.zeros((0, D), np.float32)
    dfeats = torch.from_numpy(packed).to(dev)
    if any(needs):
        _init_models(models, needs, dfeats, frames)
        for m in models:
            m._check()
    for m in models:
        m.monitor_ = ConvergenceMonitor(m.tol, m.n_iter, m.verbose)
    S = models[0].n_components
    if families[0]:
        _fit_full(models, dfeats, lengths, utt_model)
        return
    batch = FeatureBatch.from_packed(dfeats, np.asarray(lengths, dtype=np.int64))
    estep = EStep(batch, np.asarray(utt_model), W, S)
    active = [True] * W
    max_iter = max(m.n_iter for m in models)
    for _ in range(max_iter):
        if not any(active):
            break
        pack = DiagModelPack.from_models(models, device=dev, exact_only=True)  # never decoded with
        stats = estep.run(pack)
        sdist.allreduce_sum_(stats)
        host = stats.cpu().numpy()
        hyper = [(m.params, m.startprob_prior, m.transmat_prior, m.means_weight, m.covars_prior, m.covars_weight)
                 for m in models]
        if W > 1 and all(m.covariance_type == "diag" for m in models) and all(h == hyper[0] for h in hyper) \
                and all(np.ndim(m.means_prior) == 0 for m in models) \
                and len({float(m.means_prior) for m in models}) == 1:
            # one vectorised M-step for the whole vocabulary (same bits as the per-model calls, a tenth of the time)
            m0 = models[0]
            new = m_step_batch(host, estep.S, estep.D,
                               np.stack([np.asarray(m.startprob_, dtype=np.float64) for m in models]),
                               np.stack([np.asarray(m.transmat_, dtype=np.float64) for m in models]),
                               np.stack([np.asarray(m.means_, dtype=np.float64) for m in models]),
                               np.stack([np.asarray(m._covars_, dtype=np.float64) for m in models]),
                               m0.params, m0.startprob_prior, m0.transmat_prior, m0.means_prior, m0.means_weight,
                               m0.covars_prior, m0.covars_weight, S_model=estep.S_model, D_model=estep.batch.D_model)
            for w, m in enumerate(models):
                if not active[w]:
                    continue
                m.startprob_, m.transmat_, m.means_, m._covars_ = new[0][w], new[1][w], new[2][w], new[3][w]
                m.monitor_.report(float(new[4][w]))
                if m.monitor_.converged:
                    active[w] = False
            continue
        for w, m in enumerate(models):
            if not active[w]:
                continue
            st = estep.split(host[w])
            m.startprob_, m.transmat_, m.means_, cov = m_step_typed(
                st, m.covariance_type, m.startprob_, m.transmat_, m.params, m.startprob_prior, m.transmat_prior,
                m.means_prior, m.means_weight, m.covars_prior, m.covars_weight, np.asarray(m.means_, dtype=np.float64),
                np.asarray(m._covars_, dtype=np.float64))
            m._covars_ = cov
            m.monitor_.report(st["logprob"])
            if m.monitor_.converged:
                active[w] = False


def _fit_full(models, dfeats, lengths, utt_model) -> None:
    """The Baum-Welch loop of :func:`fit_models` for "full" / "tied" models (initialised and checked by the caller):
    one ``sapr_full_estep`` per iteration over every model's utterances, the M-step per model on the host."""
    from . import full_cov
    S = max(m.n_components for m in models)
    batch = full_cov.FullCovBatch(dfeats, lengths, utt_model, len(models), S)

    def pack(ms):
        return np.concatenate([full_cov.pack_models([m._full_params()], S, name=m.covariance_type) for m in ms])

    def update(m, st):
        m.startprob_, m.transmat_, m.means_, m._covars_ = m_step_typed(
            st, m.covariance_type, m.startprob_, m.transmat_, m.params, m.startprob_prior, m.transmat_prior,
            m.means_prior, m.means_weight, m.covars_prior, m.covars_weight, np.asarray(m.means_, dtype=np.float64),
            np.asarray(m._covars_, dtype=np.float64))
    baum_welch(models, batch, pack, lambda row, m: full_cov.split_stats(row, S, batch.D, m.n_components), update)


def _init_models(models, needs, dfeats, frames) -> None:
    """hmmlearn's ``_init`` for the models whose ``needs[w]`` is not empty (see :class:`GaussianHMM`).  ``dfeats``: the
    packed device features of ALL models, model after model, ``frames[w]`` of them per model (this rank's shard).  The
    models that need means share ONE batched k-means (G = their number); the column moments behind the covariances and
    the k-means threshold come from the same kernel.  The random draws run model by model in list order, each from the
    model's own ``random_state``."""
    from . import kmeans as km
    sel = [w for w, n in enumerate(needs) if "m" in n or "c" in n]
    seeds = {}
    for w, m in enumerate(models):
        if not needs[w]:
            continue
        S = m.n_components
        rs = check_random_state(m.random_state)
        if "s" in needs[w]:
            m.startprob_ = rs.dirichlet(np.full(S, 1.0 / S))
        if "t" in needs[w]:
            m.transmat_ = rs.dirichlet(np.full(S, 1.0 / S), size=S)
        if "m" in needs[w]:
            seeds[w] = kmeans_seed(rs)
    if not sel:
        return
    # the selected models' frames as the groups of one layout (the packed tensor itself when every model is selected)
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    if len(sel) == len(models):
        feats_sel = dfeats
    else:
        import torch
        feats_sel = torch.cat([dfeats[off[w]:off[w + 1]] for w in sel], dim=0)
    glen = [frames[w] for w in sel]
    stepper = km.Stepper(feats_sel, km.FrameTiles.build(glen, dfeats.device))
    count, mean, sqdev = km.column_moments(stepper)
    for g, w in enumerate(sel):
        m = models[w]
        if "c" in needs[w]:
            if count[g] < 2:
                raise ValueError(f"covariance initialisation needs at least 2 frames, model {w} has {int(count[g])}")
            if m.covariance_type == "diag":
                m._covars_ = np.tile(sqdev[g] / (count[g] - 1) + m.min_covar, (m.n_components, 1))
                continue
            # np.cov(X.T) + min_covar I in float64 on the device (run once per model)
            X = dfeats[off[w]:off[w + 1]].double()
            Xc = X - X.mean(dim=0, keepdim=True)
            cv = (Xc.T @ Xc / (X.shape[0] - 1)).cpu().numpy()
            cv = (cv + cv.T) / 2 + m.min_covar * np.eye(cv.shape[0])
            if m.covariance_type == "tied":
                m._covars_ = cv
            elif m.covariance_type == "full":
                m._covars_ = np.tile(cv, (m.n_components, 1, 1))
            else:
                m._covars_ = np.tile(cv.mean(), m.n_components)
    msel = [w for w in sel if "m" in needs[w]]
    if not msel:
        return
    if len({models[w].n_components for w in msel}) != 1:
        raise ValueError("models initialised together must share n_components")
    at = [sel.index(w) for w in msel]
    if len(msel) == len(sel):
        feats_m, moments = feats_sel, (count, mean, sqdev)
    else:
        import torch
        goff = np.concatenate([[0], np.cumsum(glen)]).astype(np.int64)
        feats_m = torch.cat([feats_sel[goff[g]:goff[g + 1]] for g in at], dim=0)
        moments = (count[at], mean[at], sqdev[at])
    centers, _, _, _ = km.kmeans(feats_m, [frames[w] for w in msel], models[msel[0]].n_components, n_init=10,
                                 seeds=[seeds[w] for w in msel], moments=moments)
    for g, w in enumerate(msel):
        models[w].means_ = centers[g]


class HMMLearnModel:
    """Same constructor, attributes and ``fit`` contract as the reference wrapper
    (``hmmlearn_hmm.py:11-108``): flat start from the global mean / variance of ``feature_set``,
    bidiagonal transitions with a_ii = exp(-1/(avg_frames_per_state-1)), startprob = e_0."""

    def __init__(self, num_states: int = 8, model_name: str = None, n_iter: int = 15, min_covar: float = 0.01):
        self.model_name = model_name
        self.num_states = num_states
        self.total_states = num_states + 2

        self.all_features = load_mfccs("feature_set")
        from .custom_hmm import pack_features
        packed = pack_features(self.all_features)   # one host->HBM copy for the three passes of the flat start
        self.global_mean = self.calc_global_mean(packed)
        self.global_cov = self.calc_global_cov(packed)

        self.model = GaussianHMM(n_components=self.total_states, covariance_type="diag", n_iter=n_iter,
                                 params="stmc", implementation="log", min_covar=min_covar, init_params="")
        self.model.means_ = np.tile(self.global_mean, (self.total_states, 1))
        self.model.covars_ = np.tile(self.global_cov, (self.total_states, 1))
        self.model.transmat_ = self.initialize_transmat()
        self.model.startprob_ = np.zeros(self.total_states)
        self.model.startprob_[0] = 1.0

    def initialize_transmat(self) -> np.ndarray:
        total_frames = sum(f.shape[1] for f in self.all_features)
        num_sequences = len(self.all_features)
        avg_frames = total_frames / num_sequences
        avg_frames_per_state = avg_frames / self.num_states
        aii = np.exp(-1 / (avg_frames_per_state - 1))
        aij = 1 - aii
        print("\nTransition probability initialization:")
        print(f"Total frames: {total_frames}")
        print(f"Number of sequences: {num_sequences}")
        print(f"Average frames per sequence: {avg_frames:.2f}")
        print(f"Average frames per state: {avg_frames_per_state:.2f}")
        print(f"Self-transition probability (aii): {aii:.3f}")
        print(f"Next-state transition probability (aij): {aij:.3f}")
        S = self.total_states
        transmat = np.zeros((S, S))
        transmat[0, 1] = 1.0
        for i in range(1, self.num_states + 1):
            transmat[i, i] = aii
            transmat[i, i + 1] = aij
        transmat[S - 1, S - 1] = 1.0
        return transmat

    def prepare_data(self, feature_set: List[np.ndarray]) -> np.ndarray:
        return np.concatenate([f.T for f in feature_set], axis=0)

    @staticmethod
    def _column_sums(feature_set, center=None):
        """Σ_frames x (``center`` None) or Σ_frames (x − center)² of the concatenated float32 features on the
        GPU, in numpy's own order for ``np.mean`` / ``np.var`` over axis 0 of a float32 array: one sequential
        float32 chain per coefficient (``sapr_colsum_f32``).  Returns (float32 sums [D], number of frames)."""
        import torch
        from .custom_hmm import pack_features
        pk = pack_features(feature_set)
        out = torch.empty(pk.D, dtype=torch.float32, device=pk.feats.device)
        c = None if center is None else torch.from_numpy(np.ascontiguousarray(center, dtype=np.float32)).to(pk.feats.device)
        _lib.check(_lib.load().sapr_colsum_f32(_lib.ptr(pk.feats), pk.total_frames, pk.D, _lib.ptr(c), _lib.ptr(out),
                                               _lib.current_stream()), "sapr_colsum_f32")
        return out.cpu().numpy(), pk.total_frames

    def calc_global_mean(self, feature_set: List[np.ndarray]) -> np.ndarray:
        """``np.mean(X, axis=0)`` of the float32 frames (hmmlearn_hmm.py:83-87): float32 result, bit-identical to
        numpy's (sequential float32 accumulation, then numpy's own division)."""
        sums, n = self._column_sums(feature_set)
        global_mean = np.true_divide(sums, n, out=sums, casting="unsafe")
        print(f"Global mean shape: {global_mean.shape}")
        return global_mean

    def calc_global_cov(self, feature_set: List[np.ndarray]) -> np.ndarray:
        """``np.var(X, axis=0)`` (hmmlearn_hmm.py:89-94): numpy's two-pass float32 form, mean first."""
        sums, n = self._column_sums(feature_set)
        mean = np.true_divide(sums, n, out=sums, casting="unsafe")
        sq, _ = self._column_sums(feature_set, center=mean)
        global_cov = np.true_divide(sq, n, out=sq, casting="unsafe")
        print(f"Global variance shape: {global_cov.shape}")
        print(f"Variance range: [{global_cov.min():.6f}, {global_cov.max():.6f}]")
        return global_cov

    def fit(self, feature_set: List[np.ndarray]):
        logging.info(f"Training {self.model_name} HMM using hmmlearn in {self.model.n_iter} iterations...")
        X = self.prepare_data(feature_set)
        lengths = [f.shape[1] for f in feature_set]
        try:
            self.model.fit(X, lengths)
            log_likelihood = self.model.score(X, lengths)
            return self.model, log_likelihood
        except Exception as e:  # the reference logs and returns None (hmmlearn_hmm.py:107-108)
            logging.error(f"Error occurred while training {self.model_name} HMM: {e}")

"""Full-covariance Gaussian HMMs: the family whose kernels are ``csrc/fullcov_ops.h`` over the per-model trellis of
``csrc/tile_trellis.h`` (host side: :mod:`sapr_amd.tile_family`), behind the C ABI of ``sapr_full_estep`` /
``sapr_full_viterbi`` (S states, D features, one Gaussian with a full covariance matrix per state).
:class:`sapr_amd.hmmlearn_hmm.GaussianHMM` runs its ``covariance_type`` "full" and "tied" through it; a tied model is
packed as S copies of its one matrix, the device only knows "full".

The host factorises: ``Sigma_s = L_s L_s^T`` (``np.linalg.cholesky``) and the pack carries ``Winv_s = L_s^-1`` and
``c_s = -(D log 2 pi + log|Sigma_s|) / 2``; the device evaluates ``c_s - |Winv_s (x - mu_s)|^2 / 2``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .tile_family import VOCAB_MODES, TileBatch, VocabPack, _vocab_scores, pack_head, stats_head

MAX_STATES, MAX_DIMS = 18, 39


def _torch():
    import torch
    return torch


def stats_width(S, D) -> int:
    n = C.c_int32(0)
    _lib.check(_lib.load().sapr_full_stats_width(S, D, C.byref(n)), "sapr_full_stats_width")
    return int(n.value)


def pack_layout(S, D):
    """(SP, DP, doubles per model): the padded shape the kernels run (S, D) at."""
    sp, dp, n = C.c_int32(0), C.c_int32(0), C.c_size_t(0)
    _lib.check(_lib.load().sapr_full_pack_layout(S, D, C.byref(sp), C.byref(dp), C.byref(n)), "sapr_full_pack_layout")
    return int(sp.value), int(dp.value), int(n.value)


def cholesky_lower(cov, name="full"):
    """``L`` with ``cov = L L^T``; a matrix that is not symmetric (``np.allclose``) or not positive-definite raises the
    ``ValueError`` hmmlearn's covariance check raises."""
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or not np.all(np.isfinite(cov)) or not np.allclose(cov, cov.T):
        raise ValueError(f"{name!r} covars must be symmetric, positive-definite")
    try:
        return np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError(f"{name!r} covars must be symmetric, positive-definite") from None


def _inv_lower(L):
    """L^-1 of a lower-triangular L, exactly lower triangular."""
    return np.tril(np.linalg.solve(L, np.eye(L.shape[0])))


def pack_models(params, S=None, name="full") -> np.ndarray:
    """``params``: W tuples ``(startprob[S_w], transmat[S_w, S_w], means[S_w, D], covars[S_w, D, D])`` that share D ->
    the kernels' operand block ``[W, doubles_per_model]`` float64 for ``S >= max S_w`` kernel states
    (include/sapr_hip.h).  States beyond a model's own are unreachable and emit nothing (``c = -inf``).  ``name`` is
    the covariance type the error message speaks of."""
    W = len(params)
    D = int(np.asarray(params[0][2]).shape[1])
    S = max(int(np.asarray(p[0]).shape[0]) for p in params) if S is None else int(S)
    SP, DP, n = pack_layout(S, D)
    out = np.zeros((W, n))
    with np.errstate(divide="ignore"):
        for w, (sp, tm, mu, cv) in enumerate(params):
            sp, tm, mu, cv = (np.asarray(a, dtype=np.float64) for a in (sp, tm, mu, cv))
            s = sp.shape[0]
            if tm.shape != (s, s) or mu.shape != (s, D) or cv.shape != (s, D, D) or s > S:
                raise ValueError("pack_models: the models must share the feature width")
            cc = np.full(SP, -np.inf)
            pmu = np.zeros((SP, DP))
            pmu[:s, :D] = mu
            wi = np.zeros((SP, DP, DP))
            for k in range(s):
                if k == 0 or not np.array_equal(cv[k], cv[k - 1]):  # (a tied model: S copies, factorised once)
                    L = cholesky_lower(cv[k], name)
                    fac = (-0.5 * (D * np.log(2 * np.pi) + 2.0 * np.log(np.diag(L)).sum()), _inv_lower(L))
                cc[k] = fac[0]
                wi[k, :D, :D] = fac[1]
            out[w] = np.concatenate([pack_head(sp, tm, SP), cc, pmu.ravel(), wi.ravel()])
    return out


def split_stats(row, S, D, S_model=None):
    """One model's row of ``sapr_full_estep``'s statistics (kernel state count S) -> a dict for the model's own
    ``S_model <= S`` states (the padding states carry exact zeros)."""
    row = np.asarray(row, dtype=np.float64)
    m = S if S_model is None else S_model
    st, o = stats_head(row, S, m)
    obs = row[o:o + S * D].reshape(S, D)[:m].copy()
    o += S * D
    oo = row[o:o + S * D * D].reshape(S, D, D)[:m].copy()
    return {**st, "obs": obs, "obs*obs.T": oo}


class FullCovBatch(TileBatch):
    """The :class:`sapr_amd.tile_family.TileBatch` of the full covariances: the utterances under the model
    ``utt_model[u]`` of W models of S kernel states (``sapr_full_estep``, ``sapr_full_viterbi``)."""
    STATS_WIDTH, WORKSPACE_BYTES = "sapr_full_stats_width", "sapr_full_workspace_bytes"
    ESTEP, VITERBI = "sapr_full_estep", "sapr_full_viterbi"
    pack_layout = staticmethod(pack_layout)

    @staticmethod
    def dims(o):
        return o.W, o.S, o.D


# ------------------------------------------------------------------------------------------
# scoring over the vocabulary: every utterance under every word model in one launch
# ------------------------------------------------------------------------------------------
class FullPack(VocabPack):
    """A vocabulary's operand block ready for the kernels: ``data`` float64 ``[W, doubles_per_model]``
    (:func:`pack_models`) with the shape it was packed for (W models, S kernel states = the largest model's, D
    features) and each model's own state count ``n_states``; the device copy is made once."""

    def __init__(self, data, S, D, n_states=None):
        super().__init__(data, S, D, pack_layout(int(S), int(D))[2], n_states)

    @staticmethod
    def from_params(params, name="full") -> "FullPack":
        """``params``: W tuples as :func:`pack_models` takes them; padded to the largest S of the vocabulary."""
        if len(params) == 0:
            raise ValueError("empty vocabulary")
        n_states = [int(np.asarray(p[0]).shape[0]) for p in params]
        D = int(np.asarray(params[0][2]).shape[1])
        return FullPack(pack_models(params, max(n_states), name=name), max(n_states), D, n_states)

    @staticmethod
    def from_models(models) -> "FullPack":
        """A list of fitted :class:`sapr_amd.hmmlearn_hmm.GaussianHMM` objects that share the feature width, of any
        ``covariance_type``: "tied" is packed as S copies of its matrix, "diag" and "spherical" as diagonal matrices."""
        for m in models:
            m._check()
        return FullPack.from_params([m._full_params() for m in models])

    def batch(self, feats, lengths, utt_model) -> FullCovBatch:
        """The utterances under ONE model each (``utt_model[u]``) of this vocabulary."""
        return FullCovBatch(feats, lengths, utt_model, self.W, self.S)

    def launch(self, feats, offsets, order, N, max_T, mode, score, best_word, word_post):
        torch = _torch()
        lib, dev, total = _lib.load(), feats.device, int(feats.shape[0])
        n = C.c_size_t(0)
        _lib.check(lib.sapr_full_vocab_workspace_bytes(N, total, self.W, self.S, self.D, C.byref(n)),
                   "sapr_full_vocab_workspace_bytes")
        ws_bytes = int(n.value)
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        _lib.check(lib.sapr_full_vocab(_lib.ptr(feats), _lib.ptr(offsets), _lib.ptr(order), N, total, self.D, max_T,
                                       _lib.ptr(self.device(dev)), self.W, self.S, VOCAB_MODES[mode],
                                       _lib.ptr(workspace), ws_bytes, _lib.ptr(score), _lib.ptr(best_word),
                                       _lib.ptr(word_post), _lib.current_stream()), "sapr_full_vocab")

    def vocab_scores(self, batch_or_feats, lengths=None, mode="forward", want_post=False):
        return vocab_scores(batch_or_feats, lengths, self, mode=mode, want_post=want_post)


def vocab_scores(batch_or_feats, lengths, pack_or_models, mode="forward", want_post=False):
    """Every utterance under EVERY word model in one call of ``sapr_full_vocab``: ``mode="forward"`` gives the forward
    log-likelihoods (``GaussianHMM.score`` per sequence), ``mode="viterbi"`` the Viterbi log-probabilities
    (``GaussianHMM.decode``'s), bit for bit what :class:`FullCovBatch` returns for each (utterance, model) pair.
    Returns ``tile_family.VocabScores`` of device tensors; the workspace is sized and owned here.  ``batch_or_feats``: a
    ``trellis.FeatureBatch`` (``lengths`` is ignored) or host / device ``feats`` with host ``lengths``.
    ``pack_or_models``: a :class:`FullPack` or a list of ``GaussianHMM`` objects (padded to the largest S of the
    vocabulary; D must match).  ``want_post`` (forward mode only): the posterior over the words."""
    return _vocab_scores(FullPack, batch_or_feats, lengths, pack_or_models, mode, want_post)

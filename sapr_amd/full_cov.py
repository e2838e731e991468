"""Full-covariance Gaussian HMMs over the HIP kernels of ``csrc/gmm_hmm.hip`` / ``csrc/fullcov_ops.h``: the C ABI of
``sapr_full_estep`` / ``sapr_full_viterbi`` (S states, D features, one Gaussian with a full covariance matrix per
state).  :class:`sapr_amd.hmmlearn_hmm.GaussianHMM` runs its ``covariance_type`` "full" and "tied" through it; a tied
model is packed as S copies of its one matrix, the device only knows "full".

The host factorises: ``Sigma_s = L_s L_s^T`` (``np.linalg.cholesky``) and the pack carries ``Winv_s = L_s^-1`` and
``c_s = -(D log 2 pi + log|Sigma_s|) / 2``; the device evaluates ``c_s - |Winv_s (x - mu_s)|^2 / 2``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .hmmlearn_hmm import VocabPack, _features_f32

MAX_STATES, MAX_DIMS = 18, 39
VOCAB_MODES = {"forward": _lib.FULL_VOCAB_FORWARD, "viterbi": _lib.FULL_VOCAB_VITERBI}


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
            ls = np.full(SP, -np.inf)
            ls[:s] = np.log(sp)
            lt = np.full((SP, SP), -np.inf)
            lt[:s, :s] = np.log(tm)
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
            out[w] = np.concatenate([ls, lt.ravel(), lt.T.ravel(), cc, pmu.ravel(), wi.ravel()])
    return out


def split_stats(row, S, D, S_model=None):
    """One model's row of ``sapr_full_estep``'s statistics (kernel state count S) -> a dict for the model's own
    ``S_model <= S`` states (the padding states carry exact zeros)."""
    row = np.asarray(row, dtype=np.float64)
    m = S if S_model is None else S_model
    o = 2
    start = row[o:o + S][:m].copy()
    o += S
    trans = row[o:o + S * S].reshape(S, S)[:m, :m].copy()
    o += S * S
    post = row[o:o + S][:m].copy()
    o += S
    obs = row[o:o + S * D].reshape(S, D)[:m].copy()
    o += S * D
    oo = row[o:o + S * D * D].reshape(S, D, D)[:m].copy()
    return {"nobs": row[0], "logprob": row[1], "start": start, "trans": trans, "post": post, "obs": obs,
            "obs*obs.T": oo}


class FullCovBatch:
    """A packed batch on the device, every utterance under the model ``utt_model[u]``: ``feats`` float32
    ``[total_frames, D]`` (device tensor, or a host array that is uploaded) and host ``lengths``; builds the tile
    layout (``trellis.TileLayout``) and owns the workspace for (W, S)."""

    def __init__(self, feats, lengths, utt_model, W, S):
        torch = _torch()
        from .trellis import TileLayout
        self.lib = _lib.load()
        dev = _lib.require_gpu()
        if not torch.is_tensor(feats):
            feats = torch.from_numpy(_features_f32(feats))
        feats = feats.to(dev)
        if feats.dtype != torch.float32 or feats.dim() != 2 or not feats.is_contiguous():
            raise ValueError("feats must be a contiguous float32 [total_frames, D] tensor")
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if self.lengths.size and self.lengths.min() < 0:
            raise ValueError("lengths must be >= 0")
        offs = np.zeros(self.lengths.size + 1, dtype=np.int64)
        np.cumsum(self.lengths, out=offs[1:])
        if feats.shape[0] != offs[-1]:
            raise ValueError("feats rows do not match sum(lengths)")
        um = np.asarray(utt_model, dtype=np.int64).reshape(-1)
        if um.shape != self.lengths.shape or (um.size and (um.min() < 0 or um.max() >= W)):
            raise ValueError("utt_model must name one model 0..W-1 per utterance")
        self.feats, self.dev = feats, dev
        self.offsets = torch.from_numpy(offs).to(dev)
        self.n_utts, self.total_frames = int(self.lengths.size), int(offs[-1])
        self.max_T = int(self.lengths.max()) if self.lengths.size else 0
        self.D, self.W, self.S = int(feats.shape[1]), int(W), int(S)
        self.layout = TileLayout.build(self.lengths, um, W, dev)
        self.width = stats_width(self.S, self.D)
        n = C.c_size_t(0)
        _lib.check(self.lib.sapr_full_workspace_bytes(self.total_frames, self.layout.n_tiles, self.S, self.D,
                                                      C.byref(n)), "sapr_full_workspace_bytes")
        self.ws_bytes = int(n.value)
        self.workspace = torch.empty(max(self.ws_bytes, 1), dtype=torch.uint8, device=dev)

    def _pack(self, pack):
        torch = _torch()
        if isinstance(pack, FullPack):
            if (pack.W, pack.S, pack.D) != (self.W, self.S, self.D):
                raise ValueError(f"pack is for (W, S, D) = {(pack.W, pack.S, pack.D)}, the batch for "
                                 f"{(self.W, self.S, self.D)}")
            return pack.device(self.dev)
        pack = np.ascontiguousarray(pack, dtype=np.float64)
        n = pack_layout(self.S, self.D)[2]
        if pack.shape != (self.W, n):
            raise ValueError(f"pack must be [W={self.W}, {n}] (pack_models), got {pack.shape}")
        return torch.from_numpy(pack).to(self.dev)

    def estep(self, pack, want_stats=True, want_post=False, want_path=False):
        """One ``sapr_full_estep`` -> device tensors ``(loglik[n_utts], stats[W, width] | None,
        post[total_frames, S] | None, path[total_frames] | None)``."""
        torch = _torch()
        dpack = self._pack(pack)
        lay = self.layout
        loglik = torch.full((self.n_utts,), float("-inf"), dtype=torch.float64, device=self.dev)
        stats = torch.zeros((self.W, self.width), dtype=torch.float64, device=self.dev) if want_stats else None
        post = torch.empty((self.total_frames, self.S), dtype=torch.float64, device=self.dev) if want_post else None
        path = torch.empty(self.total_frames, dtype=torch.int32, device=self.dev) if want_path else None
        _lib.check(self.lib.sapr_full_estep(
            _lib.ptr(self.feats), _lib.ptr(self.offsets), _lib.ptr(lay.slot_utt), _lib.ptr(lay.tile_model),
            _lib.ptr(lay.model_tile_off), self.n_utts, self.total_frames, lay.n_tiles, self.D, self.max_T,
            _lib.ptr(dpack), self.W, self.S, _lib.ptr(self.workspace), self.ws_bytes, _lib.ptr(loglik),
            _lib.ptr(stats), _lib.ptr(post), _lib.ptr(path), _lib.current_stream()), "sapr_full_estep")
        return loglik, stats, post, path

    def viterbi(self, pack):
        """One ``sapr_full_viterbi`` -> device tensors ``(logprob[n_utts], path[total_frames])``."""
        torch = _torch()
        dpack = self._pack(pack)
        lay = self.layout
        logprob = torch.full((self.n_utts,), float("-inf"), dtype=torch.float64, device=self.dev)
        path = torch.empty(self.total_frames, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.sapr_full_viterbi(
            _lib.ptr(self.feats), _lib.ptr(self.offsets), _lib.ptr(lay.slot_utt), _lib.ptr(lay.tile_model),
            self.n_utts, self.total_frames, lay.n_tiles, self.D, self.max_T, _lib.ptr(dpack), self.W, self.S,
            _lib.ptr(self.workspace), self.ws_bytes, _lib.ptr(logprob), _lib.ptr(path), _lib.current_stream()),
            "sapr_full_viterbi")
        return logprob, path


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
    Returns ``gmm_hmm.VocabScores`` of device tensors; the workspace is sized and owned here.  ``batch_or_feats``: a
    ``trellis.FeatureBatch`` (``lengths`` is ignored) or host / device ``feats`` with host ``lengths``.
    ``pack_or_models``: a :class:`FullPack` or a list of ``GaussianHMM`` objects (padded to the largest S of the
    vocabulary; D must match).  ``want_post`` (forward mode only): the posterior over the words."""
    from .gmm_hmm import _vocab_scores
    return _vocab_scores(FullPack, batch_or_feats, lengths, pack_or_models, mode, want_post)

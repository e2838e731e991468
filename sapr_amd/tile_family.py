"""What the emission families of the per-model trellis (``csrc/tile_trellis.h``) share on the host: the mixtures of
:mod:`sapr_amd.gmm_hmm` and the full covariances of :mod:`sapr_amd.full_cov`.

A family supplies its shape — ``(S, M, D)`` or ``(S, D)`` —, the names of its entry points, how its models are packed
behind the common head (:func:`pack_head`), how its statistics row continues after the common head
(:func:`stats_head`) and its M-step.  The rest is here: the validation of a packed batch
(:func:`packed_utterances`), the batch under one model per utterance (:class:`TileBatch`), the Baum-Welch loop
(:func:`baum_welch`) and the scoring over a vocabulary (:class:`VocabPack`, :func:`vocab_features`,
:func:`_vocab_scores`).  Nothing here imports a family.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

# one table for both families' scorers: _lib.FULL_VOCAB_FORWARD / _lib.FULL_VOCAB_VITERBI are the same 0 and 1
VOCAB_MODES = {"forward": _lib.GMM_VOCAB_FORWARD, "viterbi": _lib.GMM_VOCAB_VITERBI}


def _torch():
    import torch
    return torch


def _features_f32(X) -> np.ndarray:
    """The kernels read float32 features — what ``mfcc_extract.py:15-24`` produces and every reference call site
    passes (``hmmlearn_hmm.py:80-81``, ``decoder.py:59``).  hmmlearn itself would compute with a float64 ``X`` at full
    width, so silently narrowing one would change results: values that do not survive the round trip through
    float32 are refused instead (float64 arrays holding float32 values, integers etc. pass unchanged)."""
    Xa = np.asarray(X)
    out = np.ascontiguousarray(Xa, dtype=np.float32)
    if Xa.dtype != np.float32 and Xa.size and not np.array_equal(out.astype(Xa.dtype, copy=False), Xa, equal_nan=True):
        raise ValueError(f"features of dtype {Xa.dtype} do not round-trip through float32: the HIP kernels compute "
                         "on float32 features (the reference's MFCCs are float32); cast explicitly if the loss is "
                         "intended")
    return out


def packed_utterances(feats, lengths):
    """Utterances laid end to end, checked without a device: ``(feats, lengths int64[N], offsets int64[N + 1])``.
    ``feats`` comes back as it is if it is a tensor, as a contiguous float32 host array otherwise
    (:func:`_features_f32`)."""
    if hasattr(feats, "is_contiguous"):  # a tensor
        ok = feats.dtype == _torch().float32 and feats.dim() == 2 and feats.is_contiguous()
    else:
        feats = _features_f32(feats)
        ok = feats.ndim == 2
    if not ok:
        raise ValueError("feats must be a contiguous float32 [total_frames, D] tensor")
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.size and lengths.min() < 0:
        raise ValueError("lengths must be >= 0")
    offs = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=offs[1:])
    if feats.shape[0] != offs[-1]:
        raise ValueError("feats rows do not match sum(lengths)")
    return feats, lengths, offs


def _on_device(feats, dev):
    torch = _torch()
    return (feats if torch.is_tensor(feats) else torch.from_numpy(feats)).to(dev)


# ------------------------------------------------------------------------------------------
# the common head of an operand block and of a statistics row
# ------------------------------------------------------------------------------------------
def pack_head(startprob, transmat, SP) -> np.ndarray:
    """``log_start[SP]``, ``log_trans[SP, SP]`` and its transpose, flat: the head of every family's operand block.
    States beyond the model's own are unreachable (-inf)."""
    s = startprob.shape[0]
    ls = np.full(SP, -np.inf)
    lt = np.full((SP, SP), -np.inf)
    with np.errstate(divide="ignore"):
        ls[:s] = np.log(startprob)
        lt[:s, :s] = np.log(transmat)
    return np.concatenate([ls, lt.ravel(), lt.T.ravel()])


def stats_head(row, S, S_model=None):
    """The head of a statistics row of kernel state count S for the model's own ``S_model <= S`` states, and where
    the family's observation sums begin: ``({nobs, logprob, start, trans, post}, offset)``."""
    m = S if S_model is None else S_model
    o = 2 + S + S * S
    return ({"nobs": row[0], "logprob": row[1], "start": row[2:2 + S][:m].copy(),
             "trans": row[2 + S:o].reshape(S, S)[:m, :m].copy(), "post": row[o:o + S][:m].copy()}, o + S)


# ------------------------------------------------------------------------------------------
# the batch under one model per utterance
# ------------------------------------------------------------------------------------------
class TileBatch:
    """A packed batch on the device, every utterance under the model ``utt_model[u]``: ``feats`` float32
    ``[total_frames, D]`` (device tensor, or a host array that is uploaded) and host ``lengths``; builds the tile
    layout (``trellis.TileLayout``) and owns the workspace.  A family names its entry points (``STATS_WIDTH``,
    ``WORKSPACE_BYTES``, ``ESTEP``, ``VITERBI``), its ``pack_layout`` and ``dims(o)``: (W, the kernels' shape) of a
    batch or of a pack; ``shape`` is what follows W of ``dims(self)``, as the entry points take it."""

    def __init__(self, feats, lengths, utt_model, W, S):
        torch = _torch()
        from .trellis import TileLayout
        feats, self.lengths, offs = packed_utterances(feats, lengths)
        um = np.asarray(utt_model, dtype=np.int64).reshape(-1)
        if um.shape != self.lengths.shape or (um.size and (um.min() < 0 or um.max() >= W)):
            raise ValueError("utt_model must name one model 0..W-1 per utterance")
        self.lib = _lib.load()
        self.dev = dev = _lib.require_gpu()
        self.feats = _on_device(feats, dev)
        self.offsets = torch.from_numpy(offs).to(dev)
        self.n_utts, self.total_frames = int(self.lengths.size), int(offs[-1])
        self.max_T = int(self.lengths.max()) if self.lengths.size else 0
        self.D, self.W, self.S = int(feats.shape[1]), int(W), int(S)
        self.shape = self.dims(self)[1:]
        self.layout = TileLayout.build(self.lengths, um, W, dev)
        n = C.c_int32(0)
        _lib.check(getattr(self.lib, self.STATS_WIDTH)(*self.shape, C.byref(n)), self.STATS_WIDTH)
        self.width = int(n.value)
        n = C.c_size_t(0)
        _lib.check(getattr(self.lib, self.WORKSPACE_BYTES)(self.total_frames, self.layout.n_tiles, *self.shape,
                                                           C.byref(n)), self.WORKSPACE_BYTES)
        self.ws_bytes = int(n.value)
        self.workspace = torch.empty(max(self.ws_bytes, 1), dtype=torch.uint8, device=dev)

    def _pack(self, pack):
        if isinstance(pack, VocabPack):
            if self.dims(pack) != self.dims(self):
                raise ValueError(f"the pack was built for {self.dims(pack)}, the batch for {self.dims(self)}")
            return pack.device(self.dev)
        pack = np.ascontiguousarray(pack, dtype=np.float64)
        n = self.pack_layout(*self.shape)[-1]
        if pack.shape != (self.W, n):
            raise ValueError(f"pack must be [W={self.W}, {n}] (pack_models), got {pack.shape}")
        return _torch().from_numpy(pack).to(self.dev)

    def _call(self, name, dpack, tile_off, *outputs):
        lay = self.layout
        _lib.check(getattr(self.lib, name)(
            _lib.ptr(self.feats), _lib.ptr(self.offsets), _lib.ptr(lay.slot_utt), _lib.ptr(lay.tile_model), *tile_off,
            self.n_utts, self.total_frames, lay.n_tiles, self.D, self.max_T, _lib.ptr(dpack), self.W, *self.shape[:-1],
            _lib.ptr(self.workspace), self.ws_bytes, *(_lib.ptr(t) for t in outputs), _lib.current_stream()), name)
        return outputs

    def estep(self, pack, want_stats=True, want_post=False, want_path=False):
        """One E-step (``ESTEP``) -> device tensors ``(loglik[n_utts], stats[W, width] | None,
        post[total_frames, S] | None, path[total_frames] | None)``."""
        torch = _torch()
        dpack = self._pack(pack)
        loglik = torch.full((self.n_utts,), float("-inf"), dtype=torch.float64, device=self.dev)
        stats = torch.zeros((self.W, self.width), dtype=torch.float64, device=self.dev) if want_stats else None
        post = torch.empty((self.total_frames, self.S), dtype=torch.float64, device=self.dev) if want_post else None
        path = torch.empty(self.total_frames, dtype=torch.int32, device=self.dev) if want_path else None
        return self._call(self.ESTEP, dpack, (_lib.ptr(self.layout.model_tile_off),), loglik, stats, post, path)

    def viterbi(self, pack):
        """One Viterbi decoding (``VITERBI``) -> device tensors ``(logprob[n_utts], path[total_frames])``."""
        torch = _torch()
        dpack = self._pack(pack)
        logprob = torch.full((self.n_utts,), float("-inf"), dtype=torch.float64, device=self.dev)
        path = torch.empty(self.total_frames, dtype=torch.int32, device=self.dev)
        return self._call(self.VITERBI, dpack, (), logprob, path)


def baum_welch(models, batch, pack, split, update) -> None:
    """Baum-Welch over ``batch`` (a :class:`TileBatch` of every model's utterances) for models that are initialised
    and checked: per iteration ``pack(models)`` -> the operand block, one E-step, then for every model that has not
    converged ``split(row, model)`` -> its statistics, ``update(model, stats)`` (the family's M-step) and
    ``monitor_.report``."""
    active = [True] * len(models)
    for _ in range(max(m.n_iter for m in models)):
        if not any(active):
            break
        host = batch.estep(pack(models))[1].cpu().numpy()
        for w, m in enumerate(models):
            if not active[w]:
                continue
            st = split(host[w], m)
            update(m, st)
            m.monitor_.report(float(st["logprob"]))
            if m.monitor_.converged:
                active[w] = False


# ------------------------------------------------------------------------------------------
# scoring over the vocabulary: every utterance under every word model in one launch
# ------------------------------------------------------------------------------------------
class VocabPack:
    """A vocabulary's operand block ready for the kernels: ``data`` float64 ``[W, doubles_per_model]`` (the family's
    ``pack_models``) with the shape it was packed for (W models, S kernel states = the largest model's, D features)
    and each model's own state count ``n_states``; the device copy is made once.  The families
    (``gmm_hmm.GmmPack``, ``full_cov.FullPack``) add what is theirs: how a pack is built, the per-model batch class
    (:meth:`batch`) and the entry point that scores the vocabulary (:meth:`launch`, :meth:`vocab_scores`)."""

    def __init__(self, data, S, D, doubles_per_model, n_states=None):
        self.data = np.ascontiguousarray(data, dtype=np.float64)
        self.W, self.S, self.D = int(self.data.shape[0]), int(S), int(D)
        if self.data.ndim != 2 or self.data.shape[1] != doubles_per_model:
            raise ValueError(f"pack must be [W, {doubles_per_model}] (pack_models), got {self.data.shape}")
        self.n_states = [self.S] * self.W if n_states is None else [int(k) for k in n_states]
        self._dev = None

    def device(self, dev):
        if self._dev is None or self._dev.device != dev:
            self._dev = _torch().from_numpy(self.data).to(dev)
        return self._dev


@dataclass
class VocabScores:
    score: "object"      # [N, W] f64: forward log-likelihood or Viterbi log-probability under every word model
    best_word: "object"  # [N] i32 (first strict maximum in model order; -1 if no score beats -inf)
    word_post: "object"  # [N, W] f64 posterior over the words under a uniform prior (forward mode), or None


def vocab_features(batch_or_feats, lengths=None):
    """The utterances of the vocabulary scorers on the device: ``(feats[total_frames, D] float32, offsets int64[N + 1],
    order int32[N] | None, host lengths, max_T)``.  A ``trellis.FeatureBatch`` brings its length-sorted ``order`` (the
    zero columns it appends up to the single-Gaussian kernels' widths are cut off again: these kernels read rows of
    the models' own width); host ``feats`` / ``lengths`` are uploaded and sorted here."""
    torch = _torch()
    if hasattr(batch_or_feats, "offsets") and hasattr(batch_or_feats, "order"):
        b = batch_or_feats
        feats = b.feats if b.D == b.D_model else b.feats[:, :b.D_model].contiguous()
        return feats, b.offsets, b.order, np.asarray(b.lengths, dtype=np.int64), int(b.max_T)
    if lengths is None:
        raise ValueError("lengths are needed with a feature array")
    feats, lengths, offs = packed_utterances(batch_or_feats, lengths)
    dev = _lib.require_gpu()
    order = np.argsort(-lengths, kind="stable").astype(np.int32)
    return (_on_device(feats, dev), torch.from_numpy(offs).to(dev), torch.from_numpy(order).to(dev), lengths,
            int(lengths.max()) if lengths.size else 0)


def _vocab_scores(pack_type, batch_or_feats, lengths, pack_or_models, mode, want_post) -> VocabScores:
    """The one implementation behind ``gmm_hmm.vocab_scores`` and ``full_cov.vocab_scores``: ``pack_type`` is the
    family's :class:`VocabPack`, whose ``launch`` calls the family's entry point."""
    torch = _torch()
    if mode not in VOCAB_MODES:
        raise ValueError(f"mode must be one of {sorted(VOCAB_MODES)}, got {mode!r}")
    if want_post and mode != "forward":
        raise ValueError("want_post needs mode='forward': a soft-max of path scores is not a posterior")
    pack = pack_or_models if isinstance(pack_or_models, pack_type) else pack_type.from_models(list(pack_or_models))
    feats, offsets, order, lengths, max_T = vocab_features(batch_or_feats, lengths)
    if int(feats.shape[1]) != pack.D:
        raise ValueError(f"the utterances have {int(feats.shape[1])} features, the models {pack.D}")
    dev = feats.device
    N, W = int(lengths.size), pack.W
    score = torch.empty((N, W), dtype=torch.float64, device=dev)
    best_word = torch.empty(N, dtype=torch.int32, device=dev)
    word_post = torch.empty((N, W), dtype=torch.float64, device=dev) if want_post else None
    pack.launch(feats, offsets, order, N, max_T, mode, score, best_word, word_post)
    return VocabScores(score, best_word, word_post)

"""Connected-word recognition over the HIP kernels of ``csrc/connected.hip``: a one-pass Viterbi search over the word
loop, in which the end of any word may be followed by the start of any word, so a recording of several words in a row
comes back as a word string with its segment boundaries (the other scorers label a whole recording as ONE word).

Two stages (include/sapr_hip.h).  Stage 1 evaluates ``logb[total_frames, W * SP]`` for the vocabulary's emission
family: ``sapr_connected_emit_diag`` for diagonal-Gaussian word models ("diag", "spherical"),
``sapr_connected_emit_gmm`` for Gaussian mixtures (``GMMHMM``) over the vocabulary's ``gmm_hmm.GmmPack``,
``sapr_connected_emit_full`` for a vocabulary with a "full" or "tied" model over its ``full_cov.FullPack`` (both packs
are read as they are).  Stage 2, ``sapr_connected_viterbi``, runs the recursion over any ``logb`` it is given.  The CPU
restatement ``tests/_connected_ref.py`` is the definition; the recursion reproduces it bit for bit.

A network that carries a :class:`WordBigram` — word-pair log scores ``lm[v, w]``, ``lm_start``, ``lm_end``, with
``-inf`` for what a grammar forbids — is decoded by ``sapr_connected_bigram`` (``csrc/connected_bigram.hip``) instead:
the same recursion with a per-word entry score ``N(w) = max_v (X(v) + lm[v, w])``.  The definition is
``tests/_bigram_ref.py``.  Alignment and embedded training do not read the bigram.

Where the number of words is known or bounded (a PIN, a phone number), ``sapr_connected_levels``
(``csrc/connected_levels.hip``) runs level building over the same loop under the same language model: one pass returns
the best string of exactly k words for every k up to a bound of at most 8, and ``sapr_connected_levels_backtrace``
walks back from a known count, a range of counts or each count in turn (:func:`connected_levels`,
:class:`LevelResult`, ``connected_decode(..., n_words=, max_words=)``; the definition is ``tests/_levels_ref.py``).

The alternatives a rescoring pass or a confirmation dialogue needs: ``sapr_connected_nbest``
(``csrc/connected_nbest.hip``) returns the ``n_best <= 8`` best DISTINCT word strings of every utterance with their
Viterbi scores, whatever their word counts, in one recursion over the same ``logb`` under the same language model and
without a back-pointer workspace; forced alignment gives any of them its boundaries (:func:`connected_nbest`,
:class:`NBestResult`, ``connected_decode(..., n_best=)``; the definition is ``tests/_nbest_ref.py``).

Rescoring and pruning: a word lattice keeps every alternative instead of the best few: ``sapr_connected_lattice``
(``csrc/connected_lattice.hip``) leaves, for every (frame, word), the score of the best path that ends the word there and
the frame at which that path entered it — 20 W bytes per frame —, and ``sapr_connected_lattice_backward`` /
``sapr_connected_lattice_walk`` prune that table to a beam or return its best string under ANOTHER language model
without emission or recursion (:func:`connected_lattice`, :class:`WordLattice`, ``connected_decode(..., lattice=True)``;
the definition is ``tests/_lattice_ref.py``).  ``sapr_connected_lattice_posteriors`` runs forward-backward in the sum
semiring over the same records — link and word posteriors and the likelihood of the lattice under any tables and
acoustic scale (:meth:`WordLattice.posteriors`, :class:`LatticePosteriors`; ``tests/_lattice_post_ref.py``).

Recordings that are still arriving: ``sapr_connected_online_step`` / ``sapr_connected_online_commit``
(``csrc/connected_online.hip``) carry the bigram recursion's trellis column from chunk to chunk of B streams and hand
the path out by partial traceback — everything before the frame at which the back-traces of all live hypotheses pass
through one state is final —, over a ring of ``window`` back-pointer rows per stream; the final answer is the offline
decoder's bit for bit (:class:`ConnectedSession`, ``Decoder.open_connected``; the definition is
``tests/_online_ref.py``).

How much to believe a decoded string: ``sapr_connected_posteriors`` (``csrc/connected_loop_fb.hip``) runs
forward-backward over the same loop under the same language model — the sum over every word string where the search
takes the best one — and returns the total log-likelihood, the per-frame word and word-boundary posteriors and, from
these, a confidence per decoded segment (:func:`connected_posteriors`, ``connected_decode(..., posteriors=True)``;
the definition is ``tests/_loop_fb_ref.py``).

Forced alignment is the inverse question — the words of a recording are known, where does each begin and end:
``sapr_connected_align`` (``csrc/connected_align.hip``) runs the Viterbi recursion over the left-to-right chain of an
utterance's own transcript, on the same ``logb`` (:func:`align_viterbi`, :func:`connected_align`; the definition is
``tests/_align_ref.py``).

Discriminative training: maximum mutual information over the word loop with the extended Baum-Welch update
(:func:`mmi_estep`, :func:`mmi_update`, :func:`mmi_fit`).  The numerator is the embedded E-step over the transcript's
chain, the denominator forward-backward over the word loop on the same ``logb``; ``sapr_connected_loop_stats``
(``csrc/connected_loop_stats.hip``, :func:`loop_stats`) reduces the loop's state posteriors to per-word statistics rows
on the device (the definition is ``tests/_mmi_ref.py``).
"""
from __future__ import annotations

import copy
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

MAX_STATES, MAX_DIMS, MAX_FLAT = 18, 39, 256
_TINY = np.finfo(float).tiny


def _torch():
    import torch
    return torch


def layout(W, S, D=1):
    """(SP, DP, R): the padded shape the kernels run (W, S, D) at; R = W * SP flat states."""
    sp, dp, r = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.load().sapr_connected_layout(W, S, D, C.byref(sp), C.byref(dp), C.byref(r)),
               "sapr_connected_layout")
    return int(sp.value), int(dp.value), int(r.value)


def _workspace_bytes(entry, *sizes) -> int:
    """``entry(*sizes, &bytes)`` of the library: the workspace one call at these sizes takes."""
    n = C.c_size_t(0)
    _lib.check(getattr(_lib.load(), entry)(*sizes, C.byref(n)), entry)
    return int(n.value)


def _workspace(entry, dev, *sizes):
    """``(workspace, bytes)``: the uninitialised device bytes one call at these sizes takes, as the library's size
    function ``entry`` counts them (an empty workspace is one byte, so that it has an address)."""
    torch = _torch()
    ws_bytes = _workspace_bytes(entry, *sizes)
    return torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev), ws_bytes


def _stats_width(entry, *sizes) -> int:
    """``entry(*sizes, &width)`` of the library: the doubles of one statistics row at these sizes."""
    n = C.c_int32(0)
    _lib.check(getattr(_lib.load(), entry)(*sizes, C.byref(n)), entry)
    return int(n.value)


def _n_utts(batch_or_feature_list) -> int:
    """The utterances of a ``trellis.FeatureBatch`` or of a list of feature arrays, without touching a device."""
    b = batch_or_feature_list
    return len(b.lengths) if hasattr(b, "offsets") and hasattr(b, "order") else len(b)


def workspace_bytes(total_frames, n_utts, W, S) -> int:
    return _workspace_bytes("sapr_connected_workspace_bytes", total_frames, n_utts, W, S)


def emit_operands(means, vars_, gconst, n_states=None) -> np.ndarray:
    """The operand block of ``sapr_connected_emit_diag`` from the arrays ``sapr_diag_pack`` takes (``means[W, S, D]``,
    ``vars[W, S, D]``, ``gconst[W, S]``): float64 ``[W * SP, 1 + 2 DP]``, per flat state ``{gconst, mean[DP],
    1 / var[DP]}``.  Padding features carry mean 0 and coefficient 0; the states from ``n_states[w]`` on (and up to SP)
    carry ``gconst = +inf`` and emit ``-inf``."""
    means = np.asarray(means, dtype=np.float64)
    vars_ = np.asarray(vars_, dtype=np.float64)
    gconst = np.asarray(gconst, dtype=np.float64)
    W, S, D = means.shape
    if vars_.shape != (W, S, D) or gconst.shape != (W, S):
        raise ValueError("inconsistent model shapes")
    SP, DP, R = layout(W, S, D)
    n_states = [S] * W if n_states is None else list(n_states)
    ops = np.zeros((W, SP, 1 + 2 * DP))
    ops[:, :, 0] = np.inf
    for w in range(W):
        k = int(n_states[w])
        ops[w, :k, 0] = gconst[w, :k]
        ops[w, :k, 1:1 + D] = means[w, :k]
        ops[w, :k, 1 + DP:1 + DP + D] = 1.0 / vars_[w, :k]
    return ops.reshape(R, 1 + 2 * DP)


FAMILIES = ("diag", "gmm", "full")
_GAUSS_ATTRS = ("startprob_", "transmat_", "means_", "_covars_")
_GMM_ATTRS = ("startprob_", "transmat_", "weights_", "means_", "covars_")


def vocabulary_family(models, names=None, implementation=None) -> str:
    """The emission family a vocabulary is decoded with — "diag" (only "diag" / "spherical" ``GaussianHMM``), "full"
    (a ``GaussianHMM`` vocabulary in which any model is "full" or "tied") or "gmm" (``GMMHMM``) — after checking,
    before anything is packed, that every model is one of the family's class and carries fitted parameters.  A model
    that does not is refused with a ``ValueError`` that names it (``names[i]``, or its index).
    ``implementation``: "gmmhmm" demands mixtures and "hmmlearn" ``GaussianHMM`` models (a decoder's vocabulary);
    ``None`` takes a vocabulary that holds a ``GMMHMM`` as mixtures."""
    from .gmm_hmm import GMMHMM
    models = list(models)
    if not models:
        raise ValueError("empty vocabulary")

    def label(i):
        return f"word {names[i]!r}" if names is not None else f"model {i}"

    def missing(m, attrs):
        return [a for a in attrs if getattr(m, a, None) is None]

    if implementation == "gmmhmm" or (implementation is None and any(isinstance(m, GMMHMM) for m in models)):
        for i, m in enumerate(models):
            if not isinstance(m, GMMHMM):
                raise ValueError(f"{label(i)}: a {type(m).__name__} is not a GMMHMM; connected-word decoding with "
                                 f"implementation='gmmhmm' serves fitted GMMHMM models")
            if missing(m, _GMM_ATTRS):
                raise ValueError(f"{label(i)}: the GMMHMM (implementation='gmmhmm') is not fitted: "
                                 f"{', '.join(missing(m, _GMM_ATTRS))} missing")
        return "gmm"
    types = [getattr(m, "covariance_type", "diag") for m in models]
    full = any(ct in ("full", "tied") for ct in types)
    for i, (m, ct) in enumerate(zip(models, types)):
        if isinstance(m, GMMHMM):
            raise ValueError(f"{label(i)}: a GMMHMM is served by implementation='gmmhmm', not by "
                             f"implementation={implementation!r}")
        if ct not in ("diag", "spherical", "full", "tied"):
            raise ValueError(f"{label(i)}: connected-word decoding serves 'diag', 'spherical', 'full' and 'tied' "
                             f"models; got covariance_type={ct!r}")
        if missing(m, _GAUSS_ATTRS):
            raise ValueError(f"{label(i)}: the model with covariance_type={ct!r} is not fitted: "
                             f"{', '.join(missing(m, _GAUSS_ATTRS))} missing")
        if full and not (hasattr(m, "_check") and hasattr(m, "_full_params")):
            raise ValueError(f"{label(i)}: a {type(m).__name__} with covariance_type={ct!r} cannot join a vocabulary "
                             f"that holds a 'full' or 'tied' model: its members must be GaussianHMM objects")
    return "full" if full else "diag"


class WordBigram:
    """A word-pair language model over a vocabulary of W words, in log scores (float64): ``lm[v, w]`` is added when
    word ``w`` follows word ``v`` (the same word may follow itself), ``lm_start[w]`` when an utterance begins with
    ``w``, ``lm_end[v]`` when it ends with ``v``.  ``-inf`` forbids a pair, a first or a last word, so a finite-state
    word-pair grammar is a table of 0.0 and ``-inf`` (:meth:`from_grammar`).  A network that carries one
    (``ConnectedNetwork(bigram=...)``) is decoded by ``sapr_connected_bigram``; the definition is
    ``tests/_bigram_ref.py``."""

    def __init__(self, lm, lm_start, lm_end):
        self.lm = np.ascontiguousarray(lm, dtype=np.float64)
        self.lm_start = np.ascontiguousarray(lm_start, dtype=np.float64)
        self.lm_end = np.ascontiguousarray(lm_end, dtype=np.float64)
        if self.lm.ndim != 2 or self.lm.shape[0] != self.lm.shape[1] or self.lm.shape[0] == 0:
            raise ValueError(f"lm must be [W, W] with W >= 1, got {self.lm.shape}")
        self.W = int(self.lm.shape[0])
        if self.lm_start.shape != (self.W,) or self.lm_end.shape != (self.W,):
            raise ValueError(f"lm_start and lm_end must be [W={self.W}], got {self.lm_start.shape} and "
                             f"{self.lm_end.shape}")

    @staticmethod
    def from_transcripts(transcripts, W, add_k=1.0) -> "WordBigram":
        """Add-k smoothed log-probabilities from word strings (sequences of vocabulary indices 0..W-1; an empty string
        counts nothing).  Row ``v`` is normalised over the W successor words plus the end of the string:
        ``lm[v, w] = log((n(v, w) + k) / (n(v, .) + n(v, end) + k (W + 1)))`` and ``lm_end[v]`` the same with
        ``n(v, end)``; ``lm_start[w] = log((n(start, w) + k) / (n(start, .) + k W))``.  With ``add_k=0`` an unseen
        pair is ``-inf`` (and a word that never occurs has a row of ``-inf``)."""
        W = int(W)
        if W < 1:
            raise ValueError("W must be >= 1")
        k = float(add_k)
        if not k >= 0.0:
            raise ValueError(f"add_k must be >= 0, got {add_k!r}")
        pair = np.zeros((W, W + 1))
        first = np.zeros(W)
        for u, words in enumerate(transcripts):
            words = np.asarray(words, dtype=np.int64).reshape(-1)
            if words.size == 0:
                continue
            if words.min() < 0 or words.max() >= W:
                raise ValueError(f"transcript {u} names a word outside the vocabulary 0..{W - 1}")
            first[words[0]] += 1.0
            for a, b in zip(words[:-1], words[1:]):
                pair[a, b] += 1.0
            pair[words[-1], W] += 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            rows = np.log((pair + k) / (pair.sum(axis=1, keepdims=True) + k * (W + 1)))
            start = np.log((first + k) / (first.sum() + k * W))
        rows = np.where(np.isnan(rows), -np.inf, rows)   # (0 / 0: a word that never occurs, without smoothing)
        start = np.where(np.isnan(start), -np.inf, start)
        return WordBigram(rows[:, :W], start, rows[:, W])

    @staticmethod
    def from_grammar(W, pairs, starts=None, ends=None) -> "WordBigram":
        """A word-pair grammar: 0.0 for every ``(v, w)`` in ``pairs`` and ``-inf`` elsewhere; ``starts`` / ``ends``:
        the words an utterance may begin / end with (``None``: any)."""
        W = int(W)
        if W < 1:
            raise ValueError("W must be >= 1")

        def index(w, what):
            if not 0 <= int(w) < W:
                raise ValueError(f"{what} names word {w!r} outside the vocabulary 0..{W - 1}")
            return int(w)

        lm = np.full((W, W), -np.inf)
        for v, w in pairs:
            lm[index(v, "pairs"), index(w, "pairs")] = 0.0
        lm_start = np.zeros(W) if starts is None else np.full(W, -np.inf)
        lm_end = np.zeros(W) if ends is None else np.full(W, -np.inf)
        for w in ([] if starts is None else starts):
            lm_start[index(w, "starts")] = 0.0
        for w in ([] if ends is None else ends):
            lm_end[index(w, "ends")] = 0.0
        return WordBigram(lm, lm_start, lm_end)

    def scaled(self, scale, word_penalty=0.0) -> "WordBigram":
        """``scale * lm + word_penalty`` with ``lm_start`` and ``lm_end`` scaled but not penalised: the usual
        language-model weight and word insertion penalty (one penalty per word boundary, as the word loop's).
        ``scale`` must be >= 0; ``0 * -inf`` stays ``-inf`` (a forbidden pair stays forbidden)."""
        scale = float(scale)
        if not scale >= 0.0:
            raise ValueError(f"scale must be >= 0, got {scale!r}")

        def times(a):
            with np.errstate(invalid="ignore"):
                out = scale * a
            return np.where(np.isnan(out) & ~np.isnan(a), -np.inf, out)

        return WordBigram(times(self.lm) + np.float64(word_penalty), times(self.lm_start), times(self.lm_end))


class ConnectedNetwork:
    """The word loop: W word models padded to S = the largest model's states.  ``log_start[W, S]``,
    ``log_trans[W, S, S]``, ``log_exit[W, S]`` (``-inf``: a word may not end in this state; a padded state has ``-inf``
    everywhere) and the scalar ``word_penalty`` added once per word boundary.  Built from models
    (:meth:`from_models`) it also carries its emission ``family``: "diag" with the diagonal-Gaussian parameters
    ``means``, ``vars``, ``gconst``; "gmm" or "full" with the ``tile_family.VocabPack`` it was built from (``pack``: a
    ``gmm_hmm.GmmPack`` or a ``full_cov.FullPack``, whose device copy the emission reads in place).  ``bigram``: a
    :class:`WordBigram` over the W words; the decoding entry points then run ``sapr_connected_bigram``.  Such a
    network takes its penalty through ``WordBigram.scaled``: its own ``word_penalty`` must be 0.0."""

    def __init__(self, log_start, log_trans, log_exit, word_penalty=0.0, n_states=None, means=None, vars_=None,
                 gconst=None, family="diag", pack=None, bigram=None):
        self.log_start = np.ascontiguousarray(log_start, dtype=np.float64)
        self.log_trans = np.ascontiguousarray(log_trans, dtype=np.float64)
        self.log_exit = np.ascontiguousarray(log_exit, dtype=np.float64)
        if self.log_start.ndim != 2:
            raise ValueError("log_start must be [W, S]")
        self.W, self.S = (int(k) for k in self.log_start.shape)
        if self.log_trans.shape != (self.W, self.S, self.S) or self.log_exit.shape != (self.W, self.S):
            raise ValueError("log_trans must be [W, S, S] and log_exit [W, S]")
        self.word_penalty = float(word_penalty)
        self.n_states = [self.S] * self.W if n_states is None else [int(k) for k in n_states]
        self.means = None if means is None else np.ascontiguousarray(means, dtype=np.float64)
        self.vars = None if vars_ is None else np.ascontiguousarray(vars_, dtype=np.float64)
        self.gconst = None if gconst is None else np.ascontiguousarray(gconst, dtype=np.float64)
        if family not in FAMILIES:
            raise ValueError(f"family must be one of {FAMILIES}, got {family!r}")
        if (family == "diag") != (pack is None):
            raise ValueError("the 'gmm' and 'full' families come with their VocabPack, 'diag' with means / vars / gconst")
        if pack is not None and (pack.W, pack.S) != (self.W, self.S):
            raise ValueError(f"the pack was built for (W, S) = {(pack.W, pack.S)}, the network for {(self.W, self.S)}")
        self.family, self.pack = family, pack
        self.D = int(pack.D) if pack is not None else (0 if self.means is None else int(self.means.shape[2]))
        self.SP, self.DP, self.R = layout(self.W, self.S, max(self.D, 1))
        if bigram is not None:
            if not isinstance(bigram, WordBigram):
                raise ValueError(f"bigram must be a WordBigram, got a {type(bigram).__name__}")
            if bigram.W != self.W:
                raise ValueError(f"the bigram is over {bigram.W} words, the network over {self.W}")
            if self.word_penalty != 0.0:
                raise ValueError(f"a network with a bigram takes its penalty through WordBigram.scaled(scale, "
                                 f"word_penalty): its own word_penalty must be 0.0, got {self.word_penalty!r}")
        self.bigram = bigram
        self._dev = self._dev_lm = self._dev_loop_lm = None

    @staticmethod
    def from_models(models, exit_states="last", word_penalty=0.0, names=None, implementation=None,
                    pack=None, bigram=None) -> "ConnectedNetwork":
        """``models``: the fitted word models of one family (:func:`vocabulary_family` decides and validates; ``names``
        and ``implementation`` are what its messages speak of):

        * only "diag" / "spherical" ``GaussianHMM`` objects that share the feature width, read through the parameters
          ``trellis.DiagModelPack.from_models`` reads (``startprob_``, ``transmat_``, ``means_``, ``_covars_``;
          variances floored at float64 tiny, ``gconst = D log 2 pi + sum log var``);
        * ``GaussianHMM`` objects of which any is "full" or "tied": the whole vocabulary goes through
          ``full_cov.FullPack.from_models`` ("diag" / "spherical" members as diagonal matrices), as in the isolated-word
          scorer;
        * ``GMMHMM`` objects that share ``n_mix`` and the feature width (``gmm_hmm.GmmPack.from_models``).

        ``pack``: the vocabulary's ``VocabPack`` if the caller has built it already.  A mixed number of states is
        padded.  ``exit_states``: ``"last"`` (a word ends in its model's own last state), ``"any"``, or an array
        ``[W, S]`` of log exit scores."""
        models = list(models)
        family = vocabulary_family(models, names, implementation)
        means = vars_ = gconst = None
        if family == "diag":
            n_states = [int(np.asarray(m.startprob_).shape[0]) for m in models]
            D = int(np.asarray(models[0].means_).shape[1])
            W, S = len(models), max(n_states)
            log_start = np.full((W, S), -np.inf)
            log_trans = np.full((W, S, S), -np.inf)
            means = np.zeros((W, S, D))
            vars_ = np.ones((W, S, D))
            gconst = np.full((W, S), np.inf)
            with np.errstate(divide="ignore"):
                for w, (m, k) in enumerate(zip(models, n_states)):
                    mu = np.asarray(m.means_, dtype=np.float64)
                    if mu.shape != (k, D):
                        raise ValueError("the models must share the feature width")
                    cv = np.asarray(m._covars_, dtype=np.float64)
                    cv = np.broadcast_to(cv[:, None], mu.shape) if cv.ndim == 1 else cv  # (spherical)
                    var = np.maximum(cv, _TINY)
                    log_start[w, :k] = np.log(np.asarray(m.startprob_, dtype=np.float64))
                    log_trans[w, :k, :k] = np.log(np.asarray(m.transmat_, dtype=np.float64))
                    means[w, :k] = mu
                    vars_[w, :k] = var
                    gconst[w, :k] = D * np.log(2 * np.pi) + np.log(var).sum(axis=-1)
        else:
            if pack is None:
                if family == "gmm":
                    from .gmm_hmm import GmmPack
                    pack = GmmPack.from_models(models)  # (refuses models that do not share n_mix and the width)
                else:
                    from .full_cov import FullPack
                    pack = FullPack.from_models(models)
            # the head of every model in the pack (tile_family.pack_head): log_start[SP], log_trans[SP][SP] — the very
            # values the per-model kernels run on
            n_states, (W, S) = list(pack.n_states), (pack.W, pack.S)
            SP = layout(W, S, pack.D)[0]
            log_start = pack.data[:, :SP][:, :S].copy()
            log_trans = pack.data[:, SP:SP + SP * SP].reshape(W, SP, SP)[:, :S, :S].copy()
        if isinstance(exit_states, str):
            if exit_states not in ("last", "any"):
                raise ValueError(f"exit_states must be 'last', 'any' or an array [W, S], got {exit_states!r}")
            log_exit = np.full((W, S), -np.inf)
            for w, k in enumerate(n_states):
                if exit_states == "last":
                    log_exit[w, k - 1] = 0.0
                else:
                    log_exit[w, :k] = 0.0
        else:
            log_exit = np.array(exit_states, dtype=np.float64)
            if log_exit.shape != (W, S):
                raise ValueError(f"exit_states must be [W={W}, S={S}], got {log_exit.shape}")
            for w, k in enumerate(n_states):
                log_exit[w, k:] = -np.inf
        return ConnectedNetwork(log_start, log_trans, log_exit, word_penalty, n_states, means, vars_, gconst, family,
                                pack, bigram)

    def device(self, dev):
        """The device copies ``(log_start, log_trans, log_exit, ops | None)``; made once per device.  ``ops`` is the
        operand block of the family's emission: :func:`emit_operands` for "diag", the pack's own device copy else.
        A network with a bigram uploads ``(lm, lm_start, lm_end)`` beside them (``_dev_lm``)."""
        torch = _torch()
        if self.bigram is not None and (self._dev_lm is None or self._dev_lm[0].device != dev):
            self._dev_lm = tuple(torch.from_numpy(a).to(dev)
                                 for a in (self.bigram.lm, self.bigram.lm_start, self.bigram.lm_end))
        if self._dev is None or self._dev[0].device != dev:
            ops = None
            if self.pack is not None:
                ops = self.pack.device(dev)
            elif self.means is not None:
                ops = torch.from_numpy(emit_operands(self.means, self.vars, self.gconst, self.n_states)).to(dev)
            self._dev = tuple(torch.from_numpy(a).to(dev) for a in (self.log_start, self.log_trans, self.log_exit)) \
                + (ops,)
        return self._dev

    def loop_lm(self):
        """The language model the word loop runs under, on the host: the bigram's ``(lm, lm_start, lm_end)``, or
        ``lm == word_penalty``, ``lm_start == lm_end == 0`` for a network without one."""
        if self.bigram is not None:
            return self.bigram.lm, self.bigram.lm_start, self.bigram.lm_end
        return np.full((self.W, self.W), np.float64(self.word_penalty)), np.zeros(self.W), np.zeros(self.W)

    def device_lm(self, dev):
        """The device copies of :meth:`loop_lm`, made once per device beside the tables: one kernel serves a network
        with a bigram and one without (``sapr_connected_posteriors``)."""
        torch = _torch()
        if self.bigram is not None:
            self.device(dev)
            return self._dev_lm
        if self._dev_loop_lm is None or self._dev_loop_lm[0].device != dev:
            self._dev_loop_lm = tuple(torch.from_numpy(a).to(dev) for a in self.loop_lm())
        return self._dev_loop_lm


@dataclass
class ConnectedPosteriors:
    """Forward-backward over the word loop (``sapr_connected_posteriors``; the definition is
    ``tests/_loop_fb_ref.py``): the sum over every word string the network's language model allows."""
    loglik: np.ndarray      # [N] f64: log P(utterance) over all word strings; -inf without a path, NaN if one was met
    word_post: np.ndarray   # [total_frames, W] f64: the posterior of being in word w at frame t
    entry_post: np.ndarray  # [total_frames, W] f64: the posterior that a word w begins at frame t
    post: np.ndarray        # [total_frames, W * SP] f64: the posterior of flat state w * SP + s, or None
    offsets: np.ndarray     # [N + 1] i64

    def segment_confidence(self, result, u):
        """One float per segment ``(w, a, b)`` of ``result.segments(u)``: the mean of ``word_post[a:b, w]`` over the
        segment's frames — how much of the probability mass agrees that these frames belong to word ``w``."""
        lo = int(self.offsets[u])
        return [float(self.word_post[lo + a:lo + b, w].mean()) for w, a, b in result.segments(u)]

    def path_log_posterior(self, result):
        """``result.score - loglik`` per utterance: the log posterior of the decoded path among all paths (NaN where
        both are -inf)."""
        with np.errstate(invalid="ignore"):
            return np.asarray(result.score, dtype=np.float64) - self.loglik


@dataclass
class ConnectedResult:
    score: np.ndarray       # [N] f64: the best path's log score; -inf for an utterance without frames
    n_words: np.ndarray     # [N] i32: words on the best path; 0 where the score is not finite
    path_word: np.ndarray   # [total_frames] i32 (-1 where the score is not finite)
    path_state: np.ndarray  # [total_frames] i32 (-1 where the score is not finite)
    path_entry: np.ndarray  # [total_frames] u8: 1 where a word begins
    offsets: np.ndarray     # [N + 1] i64
    posteriors: ConnectedPosteriors = None  # connected_decode(..., posteriors=True): over the same logb
    level_score: np.ndarray = None  # [N, L] f64: connected_decode(..., n_words= / max_words=): the best score per count
    levels: "LevelResult" = None    # ... and the recursion it was selected from (further back-traces, N-best strings)
    nbest: "NBestResult" = None     # connected_decode(..., n_best=): the n best distinct strings over the same logb
    lattice: "WordLattice" = None   # connected_decode(..., lattice=True): the word lattice over the same logb

    def segments(self, u):
        """``[(word_index, start, end_exclusive), ...]`` of utterance ``u``, frames counted from its own start."""
        lo, hi = int(self.offsets[u]), int(self.offsets[u + 1])
        if int(self.n_words[u]) == 0:
            return []
        starts = np.flatnonzero(self.path_entry[lo:hi]).tolist()
        ends = starts[1:] + [hi - lo]
        return [(int(self.path_word[lo + a]), a, b) for a, b in zip(starts, ends)]

    def words(self, u):
        return [w for w, _, _ in self.segments(u)]


def _offsets(lengths):
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.size and lengths.min() < 0:
        raise ValueError("lengths must be >= 0")
    offs = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=offs[1:])
    return lengths, offs


def _emit(name, feats, network: ConnectedNetwork, family, *shape):
    """One stage-1 entry point: device ``feats[total_frames, D]`` float32 -> device ``logb[total_frames, R]``;
    ``shape``: what the entry point takes between D's operand block and ``logb`` (W, S and, for the mixtures, M)."""
    torch = _torch()
    if network.family != family or (network.means is None and network.pack is None):
        raise ValueError(f"{name} needs a network of the {family!r} family that carries its emission parameters "
                         f"(ConnectedNetwork.from_models); this one is {network.family!r}")
    if feats.dtype != torch.float32 or feats.dim() != 2 or not feats.is_contiguous():
        raise ValueError("feats must be a contiguous float32 [total_frames, D] tensor")
    if int(feats.shape[1]) != network.D:
        raise ValueError(f"the utterances have {int(feats.shape[1])} features, the models {network.D}")
    ops = network.device(feats.device)[3]
    total = int(feats.shape[0])
    logb = torch.empty((total, network.R), dtype=torch.float64, device=feats.device)
    _lib.check(getattr(_lib.load(), name)(_lib.ptr(feats), total, network.D, _lib.ptr(ops), *shape, _lib.ptr(logb),
                                          _lib.current_stream()), name)
    return logb


def emit_diag(feats, network: ConnectedNetwork):
    """``sapr_connected_emit_diag``: device ``feats[total_frames, D]`` float32 -> device ``logb[total_frames, R]``."""
    return _emit("sapr_connected_emit_diag", feats, network, "diag", network.W, network.S)


def emit_gmm(feats, network: ConnectedNetwork):
    """``sapr_connected_emit_gmm``: the same for a mixture vocabulary, over the network's ``GmmPack`` as it is."""
    return _emit("sapr_connected_emit_gmm", feats, network, "gmm", network.W, network.S,
                 network.pack.M if network.pack is not None else 0)


def emit_full(feats, network: ConnectedNetwork):
    """``sapr_connected_emit_full``: the same for a full-covariance vocabulary, over the network's ``FullPack``."""
    return _emit("sapr_connected_emit_full", feats, network, "full", network.W, network.S)


_EMIT = {"diag": emit_diag, "gmm": emit_gmm, "full": emit_full}


def bigram_workspace_bytes(total_frames, n_utts, W, S) -> int:
    return _workspace_bytes("sapr_connected_bigram_workspace_bytes", total_frames, n_utts, W, S)


def _path_tensors(n_utts, total, dev, want_paths=True):
    """Uninitialised device tensors (score, n_words, path_word, path_state, path_entry) for a back-trace to fill;
    ``want_paths=False``: the score alone, the other four ``None``."""
    torch = _torch()
    score = torch.empty(n_utts, dtype=torch.float64, device=dev)
    if not want_paths:
        return score, None, None, None, None
    return (score, torch.empty(n_utts, dtype=torch.int32, device=dev),
            torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev),
            torch.empty(total, dtype=torch.uint8, device=dev))


def _run_bigram(logb, offs_dev, n_utts, total, network, want_paths=True):
    """One ``sapr_connected_bigram`` -> device tensors (score, n_words, path_word, path_state, path_entry);
    ``want_paths=False``: the scores alone (the other four are ``None`` and no back-trace is launched)."""
    dev = logb.device
    ls, lt, lx, _ = network.device(dev)
    lm, lm_start, lm_end = network._dev_lm
    workspace, ws_bytes = _workspace("sapr_connected_bigram_workspace_bytes", dev, total, n_utts, network.W, network.S)
    score, n_words, path_word, path_state, path_entry = _path_tensors(n_utts, total, dev, want_paths)
    _lib.check(_lib.load().sapr_connected_bigram(
        _lib.ptr(logb), _lib.ptr(offs_dev), n_utts, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), _lib.ptr(lm),
        _lib.ptr(lm_start), _lib.ptr(lm_end), network.W, network.S, _lib.ptr(workspace), ws_bytes, _lib.ptr(score),
        _lib.ptr(n_words), _lib.ptr(path_word), _lib.ptr(path_state), _lib.ptr(path_entry), _lib.current_stream()),
        "sapr_connected_bigram")
    return score, n_words, path_word, path_state, path_entry


def _run_viterbi(logb, offs_dev, n_utts, total, network):
    """One ``sapr_connected_viterbi`` — ``sapr_connected_bigram`` where the network carries a bigram — -> device
    tensors (score, n_words, path_word, path_state, path_entry)."""
    if network.bigram is not None:
        return _run_bigram(logb, offs_dev, n_utts, total, network)
    dev = logb.device
    ls, lt, lx, _ = network.device(dev)
    workspace, ws_bytes = _workspace("sapr_connected_workspace_bytes", dev, total, n_utts, network.W, network.S)
    score, n_words, path_word, path_state, path_entry = _path_tensors(n_utts, total, dev)
    _lib.check(_lib.load().sapr_connected_viterbi(
        _lib.ptr(logb), _lib.ptr(offs_dev), n_utts, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx),
        network.word_penalty, network.W, network.S, _lib.ptr(workspace), ws_bytes, _lib.ptr(score), _lib.ptr(n_words),
        _lib.ptr(path_word), _lib.ptr(path_state), _lib.ptr(path_entry), _lib.current_stream()),
        "sapr_connected_viterbi")
    return score, n_words, path_word, path_state, path_entry


def _result(tensors, offs) -> ConnectedResult:
    host = [a.copy() for a in _lib.to_host(*tensors)]  # (out of the pinned buffers)
    return ConnectedResult(*host, offsets=offs)


def _flat_states(x, total, network, dev, pad=float("-inf"), what="logb"):
    """A caller's per-frame state array (host array or device tensor; ``[total_frames, W, S]``, ``[total_frames, W,
    SP]`` or ``[total_frames, R]``) -> device ``[total_frames, R]``; the states from S to SP are filled with ``pad``
    and the messages speak of ``what``."""
    torch = _torch()
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    x = x.to(dev)
    if x.dtype != torch.float64 or int(x.shape[0]) != total:
        raise ValueError(f"{what} must be float64 with sum(lengths) rows")
    W, S, SP, R = network.W, network.S, network.SP, network.R
    if tuple(x.shape[1:]) == (W, S) and S != SP:
        wide = torch.full((total, W, SP), pad, dtype=torch.float64, device=dev)
        wide[:, :, :S] = x
        x = wide
    if tuple(x.shape[1:]) not in ((W, SP), (R,)):
        raise ValueError(f"{what} must be [total_frames, {W}, {S}], [total_frames, {W}, {SP}] or [total_frames, {R}]; "
                         f"got {tuple(x.shape)}")
    return x.reshape(total, R).contiguous()


def _flat_feats(feats, total, dev, min_D=0):
    """A caller's ``feats`` (host array or device tensor) -> device float32 ``[total_frames, D]`` with D >= ``min_D``."""
    torch = _torch()
    if not torch.is_tensor(feats):
        feats = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32))
    feats = feats.to(dev).contiguous()
    if feats.dtype != torch.float32 or feats.dim() != 2 or int(feats.shape[0]) != total \
            or int(feats.shape[1]) < min_D:
        raise ValueError("feats must be float32 [sum(lengths), D]" + (f" with D >= {min_D}" if min_D else ""))
    return feats


def connected_viterbi(logb, lengths, network: ConnectedNetwork) -> ConnectedResult:
    """The recursion over a given ``logb``: float64 ``[total_frames, W, S]`` (the network's own S: padded here with
    ``-inf``), ``[total_frames, W, SP]`` or ``[total_frames, W * SP]``, a host array or a device tensor; host
    ``lengths``.  Any emission family may supply ``logb``.  A network with a bigram runs ``sapr_connected_bigram``."""
    torch = _torch()
    dev = _lib.require_gpu()
    lengths, offs = _offsets(lengths)
    total = int(offs[-1])
    logb = _flat_states(logb, total, network, dev)
    offs_dev = torch.from_numpy(offs).to(dev)
    return _result(_run_viterbi(logb, offs_dev, int(lengths.size), total, network), offs)


def _features(batch_or_feature_list):
    """A ``trellis.FeatureBatch`` or a list of frame-major ``(T, D)`` arrays -> ``(device feats [total_frames, D]
    float32, device offsets, host offsets)``."""
    torch = _torch()
    from .tile_family import vocab_features
    b = batch_or_feature_list
    if hasattr(b, "offsets") and hasattr(b, "order"):
        feats, offs_dev, _, lengths, _ = vocab_features(b)
        return feats, offs_dev, _offsets(lengths)[1]
    mats = [np.ascontiguousarray(np.asarray(f), dtype=np.float32) for f in b]
    if len(mats) == 0:
        raise ValueError("empty utterance list")
    D = mats[0].shape[1] if mats[0].ndim == 2 else -1
    if any(m.ndim != 2 or m.shape[1] != D for m in mats):
        raise ValueError("all utterances must be (T, D) arrays that share the feature dimension")
    _, offs = _offsets([m.shape[0] for m in mats])
    dev = _lib.require_gpu()
    packed = np.concatenate(mats, axis=0) if offs[-1] else np.zeros((0, D), np.float32)
    return torch.from_numpy(packed).to(dev), torch.from_numpy(offs).to(dev), offs


def posteriors_workspace_bytes(total_frames, n_utts, W, S) -> int:
    return _workspace_bytes("sapr_connected_posteriors_workspace_bytes", total_frames, n_utts, W, S)


def _posteriors_device(logb, offs_dev, offs, network, want_words=True, want_post=False):
    """One ``sapr_connected_posteriors`` over device ``logb[total_frames, R]``, under the network's bigram or, without
    one, under ``lm == word_penalty`` -> device tensors ``(loglik, word_post, entry_post, post)``; what was not asked
    for is ``None`` (and not computed)."""
    torch = _torch()
    dev = logb.device
    n_utts, total = int(offs.size - 1), int(offs[-1])
    ls, lt, lx, _ = network.device(dev)
    lm, lm_start, lm_end = network.device_lm(dev)
    workspace, ws_bytes = _workspace("sapr_connected_posteriors_workspace_bytes", dev, total, n_utts, network.W,
                                     network.S)
    loglik = torch.empty(n_utts, dtype=torch.float64, device=dev)
    word_post = torch.empty((total, network.W), dtype=torch.float64, device=dev) if want_words else None
    entry_post = torch.empty((total, network.W), dtype=torch.float64, device=dev) if want_words else None
    post = torch.empty((total, network.R), dtype=torch.float64, device=dev) if want_post else None
    _lib.check(_lib.load().sapr_connected_posteriors(
        _lib.ptr(logb), _lib.ptr(offs_dev), n_utts, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), _lib.ptr(lm),
        _lib.ptr(lm_start), _lib.ptr(lm_end), network.W, network.S, _lib.ptr(workspace), ws_bytes, _lib.ptr(loglik),
        _lib.ptr(word_post), _lib.ptr(entry_post), _lib.ptr(post), _lib.current_stream()), "sapr_connected_posteriors")
    return loglik, word_post, entry_post, post


def _run_posteriors(logb, offs_dev, offs, network, want_post=False) -> ConnectedPosteriors:
    """:func:`_posteriors_device` with everything copied to the host."""
    host = [None if a is None else a.cpu().numpy()
            for a in _posteriors_device(logb, offs_dev, offs, network, True, want_post)]
    return ConnectedPosteriors(*host, offsets=offs)


def connected_posteriors(logb, lengths, network: ConnectedNetwork, want_post=False) -> ConnectedPosteriors:
    """Forward-backward over the word loop on a given ``logb`` (the shapes :func:`connected_viterbi` takes): the total
    log-likelihood over every word string the network's language model allows, and per frame the posterior of each
    word and of each word boundary; ``want_post``: the state posteriors ``post[total_frames, W * SP]`` too."""
    torch = _torch()
    dev = _lib.require_gpu()
    lengths, offs = _offsets(lengths)
    logb = _flat_states(logb, int(offs[-1]), network, dev)
    return _run_posteriors(logb, torch.from_numpy(offs).to(dev), offs, network, want_post)


MAX_LEVELS = 8


def levels_workspace_bytes(total_frames, n_utts, W, S, max_words) -> int:
    return _workspace_bytes("sapr_connected_levels_workspace_bytes", total_frames, n_utts, W, S, max_words)


def _check_counts(n_words, max_words, n_utts):
    """``connected_decode``'s ``n_words`` / ``max_words`` -> ``(n_words, L)``: ``n_words`` is ``None``, an int or an
    int32 array of one count per utterance, every count inside 1 .. L; L inside 1 .. MAX_LEVELS.  ``n_words`` alone
    implies ``max_words`` = its largest count."""
    if n_words is not None:
        arr = np.asarray(n_words)
        if arr.dtype.kind not in "iu" or arr.ndim > 1:
            raise ValueError(f"n_words must be an int or one int per utterance, got {n_words!r}")
        if arr.ndim == 1 and arr.size != n_utts:
            raise ValueError(f"{arr.size} word counts for {n_utts} utterances")
        n_words = int(arr) if arr.ndim == 0 else arr.astype(np.int32)
        if max_words is None:
            max_words = int(arr.max()) if arr.size else 1
    L = int(max_words)
    if not 1 <= L <= MAX_LEVELS:
        raise ValueError(f"max_words must be inside 1..{MAX_LEVELS} (the levels one wavefront holds), got {L}")
    if n_words is not None and (np.min(n_words) < 1 or np.max(n_words) > L):
        got = f"{int(np.min(n_words))}..{int(np.max(n_words))}" if np.ndim(n_words) else f"{n_words}"
        raise ValueError(f"n_words must be inside 1..max_words = 1..{L} (max_words is at most {MAX_LEVELS}), got {got}")
    return n_words, L


class LevelResult:
    """One level-building recursion (``sapr_connected_levels``; the definition is ``tests/_levels_ref.py``):
    ``level_score[N, L]``, the best score of a string of exactly k words for k = 1 .. L, and the live device workspace
    any number of back-traces are taken from (:meth:`select`, :meth:`strings`)."""

    def __init__(self, level_score, offsets, network, max_words, level_dev, offs_dev, workspace, ws_bytes):
        self.level_score = level_score  # [N, L] f64; -inf where no string of k words explains the utterance
        self.offsets = offsets          # [N + 1] i64
        self.max_words = int(max_words)
        self._network, self._level_dev, self._offs_dev = network, level_dev, offs_dev
        self._workspace, self._ws_bytes = workspace, ws_bytes
        self._by_count = {}

    def select(self, n_words=None) -> ConnectedResult:
        """One ``sapr_connected_levels_backtrace``.  ``n_words``: ``None`` — the best count in 1 .. L; an int — exactly
        that many words; an array of one int per utterance; a tuple ``(lo, hi)`` of ints or per-utterance arrays — the
        best count inside the range.  Among counts that tie exactly the fewest words win; ``lo > hi`` selects nothing.
        A count outside 1 .. L is a ``ValueError`` for an int or an array, and is clamped in a range."""
        torch = _torch()
        n_utts, total = int(self.offsets.size - 1), int(self.offsets[-1])
        dev = self._level_dev.device
        if isinstance(n_words, tuple):
            if len(n_words) != 2:
                raise ValueError("a range of counts is a tuple (lo, hi)")
            lo, hi = n_words
        else:
            if n_words is not None:
                n_words, _ = _check_counts(n_words, self.max_words, n_utts)
            lo = hi = n_words

        def per_utt(a):
            if a is None:
                return None
            a = np.asarray(a)
            if a.dtype.kind not in "iu" or a.ndim > 1 or (a.ndim == 1 and a.size != n_utts):
                raise ValueError(f"a count is an int or one int per utterance ({n_utts}), got {a!r}")
            return torch.from_numpy(np.array(np.broadcast_to(a, (n_utts,)), dtype=np.int32)).to(dev)

        lo_dev, hi_dev = per_utt(lo), per_utt(hi)
        net = self._network
        score, count, path_word, path_state, path_entry = _path_tensors(n_utts, total, dev)
        _lib.check(_lib.load().sapr_connected_levels_backtrace(
            _lib.ptr(self._offs_dev), n_utts, total, net.W, net.S, self.max_words, _lib.ptr(self._workspace),
            self._ws_bytes, _lib.ptr(self._level_dev), _lib.ptr(lo_dev), _lib.ptr(hi_dev), _lib.ptr(score),
            _lib.ptr(count), _lib.ptr(path_word), _lib.ptr(path_state), _lib.ptr(path_entry), _lib.current_stream()),
            "sapr_connected_levels_backtrace")
        res = _result((score, count, path_word, path_state, path_entry), self.offsets)
        res.level_score, res.levels = self.level_score, self
        return res

    def strings(self, u):
        """The up to L strings of utterance ``u``, one per count with a finite score, best first (among equal scores
        the fewer words first): ``[(k, score, words, segments), ...]`` — a length-indexed N-best list.  The back-trace
        of a count is run once for the whole batch and kept."""
        out = []
        for k in range(1, self.max_words + 1):
            if not np.isfinite(self.level_score[u, k - 1]):
                continue
            if k not in self._by_count:
                self._by_count[k] = self.select(k)
            res = self._by_count[k]
            out.append((k, float(res.score[u]), res.words(u), res.segments(u)))
        out.sort(key=lambda row: -row[1])   # (stable: the fewer words first among equals)
        return out


def _run_levels(logb, offs_dev, offs, network, max_words) -> LevelResult:
    """One ``sapr_connected_levels`` over device ``logb[total_frames, R]``, under the network's bigram or, without
    one, under ``lm == word_penalty``."""
    torch = _torch()
    dev = logb.device
    n_utts, total = int(offs.size - 1), int(offs[-1])
    L = int(max_words)
    ls, lt, lx, _ = network.device(dev)
    lm, lm_start, lm_end = network.device_lm(dev)
    workspace, ws_bytes = _workspace("sapr_connected_levels_workspace_bytes", dev, total, n_utts, network.W, network.S,
                                     L)
    level = torch.empty((n_utts, L), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().sapr_connected_levels(
        _lib.ptr(logb), _lib.ptr(offs_dev), n_utts, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), _lib.ptr(lm),
        _lib.ptr(lm_start), _lib.ptr(lm_end), network.W, network.S, L, _lib.ptr(workspace), ws_bytes, _lib.ptr(level),
        _lib.current_stream()), "sapr_connected_levels")
    return LevelResult(level.cpu().numpy(), offs, network, L, level, offs_dev, workspace, ws_bytes)


def connected_levels(logb, lengths, network: ConnectedNetwork, max_words) -> LevelResult:
    """Level building over a given ``logb`` (the shapes :func:`connected_viterbi` takes): the best string of exactly
    k words for every k = 1 .. ``max_words`` (at most 8) in one pass, under the network's bigram or, without one,
    under its ``word_penalty``.  The result selects a known count, a range of counts or all the strings."""
    torch = _torch()
    L = _check_counts(None, max_words, 0)[1]
    dev = _lib.require_gpu()
    lengths, offs = _offsets(lengths)
    logb = _flat_states(logb, int(offs[-1]), network, dev)
    return _run_levels(logb, torch.from_numpy(offs).to(dev), offs, network, L)


# ---- the N best distinct word strings -------------------------------------------------------------
MAX_NBEST = 8


def _check_n_best(n_best) -> int:
    if isinstance(n_best, bool) or not isinstance(n_best, (int, np.integer)) or not 1 <= int(n_best) <= MAX_NBEST:
        raise ValueError(f"n_best must be an int inside 1..{MAX_NBEST} (the strings one list holds), got {n_best!r}")
    return int(n_best)


def nbest_capacity(W) -> int:
    """``cap(W)``: the longest word string a 64-bit code holds, the largest K with ``(W + 1)**K <= 2**64``
    (``sapr_connected_nbest_capacity``)."""
    k = C.c_int32(0)
    _lib.check(_lib.load().sapr_connected_nbest_capacity(int(W), C.byref(k)), "sapr_connected_nbest_capacity")
    return int(k.value)


class NBestResult:
    """One N-best recursion (``sapr_connected_nbest``; the definition is ``tests/_nbest_ref.py``): per utterance the
    ``n_best`` best distinct word strings with their Viterbi scores, best first.  The result keeps the device ``logb``
    it was computed on: :meth:`align` gives any rank its word boundaries."""

    def __init__(self, score, code, n_found, overflow, offsets, network, logb, offs_dev):
        self.score = score        # [N, n] f64: best first, -inf padded
        self.code = code          # [N, n] u64: the strings as base-(W + 1) numbers, 0 padded
        self.n_found = n_found    # [N] i32: the strings found
        self.overflow = overflow  # [N] bool: a string of nbest_capacity(W) words could not grow; the list may miss some
        self.offsets = offsets    # [N + 1] i64
        self._network, self._logb, self._offs_dev = network, logb, offs_dev
        self._aligned = {}

    def words(self, u, r):
        """The word indices of rank ``r`` of utterance ``u``, first word first; ``[]`` where the list is shorter."""
        code, B, out = int(self.code[u, r]), self._network.W + 1, []
        while code:
            out.append(code % B - 1)
            code //= B
        return out[::-1]

    def strings(self, u):
        """``[(score, words), ...]`` of utterance ``u``, best first."""
        return [(float(self.score[u, r]), self.words(u, r)) for r in range(int(self.n_found[u]))]

    def align(self, r) -> "RankAlignment":
        """The word boundaries of rank ``r``, an :class:`AlignResult`: one forced alignment (:func:`align_viterbi`'s
        kernel) over the kept ``logb`` for the utterances whose list has a rank ``r`` — ``result.utterances`` names
        them, in order.  The
        alignment's limit of ``max_words * SP <= 256`` chain positions applies here and only here.  The alignment's
        score is the acoustic score of the string (with the network's ``word_penalty``); it does not read a bigram."""
        r = int(r)
        if not 0 <= r < self.score.shape[1]:
            raise ValueError(f"rank {r} is outside 0..{self.score.shape[1] - 1}")
        if r in self._aligned:
            return self._aligned[r]
        torch = _torch()
        net = self._network
        utts = np.flatnonzero(self.n_found > r)
        transcripts = [self.words(int(u), r) for u in utts]
        limit = MAX_FLAT // net.SP
        for u, t in zip(utts, transcripts):
            if len(t) > limit:
                raise ValueError(f"rank {r} of utterance {int(u)} has {len(t)} words: alignment serves max_words * SP "
                                 f"<= {MAX_FLAT} chain positions ({limit} words at SP = {net.SP})")
        lengths = (self.offsets[1:] - self.offsets[:-1])[utts]
        _, offs = _offsets(lengths)
        if utts.size == self.n_found.size:
            logb, offs_dev = self._logb, self._offs_dev
        else:
            rows = np.concatenate([np.arange(self.offsets[u], self.offsets[u + 1]) for u in utts]) if utts.size \
                else np.zeros(0, np.int64)
            logb = self._logb.index_select(0, torch.from_numpy(rows.astype(np.int64)).to(self._logb.device))
            offs_dev = torch.from_numpy(offs).to(self._logb.device)
        if utts.size == 0:
            res = RankAlignment(np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8),
                                np.zeros(0, np.int32), word_offsets=np.zeros(1, np.int64), offsets=offs,
                                words=np.zeros(0, np.int32), utterances=utts)
        else:
            res = RankAlignment(**vars(_run_align(logb, offs_dev, offs, transcripts, net)), utterances=utts)
        self._aligned[r] = res
        return res


def _run_nbest(logb, offs_dev, offs, network, n_best) -> NBestResult:
    """One ``sapr_connected_nbest`` over device ``logb[total_frames, R]``, under the network's bigram or, without one,
    under ``lm == word_penalty``."""
    torch = _torch()
    dev = logb.device
    n_utts, total = int(offs.size - 1), int(offs[-1])
    ls, lt, lx, _ = network.device(dev)
    lm, lm_start, lm_end = network.device_lm(dev)
    score = torch.empty((n_utts, n_best), dtype=torch.float64, device=dev)
    code = torch.empty((n_utts, n_best), dtype=torch.int64, device=dev)  # (the uint64 codes, bit for bit)
    n_found = torch.empty(n_utts, dtype=torch.int32, device=dev)
    overflow = torch.empty(n_utts, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().sapr_connected_nbest(
        _lib.ptr(logb), _lib.ptr(offs_dev), n_utts, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), _lib.ptr(lm),
        _lib.ptr(lm_start), _lib.ptr(lm_end), network.W, network.S, n_best, _lib.ptr(score), _lib.ptr(code),
        _lib.ptr(n_found), _lib.ptr(overflow), _lib.current_stream()), "sapr_connected_nbest")
    return NBestResult(score.cpu().numpy(), code.cpu().numpy().view(np.uint64), n_found.cpu().numpy(),
                       overflow.cpu().numpy().astype(bool), offs, network, logb, offs_dev)


def connected_nbest(logb, lengths, network: ConnectedNetwork, n_best) -> NBestResult:
    """The ``n_best`` (1 .. 8) best distinct word strings of every utterance over a given ``logb`` (the shapes
    :func:`connected_viterbi` takes), in one pass, under the network's bigram or, without one, under its
    ``word_penalty``.  Rank 1 has the score of the one-pass search bit for bit; the list is exact unless two string
    scores tie exactly or ``overflow`` is set (a string would exceed :func:`nbest_capacity` words)."""
    torch = _torch()
    n_best = _check_n_best(n_best)
    dev = _lib.require_gpu()
    lengths, offs = _offsets(lengths)
    logb = _flat_states(logb, int(offs[-1]), network, dev)
    return _run_nbest(logb, torch.from_numpy(offs).to(dev), offs, network, n_best)


# ---- word lattices ------------------------------------------------------------------------------
def lattice_workspace_bytes(total_frames, n_utts, W, S) -> int:
    return _workspace_bytes("sapr_connected_lattice_workspace_bytes", total_frames, n_utts, W, S)


def _check_beam(beam) -> float:
    if isinstance(beam, bool) or not isinstance(beam, (int, float, np.integer, np.floating)) or not float(beam) >= 0.0:
        raise ValueError(f"beam must be a number >= 0 (inf keeps every record on a complete path), got {beam!r}")
    return float(beam)


@dataclass
class LatticeBackward:
    """One backward pass over a :class:`WordLattice` (``sapr_connected_lattice_backward``) under some tables."""
    beta: np.ndarray       # [total_frames, W] f64: the best completion after word w ended at frame t; -inf without one
    next_end: np.ndarray   # [total_frames, W] i32: the end frame of the record that attains it (-1 without one)
    next_word: np.ndarray  # [total_frames, W] u8: ... and its word (255 without one)
    root: np.ndarray       # [N] f64: the best complete lattice path
    first: np.ndarray      # [N, 2] i32: (end frame, word) of its first record; (-1, 255) without one
    device: tuple = None   # the same five on the device, for the walk


@dataclass
class LatticePath:
    """The best string of every utterance through a lattice under some tables (:meth:`WordLattice.rescore`)."""
    score: np.ndarray       # [N] f64: root — the best complete lattice path; -inf without one
    n_words: np.ndarray     # [N] i32
    path_word: np.ndarray   # [total_frames] i32 (-1 where the score is not finite)
    path_entry: np.ndarray  # [total_frames] u8: 1 where a word begins
    offsets: np.ndarray     # [N + 1] i64

    segments = ConnectedResult.segments
    words = ConnectedResult.words


def lattice_posteriors_workspace_bytes(total_frames, n_utts, W, S) -> int:
    return _workspace_bytes("sapr_connected_lattice_posteriors_workspace_bytes", total_frames, n_utts, W, S)


def _check_acoustic_scale(acoustic_scale) -> float:
    ok = not isinstance(acoustic_scale, bool) and isinstance(acoustic_scale, (int, float, np.integer, np.floating))
    if not ok or not np.isfinite(acoustic_scale) or not float(acoustic_scale) > 0.0:
        raise ValueError(f"acoustic_scale must be a finite number > 0, got {acoustic_scale!r}")
    return float(acoustic_scale)


@dataclass
class LatticePosteriors:
    """Forward-backward in the sum semiring over a :class:`WordLattice` (``sapr_connected_lattice_posteriors``; the
    definition is ``tests/_lattice_post_ref.py``): the sum over every path of the lattice — Viterbi within words, the
    recorded boundaries only — under some tables and an acoustic scale."""
    loglik: np.ndarray       # [N] f64: the log-sum of every complete lattice path; -inf without one
    record_post: np.ndarray  # [total_frames, W] f64: the posterior of the record (w, t), 0 where there is none
    word_post: np.ndarray    # [total_frames, W] f64: the posterior that frame f lies inside word w
    offsets: np.ndarray      # [N + 1] i64

    def segment_confidence(self, path, u):
        """One float per segment ``(w, a, b)`` of ``path.segments(u)`` (a :class:`LatticePath` or a
        :class:`ConnectedResult`): the mean of ``word_post[a:b, w]`` over the segment's frames, as
        :meth:`ConnectedPosteriors.segment_confidence` has it."""
        lo = int(self.offsets[u])
        return [float(self.word_post[lo + a:lo + b, w].mean()) for w, a, b in path.segments(u)]

    def slots(self, path, u, top=None):
        """Per segment of ``path.segments(u)`` the list ``[(word, posterior), ...]``, best first (``top``: at most that
        many): the mean of ``word_post[a:b, v]`` over the segment's frames for every word v with a posterior above 0.
        Each full slot sums to 1 where the utterance has a path.  This is a frame-based confusion network pivoted on
        the given path — host code over the returned table —, not Mangu's clustering of the lattice's links."""
        lo = int(self.offsets[u])
        out = []
        for _, a, b in path.segments(u):
            mean = self.word_post[lo + a:lo + b].mean(axis=0)
            order = sorted(np.flatnonzero(mean > 0.0).tolist(), key=lambda v: (-mean[v], v))
            out.append([(int(v), float(mean[v])) for v in order[:top]])
        return out


class WordLattice:
    """The word-end tables one pass over the word loop leaves (``sapr_connected_lattice``; the definition is
    ``tests/_lattice_ref.py``): for every (frame, word) the score ``X`` of the best path that ends the word there, the
    entry score ``N`` and the frame ``B`` at which that path entered the word.  A record is a (word, end frame) with a
    finite ``X``; it may follow any record that ends one frame before its start, so the table is a word lattice every
    path of which is a real path of the network with its real within-word score.  It is pruned to a beam around the
    best path (:meth:`prune`, :meth:`records`), rescored under another :class:`WordBigram` without emission or
    recursion (:meth:`rescore`) and exported (:meth:`to_slf`).  The tables stay on the device (``wend_score``,
    ``wend_entry``, ``wend_start``: views of one workspace); ``score`` and ``offsets`` are host arrays."""

    def __init__(self, score, final_word, offsets, network, lm_host, lm_dev, workspace, ws_bytes, offs_dev):
        self.score = score            # [N] f64: the one-pass search's score, bit for bit
        self.final_word = final_word  # [N] i32: the word that attained it
        self.offsets = offsets        # [N + 1] i64
        self.W = int(network.W)
        self._network, self._lm, self._lm_dev = network, lm_host, lm_dev
        self._workspace, self._ws_bytes, self._offs_dev = workspace, ws_bytes, offs_dev
        total, a16 = int(offsets[-1]), lambda n: (n + 15) // 16 * 16
        x_bytes = a16(8 * total * self.W)
        view = lambda lo, size, dt: workspace[lo:lo + size * total * self.W].view(dt).view(total, self.W)  # noqa: E731
        torch = _torch()
        self.wend_score = view(0, 8, torch.float64)
        self.wend_entry = view(x_bytes, 8, torch.float64)
        self.wend_start = view(2 * x_bytes, 4, torch.int32)
        self._host, self._own, self._eps = None, None, None

    def tables(self):
        """``(X, N, B)`` on the host: ``[total_frames, W]`` float64, float64 and int32 (copied once)."""
        if self._host is None:
            self._host = tuple(a.copy() for a in _lib.to_host(self.wend_score, self.wend_entry, self.wend_start))
        return self._host

    def eps(self):
        """``eps_u = 4 T_u 2^-52 M_u`` per utterance, M_u the largest finite ``|X|`` or ``|N|``: the rounding slack of
        a lattice path's score against the state path it stands for."""
        if self._eps is None:
            X, N, _ = self.tables()
            out = np.zeros(self.offsets.size - 1)
            for u, (lo, hi) in enumerate(zip(self.offsets[:-1], self.offsets[1:])):
                v = np.abs(np.concatenate([X[lo:hi].ravel(), N[lo:hi].ravel()]))
                v = v[np.isfinite(v)]
                out[u] = 4.0 * (hi - lo) * 2.0 ** -52 * (v.max() if v.size else 0.0)
            self._eps = out
        return self._eps

    def _check_bigram(self, bigram):
        if bigram is not None and (not isinstance(bigram, WordBigram) or bigram.W != self.W):
            raise ValueError(f"a lattice over {self.W} words is rescored under a WordBigram over {self.W} words, got "
                             f"{bigram!r}" + (f" over {bigram.W}" if isinstance(bigram, WordBigram) else ""))

    def _device_tables(self, bigram):
        """``(lm, lm_start, lm_end)`` of ``bigram`` on the lattice's device; ``None``: the lattice's own."""
        if bigram is None:
            return self._lm_dev
        torch = _torch()
        dev = self._workspace.device
        return tuple(torch.from_numpy(a).to(dev) for a in (bigram.lm, bigram.lm_start, bigram.lm_end))

    def backward(self, bigram=None) -> LatticeBackward:
        """``beta`` / ``next`` / ``root`` / ``first`` under the tables of ``bigram`` (a :class:`WordBigram` over the
        same W words), or under the tables the lattice was made under; that result is kept."""
        if bigram is None and self._own is not None:
            return self._own
        torch = _torch()
        self._check_bigram(bigram)
        dev = self._workspace.device
        lm, lm_start, lm_end = self._device_tables(bigram)
        n_utts, total = int(self.offsets.size - 1), int(self.offsets[-1])
        beta = torch.empty((total, self.W), dtype=torch.float64, device=dev)
        next_end = torch.empty((total, self.W), dtype=torch.int32, device=dev)
        next_word = torch.empty((total, self.W), dtype=torch.uint8, device=dev)
        root = torch.empty(n_utts, dtype=torch.float64, device=dev)
        first = torch.empty((n_utts, 2), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().sapr_connected_lattice_backward(
            _lib.ptr(self._offs_dev), n_utts, total, self.W, self._network.S, _lib.ptr(self._workspace), self._ws_bytes,
            _lib.ptr(self._lm_dev[1]), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), _lib.ptr(beta),
            _lib.ptr(next_end), _lib.ptr(next_word), _lib.ptr(root), _lib.ptr(first), _lib.current_stream()),
            "sapr_connected_lattice_backward")
        tensors = (beta, next_end, next_word, root, first)
        out = LatticeBackward(*[a.copy() for a in _lib.to_host(*tensors)], device=tensors)
        if bigram is None:
            self._own = out
        return out

    def rescore(self, bigram) -> LatticePath:
        """The best string of every utterance through the lattice under another :class:`WordBigram` — for example
        ``network.bigram.scaled(scale, word_penalty)`` — from one backward pass and one walk: no emission and no
        recursion.  The score is never above a full decode under ``bigram`` by more than :meth:`eps`; it reaches it
        where that decode's best path keeps the word boundaries this lattice recorded."""
        torch = _torch()
        back = self.backward(bigram)
        _, next_end, next_word, root, first = back.device
        n_utts, total = int(self.offsets.size - 1), int(self.offsets[-1])
        dev = self._workspace.device
        n_words = torch.empty(n_utts, dtype=torch.int32, device=dev)
        path_word = torch.empty(total, dtype=torch.int32, device=dev)
        path_entry = torch.empty(total, dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().sapr_connected_lattice_walk(
            _lib.ptr(self._offs_dev), n_utts, total, self.W, self._network.S, _lib.ptr(next_end), _lib.ptr(next_word),
            _lib.ptr(root), _lib.ptr(first), _lib.ptr(n_words), _lib.ptr(path_word), _lib.ptr(path_entry),
            _lib.current_stream()), "sapr_connected_lattice_walk")
        host = [a.copy() for a in _lib.to_host(n_words, path_word, path_entry)]
        return LatticePath(back.root, *host, offsets=self.offsets)

    def posteriors(self, bigram=None, acoustic_scale=1.0, beam=None) -> LatticePosteriors:
        """Link and word posteriors over the lattice (``sapr_connected_lattice_posteriors``): forward-backward in the
        sum semiring over the records under the tables of ``bigram`` (as for :meth:`backward`; ``None``: the tables
        the lattice was made under) with every record's acoustic score multiplied by ``acoustic_scale`` — no
        emission and no recursion over states, so another language-model weight, penalty or grammar costs one more
        call.  ``beam``: ``None`` takes every record, otherwise only the records :meth:`prune` keeps at that beam.  A
        bigram over another vocabulary, an ``acoustic_scale`` that is not a finite number above 0 and a negative beam
        are a ``ValueError`` before any device call."""
        self._check_bigram(bigram)
        kappa = _check_acoustic_scale(acoustic_scale)
        keep = None if beam is None else self.prune(_check_beam(beam))
        torch = _torch()
        dev = self._workspace.device
        lm, lm_start, lm_end = self._device_tables(bigram)
        n_utts, total = int(self.offsets.size - 1), int(self.offsets[-1])
        keep_dev = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8)).to(dev)
        workspace, ws_bytes = _workspace("sapr_connected_lattice_posteriors_workspace_bytes", dev, total, n_utts,
                                         self.W, self._network.S)
        loglik = torch.empty(n_utts, dtype=torch.float64, device=dev)
        record_post = torch.empty((total, self.W), dtype=torch.float64, device=dev)
        word_post = torch.empty((total, self.W), dtype=torch.float64, device=dev)
        _lib.check(_lib.load().sapr_connected_lattice_posteriors(
            _lib.ptr(self._offs_dev), n_utts, total, self.W, self._network.S, _lib.ptr(self._workspace), self._ws_bytes,
            _lib.ptr(self._lm_dev[1]), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), kappa,
            _lib.ptr(keep_dev), _lib.ptr(workspace), ws_bytes, _lib.ptr(loglik),
            _lib.ptr(record_post), _lib.ptr(word_post), _lib.current_stream()), "sapr_connected_lattice_posteriors")
        host = [a.copy() for a in _lib.to_host(loglik, record_post, word_post)]
        return LatticePosteriors(*host, offsets=self.offsets)

    def best(self) -> LatticePath:
        """:meth:`rescore` under the tables the lattice was made under: the one-pass search's string."""
        return self.rescore(None)

    def margins(self):
        """``[total_frames, W]`` float64: ``(X_t(w) + beta_t(w)) - score`` under the lattice's own tables — how far
        the best complete path through the record (w, t) falls below the best path; -inf for a record on no complete
        path."""
        X = self.tables()[0]
        lengths = self.offsets[1:] - self.offsets[:-1]
        with np.errstate(invalid="ignore"):
            m = X + self.backward().beta
            return np.where(m > -np.inf, m - np.repeat(self.score, lengths)[:, None], -np.inf)

    def prune(self, beam):
        """A boolean mask ``[total_frames, W]``: the records kept at ``beam`` — on a complete path and with a margin
        ``>= -(beam + eps_u)``.  ``beam=0`` keeps the best path's records, ``beam=inf`` every record on a complete
        path; a negative beam is a ``ValueError``."""
        beam = _check_beam(beam)
        m = self.margins()
        lengths = self.offsets[1:] - self.offsets[:-1]
        return (m > -np.inf) & (m >= -(beam + np.repeat(self.eps(), lengths))[:, None])

    def _records(self, u, keep):
        """``[(t, w, tau, in, ac, margin), ...]`` of utterance ``u`` where ``keep[t, w]``, end ascending, then word."""
        X, N, B = self.tables()
        lo, hi = int(self.offsets[u]), int(self.offsets[u + 1])
        X, N, B, m = X[lo:hi], N[lo:hi], B[lo:hi], self.margins()[lo:hi]
        out = []
        for t, w in zip(*np.nonzero((X > -np.inf) & (B >= 0) & (B <= np.arange(hi - lo)[:, None]) & keep[lo:hi])):
            tau = int(B[t, w])
            inc = self._lm[1][w] if tau == 0 else N[tau - 1, w]
            with np.errstate(invalid="ignore"):
                out.append((int(t), int(w), tau, float(inc), float(X[t, w] - inc), float(m[t, w])))
        return out

    def records(self, u, beam=None):
        """The records of utterance ``u`` kept at ``beam`` (``None``: every record, on a complete path or not):
        ``[(word, start, end_exclusive, acoustic, margin), ...]`` sorted by end and then by word, frames counted from
        the utterance's own start.  ``acoustic`` is the within-word score ``X - in``: the language model is not in it."""
        keep = np.ones((int(self.offsets[-1]), self.W), bool) if beam is None else self.prune(beam)
        return [(w, tau, t + 1, ac, m) for t, w, tau, _, ac, m in self._records(u, keep)]

    def to_slf(self, u, names, frame_shift=0.01, beam=None) -> str:
        """The part of utterance ``u`` kept at ``beam`` (``None``: every record on a complete path) as HTK Standard
        Lattice Format text.  One node per kept record — ``W=`` its word's name, ``t=`` its end time — plus a start and
        an end node (``!NULL``).  The link from record (v, tau - 1) to record (w, t) carries ``a=`` the acoustic score
        of (w, t) and ``l=`` ``lm[v][w]``; the start node links to the records with tau = 0 under ``lm_start`` and the
        records that end the utterance link to the end node with ``a=0`` and ``l=lm_end``.  A link exists only where
        both records are kept and its language-model score is finite.  Scores are printed with 17 significant digits.
        Host code only."""
        if len(names) != self.W:
            raise ValueError(f"{len(names)} names for {self.W} words")
        recs = self._records(u, self.prune(float("inf") if beam is None else beam))
        lm, lm_start, lm_end = self._lm
        T = int(self.offsets[u + 1] - self.offsets[u])
        node = {(t, w): k + 1 for k, (t, w, *_) in enumerate(recs)}
        end = len(recs) + 1
        ends_at = {}
        for t, w, *_ in recs:
            ends_at.setdefault(t, []).append(w)
        links = []
        for t, w, tau, _, ac, _ in recs:
            if tau == 0:
                if lm_start[w] > -np.inf:
                    links.append((0, node[t, w], ac, lm_start[w]))
            else:
                links += [(node[tau - 1, v], node[t, w], ac, lm[v, w]) for v in ends_at.get(tau - 1, [])
                          if lm[v, w] > -np.inf]
            if t == T - 1 and lm_end[w] > -np.inf:
                links.append((node[t, w], end, 0.0, lm_end[w]))
        num = lambda x: repr(float(x))  # noqa: E731
        lines = ["VERSION=1.0", f"UTTERANCE={u}", "lmscale=1.00 wdpenalty=0.00", f"N={end + 1} L={len(links)}",
                 "I=0 t=0.00 W=!NULL"]
        lines += [f"I={node[t, w]} t={(t + 1) * frame_shift:.4f} W={names[w]}" for t, w, *_ in recs]
        lines.append(f"I={end} t={T * frame_shift:.4f} W=!NULL")
        lines += [f"J={j} S={a} E={b} a={num(ac)} l={num(l)}" for j, (a, b, ac, l) in enumerate(links)]
        return "\n".join(lines) + "\n"


def _run_lattice(logb, offs_dev, offs, network) -> WordLattice:
    """One ``sapr_connected_lattice`` over device ``logb[total_frames, R]``, under the network's bigram or, without
    one, under ``lm == word_penalty``."""
    torch = _torch()
    dev = logb.device
    n_utts, total = int(offs.size - 1), int(offs[-1])
    ls, lt, lx, _ = network.device(dev)
    lm_dev = network.device_lm(dev)
    workspace, ws_bytes = _workspace("sapr_connected_lattice_workspace_bytes", dev, total, n_utts, network.W,
                                     network.S)
    score = torch.empty(n_utts, dtype=torch.float64, device=dev)
    final = torch.empty(n_utts, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().sapr_connected_lattice(
        _lib.ptr(logb), _lib.ptr(offs_dev), n_utts, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx),
        _lib.ptr(lm_dev[0]), _lib.ptr(lm_dev[1]), _lib.ptr(lm_dev[2]), network.W, network.S, _lib.ptr(workspace),
        ws_bytes, _lib.ptr(score), _lib.ptr(final), _lib.current_stream()), "sapr_connected_lattice")
    return WordLattice(score.cpu().numpy(), final.cpu().numpy(), offs, network, network.loop_lm(), lm_dev, workspace,
                       ws_bytes, offs_dev)


def connected_lattice(logb, lengths, network: ConnectedNetwork) -> WordLattice:
    """The word lattice of every utterance over a given ``logb`` (the shapes :func:`connected_viterbi` takes), in one
    pass, under the network's bigram or, without one, under its ``word_penalty``.  ``score`` is the one-pass search's
    bit for bit; the lattice costs 20 W bytes per frame and no per-state back-pointer."""
    torch = _torch()
    dev = _lib.require_gpu()
    lengths, offs = _offsets(lengths)
    logb = _flat_states(logb, int(offs[-1]), network, dev)
    return _run_lattice(logb, torch.from_numpy(offs).to(dev), offs, network)


def connected_decode(batch_or_feature_list, network: ConnectedNetwork, posteriors=False, n_words=None,
                     max_words=None, n_best=None, lattice=False) -> ConnectedResult:
    """Emission (by the network's family) and recursion: a ``trellis.FeatureBatch`` or a list of frame-major
    ``(T, D)`` feature arrays -> :class:`ConnectedResult`.  ``posteriors``: forward-backward over the same ``logb``
    as well (one emission, both recursions); the result then carries its :class:`ConnectedPosteriors`.  ``n_best``
    (1 .. 8): the N-best recursion over the same ``logb`` as well; the result then carries its :class:`NBestResult`
    as ``.nbest``.  ``lattice=True``: the lattice recursion over the same ``logb`` as well; the result then carries
    its :class:`WordLattice` as ``.lattice``.

    ``n_words`` (an int or one per utterance): the number of words is known; ``max_words``: it is at most this.  Either
    runs level building (``sapr_connected_levels``) instead of the free loop and the result carries ``level_score`` and
    its :class:`LevelResult`; ``n_words`` alone implies ``max_words`` = its largest count.  ``max_words`` above 8 or an
    ``n_words`` outside 1 .. ``max_words`` is a ``ValueError``, and so is an ``n_best`` outside 1 .. 8."""
    if n_best is not None:
        n_best = _check_n_best(n_best)  # (refused before a device is asked for)
    if n_words is None and max_words is None:
        feats, offs_dev, offs = _features(batch_or_feature_list)
        logb = _EMIT[network.family](feats, network)
        res = _result(_run_viterbi(logb, offs_dev, int(offs.size - 1), int(offs[-1]), network), offs)
    else:
        # (refused before a device is asked for)
        n_words, L = _check_counts(n_words, max_words, _n_utts(batch_or_feature_list))
        feats, offs_dev, offs = _features(batch_or_feature_list)
        logb = _EMIT[network.family](feats, network)
        res = _run_levels(logb, offs_dev, offs, network, L).select(n_words)
    if posteriors:
        res.posteriors = _run_posteriors(logb, offs_dev, offs, network)
    if n_best is not None:
        res.nbest = _run_nbest(logb, offs_dev, offs, network, n_best)
    if lattice:
        res.lattice = _run_lattice(logb, offs_dev, offs, network)
    return res


# ---- online decoding: recordings that are still arriving ----------------------------------------
def online_state_bytes(n_streams, W, S, window) -> int:
    return _workspace_bytes("sapr_connected_online_state_bytes", n_streams, W, S, window)


@dataclass
class OnlineUpdate:
    """What one :meth:`ConnectedSession.push` hands out for one stream: the rows that became final."""
    first_frame: int        # the absolute frame of the first new row
    path_word: np.ndarray   # [n_new] i32
    path_state: np.ndarray  # [n_new] i32
    path_entry: np.ndarray  # [n_new] u8
    segments: list          # newly complete (word_index, start, end_exclusive), absolute frames
    frames: int             # frames of the recording consumed so far
    stable_frames: int      # ... of which final
    forced: int             # ... of which committed by force (the window was too small for the path to settle)
    hypothesis: list = None  # push(..., hypothesis=True): the words of the best string over the pending frames
    hypothesis_rows: tuple = None  # ... and its (path_word, path_state, path_entry) over them, as a flush would write


@dataclass
class OnlineResult:
    """What :meth:`ConnectedSession.finish` returns for one stream: the fields of a :class:`ConnectedResult` for the
    whole recording — the concatenation of every row handed out — and ``forced``.  With ``forced == 0`` and a finite
    score they are the offline decoder's bit for bit; a score that is not finite leaves the rows handed out before the
    flush as they are and ``n_words == 0``."""
    score: float
    n_words: int
    path_word: np.ndarray
    path_state: np.ndarray
    path_entry: np.ndarray
    forced: int
    update: OnlineUpdate    # what the flush itself handed out

    def segments(self):
        if self.n_words == 0:
            return []
        starts = np.flatnonzero(self.path_entry).tolist()
        return [(int(self.path_word[a]), a, b) for a, b in zip(starts, starts[1:] + [len(self.path_word)])]

    def words(self):
        return [w for w, _, _ in self.segments()]


class ConnectedSession:
    """Online connected-word decoding (``sapr_connected_online_step`` / ``sapr_connected_online_commit``,
    ``csrc/connected_online.hip``; the definition is ``tests/_online_ref.py``): ``n_streams`` recordings that arrive in
    chunks over one network.  The device keeps the trellis column and ``window`` back-pointer rows per stream; a path
    prefix is handed out as soon as every live hypothesis agrees on it, and the final answer is the offline decoder's
    bit for bit unless ``forced`` says that the window was too small.  A network without a bigram runs under
    ``lm == word_penalty``.  ``1 <= max_chunk < window``."""

    def __init__(self, network: ConnectedNetwork, n_streams, window=256, max_chunk=64):
        torch = _torch()
        self.network, self.n_streams = network, int(n_streams)
        self.window, self.max_chunk = int(window), int(max_chunk)
        if self.n_streams < 1:
            raise ValueError(f"n_streams must be >= 1, got {n_streams!r}")
        if not 1 <= self.max_chunk < self.window:
            raise ValueError(f"1 <= max_chunk < window is required, got max_chunk={max_chunk!r} window={window!r}")
        self._dev = dev = _lib.require_gpu()
        self._state_bytes = online_state_bytes(self.n_streams, network.W, network.S, self.window)
        self._state = torch.zeros(max(self._state_bytes, 1), dtype=torch.uint8, device=dev)  # all zero: fresh
        B, win = self.n_streams, self.window
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
        u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        self._n_new, self._first = i32(B), torch.empty(B, dtype=torch.int64, device=dev)
        self._rows = (i32(B, win), i32(B, win), u8(B, win))
        self._score, self._n_words = torch.empty(B, dtype=torch.float64, device=dev), i32(B)
        self._forced = torch.empty(B, dtype=torch.int64, device=dev)
        self._hyp = (i32(B), i32(B, win), i32(B, win), u8(B, win))
        self._truncated = u8(B)
        self.frames = [0] * B
        self.stable_frames = [0] * B
        self._open = [None] * B                      # (word, start) of the segment whose end is not final yet
        self._kept = [[] for _ in range(B)]          # the rows handed out, for finish()

    def _chunks(self, chunks, dtype):
        """One host array per stream (``None``: no frames) -> ``(arrays, host offsets)``."""
        if len(chunks) != self.n_streams:
            raise ValueError(f"one chunk per stream: got {len(chunks)} for {self.n_streams} streams")
        mats = []
        for u, c in enumerate(chunks):
            m = np.zeros(0, dtype) if c is None else np.asarray(c, dtype=dtype)
            if m.shape[0] > self.max_chunk:
                raise ValueError(f"the chunk of stream {u} has {m.shape[0]} frames, max_chunk is {self.max_chunk}")
            mats.append(m)
        _, offs = _offsets([m.shape[0] for m in mats])
        return mats, offs

    def push(self, feats=None, logb=None, hypothesis=False):
        """One chunk per stream — ``feats``: frame-major ``(t, D)`` feature arrays for a network that carries its
        emission parameters, or ``logb``: float64 ``[t, W, S]``, ``[t, W, SP]`` or ``[t, R]`` arrays; ``None`` or an
        empty array for a stream without new frames, at most ``max_chunk`` frames each (a ``ValueError`` names the
        stream otherwise).  Emission over the concatenated chunk frames, one step, one commit.  Returns one
        :class:`OnlineUpdate` per stream."""
        torch = _torch()
        net, dev = self.network, self._dev
        if (feats is None) == (logb is None):
            raise ValueError("push takes either feats or logb")
        if logb is None:
            mats, offs = self._chunks(feats, np.float32)
            total = int(offs[-1])
            if any(m.ndim != 2 or m.shape[1] != net.D for m in mats if m.shape[0]):
                raise ValueError(f"feature chunks must be (t, D = {net.D}) arrays")
            packed = np.concatenate([m.reshape(-1, net.D) for m in mats]) if total else np.zeros((0, net.D), np.float32)
            if total:
                rows = _EMIT[net.family](torch.from_numpy(np.ascontiguousarray(packed, np.float32)).to(dev), net)
            else:
                rows = torch.empty((0, net.R), dtype=torch.float64, device=dev)
        else:
            mats, offs = self._chunks(logb, np.float64)
            total = int(offs[-1])
            live = [m for m in mats if m.shape[0]]
            packed = np.concatenate(live) if live else np.zeros((0, net.R))
            rows = _flat_states(packed, total, net, dev)
        self._step(rows, offs, total)
        return self._commit(None, hypothesis)

    def _step(self, rows, offs, total, reset=None):
        torch = _torch()
        net, dev = self.network, self._dev
        ls, lt, lx, _ = net.device(dev)
        lm, lm_start, lm_end = net.device_lm(dev)
        offs_dev = torch.from_numpy(offs).to(dev)
        reset_dev = None if reset is None else torch.from_numpy(np.asarray(reset, np.uint8)).to(dev)
        _lib.check(_lib.load().sapr_connected_online_step(
            _lib.ptr(rows), _lib.ptr(offs_dev), self.n_streams, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx),
            _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), net.W, net.S, self.window, self.max_chunk,
            _lib.ptr(self._state), self._state_bytes, _lib.ptr(reset_dev), _lib.ptr(self._truncated),
            _lib.current_stream()), "sapr_connected_online_step")
        for u in range(self.n_streams):
            if reset is not None and reset[u]:
                self._forget(u)
            self.frames[u] += int(offs[u + 1] - offs[u])

    def _forget(self, u):
        self.frames[u] = self.stable_frames[u] = 0
        self._open[u] = None
        self._kept[u] = []

    def reset(self, streams=None):
        """Abandon the recordings of ``streams`` (all by default): they start fresh, nothing is handed out."""
        flags = np.zeros(self.n_streams, np.uint8)
        flags[list(range(self.n_streams)) if streams is None else list(streams)] = 1
        self._step(None, np.zeros(self.n_streams + 1, np.int64), 0, flags)

    def _commit(self, flush, hypothesis):
        torch = _torch()
        net = self.network
        flush_dev = None if flush is None else torch.from_numpy(flush).to(self._dev)
        hyp = self._hyp if hypothesis else (None,) * 4
        _lib.check(_lib.load().sapr_connected_online_commit(
            self.n_streams, net.W, net.S, self.window, self.max_chunk, _lib.ptr(self._state), self._state_bytes,
            _lib.ptr(flush_dev), _lib.ptr(self._n_new), _lib.ptr(self._first), *(_lib.ptr(t) for t in self._rows),
            _lib.ptr(self._score), _lib.ptr(self._n_words), _lib.ptr(self._forced), *(_lib.ptr(t) for t in hyp),
            _lib.current_stream()), "sapr_connected_online_commit")
        host = _lib.to_host(self._n_new, self._first, *self._rows, self._score, self._n_words, self._forced,
                            self._truncated, *(self._hyp if hypothesis else ()))
        n_new, first, pw, ps, pe, score, n_words, forced, truncated = host[:9]
        if truncated.any():  # (push refuses over-long chunks, so this is a session used against its contract)
            raise _lib.SaprHipError(f"stream {int(np.flatnonzero(truncated)[0])}: the ring had no room for its chunk")
        out = []
        for u in range(self.n_streams):
            n = int(n_new[u])
            up = OnlineUpdate(int(first[u]), pw[u, :n].copy(), ps[u, :n].copy(), pe[u, :n].copy(), [],
                              self.frames[u], int(first[u]) + n, int(forced[u]))
            flushed = flush is not None and bool(flush[u])
            for i in np.flatnonzero(up.path_entry).tolist():   # an entry closes the segment before it
                if self._open[u] is not None:
                    up.segments.append((*self._open[u], up.first_frame + i))
                self._open[u] = (int(up.path_word[i]), up.first_frame + i)
            if flushed and self._open[u] is not None and np.isfinite(score[u]):
                up.segments.append((*self._open[u], self.frames[u]))
            self.stable_frames[u] = up.stable_frames
            self._kept[u].append((up.path_word, up.path_state, up.path_entry))
            if hypothesis:
                k = int(host[9][u])
                ent = host[12][u, :k]
                up.hypothesis_rows = (host[10][u, :k].copy(), host[11][u, :k].copy(), ent.copy())
                up.hypothesis = [int(w) for w in host[10][u, :k][ent != 0]]
                if k and not ent[0] and self._open[u] is not None:
                    up.hypothesis.insert(0, self._open[u][0])  # (they begin inside the word whose start is final)
            if flushed:
                kept = self._kept[u]
                cat = lambda j, dt: np.concatenate([r[j] for r in kept]).astype(dt)  # noqa: E731
                out.append(OnlineResult(float(score[u]), int(n_words[u]), cat(0, np.int32), cat(1, np.int32),
                                        cat(2, np.uint8), int(forced[u]), up))
                self._forget(u)
            else:
                out.append(up)
        return out

    def finish(self, streams=None):
        """End the recordings of ``streams`` (all by default): the pending frames are walked back from the best final
        word and handed out, and the streams are fresh again.  One :class:`OnlineResult` per flushed stream, in the
        order given."""
        order = list(range(self.n_streams)) if streams is None else [int(u) for u in streams]
        flags = np.zeros(self.n_streams, np.uint8)
        flags[order] = 1
        out = self._commit(flags, False)
        return [out[u] for u in order]


# ---- forced alignment ---------------------------------------------------------------------------
def align_workspace_bytes(total_frames, n_utts, max_words, S) -> int:
    return _workspace_bytes("sapr_connected_align_workspace_bytes", total_frames, n_utts, max_words, S)


@dataclass
class AlignResult:
    score: np.ndarray         # [N] f64: the best path's log score through the transcript; -inf without a path
    path_word: np.ndarray     # [total_frames] i32: vocabulary indices (-1 where there is no path)
    path_state: np.ndarray    # [total_frames] i32 (-1 where there is no path)
    path_entry: np.ndarray    # [total_frames] u8: 1 where a word begins
    word_start: np.ndarray    # [total_words] i32: the frame, from the utterance's start, at which word k begins (-1)
    word_offsets: np.ndarray  # [N + 1] i64: transcript k of utterance u is entry word_offsets[u] + k
    offsets: np.ndarray       # [N + 1] i64
    words: np.ndarray         # [total_words] i32: the transcripts, one after the other
    optional: np.ndarray = None  # [total_words] u8: 1 where the slot could be stepped over; None: no flags were given

    def segments(self, u):
        """``[(word_index, start, end_exclusive), ...]`` of utterance ``u``: one entry per transcript slot the path
        took (every slot, unless optional slots were given: a slot the path stepped over has ``word_start`` -1 and no
        entry), frames counted from the utterance's own start; a slot ends where the next taken slot begins.  ``[]``
        where there is no path."""
        lo, hi = int(self.word_offsets[u]), int(self.word_offsets[u + 1])
        if self.optional is None:
            if hi == lo or int(self.word_start[lo]) < 0:
                return []
            starts = [int(a) for a in self.word_start[lo:hi]]
            ends = starts[1:] + [int(self.offsets[u + 1] - self.offsets[u])]
            return [(int(w), a, b) for w, a, b in zip(self.words[lo:hi], starts, ends)]
        taken = [(int(w), int(a)) for w, a in zip(self.words[lo:hi], self.word_start[lo:hi]) if int(a) >= 0]
        if not taken or not np.isfinite(self.score[u]):
            return []
        ends = [a for _, a in taken[1:]] + [int(self.offsets[u + 1] - self.offsets[u])]
        return [(w, a, b) for (w, a), b in zip(taken, ends)]

    def word_examples(self, features):
        """Cut the utterances at the word boundaries: ``features`` are the frame-major ``(T, D)`` arrays that were
        aligned; returns ``{word_index: [array, ...]}`` (views), the per-word training examples ``GaussianHMM.fit`` /
        ``GMMHMM.fit`` take.  Utterances without a path contribute nothing."""
        if len(features) != len(self.offsets) - 1:
            raise ValueError(f"{len(features)} feature arrays for {len(self.offsets) - 1} aligned utterances")
        out = {}
        for u, x in enumerate(features):
            x = np.asarray(x)
            if x.shape[0] != int(self.offsets[u + 1] - self.offsets[u]):
                raise ValueError(f"utterance {u} has {x.shape[0]} frames, the alignment "
                                 f"{int(self.offsets[u + 1] - self.offsets[u])}")
            for w, a, b in self.segments(u):
                out.setdefault(w, []).append(x[a:b])
        return out


@dataclass
class RankAlignment(AlignResult):
    """:meth:`NBestResult.align`: the alignment of one rank's strings, over the utterances whose list has that rank."""
    utterances: np.ndarray = None  # [n] the utterances of the list's batch this result covers, in order


def with_optional(transcripts, word):
    """``(transcripts', optional')`` with vocabulary index ``word`` as an optional slot in front of, between and behind
    the words of every transcript: ``word? w1 word? w2 ... wK word?`` — silence nobody wrote down, a filler the speaker
    may have said.  Where a transcript already names ``word`` no second one is put beside it."""
    word = int(word)
    out_t, out_o = [], []
    for t in transcripts:
        t = [int(w) for w in t]
        nt, no = [], []
        for k, w in enumerate(t):
            if w != word and (k == 0 or t[k - 1] != word):
                nt.append(word)
                no.append(1)
            nt.append(w)
            no.append(0)
        if t and t[-1] != word:
            nt.append(word)
            no.append(1)
        out_t.append(nt)
        out_o.append(no)
    return out_t, out_o


def _optional(optional, transcripts):
    """Validated flags -> ``optional[total_words] u8`` (``None`` stays ``None``: the kernels without flags)."""
    if optional is None:
        return None
    optional = [np.asarray(o).reshape(-1) for o in optional]
    if len(optional) != len(transcripts):
        raise ValueError(f"{len(optional)} optional-flag sequences for {len(transcripts)} transcripts")
    for u, (o, t) in enumerate(zip(optional, transcripts)):
        if o.size != t.size:
            raise ValueError(f"utterance {u} has {o.size} optional flags for {t.size} transcript slots")
        if not np.isin(o, (0, 1)).all():
            raise ValueError(f"the optional flags of utterance {u} must be 0 or 1")
        o = o.astype(bool)
        if (o[1:] & o[:-1]).any():
            raise ValueError(f"utterance {u} has two neighbouring optional slots: at most one slot in a row may be "
                             f"stepped over")
        if o.all():
            raise ValueError(f"every slot of utterance {u} is optional: at least one slot must be mandatory")
    return (np.concatenate(optional).astype(np.uint8) if optional else np.zeros(0, np.uint8))


def _transcripts(transcripts, n_utts, network, optional=None):
    """Validated transcripts and flags -> ``(words[total_words] i32, word_offsets[N + 1] i64, max_words,
    flags[total_words] u8)``; ``flags`` is ``None`` where no ``optional`` was given."""
    transcripts = [np.asarray(t, dtype=np.int64).reshape(-1) for t in transcripts]
    if len(transcripts) != n_utts:
        raise ValueError(f"{len(transcripts)} transcripts for {n_utts} utterances")
    limit = MAX_FLAT // network.SP
    for u, t in enumerate(transcripts):
        if t.size == 0:
            raise ValueError(f"the transcript of utterance {u} is empty")
        if t.min() < 0 or t.max() >= network.W:
            raise ValueError(f"the transcript of utterance {u} names a word outside the vocabulary 0..{network.W - 1}")
        if t.size * network.SP > MAX_FLAT:
            raise ValueError(f"the transcript of utterance {u} has {t.size} words: K * SP = {t.size * network.SP} "
                             f"exceeds the limit of {MAX_FLAT} chain positions ({limit} words at SP = {network.SP})")
    _, word_offs = _offsets([t.size for t in transcripts])
    words = np.concatenate(transcripts).astype(np.int32) if transcripts else np.zeros(0, np.int32)
    max_words = max((t.size for t in transcripts), default=1)
    return words, word_offs, max_words, _optional(optional, transcripts)


def align_opt_workspace_bytes(total_frames, n_utts, max_words, S) -> int:
    return _workspace_bytes("sapr_connected_align_opt_workspace_bytes", total_frames, n_utts, max_words, S)


def _run_align(logb, offs_dev, offs, transcripts, network, optional=None) -> AlignResult:
    """One ``sapr_connected_align_opt`` over device ``logb[total_frames, R]``: with the flags of ``optional``, or
    without flags (NULL), which is ``sapr_connected_align`` on its own, smaller workspace."""
    torch = _torch()
    dev = logb.device
    n_utts, total = int(offs.size - 1), int(offs[-1])
    words, word_offs, max_words, flags = _transcripts(transcripts, n_utts, network, optional)
    total_words = int(word_offs[-1])
    ls, lt, lx, _ = network.device(dev)
    words_dev = torch.from_numpy(words).to(dev)
    word_offs_dev = torch.from_numpy(word_offs).to(dev)
    flags_dev = None if flags is None else torch.from_numpy(flags).to(dev)
    name = "sapr_connected_align" if flags is None else "sapr_connected_align_opt"
    workspace, ws_bytes = _workspace(name + "_workspace_bytes", dev, total, n_utts, max_words, network.S)
    score = torch.empty(n_utts, dtype=torch.float64, device=dev)
    path_word = torch.empty(total, dtype=torch.int32, device=dev)
    path_state = torch.empty(total, dtype=torch.int32, device=dev)
    path_entry = torch.empty(total, dtype=torch.uint8, device=dev)
    word_start = torch.empty(total_words, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().sapr_connected_align_opt(
        _lib.ptr(logb), _lib.ptr(offs_dev), n_utts, total, _lib.ptr(words_dev), _lib.ptr(word_offs_dev),
        _lib.ptr(flags_dev), total_words, max_words, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), network.word_penalty,
        network.W, network.S, _lib.ptr(workspace), ws_bytes, _lib.ptr(score), _lib.ptr(path_word),
        _lib.ptr(path_state), _lib.ptr(path_entry), _lib.ptr(word_start), _lib.current_stream()), name)
    host = [a.copy() for a in _lib.to_host(score, path_word, path_state, path_entry, word_start)]
    return AlignResult(*host, word_offsets=word_offs, offsets=offs, words=words, optional=flags)


def align_viterbi(logb, lengths, transcripts, network: ConnectedNetwork, optional=None) -> AlignResult:
    """Forced alignment over a given ``logb`` (the shapes :func:`connected_viterbi` takes): ``transcripts`` is one
    sequence of vocabulary indices per utterance, the words the utterance is known to hold, in order.  ``optional``:
    one 0/1 sequence per utterance, as long as its transcript — a slot marked 1 may be walked through or stepped over
    (no two neighbours, not every slot; :func:`with_optional` builds ``sil? w1 sil? ... wK sil?``).  The definition is
    ``tests/_optional_ref.py``; a stepped-over slot has ``word_start`` -1 and no entry in ``segments``."""
    torch = _torch()
    lengths, offs = _offsets(lengths)
    _transcripts(transcripts, int(lengths.size), network, optional)  # (refused before a device is asked for)
    dev = _lib.require_gpu()
    logb = _flat_states(logb, int(offs[-1]), network, dev)
    return _run_align(logb, torch.from_numpy(offs).to(dev), offs, transcripts, network, optional)


def connected_align(batch_or_feature_list, transcripts, network: ConnectedNetwork, optional=None) -> AlignResult:
    """Emission (by the network's family) and the alignment recursion: a ``trellis.FeatureBatch`` or a list of
    frame-major ``(T, D)`` feature arrays, with one transcript of vocabulary indices per utterance (and ``optional``
    as :func:`align_viterbi` takes it)."""
    # (refused before a device is asked for)
    _transcripts(transcripts, _n_utts(batch_or_feature_list), network, optional)
    feats, offs_dev, offs = _features(batch_or_feature_list)
    logb = _EMIT[network.family](feats, network)
    return _run_align(logb, offs_dev, offs, transcripts, network, optional)


# ---- embedded Baum-Welch --------------------------------------------------------------------------
def embed_stats_width(S, D) -> int:
    return _stats_width("sapr_connected_embed_stats_width", S, D)


def embed_workspace_bytes(total_frames, n_utts, total_words, max_words, S, D) -> int:
    return _workspace_bytes("sapr_connected_embed_workspace_bytes", total_frames, n_utts, total_words, max_words, S, D)


def embed_full_stats_width(S, D) -> int:
    return _stats_width("sapr_connected_embed_full_stats_width", S, D)


def embed_full_workspace_bytes(total_frames, n_utts, total_words, max_words, W, S, D) -> int:
    return _workspace_bytes("sapr_connected_embed_full_workspace_bytes", total_frames, n_utts, total_words, max_words,
                            W, S, D)


def embed_gmm_stats_width(S, M, D) -> int:
    return _stats_width("sapr_connected_embed_gmm_stats_width", S, M, D)


def embed_gmm_workspace_bytes(total_frames, n_utts, total_words, max_words, W, S, M, D) -> int:
    return _workspace_bytes("sapr_connected_embed_gmm_workspace_bytes", total_frames, n_utts, total_words, max_words,
                            W, S, M, D)


@dataclass
class EmbeddedStats:
    loglik: np.ndarray        # [N] f64: log P(utterance | its transcript's chain); -inf (or NaN) without a path
    stats: np.ndarray         # [W, width] f64 (sapr_connected_embed[_full | _gmm]_stats_width), or None
    post: np.ndarray          # [total_frames, max_words * SP] f64: gamma_t at chain position k * SP + s, or None
    offsets: np.ndarray       # [N + 1] i64
    word_offsets: np.ndarray  # [N + 1] i64
    words: np.ndarray         # [total_words] i32: the transcripts, one after the other
    S: int = 0                # the network's states (the layout of a statistics row) ...
    SP: int = 0               # ... and the padded states of a chain position
    D: int = 0                # feature width of the obs blocks (0: none)
    n_states: tuple = ()      # every word model's own states
    layout: str = "diag"      # the row's observation blocks: "diag" {obs, obs**2}, "full" {obs, obs*obs.T} or "gmm"
    M: int = 0                # ... {post_mix, obs, obs**2} per component, M of them per state (0: no mixtures)

    def split(self, w):
        """hmmlearn's statistics dict of word model ``w``, cut to the model's own states; ``logprob`` is the row's
        reserved 0.0.  A "diag" row gives ``trellis.split_stats``' dict (``obs**2``), a "full" row
        ``full_cov.split_stats``' (``obs*obs.T``), a "gmm" row ``gmm_hmm.split_stats``' (``post_mix`` and the
        per-component ``obs`` / ``obs**2``)."""
        from .trellis import split_stats
        if self.stats is None:
            raise ValueError("the statistics were not asked for")
        if self.layout == "gmm":
            from .gmm_hmm import split_stats as split_gmm
            return split_gmm(self.stats[w], self.S, self.M, self.D, self.n_states[w] if self.n_states else None)
        if self.layout == "full":
            from .full_cov import split_stats as split_full
            return split_full(self.stats[w], self.S, self.D, self.n_states[w] if self.n_states else None)
        return split_stats(self.stats[w], self.S, self.D, self.n_states[w] if self.n_states else None, self.D)

    def posteriors(self, u):
        """``gamma[T, K, SP]`` of utterance ``u`` (zeros where it has no path)."""
        if self.post is None:
            raise ValueError("the posteriors were not asked for (want_post=True)")
        lo, hi = int(self.offsets[u]), int(self.offsets[u + 1])
        K = int(self.word_offsets[u + 1] - self.word_offsets[u])
        return self.post[lo:hi].reshape(hi - lo, -1, self.SP)[:, :K]


def _run_embed(logb, feats, offs_dev, offs, transcripts, network, want_stats, want_post,
               second_moments=False, mixtures=False, optional=None) -> EmbeddedStats:
    """One embedded E-step over device ``logb[total_frames, R]`` (and device ``feats`` or ``None``), by the ``_opt``
    entry of the statistics' layout with the flags of ``optional`` or NULL: ``sapr_connected_embed``;
    ``second_moments``: ``sapr_connected_embed_full``, whose rows carry ``obs*obs.T``; ``mixtures``:
    ``sapr_connected_embed_gmm``, whose rows carry the statistics per mixture component of the network's ``GmmPack``
    as the emission read it.  Without ``want_stats`` either switch is the plain entry without features."""
    torch = _torch()
    layout = "gmm" if mixtures and want_stats else "full" if second_moments and want_stats else "diag"
    D = 0 if feats is None else int(feats.shape[1])
    if layout != "diag" and D == 0:
        raise ValueError(f"the {'mixture statistics' if layout == 'gmm' else 'second moments'} need the frames: feats "
                         f"[total_frames, D] with D >= 1")
    dev = logb.device
    n_utts, total = int(offs.size - 1), int(offs[-1])
    words, word_offs, max_words, flags = _transcripts(transcripts, n_utts, network, optional)
    total_words = int(word_offs[-1])
    if layout == "gmm" and D != network.D:
        raise ValueError(f"the utterances have {D} features, the models {network.D}")
    W, S, M = network.W, network.S, int(network.pack.M) if layout == "gmm" else 0
    ls, lt, lx, pack = network.device(dev)
    # per layout: the entry's stem, what its size and width functions take in front of D, its arguments behind D
    entry, size_shape, width_shape, lead = {
        "diag": ("sapr_connected_embed", (S,), (S,), ()),
        "full": ("sapr_connected_embed_full", (W, S), (S,), ()),
        "gmm": ("sapr_connected_embed_gmm", (W, S, M), (S, M), (_lib.ptr(pack), M)),
    }[layout]
    words_dev = torch.from_numpy(words).to(dev)
    word_offs_dev = torch.from_numpy(word_offs).to(dev)
    flags_dev = None if flags is None else torch.from_numpy(flags).to(dev)
    workspace, ws_bytes = _workspace(entry + "_workspace_bytes", dev, total, n_utts, total_words, max_words,
                                     *size_shape, D)
    loglik = torch.empty(n_utts, dtype=torch.float64, device=dev)
    stats = torch.empty((W, _stats_width(entry + "_stats_width", *width_shape, D)), dtype=torch.float64, device=dev) \
        if want_stats else None
    post = torch.zeros((total, max_words * network.SP), dtype=torch.float64, device=dev) if want_post else None
    _lib.check(getattr(_lib.load(), entry + "_opt")(
        _lib.ptr(logb), _lib.ptr(feats), D, *lead, _lib.ptr(offs_dev), n_utts, total, _lib.ptr(words_dev),
        _lib.ptr(word_offs_dev), _lib.ptr(flags_dev), total_words, max_words, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx),
        network.word_penalty, W, S, _lib.ptr(workspace), ws_bytes, _lib.ptr(loglik), _lib.ptr(stats), _lib.ptr(post),
        _lib.current_stream()), entry + ("" if flags is None else "_opt"))
    host = [None if a is None else a.cpu().numpy() for a in (loglik, stats, post)]
    return EmbeddedStats(*host, offsets=offs, word_offsets=word_offs, words=words, S=S, SP=network.SP, D=D,
                         n_states=tuple(network.n_states), layout=layout, M=M)


def _refuse_stats(network, second_moments=False, mixtures=False):
    if mixtures:
        if second_moments:
            raise ValueError("mixtures=True and second_moments=True exclude each other: a statistics row carries "
                             "either the per-component sums of a 'gmm' network or the second-moment matrices")
        if network.family != "gmm":
            raise ValueError(f"mixtures=True serves a network of the 'gmm' family (GMMHMM word models with their "
                             f"GmmPack); this one is {network.family!r}")
        return
    if second_moments:
        if network.family == "gmm":
            raise NotImplementedError(
                "embedded statistics with second_moments=True are served for the 'diag' and 'full' families; the "
                "'gmm' family needs mixture responsibilities, which mixtures=True accumulates (loglik and post are "
                "served either way: want_stats=False)")
        return
    if network.family != "diag":
        raise NotImplementedError(
            f"embedded statistics are served for the 'diag' family by default; the {network.family!r} family needs "
            f"{'mixture responsibilities (mixtures=True)' if network.family == 'gmm' else 'second-moment matrices'} "
            f"(loglik and post are served: want_stats=False)")


def embedded_forward_backward(logb, lengths, transcripts, network: ConnectedNetwork, feats=None,
                              want_post=False, second_moments=False, mixtures=False, optional=None) -> EmbeddedStats:
    """Forward-backward over every utterance's transcript chain on a given ``logb`` (the shapes
    :func:`connected_viterbi` takes) — the counterpart of :func:`align_viterbi`.  ``feats``: the float32 frames
    ``[total_frames, D]`` (host array or device tensor) for the ``obs`` blocks of the statistics; without them the
    statistics carry ``start``, ``trans``, ``post`` and ``nobs`` only.  The definition is ``tests/_embedded_ref.py``.
    ``second_moments=True`` (needs ``feats``): the rows carry ``obs*obs.T`` in place of ``obs**2``
    (``sapr_connected_embed_full``; definition ``tests/_embedded_full_ref.py``).  ``mixtures=True`` (needs ``feats``
    and a "gmm" network, whose ``GmmPack`` supplies the components): the rows carry ``post_mix`` and the per-component
    ``obs`` / ``obs**2`` (``sapr_connected_embed_gmm``; definition ``tests/_embedded_gmm_ref.py``).  ``optional``: the
    flags :func:`align_viterbi` takes — the ``_opt`` entry points; definition ``tests/_optional_ref.py``."""
    torch = _torch()
    lengths, offs = _offsets(lengths)
    _transcripts(transcripts, int(lengths.size), network, optional)  # (refused before a device is asked for)
    if mixtures:
        _refuse_stats(network, second_moments, mixtures)
        if network.pack is None or not hasattr(network.pack, "M"):
            raise ValueError("mixtures=True needs the network's GmmPack (ConnectedNetwork.from_models)")
    if (second_moments or mixtures) and (feats is None or np.ndim(feats) != 2 or int(np.shape(feats)[1]) == 0):
        raise ValueError(f"{'mixtures' if mixtures else 'second_moments'}=True needs the frames: feats "
                         f"[sum(lengths), D] with D >= 1")
    dev = _lib.require_gpu()
    total = int(offs[-1])
    logb = _flat_states(logb, total, network, dev)
    if feats is not None:
        feats = _flat_feats(feats, total, dev)
        if int(feats.shape[1]) == 0:
            feats = None
    return _run_embed(logb, feats, torch.from_numpy(offs).to(dev), offs, transcripts, network, True, want_post,
                      second_moments, mixtures, optional)


def embedded_estep(batch_or_feature_list, transcripts, network: ConnectedNetwork, want_post=False,
                   want_stats=True, second_moments=False, mixtures=False, optional=None) -> EmbeddedStats:
    """Emission (by the network's family) and forward-backward over the transcript chains — the counterpart of
    :func:`connected_align`.  ``loglik`` and ``post`` are served for all three families; the statistics for "diag"
    by default (for "gmm" and "full" asking for them without their switch raises ``NotImplementedError``).  With
    ``second_moments=True`` the statistics of a "diag" or "full" network carry ``obs*obs.T``
    (``sapr_connected_embed_full``), what the M-step of a "full" or "tied" model reads.  With ``mixtures=True`` the
    statistics of a "gmm" network carry ``post_mix`` and the per-component ``obs`` / ``obs**2``
    (``sapr_connected_embed_gmm``), what ``gmm_hmm.gmm_m_step`` reads; on another family, or together with
    ``second_moments=True``, the switch is a ``ValueError``.  ``optional``: the flags :func:`align_viterbi` takes."""
    # (refused before a device is asked for)
    _transcripts(transcripts, _n_utts(batch_or_feature_list), network, optional)
    if want_stats or mixtures:
        _refuse_stats(network, second_moments, mixtures)
    feats, offs_dev, offs = _features(batch_or_feature_list)
    logb = _EMIT[network.family](feats, network)
    return _run_embed(logb, feats if want_stats else None, offs_dev, offs, transcripts, network, want_stats, want_post,
                      second_moments, mixtures, optional)


def _diag_of_moments(st, covariance_type):
    """The statistics dict the M-step of ``covariance_type`` reads, from a row with ``obs*obs.T``: a "diag" or
    "spherical" member of a mixed vocabulary takes ``obs**2`` = the diagonal of each matrix (the float64 square of
    the widened frame, where the all-diagonal route adds the float32 square: one ulp of float32 per term)."""
    if covariance_type in ("diag", "spherical"):
        st = dict(st)
        st["obs**2"] = np.ascontiguousarray(np.diagonal(st["obs*obs.T"], axis1=1, axis2=2))
    return st


def embedded_fit(models, features, transcripts, n_iter=10, tol=1e-2, exit_states="last", word_penalty=0.0,
                 names=None, second_moments=False, optional=None):
    """Embedded Baum-Welch: train the word models of a ``GaussianHMM`` vocabulary in place from recordings of several
    words (``features``: frame-major ``(T, D)`` arrays) and their transcripts (vocabulary indices), without cutting
    the recordings.  Each iteration: ``ConnectedNetwork.from_models``, the emission, the E-step, then
    ``hmmlearn_hmm.m_step_typed`` per model with the model's own covariance type and hyper-parameters; a word that
    never occurs (in an utterance with a path) stays untouched.  One ``ConvergenceMonitor`` runs on the sum of
    ``loglik`` over the utterances with a path; returns its history as a list.

    ``second_moments=False`` serves "diag" / "spherical" vocabularies (``sapr_connected_embed``).  With
    ``second_moments=True`` any ``GaussianHMM`` vocabulary trains, "full" and "tied" members included: the E-step is
    ``sapr_connected_embed_full``, a "tied" model ends with one ``(D, D)`` matrix, and a "diag" / "spherical" member
    reads the diagonal of its second-moment matrices.

    A list of ``GMMHMM`` objects (that share ``n_mix`` and the feature width) trains through
    ``sapr_connected_embed_gmm``: per iteration the network over the vocabulary's ``GmmPack``, ``emit_gmm``, the E-step
    with mixture responsibilities, then ``gmm_hmm.gmm_m_step`` per model with the model's own hyper-parameters.  A
    list that mixes ``GMMHMM`` and ``GaussianHMM`` objects is a ``ValueError``.

    ``optional``: the flags :func:`align_viterbi` takes, e.g. ``embedded_fit(models, features,
    *with_optional(transcripts, sil))`` — a skippable silence model between the words, trained with them; every
    family goes through its ``_opt`` entry point."""
    from .hmmlearn_hmm import ConvergenceMonitor, m_step_typed
    models = list(models)
    family = vocabulary_family(models, names, None)
    if family == "gmm":
        if second_moments:
            raise ValueError("second_moments=True serves GaussianHMM vocabularies; GMMHMM word models train on "
                             "mixture responsibilities")
    else:
        family = vocabulary_family(models, names, "hmmlearn")
        if family != "diag" and not second_moments:
            raise ValueError("embedded_fit serves 'diag' and 'spherical' GaussianHMM vocabularies by default: a 'full' "
                             "or 'tied' model needs second-moment matrices, which second_moments=True accumulates")
    gmm = family == "gmm"

    def network():
        # (packing a 'gmm' or 'full' vocabulary validates every model and notes what it found on the object: done on
        # shallow copies, so that a word that is never trained keeps its bytes)
        return ConnectedNetwork.from_models(models if family == "diag" else [copy.copy(m) for m in models],
                                            exit_states, word_penalty, names, "gmmhmm" if gmm else "hmmlearn")

    def m_step(m, st):
        """The one family-specific piece: a model's new parameters from its statistics dict, by its own M-step."""
        if gmm:
            from .gmm_hmm import gmm_m_step
            m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_ = gmm_m_step(
                st, m.startprob_, m.transmat_, m.weights_, m.means_, m.covars_, m.params, m.startprob_prior,
                m.transmat_prior, m.weights_prior, m.means_prior, m.means_weight, m.covars_prior, m.covars_weight,
                m.min_covar)
            return
        if second_moments:
            st = _diag_of_moments(st, m.covariance_type)
        m.startprob_, m.transmat_, m.means_, m._covars_ = m_step_typed(
            st, m.covariance_type, m.startprob_, m.transmat_, m.params, m.startprob_prior, m.transmat_prior,
            m.means_prior, m.means_weight, m.covars_prior, m.covars_weight, np.asarray(m.means_, dtype=np.float64),
            np.asarray(m._covars_, dtype=np.float64))

    net = network()
    _transcripts(transcripts, len(features), net, optional)  # (refused before a device is asked for)
    feats, offs_dev, offs = _features(features)
    monitor = ConvergenceMonitor(tol, n_iter)
    for _ in range(n_iter):
        net = network()
        res = _run_embed(_EMIT[net.family](feats, net), feats, offs_dev, offs, transcripts, net, True, False,
                         second_moments, gmm, optional)
        for w, m in enumerate(models):
            st = res.split(w)
            if st["nobs"] != 0:  # (a word that never occurs stays untouched)
                m_step(m, st)
        monitor.report(float(res.loglik[np.isfinite(res.loglik)].sum()))
        if monitor.converged:
            break
    return list(monitor.history)


# ---- discriminative (MMI) training ------------------------------------------------------------------
def loop_stats_workspace_bytes(total_frames, n_utts, W, S, D) -> int:
    return _workspace_bytes("sapr_connected_loop_stats_workspace_bytes", total_frames, n_utts, W, S, D)


def _run_loop_stats(post, feats, offs_dev, n_utts, total, network, keep_dev=None):
    """One ``sapr_connected_loop_stats`` over device ``post[total_frames, R]`` and device ``feats`` -> the device rows
    ``[W, sapr_connected_embed_stats_width(S, D)]``; ``keep_dev``: a device uint8 per utterance, or ``None`` (all)."""
    torch = _torch()
    dev = post.device
    D = int(feats.shape[1])
    workspace, ws_bytes = _workspace("sapr_connected_loop_stats_workspace_bytes", dev, total, n_utts, network.W,
                                     network.S, D)
    stats = torch.empty((network.W, embed_stats_width(network.S, D)), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().sapr_connected_loop_stats(
        _lib.ptr(post), _lib.ptr(feats), D, _lib.ptr(offs_dev), n_utts, total, _lib.ptr(keep_dev), network.W,
        network.S, _lib.ptr(workspace), ws_bytes, _lib.ptr(stats), _lib.current_stream()), "sapr_connected_loop_stats")
    return stats


def _keep_flags(keep, n_utts):
    if keep is None:
        return None
    keep = np.asarray(keep).reshape(-1)
    if keep.size != n_utts:
        raise ValueError(f"{keep.size} keep flags for {n_utts} utterances")
    return np.ascontiguousarray(keep != 0, dtype=np.uint8)


def loop_stats(post, feats, lengths, network: ConnectedNetwork, keep=None) -> np.ndarray:
    """The word loop's state posteriors reduced to per-word statistics (``sapr_connected_loop_stats``; the definition
    is ``tests/_mmi_ref.py``): ``post`` is float64 ``[total_frames, W * SP]``, ``[total_frames, W, SP]`` or
    ``[total_frames, W, S]`` (what :func:`connected_posteriors` returns with ``want_post=True``), ``feats`` the float32
    frames ``[total_frames, D]``, either a host array or a device tensor; ``keep``: one flag per utterance, the
    utterances that count (``None``: all).  Returns the rows ``[W, width]`` of ``sapr_connected_embed``'s layout with
    ``post``, ``obs`` and ``obs**2`` filled, ``nobs`` = the kept utterances with a frame and zeros elsewhere:
    ``trellis.split_stats(rows[w], S, D, n_states[w], D)`` reads them, as ``EmbeddedStats.split`` does."""
    torch = _torch()
    lengths, offs = _offsets(lengths)
    n_utts, total = int(lengths.size), int(offs[-1])
    keep = _keep_flags(keep, n_utts)
    dev = _lib.require_gpu()
    post = _flat_states(post, total, network, dev, 0.0, "post")
    feats = _flat_feats(feats, total, dev, 1)
    keep_dev = None if keep is None else torch.from_numpy(keep).to(dev)
    return _run_loop_stats(post, feats, torch.from_numpy(offs).to(dev), n_utts, total, network, keep_dev).cpu().numpy()


@dataclass
class MmiStats:
    """One E-step of MMI training (:func:`mmi_estep`; the definition is ``tests/_mmi_ref.py``)."""
    num: EmbeddedStats        # the numerator: sapr_connected_embed over the kept utterances' transcript chains
    den_stats: np.ndarray     # [W, width] f64: the denominator rows of sapr_connected_loop_stats, num.stats' layout
    num_loglik: np.ndarray    # [N] f64: the transcript chain's log-likelihood plus the transcript's lmscore
    den_loglik: np.ndarray    # [N] f64: the word loop's log-likelihood, over every word string the grammar allows
    lmscore: np.ndarray       # [N] f64: the language-model score of the transcript
    keep: np.ndarray          # [N] bool: both likelihoods finite — the utterances that count
    objective: float          # F = the sum over the kept utterances of num_loglik - den_loglik (<= 0 up to rounding)

    def split(self, w):
        """``(numerator dict, denominator dict)`` of word model ``w``: hmmlearn's statistics dicts, cut to the model's
        own states; the denominator's ``start`` and ``trans`` are zeros."""
        from .trellis import split_stats
        n = self.num
        return n.split(w), split_stats(self.den_stats[w], n.S, n.D, n.n_states[w] if n.n_states else None, n.D)


def _lm_scores(transcripts, network):
    """``lmscore[u] = lm_start[w_0] + sum_k lm[w_{k-1}, w_k] + lm_end[w_{K-1}]`` under :meth:`loop_lm`, float64 on the
    host, added in transcript order.  A transcript the language model forbids is a ``ValueError`` that names it."""
    lm, lm_start, lm_end = network.loop_lm()
    out = np.zeros(len(transcripts))
    for u, t in enumerate(transcripts):
        t = [int(w) for w in t]
        sc = np.float64(lm_start[t[0]])
        for a, b in zip(t[:-1], t[1:]):
            sc = sc + lm[a, b]
        sc = sc + lm_end[t[-1]]
        if not np.isfinite(sc):
            raise ValueError(f"the grammar forbids the transcript of utterance {u} ({t}): its language-model score is "
                             f"{float(sc)!r}")
        out[u] = sc
    return out


def _refuse_mmi_family(family):
    if family != "diag":
        raise NotImplementedError(
            f"MMI training is served for 'diag' and 'spherical' GaussianHMM word models; the {family!r} family needs a "
            f"denominator kernel of its own ({'mixture responsibilities' if family == 'gmm' else 'second moments'} "
            f"over the word loop's posteriors)")


def _check_mmi_transcripts(transcripts, n_utts, network, names=None):
    """The transcripts validated on the host (an unknown word is named), and their language-model scores."""
    rows = [np.asarray(t, dtype=np.int64).reshape(-1) for t in transcripts]
    for u, t in enumerate(rows):
        for w in t:
            if not 0 <= int(w) < network.W:
                raise ValueError(f"the transcript of utterance {u} names word {int(w)}, which is outside the "
                                 f"vocabulary 0..{network.W - 1}"
                                 + (f" ({', '.join(map(str, names))})" if names is not None else ""))
    _transcripts(rows, n_utts, network)
    return _lm_scores(rows, network)


def mmi_estep(batch_or_feature_list, transcripts, network: ConnectedNetwork, acoustic_scale=1.0) -> MmiStats:
    """One E-step of maximum-mutual-information training on a "diag" network.  With ``logb' = acoustic_scale * logb``
    (at 1.0 ``logb`` as it is): the numerator is ``sapr_connected_embed`` over each transcript's chain with
    ``word_penalty = 0.0`` plus the transcript's language-model score under ``network.loop_lm()``; the denominator is
    ``sapr_connected_posteriors`` over the word loop on the same ``logb'``, whose state posteriors
    ``sapr_connected_loop_stats`` reduces to per-word rows on the device (they never reach the host).  An utterance
    counts (``keep``) where both likelihoods are finite.  Where an utterance was dropped the numerator statistics come
    from a second run of the E-step over the kept utterances alone.  A transcript the grammar forbids is refused with a
    ``ValueError`` that names the utterance, before a device is asked for; optional transcript slots are not
    offered (the transcript's language-model score would depend on the path)."""
    import dataclasses
    torch = _torch()
    n_utts = _n_utts(batch_or_feature_list)
    scale = float(acoustic_scale)
    if not (scale > 0.0 and np.isfinite(scale)):
        raise ValueError(f"acoustic_scale must be a positive number, got {acoustic_scale!r}")
    _refuse_mmi_family(network.family)
    lmscore = _check_mmi_transcripts(transcripts, n_utts, network)  # (refused before a device is asked for)
    feats, offs_dev, offs = _features(batch_or_feature_list)
    total = int(offs[-1])
    logb = emit_diag(feats, network)
    if scale != 1.0:
        logb = logb * scale
    chain = copy.copy(network)  # the transcript's chain pays its word boundaries through lmscore
    chain.word_penalty = 0.0
    num = _run_embed(logb, feats, offs_dev, offs, transcripts, chain, True, False)
    den_ll, _, _, post = _posteriors_device(logb, offs_dev, offs, network, False, True)
    den_loglik = den_ll.cpu().numpy()
    with np.errstate(invalid="ignore"):
        num_loglik = num.loglik + lmscore
    keep = np.isfinite(num_loglik) & np.isfinite(den_loglik)
    if not keep.all() and np.isfinite(num.loglik[~keep]).any():
        # an utterance that is dropped although its chain has a path: the numerator again, over the kept ones alone
        kept = np.flatnonzero(keep)
        if kept.size == 0:  # (nothing counts: a NaN in the language model makes every denominator NaN)
            num = dataclasses.replace(num, stats=np.zeros_like(num.stats))
        else:
            rows = np.concatenate([np.arange(offs[u], offs[u + 1]) for u in kept])
            idx = torch.from_numpy(rows.astype(np.int64)).to(logb.device)
            _, offs_k = _offsets(np.diff(offs)[kept])
            again = _run_embed(logb.index_select(0, idx), feats.index_select(0, idx),
                               torch.from_numpy(offs_k).to(idx.device), offs_k, [transcripts[u] for u in kept], chain,
                               True, False)
            num = dataclasses.replace(num, stats=again.stats)
    keep_dev = torch.from_numpy(keep.astype(np.uint8)).to(logb.device)
    den_stats = _run_loop_stats(post, feats, offs_dev, n_utts, total, network, keep_dev).cpu().numpy()
    objective = float((num_loglik[keep] - den_loglik[keep]).sum())
    return MmiStats(num, den_stats, num_loglik, den_loglik, lmscore, keep, objective)


def mmi_update(num, den, means, covars, covariance_type, E=2.0, tau=0.0, min_covar=1e-3):
    """The extended Baum-Welch update of one word model's Gaussians (numpy float64): ``num`` / ``den`` are the
    statistics dicts of :meth:`MmiStats.split`, ``means[S, D]``, ``covars`` ``[S, D]`` ("diag") or ``[S]``
    ("spherical").  Per state, with I-smoothing ``tau`` on the numerator::

        n = num * (1 + tau / num.post)      occ = n.post - den.post   th1 = n.obs - den.obs   th2 = n.obs2 - den.obs2
        D_min = max(0, -occ, the larger real root over d of  var D^2 + (th2 + occ (var + mu^2) - 2 mu th1) D
                                                             + occ th2 - th1^2)
        D     = max(E den.post, 2 D_min)
        mu'   = (th1 + D mu) / (occ + D)    var' = max((th2 + D (var + mu^2)) / (occ + D) - mu'^2, min_covar)

    A state with ``occ + D == 0`` keeps its parameters; "spherical" takes the mean of ``var'`` over the features.
    Returns ``(means, covars)`` as new arrays."""
    if covariance_type not in ("diag", "spherical"):
        raise NotImplementedError(f"mmi_update serves 'diag' and 'spherical' covariances, not {covariance_type!r} "
                                  f"(the 'full' family)")
    mu = np.array(means, dtype=np.float64)
    cv = np.array(covars, dtype=np.float64)
    var = np.broadcast_to(cv[:, None], mu.shape).copy() if covariance_type == "spherical" else cv.copy()
    if var.shape != mu.shape:
        raise ValueError(f"covars of shape {cv.shape} do not fit means of shape {mu.shape}")
    n_post = np.asarray(num["post"], dtype=np.float64)
    scale = np.ones_like(n_post)
    if tau != 0.0:
        live = n_post != 0.0
        scale[live] = 1.0 + float(tau) / n_post[live]
    occ = n_post * scale - np.asarray(den["post"], dtype=np.float64)
    th1 = np.asarray(num["obs"], dtype=np.float64) * scale[:, None] - np.asarray(den["obs"], dtype=np.float64)
    th2 = np.asarray(num["obs**2"], dtype=np.float64) * scale[:, None] - np.asarray(den["obs**2"], dtype=np.float64)
    m2 = var + mu * mu
    b = th2 + occ[:, None] * m2 - 2.0 * mu * th1
    c = occ[:, None] * th2 - th1 * th1
    disc = b * b - 4.0 * var * c
    with np.errstate(invalid="ignore"):
        root = np.where(disc >= 0.0, (-b + np.sqrt(np.maximum(disc, 0.0))) / (2.0 * var), 0.0)
    d_min = np.maximum(np.maximum(root.max(axis=1), -occ), 0.0)
    d_s = np.maximum(float(E) * np.asarray(den["post"], dtype=np.float64), 2.0 * d_min)
    denom = occ + d_s
    moved = denom != 0.0
    safe = np.where(moved, denom, 1.0)[:, None]
    mu_new = (th1 + d_s[:, None] * mu) / safe
    var_new = np.maximum((th2 + d_s[:, None] * m2) / safe - mu_new * mu_new, float(min_covar))
    mu_out = np.where(moved[:, None], mu_new, mu)
    if covariance_type == "spherical":
        return mu_out, np.where(moved, var_new.mean(axis=1), cv)
    return mu_out, np.where(moved[:, None], var_new, cv)


def mmi_fit(models, features, transcripts, bigram=None, n_iter=4, E=2.0, tau=0.0, acoustic_scale=1.0,
            exit_states="last", word_penalty=0.0, names=None):
    """Discriminative training of a "diag" / "spherical" ``GaussianHMM`` vocabulary IN PLACE by maximum mutual
    information with the extended Baum-Welch update: ``features`` are frame-major ``(T, D)`` arrays, ``transcripts``
    vocabulary indices.  ``bigram``: the :class:`WordBigram` (or grammar) the word loop runs under, as
    ``bigram.scaled(1.0, word_penalty)``; without one the loop pays ``word_penalty`` per word boundary.  Each
    iteration: the network of the current models, :func:`mmi_estep`, then :func:`mmi_update` per word with the model's
    own covariance type and ``min_covar``; ``startprob_`` and ``transmat_`` are left as they are and a word that occurs
    in no kept transcript is left untouched.  Returns the history of the objective F, one entry per iteration, each
    evaluated before that iteration's update.  A ``GMMHMM`` vocabulary and one that holds a "full" or "tied" model are a
    ``NotImplementedError`` that names the family."""
    models = list(models)
    _refuse_mmi_family(vocabulary_family(models, names, None))
    if bigram is not None and not isinstance(bigram, WordBigram):
        raise ValueError(f"bigram must be a WordBigram, got a {type(bigram).__name__}")

    def network():
        if bigram is None:
            return ConnectedNetwork.from_models(models, exit_states, word_penalty, names, "hmmlearn")
        return ConnectedNetwork.from_models(models, exit_states, 0.0, names, "hmmlearn",
                                            bigram=bigram.scaled(1.0, word_penalty))

    _check_mmi_transcripts(transcripts, len(features), network(), names)  # (refused before a device is asked for)
    history = []
    for _ in range(int(n_iter)):
        st = mmi_estep(features, transcripts, network(), acoustic_scale)
        history.append(st.objective)
        for w, m in enumerate(models):
            num, den = st.split(w)
            if num["nobs"] == 0:
                continue
            m.means_, m._covars_ = mmi_update(num, den, m.means_, m._covars_, m.covariance_type, E, tau,
                                              getattr(m, "min_covar", 1e-3))
    return history

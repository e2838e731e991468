"""Host-side mirror of ``assignment2/decoder.py``: same ``Decoder`` API and result dictionaries,
but every utterance is scored against every word model in ONE kernel launch sequence instead of W Python
calls to ``model.decode`` per utterance (``decoder.py:42-47``).  ``decode_sequence`` returns the best word, ITS
score and ITS states (``decoder.py:35-49``) — the other W - 1 exact scores are thrown away — so the hmmlearn
models go through ``sapr_viterbi_decode_pruned`` (bounding pass over the vocabulary, exact lattice only for the
words that can still win; same bits as scoring every word) whenever the model pack allows it, and through
``sapr_viterbi_diag_scores`` + ``sapr_viterbi_backtrace`` otherwise; the reference's from-scratch models use
``sapr_custom_decode``.

Beyond the reference's API the hmmlearn models can be scored by total (forward) likelihood, ``GaussianHMM.score``
(hmmlearn_hmm.py:104) under every word model in one launch of ``sapr_forward_vocab``: ``score_batch`` returns the
[N, W] matrix, ``nbest`` the best words of each utterance with their posteriors, and ``scoring="forward"`` makes
``decode_batch`` classify by forward likelihood instead of by the Viterbi score.  ``state_posteriors`` returns the
state posterior lattice of every utterance under the decoder's word (or a named one) through
``sapr_state_posteriors_diag``.

``implementation="gmmhmm"`` serves Gaussian-mixture word models (``sapr_amd.GMMHMM`` pickles named
``<word>_gmmhmm_<n_iter>.pkl`` under ``models_dir/gmmhmm/``) through the same API: one launch of
``sapr_gmm_vocab_diag`` scores every utterance under every word model (Viterbi or forward mode, by ``scoring``), one
``sapr_gmm_viterbi_diag`` over the utterances grouped by their best word walks the winner's path.

Under ``implementation="hmmlearn"`` a vocabulary in which ANY model has ``covariance_type`` "full" or "tied" runs the
same way on the full-covariance kernels: ``sapr_full_vocab`` scores, ``sapr_full_viterbi`` under the winner walks
the path, ``sapr_full_estep`` gives the state posteriors.  "diag" and "spherical" members of such a vocabulary are
packed as diagonal matrices; a vocabulary of only "diag" / "spherical" models keeps the single-Gaussian kernels.
"""
from __future__ import annotations

import logging
import pickle
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np

from . import _lib
from .mfcc_extract import load_mfccs_by_word


class DecoderSession:
    """What ``Decoder.open_connected`` returns: a ``sapr_amd.ConnectedSession`` that speaks the decoder's language —
    (D, t) feature chunks in, word names out."""

    def __init__(self, session, words: List[str]):
        self.session, self.words = session, words

    def push(self, chunks, hypothesis: bool = False) -> List[Dict]:
        """One (D, t) feature array per stream (``None``: no new frames; more than ``max_chunk`` frames is a
        ``ValueError`` that names the stream).  Per stream ``{"segments": the newly complete (word, start,
        end_exclusive) in frames of the recording, "state_sequence": the newly final states, "first_frame",
        "frames", "stable_frames", "forced"}`` and, with ``hypothesis=True``, ``"hypothesis"``: the words of the best
        string over the frames that are not final yet."""
        ups = self.session.push(feats=[None if c is None else np.asarray(c).T for c in chunks],
                                hypothesis=hypothesis)
        out = []
        for up in ups:
            row = {"segments": [(self.words[w], a, b) for w, a, b in up.segments],
                   "state_sequence": up.path_state.astype(np.int64), "first_frame": up.first_frame,
                   "frames": up.frames, "stable_frames": up.stable_frames, "forced": up.forced}
            if hypothesis:
                row["hypothesis"] = [self.words[w] for w in up.hypothesis]
            out.append(row)
        return out

    def finish(self, streams=None) -> List[Dict]:
        """End the recordings of ``streams`` (all by default): per stream the dict of ``Decoder.decode_connected`` for
        the whole recording plus ``"forced"``; the streams are fresh again."""
        out = []
        for res in self.session.finish(streams):
            segs = res.segments()
            out.append({"words": [self.words[w] for w, _, _ in segs], "log_likelihood": res.score,
                        "segments": [(self.words[w], a, b) for w, a, b in segs],
                        "state_sequence": res.path_state.astype(np.int64), "forced": res.forced})
        return out


class Decoder:
    def __init__(self, models_dir: str = "trained_models", implementation: str = "hmmlearn", n_iter: int = 15,
                 scoring: str = "viterbi"):
        """``scoring="viterbi"`` (default): decoder.py:35-49 — the word whose best state path scores highest, that
        score, that path.  ``scoring="forward"``: the word with the highest forward log-likelihood (first strict maximum
        in load order), that log-likelihood, and the Viterbi path of that word; the path costs one all-vocabulary exact
        Viterbi pass (scores + back-pointers for every word, back-trace of the chosen one) on top of the forward launch,
        not the pruned decoder's pass over the surviving words (``implementation="gmmhmm"``: one Viterbi launch under
        the chosen word only, whatever the scoring).

        A vocabulary with a "full" or "tied" ``GaussianHMM`` (``implementation="hmmlearn"``) is served like the
        mixtures: one ``sapr_full_vocab`` launch picks the word, one ``sapr_full_viterbi`` under that word walks its
        path.  Viterbi ties go to the first maximum there, as in hmmlearn's own ``_hmmc`` code: the models'
        ``tie_break`` does not apply on this path."""
        if scoring not in ("viterbi", "forward"):
            raise ValueError(f"scoring must be 'viterbi' or 'forward', got {scoring!r}")
        if scoring == "forward" and implementation == "custom":
            raise ValueError("scoring='forward' needs implementation='hmmlearn': the from-scratch model has no forward "
                             "scorer over a vocabulary")
        self.models_dir = Path(models_dir)
        self.implementation = implementation
        self.scoring = scoring
        self.n_iter = n_iter
        self.models: Dict = {}
        self.vocab: List[str] = []
        self._pack = None
        self._vocab = None
        self.load_models()

    def load_models(self) -> None:
        impl_dir = self.models_dir / self.implementation
        pattern = f"*_{self.implementation}_{self.n_iter}.pkl"
        for model_path in impl_dir.glob(pattern):  # vocabulary order = glob order, like the reference
            word = model_path.stem.split("_")[0]
            with open(model_path, "rb") as f:
                self.models[word] = pickle.load(f)
                self.vocab.append(word)
        if not self.models:
            raise ValueError(f"No models found in {impl_dir} with pattern {pattern}")
        logging.info(f"Loaded {len(self.models)} models from {impl_dir} for words: {', '.join(self.vocab)}")

    # ---- batched core -------------------------------------------------------------------------
    def _model_list(self):
        return [self.models[w] for w in self.models]  # dict order = load order (decoder.py:42)

    def decode_batch(self, feature_list: List[np.ndarray]) -> List[Tuple[str, float, object]]:
        """``feature_list``: (D, T) arrays as stored by mfcc_extract (the ``feat_seq`` of
        decoder.py:58).  Returns one ``(word, score, states)`` per utterance with decode_sequence's
        semantics: first strict maximum over the models in load order."""
        words = list(self.models)
        if self.implementation == "custom":
            return self._decode_custom(feature_list)
        if self._uses_vocab_pack():
            return self._decode_vocab(*self._gmm_features(feature_list))
        from .trellis import FeatureBatch
        return self._decode_feature_batch(FeatureBatch.from_arrays(feature_list, layout="DT"))

    def decode_store(self, store) -> List[Tuple[str, float, object]]:
        """Every utterance of a packed ``store.FeatureStore`` (one host→HBM copy, one launch
        sequence); same tuples as ``decode_batch``."""
        if self.implementation == "custom":
            return self._decode_custom(store.to_batch())
        if self._uses_vocab_pack():
            from .tile_family import vocab_features
            feats, _, _, lengths, _ = vocab_features(store.to_batch())
            return self._decode_vocab(feats, lengths)
        return self._decode_feature_batch(store.to_batch())

    # ---- connected words ------------------------------------------------------------------------
    def decode_connected(self, feature_list: List[np.ndarray], word_penalty: float = 0.0,
                         exit_states="last", bigram=None, confidence=False, n_words=None, max_words=None,
                         nbest=False, alternatives=None, lattice=None, acoustic_scale: float = 1.0) -> List[Dict]:
        """Recordings that hold several words in a row: one-pass Viterbi over the word loop (``sapr_amd.connected``:
        the emission stage of the vocabulary's family, then ``sapr_connected_viterbi``).  ``feature_list``: (D, T)
        arrays as in ``decode_batch``.  Per utterance ``{"words": [...], "log_likelihood": float, "segments": [(word,
        start, end_exclusive), ...], "state_sequence": ndarray}`` with the words in load order of the vocabulary; an
        utterance no word string can explain (or one without frames) has no words, ``-inf`` and states of -1.
        ``word_penalty`` is added once per word boundary; ``exit_states``: "last", "any" or an array [W, S]
        (``ConnectedNetwork.from_models``).

        ``bigram``: a word-pair language model or grammar — a ``sapr_amd.WordBigram`` over the vocabulary in load order,
        or a list of transcripts of word names, which ``WordBigram.from_transcripts`` turns into add-one smoothed
        log-probabilities (a word that is not in the vocabulary is refused with a ``ValueError`` that names it, as
        ``align`` does).  The search then runs ``sapr_connected_bigram`` over ``bigram.scaled(1.0, word_penalty)``: the
        step from word v to word w costs ``lm[v, w] + word_penalty``, and ``-inf`` forbids it.

        ``confidence=True``: forward-backward over the same word loop under the same language model, on the same
        emission (``sapr_connected_posteriors``).  Each dict gains ``"confidence"`` — one float per segment, the mean
        posterior of the segment's word over its frames —, ``"total_log_likelihood"`` — the log-likelihood of the
        recording over every word string the language model allows — and ``"log_posterior"`` =
        ``log_likelihood - total_log_likelihood``, the log posterior of the decoded path among all paths.

        ``confidence="lattice"``: the confidences come from the word lattice instead — the lattice recursion over the
        same emission (``sapr_connected_lattice``), then forward-backward over its records under the search's own
        tables with the acoustic scores multiplied by ``acoustic_scale`` (``sapr_connected_lattice_posteriors``,
        ``sapr_amd.LatticePosteriors``); ``sapr_connected_posteriors`` is not launched.  Each dict gains
        ``"confidence"`` — one float per segment —, ``"lattice_log_likelihood"`` — the log-sum over every path of the
        lattice — and ``"slots"``, per segment the list of ``(word, posterior)`` of the words that compete for its
        frames, best first (``LatticePosteriors.slots``).  It is a different quantity from ``confidence=True``: Viterbi
        within words and the recorded boundaries only.  ``lattice=`` may be combined with it: one lattice recursion
        serves both.  Any other string, or an ``acoustic_scale`` that is not a finite number above 0, is a
        ``ValueError``.

        ``n_words`` (an int, or one per recording): the number of words is known; ``max_words``: it is at most this (up
        to 8).  The search then runs level building (``sapr_connected_levels``): one pass that returns the best string
        of exactly k words for every k up to the bound, under the same language model.  Each dict gains
        ``"level_log_likelihoods"``, one float per count 1 .. ``max_words`` (``-inf`` where no string of that many
        words explains the recording).  ``nbest=True`` (with ``max_words=8`` unless a bound is given): each dict gains
        ``"strings"``, a list of ``{"words", "log_likelihood", "segments"}``, one per count with a finite score, best
        first; its first entry is the result itself unless ``n_words`` asked for another count.

        ``alternatives`` (an int 1 .. 8): that many of the best DISTINCT word strings of each recording, whatever their
        word counts, from one more recursion over the same emission (``sapr_connected_nbest``).  Each dict gains
        ``"alternatives"``, a list of ``{"words", "log_likelihood", "segments"}`` best first — the segments come from
        a forced alignment of each string —, and ``"alternatives_complete"``: False where a string grew past what a
        64-bit code holds (``sapr_amd.nbest_capacity``) and the list may miss strings.  A value outside 1 .. 8 is a
        ``ValueError``.

        ``lattice`` (``True`` or a beam >= 0 in log score): the word lattice over the same emission under the same
        language model (``sapr_connected_lattice``, ``sapr_amd.WordLattice``).  Each dict gains ``"lattice"``, a list
        of ``(word, start, end_exclusive, acoustic, margin)`` sorted by end and then by word: the records whose best
        complete path scores within the beam of the best path (``True``: every record on a complete path).  A
        negative beam is a ``ValueError``.  With ``lattice=None`` the call makes exactly the launches it makes
        without the argument.

        Served for ``implementation="hmmlearn"`` — "diag" / "spherical" vocabularies through
        ``sapr_connected_emit_diag``, a vocabulary with a "full" or "tied" model through ``sapr_connected_emit_full``
        over the decoder's ``FullPack`` — and for ``implementation="gmmhmm"`` through ``sapr_connected_emit_gmm`` over
        its ``GmmPack``.  A loaded object that is not a fitted model of the implementation's class is refused with a
        ``ValueError`` that names its word."""
        if self.implementation not in ("hmmlearn", "gmmhmm"):
            raise ValueError(f"connected-word decoding needs implementation='hmmlearn' with 'diag' or 'spherical' "
                             f"models: it has no emission stage for implementation={self.implementation!r}")
        from .connected import _check_acoustic_scale, _check_beam, connected_decode
        if isinstance(confidence, str) and confidence != "lattice":  # (refused before a device is asked for)
            raise ValueError(f"confidence must be True, False or 'lattice', got {confidence!r}")
        by_lattice = isinstance(confidence, str)
        acoustic_scale = _check_acoustic_scale(acoustic_scale)
        if lattice is None or lattice is False:
            beam = None
        else:
            beam = float("inf") if lattice is True else _check_beam(lattice)  # (refused before a device is asked for)
        if len(feature_list) == 0:
            raise ValueError("empty utterance list")
        words = list(self.models)
        if bigram is None:
            net = self._connected_network(exit_states, word_penalty)
        else:
            net = self._connected_network(exit_states, 0.0, self._word_bigram(bigram).scaled(1.0, word_penalty))
        if nbest and n_words is None and max_words is None:
            from .connected import MAX_LEVELS as max_words
        res = connected_decode([np.asarray(f).T for f in feature_list], net,
                               posteriors=bool(confidence) and not by_lattice, n_words=n_words, max_words=max_words,
                               n_best=alternatives, lattice=beam is not None or by_lattice)
        out = []
        for u in range(len(feature_list)):
            segs = res.segments(u)
            lo, hi = int(res.offsets[u]), int(res.offsets[u + 1])
            out.append({"words": [words[w] for w, _, _ in segs], "log_likelihood": float(res.score[u]),
                        "segments": [(words[w], a, b) for w, a, b in segs],
                        "state_sequence": res.path_state[lo:hi].astype(np.int64)})
        if res.level_score is not None:
            for u, row in enumerate(out):
                row["level_log_likelihoods"] = [float(v) for v in res.level_score[u]]
                if nbest:
                    row["strings"] = [{"words": [words[w] for w in ws], "log_likelihood": sc,
                                       "segments": [(words[w], a, b) for w, a, b in segs]}
                                      for _, sc, ws, segs in res.levels.strings(u)]
        if res.nbest is not None:
            nb = res.nbest
            for row in out:
                row["alternatives"] = []
            for r in range(int(nb.n_found.max()) if nb.n_found.size else 0):
                al = nb.align(r)
                for k, u in enumerate(al.utterances):
                    out[u]["alternatives"].append({"words": [words[w] for w in nb.words(u, r)],
                                                   "log_likelihood": float(nb.score[u, r]),
                                                   "segments": [(words[w], a, b) for w, a, b in al.segments(k)]})
            for u, row in enumerate(out):
                row["alternatives_complete"] = not bool(nb.overflow[u])
        if beam is not None:
            for u, row in enumerate(out):
                row["lattice"] = [(words[w], a, b, ac, m) for w, a, b, ac, m in res.lattice.records(u, beam)]
        if by_lattice:
            lp = res.lattice.posteriors(None, acoustic_scale)
            for u, row in enumerate(out):
                row["confidence"] = lp.segment_confidence(res, u)
                row["lattice_log_likelihood"] = float(lp.loglik[u])
                row["slots"] = [[(words[w], p) for w, p in slot] for slot in lp.slots(res, u)]
        elif confidence:
            log_post = res.posteriors.path_log_posterior(res)
            for u, row in enumerate(out):
                row["confidence"] = res.posteriors.segment_confidence(res, u)
                row["total_log_likelihood"] = float(res.posteriors.loglik[u])
                row["log_posterior"] = float(log_post[u])
        return out

    def open_connected(self, n_streams: int, bigram=None, word_penalty: float = 0.0, exit_states="last",
                       window: int = 256, max_chunk: int = 64) -> "DecoderSession":
        """Online ``decode_connected``: ``n_streams`` recordings that are still arriving, decoded chunk by chunk over
        the word loop under the same ``bigram`` / ``word_penalty`` / ``exit_states`` (``sapr_amd.ConnectedSession``:
        the vocabulary's emission stage on each chunk, ``sapr_connected_online_step``, then
        ``sapr_connected_online_commit``).  The returned :class:`DecoderSession` takes (D, t) feature chunks of at
        most ``max_chunk`` frames; the device keeps ``window`` frames of back-pointers per stream.  Its ``finish``
        returns the dicts of ``decode_connected`` — bit for bit where ``"forced"`` is 0.  The features are the
        caller's: an MFCC front end that needs context across a chunk edge (deltas) must supply it itself.

        Served for the implementations and families ``decode_connected`` serves."""
        if self.implementation not in ("hmmlearn", "gmmhmm"):
            raise ValueError(f"connected-word decoding needs implementation='hmmlearn' with 'diag' or 'spherical' "
                             f"models: it has no emission stage for implementation={self.implementation!r}")
        from .connected import ConnectedSession
        if bigram is None:
            net = self._connected_network(exit_states, word_penalty)
        else:
            net = self._connected_network(exit_states, 0.0, self._word_bigram(bigram).scaled(1.0, word_penalty))
        return DecoderSession(ConnectedSession(net, n_streams, window, max_chunk), list(self.models))

    def _word_bigram(self, bigram):
        """``decode_connected``'s ``bigram`` as a ``WordBigram`` over the vocabulary in load order."""
        from .connected import WordBigram
        words = list(self.models)
        if isinstance(bigram, WordBigram):
            if bigram.W != len(words):
                raise ValueError(f"the bigram is over {bigram.W} words, the vocabulary has {len(words)} "
                                 f"({', '.join(words)})")
            return bigram
        index = {w: i for i, w in enumerate(words)}
        rows = []
        for u, names in enumerate(bigram):
            if isinstance(names, str):
                raise ValueError(f"transcript {u} of the bigram is a string; a transcript is a list of word names")
            for name in names:
                if name not in index:
                    raise ValueError(f"transcript {u} of the bigram names {name!r}, which is not in the vocabulary "
                                     f"({', '.join(words)})")
            rows.append([index[name] for name in names])
        return WordBigram.from_transcripts(rows, len(words))

    def _connected_network(self, exit_states, word_penalty, bigram=None):
        """The vocabulary as a ``ConnectedNetwork`` of its emission family, over the decoder's own pack."""
        from .connected import ConnectedNetwork, vocabulary_family
        words = list(self.models)
        # (validated before the pack is built: packing reads the fitted attributes)
        family = vocabulary_family(self._model_list(), words, self.implementation)
        return ConnectedNetwork.from_models(self._model_list(), exit_states=exit_states, word_penalty=word_penalty,
                                            names=words, implementation=self.implementation,
                                            pack=None if family == "diag" else self._vocab_pack(), bigram=bigram)

    def _silence_index(self, optional_silence):
        """The vocabulary index of the word that may stand, unwritten, around the words of a transcript."""
        words = list(self.models)
        if optional_silence not in words:
            raise ValueError(f"optional_silence names {optional_silence!r}, which is not in the vocabulary "
                             f"({', '.join(words)})")
        return words.index(optional_silence)

    def _transcript_rows(self, transcripts, optional_silence=None):
        """Transcripts of word names -> ``(rows, flags, said)``: ``said`` is one row of vocabulary indices per
        transcript, and without ``optional_silence`` ``rows`` is ``said`` and ``flags`` ``None``; with it they are
        ``connected.with_optional(said, that word's index)``."""
        words = list(self.models)
        index = {w: i for i, w in enumerate(words)}
        said = []
        for u, names in enumerate(transcripts):
            for name in names:
                if name not in index:
                    raise ValueError(f"the transcript of utterance {u} names {name!r}, which is not in the vocabulary "
                                     f"({', '.join(words)})")
            said.append([index[name] for name in names])
        if optional_silence is None:
            return said, None, said
        from .connected import with_optional
        return (*with_optional(said, self._silence_index(optional_silence)), said)

    def align(self, feature_list: List[np.ndarray], transcripts, word_penalty: float = 0.0,
              exit_states="last", optional_silence=None) -> List[Dict]:
        """Forced alignment: the words of every recording are known (``transcripts``: one list of word names per
        utterance, in spoken order; a word may follow itself), where does each begin and end.  Viterbi over the chain
        of the transcript's word models (``sapr_amd.connected.connected_align``: the emission stage of the vocabulary's
        family, then ``sapr_connected_align``).  ``feature_list``: (D, T) arrays as in ``decode_connected``.  Per
        utterance ``{"words": [...], "log_likelihood": float, "segments": [(word, start, end_exclusive), ...],
        "state_sequence": ndarray}`` with one segment per transcript word; an utterance its transcript cannot explain
        (too few frames, no path) has no words, no segments, ``-inf`` and states of -1.

        ``optional_silence``: the name of a vocabulary word that may have been spoken, unwritten, before, between and
        after the transcript's words (``sil? w1 sil? ... wK sil?``, ``connected.with_optional``; the path walks through
        each of these slots or steps over it, and ``word_penalty`` is paid for the ones it walks through).  ``words``
        is then still the caller's transcript, and ``segments`` gets one more entry under that word's name for every
        pause the path took.

        Served for the implementations and families ``decode_connected`` serves.  A word that is not in the
        vocabulary is refused with a ``ValueError`` that names it."""
        if self.implementation not in ("hmmlearn", "gmmhmm"):
            raise ValueError(f"forced alignment needs implementation='hmmlearn' or 'gmmhmm': it has no emission stage "
                             f"for implementation={self.implementation!r}")
        from .connected import connected_align
        if len(feature_list) == 0:
            raise ValueError("empty utterance list")
        words = list(self.models)
        rows, flags, said = self._transcript_rows(transcripts, optional_silence)
        net = self._connected_network(exit_states, word_penalty)
        res = connected_align([np.asarray(f).T for f in feature_list], rows, net, flags)
        out = []
        for u in range(len(feature_list)):
            segs = res.segments(u)
            lo, hi = int(res.offsets[u]), int(res.offsets[u + 1])
            spoken = [words[w] for w, _, _ in segs] if flags is None else [words[w] for w in said[u]] if segs else []
            out.append({"words": spoken, "log_likelihood": float(res.score[u]),
                        "segments": [(words[w], a, b) for w, a, b in segs],
                        "state_sequence": res.path_state[lo:hi].astype(np.int64)})
        return out

    def train_embedded(self, feature_list: List[np.ndarray], transcripts, n_iter: int = 10, tol: float = 1e-2,
                       word_penalty: float = 0.0, exit_states="last", optional_silence=None) -> List[float]:
        """Embedded Baum-Welch over recordings of several words: the loaded word models are re-estimated IN PLACE from
        ``feature_list`` ((D, T) arrays as in ``align``) and ``transcripts`` (one list of word names per utterance, in
        spoken order), without cutting the recordings at word boundaries (``sapr_amd.connected.embedded_fit``:
        forward-backward over the chain of each transcript's word models, ``sapr_connected_embed``).  Returns the
        history of the summed log-likelihood, one entry per iteration.  A word that is in no transcript keeps its
        parameters.  ``optional_silence``: as in ``align`` — the named word's model is a skippable slot around every
        transcript word and is trained with them on the pauses the recordings hold.

        Served for ``implementation="hmmlearn"``: "diag" / "spherical" vocabularies through ``sapr_connected_embed``,
        a vocabulary that holds a "full" or "tied" model through ``sapr_connected_embed_full`` (second-moment
        matrices; ``embedded_fit(..., second_moments=True)``).  Served for ``implementation="gmmhmm"`` through
        ``sapr_connected_embed_gmm`` (mixture responsibilities over the chain posteriors, then
        ``gmm_hmm.gmm_m_step`` per word).  Another implementation is refused with a ``ValueError`` that says why.  A
        word that is not in the vocabulary is refused with a ``ValueError`` that names it."""
        if self.implementation not in ("hmmlearn", "gmmhmm"):
            raise ValueError(f"embedded training needs implementation='hmmlearn' (GaussianHMM word models) or "
                             f"'gmmhmm' (GMMHMM word models): the embedded E-step accumulates Gaussian and "
                             f"Gaussian-mixture statistics, not those of implementation={self.implementation!r}")
        from .connected import embedded_fit
        if len(feature_list) == 0:
            raise ValueError("empty utterance list")
        words = list(self.models)
        rows, flags, _ = self._transcript_rows(transcripts, optional_silence)
        history = embedded_fit(self._model_list(), [np.asarray(f).T for f in feature_list], rows, n_iter=n_iter,
                               tol=tol, exit_states=exit_states, word_penalty=word_penalty, names=words,
                               second_moments=self._is_full(), optional=flags)
        self._pack = self._vocab = None  # (packed from the old parameters)
        return history

    def train_discriminative(self, feature_list: List[np.ndarray], transcripts, bigram=None, n_iter: int = 4,
                             E: float = 2.0, tau: float = 0.0, acoustic_scale: float = 1.0,
                             word_penalty: float = 0.0, exit_states="last") -> List[float]:
        """Discriminative (maximum mutual information) training over recordings of several words: the means and
        variances of the loaded word models are re-estimated IN PLACE so that each recording's transcript gains
        probability against every other word string the word loop allows (``sapr_amd.connected.mmi_fit``: the
        numerator from ``sapr_connected_embed`` over the transcript's chain, the denominator from
        ``sapr_connected_posteriors`` over the word loop reduced by ``sapr_connected_loop_stats``, then the extended
        Baum-Welch update with the constant ``E`` and the I-smoothing weight ``tau``).  ``feature_list`` and
        ``transcripts`` (word names) are as in ``train_embedded``; ``bigram`` as in ``decode_connected``.  Returns the
        history of the objective, the summed log posterior of the transcripts, one entry per iteration (evaluated
        before the iteration's update).  Start and transition probabilities stay as they are; a word that is in no
        transcript keeps its parameters.

        Served for ``implementation="hmmlearn"`` with "diag" / "spherical" models.  A ``GMMHMM`` vocabulary
        (``implementation="gmmhmm"``) and one that holds a "full" or "tied" model are a ``NotImplementedError`` that
        names the family; a transcript the grammar forbids is a ``ValueError`` that names the utterance, a word that
        is not in the vocabulary one that names the word."""
        if self.implementation == "gmmhmm":
            raise NotImplementedError("MMI training is served for 'diag' and 'spherical' GaussianHMM word models; the "
                                      "'gmm' family (implementation='gmmhmm') needs a denominator kernel of its own")
        if self.implementation != "hmmlearn":
            raise ValueError(f"discriminative training needs implementation='hmmlearn' (GaussianHMM word models): the "
                             f"MMI E-step accumulates Gaussian statistics, not those of "
                             f"implementation={self.implementation!r}")
        from .connected import mmi_fit
        if len(feature_list) == 0:
            raise ValueError("empty utterance list")
        words = list(self.models)
        rows, _, _ = self._transcript_rows(transcripts)
        history = mmi_fit(self._model_list(), [np.asarray(f).T for f in feature_list], rows,
                          bigram=None if bigram is None else self._word_bigram(bigram), n_iter=n_iter, E=E, tau=tau,
                          acoustic_scale=acoustic_scale, exit_states=exit_states, word_penalty=word_penalty,
                          names=words)
        self._pack = self._vocab = None  # (packed from the old parameters)
        return history

    def _decode_custom(self, features) -> List[Tuple[str, float, object]]:
        """The reference's from-scratch models: emission rows, trellis and the arg-max over the models
        (decoder.py:42-47, first strict maximum in load order) all on the device."""
        from .custom_hmm import decode_batch
        words = list(self.models)
        _, _, bw, bs, bp = decode_batch(self._model_list(), features, with_best=True)
        return [(words[w], float(sc), [int(x) for x in p]) if w >= 0 else (None, float("-inf"), None)
                for w, sc, p in zip(bw, bs, bp)]

    # ---- Gaussian-mixture and full-covariance word models --------------------------------------
    def _is_full(self) -> bool:
        """A vocabulary of hmmlearn-shaped models of which at least one has a "full" or "tied" covariance: all of it
        runs on the full-covariance kernels (``DiagModelPack`` refuses such models)."""
        return self.implementation == "hmmlearn" and any(
            getattr(m, "covariance_type", "diag") in ("full", "tied") for m in self.models.values())

    def _uses_vocab_pack(self) -> bool:
        return self.implementation == "gmmhmm" or self._is_full()

    def _vocab_pack(self):
        """The vocabulary's operand block (``gmm_hmm.GmmPack`` for the mixtures, ``full_cov.FullPack`` for a
        full-covariance vocabulary), padded to its largest model; built once.  The pack names what is the family's
        own: the per-model batch class (``pack.batch``) and the scorer over the vocabulary (``pack.vocab_scores``)."""
        if self._vocab is None:
            if self.implementation == "gmmhmm":
                from .gmm_hmm import GmmPack as Pack
            else:
                from .full_cov import FullPack as Pack
            self._vocab = Pack.from_models(self._model_list())
        return self._vocab

    @staticmethod
    def _gmm_features(feature_list):
        """(D, T) arrays -> ``(device feats [total_frames, D] float32, host lengths)``, rows of the models' own width."""
        import torch
        if len(feature_list) == 0:
            raise ValueError("empty utterance list")
        mats = [np.ascontiguousarray(np.asarray(f).T, dtype=np.float32) for f in feature_list]
        D = mats[0].shape[1]
        if any(m.ndim != 2 or m.shape[1] != D for m in mats):
            raise ValueError("all utterances must share the feature dimension")
        lengths = np.asarray([m.shape[0] for m in mats], dtype=np.int64)
        packed = np.concatenate(mats, axis=0) if lengths.sum() else np.zeros((0, D), np.float32)
        return torch.from_numpy(packed).to(_lib.require_gpu()), lengths

    def _decode_vocab(self, feats, lengths) -> List[Tuple[str, float, object]]:
        """One launch over the vocabulary (``sapr_gmm_vocab_diag`` / ``sapr_full_vocab``: Viterbi log-probabilities, or
        forward log-likelihoods with ``scoring="forward"``) picks the word; one Viterbi launch
        (``sapr_gmm_viterbi_diag`` / ``sapr_full_viterbi``) over the utterances grouped by that word walks its path
        (first maximum on ties).  The returned score is the vocabulary launch's (in Viterbi mode the second launch's
        ``logprob`` carries the same bits)."""
        words = list(self.models)
        pack = self._vocab_pack()
        vs = pack.vocab_scores(feats, lengths, mode=self.scoring)
        bw = _lib.to_host(vs.best_word)[0].astype(np.int64)
        # an utterance no model scores above -inf has no word (-1): model 0's path is walked and then dropped
        _, path = pack.batch(feats, lengths, np.maximum(bw, 0)).viterbi(pack)
        score, path = _lib.to_host(vs.score, path)
        offs = np.r_[0, np.cumsum(lengths)].tolist()
        path = path.astype(np.int64)
        return [(words[w], float(score[u, w]), path[lo:hi]) if w >= 0 else (None, float("-inf"), None)
                for u, (w, lo, hi) in enumerate(zip(bw.tolist(), offs[:-1], offs[1:]))]

    def _state_posteriors_vocab(self, feature_list, words) -> List[np.ndarray]:
        pack = self._vocab_pack()
        feats, lengths = self._gmm_features(feature_list)
        if words is None:
            vs = pack.vocab_scores(feats, lengths, mode="viterbi")
            utt_model = np.maximum(_lib.to_host(vs.best_word)[0].astype(np.int64), 0)
        else:
            utt_model = self._named_models(words, len(lengths))
        batch = pack.batch(feats, lengths, utt_model)
        post = _lib.to_host(batch.estep(pack, want_stats=False, want_post=True)[2])[0].copy()
        offs = np.r_[0, np.cumsum(lengths)].tolist()
        return [post[lo:hi, :pack.n_states[w]] for w, lo, hi in zip(utt_model.tolist(), offs[:-1], offs[1:])]

    def _named_models(self, words, n_utts) -> np.ndarray:
        """Model index per utterance for the words named by the caller."""
        vocab = list(self.models)
        if len(words) != n_utts:
            raise ValueError("one word per utterance")
        unknown = sorted({w for w in words if w not in self.models})
        if unknown:
            raise ValueError(f"words not in vocabulary {vocab}: {unknown}")
        return np.asarray([vocab.index(w) for w in words], dtype=np.int64)

    def _decode_feature_batch(self, batch) -> List[Tuple[str, float, object]]:
        from .trellis import DiagModelPack, viterbi_decode_best
        words = list(self.models)
        if self._pack is None:
            self._pack = DiagModelPack.from_models(self._model_list())
        tie = _lib.TIE_HIGH if getattr(self._model_list()[0], "tie_break", "high") == "high" else _lib.TIE_LOW
        if self.scoring == "forward":
            return self._decode_forward(batch, tie)
        # decoder.py:59 hands hmmlearn the transposed VIEW of the (D,T) array → numpy's left-to-right sum.
        # Pruned decoder when the pack is prunable, all-vocabulary evaluation otherwise: identical outputs.
        best_word, best_score, best_path = viterbi_decode_best(batch, self._pack, tie=tie, sum_order=_lib.SUM_TVIEW)
        bw, bs, path = _lib.to_host(best_word, best_score, best_path)
        offs = np.r_[0, np.cumsum(batch.lengths)].tolist()
        path = path.astype(np.int64)  # one conversion for the batch; the per-utterance results are views of it
        bw_l, bs_l = bw.tolist(), bs.tolist()
        return [(words[w], sc, path[lo:hi]) if w >= 0 else (None, float("-inf"), None)
                for w, sc, lo, hi in zip(bw_l, bs_l, offs[:-1], offs[1:])]

    def _decode_forward(self, batch, tie) -> List[Tuple[str, float, object]]:
        """Forward arg-max word, its forward log-likelihood, and the Viterbi path of that word."""
        from .trellis import forward_scores, viterbi_decode
        words = list(self.models)
        fs = forward_scores(batch, self._pack, want_post=False)
        # an utterance no model scores above -inf has no word (-1): model 0's path is walked and then dropped
        vit = viterbi_decode(batch, self._pack, tie=tie, sum_order=_lib.SUM_TVIEW,
                             word_sel=fs.best_word.clamp(min=0))
        ll, bw, path = _lib.to_host(fs.loglik, fs.best_word, vit.path)
        offs = np.r_[0, np.cumsum(batch.lengths)].tolist()
        path = path.astype(np.int64)
        return [(words[w], float(ll[u, w]), path[lo:hi]) if w >= 0 else (None, float("-inf"), None)
                for u, (w, lo, hi) in enumerate(zip(bw.tolist(), offs[:-1], offs[1:]))]

    # ---- forward scoring over the vocabulary --------------------------------------------------
    def _forward_scores(self, feature_list, want_post):
        if self.implementation == "custom":
            raise ValueError("forward scoring over the vocabulary needs implementation='hmmlearn': the from-scratch "
                             "model has no forward scorer over a vocabulary")
        if self._uses_vocab_pack():
            from .trellis import ForwardScores
            vs = self._vocab_pack().vocab_scores(*self._gmm_features(feature_list), mode="forward",
                                                 want_post=want_post)
            return ForwardScores(vs.score, vs.best_word, vs.word_post)
        from .trellis import DiagModelPack, FeatureBatch, forward_scores
        if self._pack is None:
            self._pack = DiagModelPack.from_models(self._model_list())
        return forward_scores(FeatureBatch.from_arrays(feature_list, layout="DT"), self._pack, want_post=want_post)

    def score_batch(self, feature_list: List[np.ndarray]) -> np.ndarray:
        """Forward log-likelihood (``GaussianHMM.score``) of every utterance of ``feature_list`` ((D, T) arrays as
        in ``decode_batch``) under every word model: float64 [N, W], columns in ``self.vocab`` order."""
        return _lib.to_host(self._forward_scores(feature_list, False).loglik)[0].copy()  # (out of the pinned buffer)

    @staticmethod
    def _nbest_rows(loglik: np.ndarray, word_post: np.ndarray, vocab: List[str],
                    n: int) -> List[List[Tuple[str, float, float]]]:
        """Host ordering of a score matrix [N, W] (columns in ``vocab`` order): per utterance the ``n`` best
        ``(word, log_likelihood, posterior)``, best first; equal scores stay in load order, NaN scores sort last."""
        loglik = np.asarray(loglik, dtype=np.float64)
        word_post = np.asarray(word_post, dtype=np.float64)
        W = loglik.shape[1]
        n = max(0, min(int(n), W))
        nan = np.isnan(loglik)
        with np.errstate(invalid="ignore"):
            key = np.where(nan, 0.0, -loglik)
        idx = np.lexsort((key, nan), axis=-1)[:, :n]  # stable: by NaN-ness, then descending score, then column
        return [[(vocab[w], float(loglik[u, w]), float(word_post[u, w])) for w in row] for u, row in enumerate(idx)]

    def nbest(self, feature_list: List[np.ndarray], n: int = 3) -> List[List[Tuple[str, float, float]]]:
        """The ``n`` most likely words of every utterance by forward log-likelihood: lists of ``(word,
        log_likelihood, posterior)``, best first, the posterior over the vocabulary under a uniform prior.  ``n`` is
        clipped to the vocabulary size.  The device returns the [N, W] matrices; the ordering is host work."""
        fs = self._forward_scores(feature_list, True)
        ll, post = _lib.to_host(fs.loglik, fs.word_post)
        return self._nbest_rows(ll, post, list(self.models), n)

    # ---- state posteriors ---------------------------------------------------------------------
    def state_posteriors(self, feature_list: List[np.ndarray], words: List[str] = None) -> List[np.ndarray]:
        """Per utterance of ``feature_list`` ((D, T) arrays as in ``score_batch``) the ``(T, S)`` float64 lattice of
        state posteriors P(q_t = s | x_1..T) under one word model: the word the decoder picks (``words=None``: the
        pruned decoder's best word; an utterance without a word gets the first model) or the one named in ``words``.
        One launch sequence for the whole batch, utterances grouped into tiles by word."""
        if self.implementation == "custom":
            raise ValueError("state posteriors need implementation='hmmlearn': the from-scratch model has no posterior "
                             "kernel")
        if self._uses_vocab_pack():
            return self._state_posteriors_vocab(feature_list, words)
        from .trellis import DiagModelPack, FeatureBatch, state_posteriors, viterbi_decode_best
        if self._pack is None:
            self._pack = DiagModelPack.from_models(self._model_list())
        batch = FeatureBatch.from_arrays(feature_list, layout="DT")
        if words is None:
            tie = _lib.TIE_HIGH if getattr(self._model_list()[0], "tie_break", "high") == "high" else _lib.TIE_LOW
            best_word, _, _ = viterbi_decode_best(batch, self._pack, tie=tie, sum_order=_lib.SUM_TVIEW)
            utt_model = np.maximum(_lib.to_host(best_word)[0].astype(np.int64), 0)
        else:
            utt_model = self._named_models(words, batch.n_utts)
        res = state_posteriors(batch, self._pack, utt_model, want_path=False)
        post = _lib.to_host(res.post)[0].copy()  # (out of the pinned buffer)
        offs = np.r_[0, np.cumsum(batch.lengths)].tolist()
        return [post[lo:hi] for lo, hi in zip(offs[:-1], offs[1:])]

    # ---- the reference's API ------------------------------------------------------------------
    def decode_sequence(self, features: np.ndarray) -> Tuple[str, float, List[int]]:
        """``features`` is the (T, D) view decoder.py:59 builds."""
        return self.decode_batch([np.asarray(features).T])[0]

    @staticmethod
    def _rows(word: str, decoded) -> List[Dict]:
        """Result dictionaries of one word's samples (schema of decoder.py:62-69)."""
        return [{"sample_index": i, "true_word": word, "predicted_word": pred, "log_likelihood": score,
                 "correct": pred == word, "state_sequence": states}
                for i, (pred, score, states) in enumerate(decoded, start=1)]

    def decode_word_samples(self, word: str, feature_set: str = "feature_set") -> List[Dict]:
        if word not in self.vocab:
            raise ValueError(f"Word '{word}' not in vocabulary: {self.vocab}")
        features = load_mfccs_by_word(feature_set, word)
        return self._rows(word, self.decode_batch(features) if features else [])

    def decode_vocabulary(self, feature_set: str = "feature_set", verbose: bool = True) -> Dict[str, List[Dict]]:
        """Every word's samples (decoder.py:74-93) — loaded word by word like the reference, decoded as ONE
        batch (one launch sequence for the whole vocabulary), reported word by word."""
        per_word = [load_mfccs_by_word(feature_set, word) for word in self.vocab]
        flat = [f for feats in per_word for f in feats]
        decoded = self.decode_batch(flat) if flat else []
        all_results, start = {}, 0
        for word, feats in zip(self.vocab, per_word):
            rows = self._rows(word, decoded[start:start + len(feats)])
            start += len(feats)
            all_results[word] = rows
            if verbose:
                hits = sum(1 for r in rows if r["correct"])
                print(f"\nResults for '{word}':")
                print(f"Accuracy: {hits}/{len(rows)} ({hits/len(rows):.1%})")
                for r in rows:
                    mark = "✓" if r["correct"] else "✗"
                    print(f"\nSample {r['sample_index']}:\nPredicted: {r['predicted_word']}\n"
                          f"Log likelihood: {r['log_likelihood']:.2f}\nCorrect: {mark}")
        return all_results


if __name__ == "__main__":
    decoder = Decoder(implementation="hmmlearn", n_iter=15)
    results = decoder.decode_vocabulary()
    all_predictions = [result["correct"] for word_results in results.values() for result in word_results]
    print(f"\nOverall accuracy: {sum(all_predictions) / len(all_predictions):.1%}")

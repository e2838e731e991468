"""sapr_amd — MI355X-native hot path of frankcholula/sapr assignment2.

Host-side mirror of the reference's module API (same names, arguments and error
behaviour) over hand-written HIP kernels in ``libsapr_hip.so``:

* ``sapr_amd.mfcc_extract``  ↔ assignment2/mfcc_extract.py
* ``sapr_amd.custom_hmm``    ↔ assignment2/custom_hmm.py
* ``sapr_amd.hmmlearn_hmm``  ↔ assignment2/hmmlearn_hmm.py (+ a GaussianHMM-shaped model object)
* ``sapr_amd.decoder``       ↔ assignment2/decoder.py
* ``sapr_amd.gmm_hmm``       hmmlearn's other Gaussian model class, ``GMMHMM`` (no counterpart in the reference)
* ``sapr_amd.full_cov``      the full-covariance kernels behind ``GaussianHMM(covariance_type="full" | "tied")`` and the
                             recogniser's scoring over a vocabulary of such models
* ``sapr_amd.connected``     connected-word recognition: one-pass Viterbi over the word loop (under a word bigram or a
                             word-pair grammar where one is given: ``WordBigram``; with a known or bounded number of
                             words by level building: ``connected_levels``; the N best distinct word strings
                             in one pass: ``connected_nbest``; a word lattice that is pruned to a beam and rescored
                             under another language model: ``connected_lattice``; recordings that are still
                             arriving, decoded chunk by chunk: ``ConnectedSession``), word and segment confidences
                             from forward-backward over the same loop (``connected_posteriors``), forced alignment of
                             a recording to its known word string, embedded Baum-Welch training from such
                             recordings, and discriminative (MMI) training of the word models against the word loop
                             (``mmi_fit``) (no counterpart in the reference, whose decoder labels a recording as one word)

``sapr_amd/compat`` holds same-named top-level shims so the reference's ``train.py`` /
``eval.py`` / tests import the drop-in unmodified.
"""
__version__ = "0.1.0"


def __getattr__(name):
    """``sapr_amd.GMMHMM`` / ``sapr_amd.fit_gmm_models`` / ``sapr_amd.vocab_scores`` / ``sapr_amd.full_vocab_scores``
    / ``sapr_amd.ConnectedNetwork`` / ``sapr_amd.WordBigram`` / ``sapr_amd.connected_viterbi`` /
    ``sapr_amd.connected_decode`` / ``sapr_amd.AlignResult`` / ``sapr_amd.align_viterbi`` / ``sapr_amd.connected_align`` /
    ``sapr_amd.EmbeddedStats`` / ``sapr_amd.embedded_forward_backward`` / ``sapr_amd.embedded_estep`` /
    ``sapr_amd.embedded_fit`` / ``sapr_amd.embed_full_stats_width`` / ``sapr_amd.embed_full_workspace_bytes`` /
    ``sapr_amd.embed_gmm_stats_width`` / ``sapr_amd.embed_gmm_workspace_bytes`` / ``sapr_amd.ConnectedPosteriors`` /
    ``sapr_amd.connected_posteriors`` / ``sapr_amd.posteriors_workspace_bytes`` / ``sapr_amd.LevelResult`` /
    ``sapr_amd.connected_levels`` / ``sapr_amd.levels_workspace_bytes`` / ``sapr_amd.with_optional`` /
    ``sapr_amd.align_opt_workspace_bytes`` / ``sapr_amd.loop_stats`` / ``sapr_amd.loop_stats_workspace_bytes`` /
    ``sapr_amd.MmiStats`` / ``sapr_amd.mmi_estep`` / ``sapr_amd.mmi_update`` / ``sapr_amd.mmi_fit`` /
    ``sapr_amd.NBestResult`` / ``sapr_amd.connected_nbest`` / ``sapr_amd.nbest_capacity`` / ``sapr_amd.WordLattice`` /
    ``sapr_amd.LatticePath`` / ``sapr_amd.LatticeBackward`` / ``sapr_amd.connected_lattice`` /
    ``sapr_amd.lattice_workspace_bytes`` / ``sapr_amd.LatticePosteriors`` /
    ``sapr_amd.lattice_posteriors_workspace_bytes`` / ``sapr_amd.ConnectedSession`` / ``sapr_amd.OnlineUpdate`` /
    ``sapr_amd.OnlineResult`` / ``sapr_amd.online_state_bytes``
    (resolved on first use: importing the package stays light)."""
    if name in ("GMMHMM", "fit_gmm_models", "vocab_scores"):
        from . import gmm_hmm
        return getattr(gmm_hmm, name)
    if name in ("ConnectedNetwork", "WordBigram", "ConnectedResult", "connected_viterbi", "connected_decode",
                "AlignResult", "align_viterbi", "connected_align", "EmbeddedStats", "embedded_forward_backward", "embedded_estep",
                "embedded_fit", "embed_full_stats_width", "embed_full_workspace_bytes", "embed_gmm_stats_width",
                "embed_gmm_workspace_bytes", "ConnectedPosteriors", "connected_posteriors",
                "posteriors_workspace_bytes", "LevelResult", "connected_levels", "levels_workspace_bytes",
                "with_optional", "align_opt_workspace_bytes", "loop_stats", "loop_stats_workspace_bytes", "MmiStats",
                "mmi_estep", "mmi_update", "mmi_fit", "NBestResult", "connected_nbest", "nbest_capacity", "WordLattice",
                "LatticePath", "LatticeBackward", "connected_lattice", "lattice_workspace_bytes", "LatticePosteriors",
                "lattice_posteriors_workspace_bytes", "ConnectedSession", "OnlineUpdate", "OnlineResult",
                "online_state_bytes"):
        from . import connected
        return getattr(connected, name)
    if name == "full_vocab_scores":
        from . import full_cov
        return full_cov.vocab_scores
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

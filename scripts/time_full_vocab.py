"""Ad-hoc timing of scoring over the vocabulary for the full-covariance HMMs (dev tool):
    python scripts/time_full_vocab.py [N] [--shapes 13,10 39,18] [--trace DIR]
sapr_full_vocab (one call: every utterance under every word model, + the arg-max epilogue) in FORWARD and in VITERBI
mode against the only other way to the same [N, W] matrix: W FullCovBatch objects over the same features, every
utterance assigned to word w, and W estep(want_stats=False) resp. viterbi calls (tile layouts, workspaces and the device
pack built beforehand, outside the timed region).  Workload: N x 101 frames, W = 11 word models, bidiagonal
transitions, full covariances with real off-diagonals (scripts/time_fullcov.py's), (D, S) = (13, 10) and (39, 18).
Every path is warmed twice, then the two routes are timed alternately, five times each, between device events; the two
matrices must be EQUAL (the kernels share their device functions).  Prints one JSON line per shape, with the workspace
bytes the one-call route does without and the float64 operations it needs from the shapes alone, per frame and word:
S D (D + 1) / 2 FMAs (2 flops) and as many subtractions for the triangles, 2 S D for the squares, ~45 (3 in VITERBI
mode) per finite transition.

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of every route per shape) and writes DIR/full_vocab_rocprofv3_summary.txt."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import summary, timed_rounds, trace_run, write_summary

F64_VECTOR_FLOPS = 78.6e12
T, W, REPEATS = 101, 11, 5


def setup(N, D, S):
    import torch
    from sapr_amd import full_cov
    from sapr_amd.trellis import FeatureBatch
    from tests._synth import trained_like_models
    torch.manual_seed(0)
    utt_word = np.arange(N) // ((N + W - 1) // W)
    sp, A, mu, cv = trained_like_models(W, S - 2, D, seed=3)
    # frames scattered about the state means of the utterance's own word, so that every state is visited
    seg = torch.arange(T, device="cuda").repeat(N) * S // T
    grp = torch.from_numpy(np.repeat(utt_word, T)).cuda()
    feats = (torch.from_numpy(mu).cuda()[grp, seg] + torch.randn(N * T, D, device="cuda", dtype=torch.float64) * 5)
    feats = feats.float().contiguous()
    del seg, grp
    lengths = np.full(N, T)
    # full covariances on the models' own variances: Sigma = diag(sd) R diag(sd), R a fixed correlation matrix
    rng = np.random.default_rng(0)
    B = rng.standard_normal((D, D))
    R = 0.7 * np.eye(D) + 0.3 * (B @ B.T) / D
    R /= np.sqrt(np.outer(np.diag(R), np.diag(R)))
    sd = np.sqrt(cv)
    full = sd[:, :, :, None] * R[None, None] * sd[:, :, None, :]
    full = (full + full.transpose(0, 1, 3, 2)) / 2
    pack = full_cov.FullPack.from_params([(sp[w], A[w], mu[w], full[w]) for w in range(W)])
    pack.device(feats.device)                                           # (the upload of the pack stays outside)
    fb = FeatureBatch.from_packed(feats, lengths)                       # offsets and the length-sorted order, once
    per_word = [full_cov.FullCovBatch(feats, lengths, np.full(N, w), W, S) for w in range(W)]
    routes = {
        "forward": (lambda: full_cov.vocab_scores(fb, None, pack, mode="forward").score,
                    lambda: torch.stack([b.estep(pack, want_stats=False)[0] for b in per_word], dim=1)),
        "viterbi": (lambda: full_cov.vocab_scores(fb, None, pack, mode="viterbi").score,
                    lambda: torch.stack([b.viterbi(pack)[0] for b in per_word], dim=1)),
    }
    nnz = int((A[0] > 0).sum())
    tri = S * D * (D + 1) // 2
    flops = {"forward": N * T * W * (3 * tri + 2 * S * D + 45 * nnz), "viterbi": N * T * W * (3 * tri + 2 * S * D + 3 * nnz)}
    return routes, per_word, flops, full_cov.pack_layout(S, D)[0]


def measure(args):
    import torch
    N = args.N
    for shape in args.shapes:
        D, S = (int(v) for v in shape.split(","))
        routes, per_word, flops, SP = setup(N, D, S)
        out = {"shape": {"N": N, "T": T, "D": D, "S": S, "W": W},
               "per_word_workspace_GB_each": round(per_word[0].ws_bytes / 1e9, 3),
               "per_word_workspace_GB_all_W": round(sum(b.ws_bytes for b in per_word) / 1e9, 3),
               "lattice_and_logb_bytes_per_frame_and_word": 2 * 8 * SP,
               "vocab_flops_ms_at_f64_vector_peak": {k: round(v / F64_VECTOR_FLOPS * 1e3, 3) for k, v in flops.items()}}
        for mode, (vocab, words) in routes.items():
            for _ in range(1 if args.child else 2):
                new, old = vocab(), words()
            torch.cuda.synchronize()
            assert torch.isfinite(old).all() and torch.equal(new, old), f"{mode}: the two matrices differ"
            t_new, t_old = timed_rounds({"vocab": vocab, "per_word": words}, REPEATS, args.child).values()
            med_new, med_old = float(np.median(t_new)), float(np.median(t_old))
            out[f"{mode}_vocab_ms"] = summary(t_new)
            out[f"{mode}_per_word_ms"] = summary(t_old)
            out[f"{mode}_ratio_per_word_over_vocab"] = round(med_old / med_new, 3)
            out[f"{mode}_share_of_f64_vector_peak"] = round(flops[mode] / F64_VECTOR_FLOPS * 1e3 / med_new, 3)
            del new, old
        print(json.dumps(out), flush=True)
        del routes, per_word
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=100000)
    ap.add_argument("--shapes", nargs="+", default=["13,10", "39,18"])
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 summary (a second run of its own)")
    ap.add_argument("--child", action="store_true", help="(internal) the run under rocprofv3")
    args = ap.parse_args()
    measure(args)
    if args.child or not args.trace:
        return
    argv = [str(args.N), "--shapes", *args.shapes]
    header = [
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_full_vocab.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (one call over the vocabulary; W per-word calls) per shape and",
        "# mode; sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "full_vocab_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

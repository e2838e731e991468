"""Ad-hoc timing of the full-covariance E-step and Viterbi decode (dev tool):
    python scripts/time_fullcov.py [N] [--shapes 13,10 39,18] [--out DIR]
One sapr_full_estep (statistics only) and one sapr_full_viterbi over the config-3 batch — N x 101 frames, W = 11 word
models, bidiagonal transitions, full covariances with real off-diagonals — at (D, S) = (13, 10) and (39, 18).  Beside
them, in the same run on the same batch and ALTERNATING with them: one EStep.run (sapr_estep_diag) and one
sapr_gmm_estep_diag at M = 1, both on the diagonals of the same covariances.  Every configuration is warmed twice, then
timed five times between device events (workspace and outputs held outside the timed region); one JSON line per shape.

The split per kernel comes from a rocprofv3 --kernel-trace --stats run of its own: without --child the script starts
itself once more under rocprofv3 (one warm-up and one timed launch of each entry point per shape), reads the kernel
statistics and writes DIR/fullcov_rocprofv3_summary.txt (the sapr kernels only) next to the JSON lines.

full_accum_kernel against the float64 matrix-core peak: the kernel issues S * NTU * (frames / 4) instructions of
16 * 16 * 4 FMAs (NTU = 1, 3, 6 tiles on or above the diagonal at DP = 13, 26, 39); `mfma_flops` counts what it issues,
`useful_flops` the 2 * S * D * (D + 1) / 2 + 2 * S * D per frame a symmetric update needs."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import summary, timed_rounds, trace_run, write_summary

F64_MATRIX_FLOPS = 78.6e12   # MI355X float64 matrix peak (equal to the vector peak)
T, W, REPEATS = 101, 11, 5


def setup(N, D, S):
    import torch
    from sapr_amd import full_cov, gmm_hmm as gh
    from sapr_amd.trellis import DiagModelPack, EStep, FeatureBatch
    from tests._synth import trained_like_models
    torch.manual_seed(0)
    utt_model = np.arange(N) // ((N + W - 1) // W)
    sp, A, mu, cv = trained_like_models(W, S - 2, D, seed=3)
    seg = torch.arange(T, device="cuda").repeat(N) * S // T
    grp = torch.from_numpy(np.repeat(utt_model, T)).cuda()
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
    fbatch = full_cov.FullCovBatch(feats, lengths, utt_model, W, S)
    fpack = fbatch._pack(full_cov.pack_models([(sp[w], A[w], mu[w], full[w]) for w in range(W)]))
    fbatch._pack = lambda _p, d=fpack: d                                 # (the upload of the pack stays outside)
    gbatch = gh.GmmBatch(feats, lengths, utt_model, W, S, 1)
    gpack = gbatch._pack(gh.pack_models([(sp[w], A[w], np.ones((S, 1)), mu[w][:, None], cv[w][:, None])
                                         for w in range(W)]))
    gbatch._pack = lambda _p, d=gpack: d
    es = EStep(FeatureBatch.from_packed(feats, lengths), utt_model, W, S)
    old_pack = DiagModelPack.from_params(sp, A, mu, cv)
    runs = {"full_estep": lambda: fbatch.estep(None), "full_viterbi": lambda: fbatch.viterbi(None),
            "gmm_estep_M1": lambda: gbatch.estep(None), "estep_diag": lambda: es.run(old_pack)}
    return runs, fbatch


def accum_flops(frames, S, D):
    ntu = {13: 1, 26: 3, 39: 6}[13 if D <= 13 else (26 if D <= 26 else 39)]
    return {"mfma_flops": 2.0 * 16 * 16 * 4 * S * ntu * frames / 4, "useful_flops": frames * (S * D * (D + 1) + 2.0 * S * D)}


def measure(args):
    import torch
    N = args.N
    for shape in args.shapes:
        D, S = (int(v) for v in shape.split(","))
        runs, fbatch = setup(N, D, S)
        for fn in runs.values():
            fn()
            if not args.child:
                fn()
        torch.cuda.synchronize()
        times = timed_rounds(runs, REPEATS, args.child)                  # alternating
        ll, stats, _, _ = fbatch.estep(None)
        assert torch.isfinite(ll).all() and torch.isfinite(stats).all()
        assert abs(stats[:, 0].sum().item() - N) < 0.5
        out = {"shape": {"N": N, "T": T, "D": D, "S": S, "W": W}, "workspace_GB": round(fbatch.ws_bytes / 1e9, 3)}
        out.update({k + "_ms": summary(t) for k, t in times.items()})
        out["accum"] = accum_flops(N * T, S, D)
        print(json.dumps(out), flush=True)
        del runs, fbatch
        torch.cuda.empty_cache()


def accum_lines(args, rows):
    """The accumulation kernel against the float64 matrix-core peak, from its traced time."""
    lines = []
    for shape in args.shapes:
        D, S = (int(v) for v in shape.split(","))
        dp = 13 if D <= 13 else (26 if D <= 26 else 39)
        for r in rows:
            if f"full_accum_kernel<{dp}>" in r["Name"]:
                fl, sec = accum_flops(args.N * T, S, D), float(r["AverageNs"]) / 1e9
                lines.append("# full_accum_kernel<%d> at (D, S) = (%d, %d): %.3f ms, issued %.1f%% and useful %.1f%% of the "
                             "%.1f TFLOP/s float64 matrix peak" % (dp, D, S, sec * 1e3, 100 * fl["mfma_flops"] / sec /
                                                                    F64_MATRIX_FLOPS, 100 * fl["useful_flops"] / sec /
                                                                    F64_MATRIX_FLOPS, F64_MATRIX_FLOPS / 1e12))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=100000)
    ap.add_argument("--shapes", nargs="+", default=["13,10", "39,18"])
    ap.add_argument("--out", default="build/fullcov")
    ap.add_argument("--child", action="store_true", help="(internal) the run under rocprofv3")
    args = ap.parse_args()
    measure(args)
    if args.child:
        return
    argv = [str(args.N), "--shapes", *args.shapes]
    header = [
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_fullcov.py {' '.join(argv)} --child",
        "# one warm-up and one timed launch of each entry point per shape; sapr kernels only",
    ]
    rows = trace_run(__file__, argv, args.out, 600)
    write_summary(os.path.join(args.out, "fullcov_rocprofv3_summary.txt"), header, rows, accum_lines(args, rows))


if __name__ == "__main__":
    main()

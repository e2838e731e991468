"""Ad-hoc timing of the Gaussian-mixture E-step (dev tool):
    python scripts/time_gmmhmm.py [N] [--shapes 13,10 39,18] [--mix 1 2 4 8]
One sapr_gmm_estep_diag (statistics only) over the config-3 batch — N x 101 frames, W = 11 word models, bidiagonal
transitions — at (D, S) = (13, 10) and (39, 18) for M = 1, 2, 4, 8 components per state.  Every configuration is warmed
twice, then timed five times between device events (workspace and outputs held outside the timed region, as
fit_gmm_models holds them over its iterations); prints min - max and the median, one JSON line per shape.

Yardstick, timed in the same run on the same batch and ALTERNATING with the mixture E-step: one EStep.run
(sapr_estep_diag, the single-Gaussian E-step).  The M = 1 time against it is the figure to look at first.

The two bounds, from the shapes alone:
  bytes   the traffic the launch sequence needs: features twice (emission and accumulation, 4 D per frame each), logb
          written once and read twice, the lattice written by the forward pass, read and rewritten as gamma by the
          backward pass and read by the accumulation (8 SP each), the finite transitions' xi sums read and written per
          frame (16 per finite transition), over 8 TB/s of HBM
  flops   emission and accumulation: S M D (subtraction, product, FMA = 4 flops) each; accumulation S M (D + 1) two
          FMAs; recursions: 3 passes (forward, backward, xi) over the finite transitions, ~45 flops per term
          (exponential + logarithm share), over the 78.6 TFLOP/s float64 vector peak
and the share of the larger of the two that the measured median reaches."""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from _timing import ev_time, summary
from sapr_amd import gmm_hmm as gh
from sapr_amd.trellis import DiagModelPack, EStep, FeatureBatch
from tests._synth import trained_like_models

HBM_BYTES_PER_S = 8.0e12
F64_VECTOR_FLOPS = 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=100000)
ap.add_argument("--shapes", nargs="+", default=["13,10", "39,18"])
ap.add_argument("--mix", nargs="+", type=int, default=[1, 2, 4, 8])
args = ap.parse_args()
N, T, W, REPEATS = args.N, 101, 11, 5


def bounds_ms(frames, S, M, D, SP, nnz):
    nbytes = frames * (2 * 4 * D + 3 * 8 * SP + 4 * 8 * SP + 16 * nnz)
    flops = frames * (2 * 4 * S * M * D + 4 * S * M * (D + 1) + 3 * 45 * nnz)
    return {"bytes_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 3), "flops_ms": round(flops / F64_VECTOR_FLOPS * 1e3, 3)}


for shape in args.shapes:
    D, S = (int(v) for v in shape.split(","))
    torch.manual_seed(0)
    utt_model = np.arange(N) // ((N + W - 1) // W)
    sp, A, mu, cv = trained_like_models(W, S - 2, D, seed=3)
    # frames scattered about the models' own state means, so that every state and component is visited
    seg = torch.arange(T, device="cuda").repeat(N) * S // T
    grp = torch.from_numpy(np.repeat(utt_model, T)).cuda()
    feats = (torch.from_numpy(mu).cuda()[grp, seg] + torch.randn(N * T, D, device="cuda", dtype=torch.float64) * 5)
    feats = feats.float().contiguous()
    del seg, grp
    lengths = np.full(N, T)
    out = {"shape": {"N": N, "T": T, "D": D, "S": S, "W": W}}

    fb = FeatureBatch.from_packed(feats, lengths)
    es = EStep(fb, utt_model, W, S)
    old_pack = DiagModelPack.from_params(sp, A, mu, cv)
    es.run(old_pack)
    es.run(old_pack)
    torch.cuda.synchronize()
    estep_t = []
    rng = np.random.default_rng(0)
    for M in args.mix:
        prm = []
        for w in range(W):
            means = mu[w][:, None, :] + rng.normal(0, 3.0, (S, M, D))
            prm.append((sp[w], A[w], rng.dirichlet(np.full(M, 5.0), size=S), means, np.repeat(cv[w][:, None, :], M, 1)))
        batch = gh.GmmBatch(feats, lengths, utt_model, W, S, M)
        dpack = batch._pack(gh.pack_models(prm))
        batch._pack = lambda _p, d=dpack: d                           # (the upload of the pack stays outside)
        run = lambda: batch.estep(None)                               # noqa: E731
        run()
        run()
        torch.cuda.synchronize()
        t = []
        for _ in range(REPEATS):                                      # alternating with the yardstick
            t.append(ev_time(run))
            estep_t.append(ev_time(lambda: es.run(old_pack)))
        ll, stats, _, _ = batch.estep(None)
        assert torch.isfinite(ll).all() and torch.isfinite(stats).all()
        assert abs(stats[:, 0].sum().item() - N) < 0.5
        SP = gh.pack_layout(S, M, D)[0]
        b = bounds_ms(N * T, S, M, D, SP, int((A[0] > 0).sum()))
        med = float(np.median(t))
        out[f"gmm_estep_M{M}_ms"] = summary(t)
        out[f"gmm_estep_M{M}_bounds"] = dict(b, workspace_GB=round(batch.ws_bytes / 1e9, 3),
                                             share_of_larger_bound=round(max(b.values()) / med, 3))
        del batch, dpack
        torch.cuda.empty_cache()
    out["estep_diag_ms"] = summary(estep_t)
    print(json.dumps(out), flush=True)
    del feats, es, fb
    torch.cuda.empty_cache()

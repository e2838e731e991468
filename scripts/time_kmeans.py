"""Ad-hoc timing of the batched k-means step and of GaussianHMM's from-scratch initialisation (dev tool):
    python scripts/time_kmeans.py [N] [--shapes 13,10 39,18] [--no-init] [--no-sklearn]
sapr_kmeans_step on N x 101 frames in 11 groups (words) at (D, K) = (13, 10) and (39, 18), one step at R = 1 and at
R = 10 restarts.  Every configuration is warmed twice, then timed five times between device events (workspace and
outputs held outside the timed region, as kmeans() holds them over its iterations); prints min - max and the median,
one JSON line per shape.

Yardsticks, timed in the same run on the same batch and ALTERNATING with the step: one EStep.run (sapr_estep_diag, the
EM iteration that follows the initialisation) and, where scikit-learn imports, one host Lloyd iteration of
sklearn.cluster.KMeans(init=array, n_init=1, max_iter=1, algorithm="lloyd") on a 1 M-frame subsample of one group.

The step's two bounds, from the shapes alone:
  bytes   features once (4 D per frame) + labels out when asked + the per-tile partial statistics written and read back
          (2 x n_tiles R K (2 D + 1) 8) + the centres, over 8 TB/s of HBM
  flops   assign: R K D (one subtraction + one FMA = 3 flops); gather: R D (one subtraction, one addition, one FMA = 4)
          per frame, over the 78.6 TFLOP/s float64 vector peak
and the share of the larger of the two that the measured median reaches.

Then the whole initialisation of 11 default-constructed GaussianHMM(n_components=K) models (fit_models with n_iter=0:
upload, column moments, seeding on the subsample, the Lloyd loop with n_init=10, the final step), wall clock."""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from _timing import ev_time
from sapr_amd import _lib
from sapr_amd.kmeans import FrameTiles
from sapr_amd.trellis import DiagModelPack, EStep, FeatureBatch, kernel_states
from tests._synth import trained_like_models

HBM_BYTES_PER_S = 8.0e12
F64_VECTOR_FLOPS = 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=100000)
ap.add_argument("--shapes", nargs="+", default=["13,10", "39,18"])
ap.add_argument("--no-init", action="store_true")
ap.add_argument("--no-sklearn", action="store_true")
args = ap.parse_args()
N, T, W, REPEATS = args.N, 101, 11, 5
lib = _lib.load()


def summary(t):
    return {"min": round(min(t), 4), "max": round(max(t), 4), "median": round(float(np.median(t)), 4)}


def bounds_ms(frames, n_tiles, G, R, K, D, labels):
    nbytes = frames * 4 * D + (frames * 4 * R if labels else 0) + 2 * n_tiles * R * K * (2 * D + 1) * 8 \
        + G * R * K * D * 8 + G * R * K * (2 * D + 1) * 8
    flops = frames * R * D * (3 * K + 4)
    return {"bytes": nbytes, "flops": flops, "bytes_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4),
            "flops_ms": round(flops / F64_VECTOR_FLOPS * 1e3, 4)}


for shape in args.shapes:
    D, K = (int(v) for v in shape.split(","))
    torch.manual_seed(0)
    utt_model = np.arange(N) // ((N + W - 1) // W)                  # word after word, as fit_models packs them
    glen = np.bincount(utt_model, minlength=W) * T
    protos = torch.randn(W, K, D, device="cuda") * 20
    feats = torch.randn(N * T, D, device="cuda") * 5
    seg = torch.randint(0, K, (N * T,), device="cuda")
    grp = torch.from_numpy(np.repeat(np.arange(W), glen)).cuda()
    feats += protos[grp, seg]
    feats[:, 0] -= 300
    feats = feats.contiguous()
    del seg
    tiles = FrameTiles.build(glen, feats.device)
    goff = tiles.group_off
    out = {"shape": {"N": N, "T": T, "D": D, "K": K, "G": W, "tiles": tiles.n_tiles}}

    # the yardstick on the same batch: one EM iteration of the model that the initialisation is for
    S = kernel_states(K)
    sp, A, mu, cv = trained_like_models(W, S - 2, D, seed=3)
    batch = FeatureBatch.from_packed(feats, np.full(N, T))
    pack = DiagModelPack.from_params(sp, A, mu, cv)
    es = EStep(batch, utt_model, W, S)
    es.run(pack)
    es.run(pack)
    torch.cuda.synchronize()
    estep_t = []

    for R in (1, 10):
        rows = torch.stack([torch.randint(int(goff[g]), int(goff[g + 1]), (R * K,), device="cuda") for g in range(W)])
        centres = feats[rows.reshape(-1)].double().reshape(W, R, K, D).contiguous()
        nb = C.c_size_t(0)
        _lib.check(lib.sapr_kmeans_workspace_bytes(tiles.n_tiles, R, K, D, C.byref(nb)), "sapr_kmeans_workspace_bytes")
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device="cuda")
        stats = torch.empty((W, R, K, 2 * D + 1), dtype=torch.float64, device="cuda")

        def run():
            _lib.check(lib.sapr_kmeans_step(
                _lib.ptr(feats), tiles.total_frames, _lib.ptr(tiles.tile_begin), _lib.ptr(tiles.tile_len),
                _lib.ptr(tiles.tile_group), _lib.ptr(tiles.group_tile_off), tiles.n_tiles, W, R, K, D,
                _lib.ptr(centres), _lib.ptr(ws), int(nb.value), _lib.ptr(stats), None, _lib.current_stream()),
                "sapr_kmeans_step")

        run()
        run()
        torch.cuda.synchronize()
        t = []
        for _ in range(REPEATS):                                     # alternating with the yardstick
            t.append(ev_time(run))
            estep_t.append(ev_time(lambda: es.run(pack)))
        assert stats[..., 0].sum().item() == R * N * T and torch.isfinite(stats).all()
        b = bounds_ms(N * T, tiles.n_tiles, W, R, K, D, labels=False)
        med = float(np.median(t))
        out[f"step_R{R}_ms"] = summary(t)
        out[f"step_R{R}_bounds"] = dict(b, workspace_GB=round(nb.value / 1e9, 3),
                                        share_of_larger_bound=round(max(b["bytes_ms"], b["flops_ms"]) / med, 3))
        del ws, stats, centres
    out["estep_run_ms"] = summary(estep_t)
    del es, batch, pack

    if not args.no_sklearn:
        try:
            from sklearn.cluster import KMeans
            n_sub = min(1_000_000, int(glen[0]))
            Xs = feats[:n_sub].double().cpu().numpy()
            c0 = Xs[np.random.default_rng(0).choice(n_sub, K, replace=False)]
            t = []
            for i in range(3):
                t0 = time.perf_counter()
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    KMeans(n_clusters=K, init=c0, n_init=1, max_iter=1, algorithm="lloyd").fit(Xs)
                if i:
                    t.append((time.perf_counter() - t0) * 1e3)
            out["sklearn_one_lloyd_iteration_ms"] = dict(summary(t), frames=n_sub)
        except ImportError:
            out["sklearn_one_lloyd_iteration_ms"] = None

    if not args.no_init:
        from sapr_amd.hmmlearn_hmm import GaussianHMM, fit_models
        host = feats.cpu().numpy()
        per = [int(x) // T for x in glen]
        data = [(host[int(goff[g]):int(goff[g + 1])], [T] * per[g]) for g in range(W)]
        t = []
        for i in range(3):
            models = [GaussianHMM(n_components=K, random_state=g, n_iter=0) for g in range(W)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit_models(models, data)
            torch.cuda.synchronize()
            if i:
                t.append((time.perf_counter() - t0) * 1e3)
        out["init_11_words_ms"] = summary(t)
        del host, data
    print(json.dumps(out), flush=True)
    del feats
    torch.cuda.empty_cache()

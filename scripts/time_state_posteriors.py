"""Ad-hoc timing of the state posteriors / MAP decoding (dev tool):
    python scripts/time_state_posteriors.py [N] [--shapes 13,10 39,18] [--configs post+path path post] [--yardstick]
sapr_state_posteriors_diag on N x 101 frames, 11 bidiagonal models assigned round-robin, at (D, S) = (13, 10) and
(39, 18), in three configurations: post + path, path only (MAP decoding: 4 bytes per frame out) and post only.  Every
configuration is warmed twice, then timed five times between device events (workspace and outputs allocated outside the
timed region, as a caller that decodes batch after batch would hold them); prints min - max and the median, one JSON
line per shape.

--yardstick: additionally runs the only other producer of the same lattice, the E-step's split path, five times after
two warm-ups WITH its staging copy every time (a one-shot call has no EM iterations to amortise it).  Its three lattice
kernels (fb_stage_kernel + fb_forward_kernel + fb_smooth_kernel) cannot be separated from the observation sums by
device events: run this under  SAPR_ESTEP_OBS=split rocprofv3 --kernel-trace --stats -- python ...  (scripts/prof_any.sh)
and add their durations up from the trace."""
import argparse
import ctypes as C
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from _timing import ev_time
from sapr_amd import _lib
from sapr_amd.trellis import DiagModelPack, EStep, FeatureBatch, TileLayout
from tests._synth import trained_like_models

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=100000)
ap.add_argument("--shapes", nargs="+", default=["13,10", "39,18"])
ap.add_argument("--configs", nargs="+", default=["post+path", "path", "post"], choices=["post+path", "path", "post"])
ap.add_argument("--yardstick", action="store_true")
args = ap.parse_args()
N, T, W, REPEATS = args.N, 101, 11, 5
lib = _lib.load()


for shape in args.shapes:
    D, S = (int(v) for v in shape.split(","))
    sp, A, mu, cv = trained_like_models(W, S - 2, D, seed=3)
    feats = torch.randn(N * T, D, device="cuda") * 20
    feats[:, 0] -= 300
    batch = FeatureBatch.from_packed(feats.contiguous(), np.full(N, T))
    pack = DiagModelPack.from_params(sp, A, mu, cv)
    utt_model = np.arange(N) % W
    layout = TileLayout.build(batch.lengths, utt_model, W, feats.device)
    nb = C.c_size_t(0)
    _lib.check(lib.sapr_state_posteriors_workspace_bytes(layout.n_tiles, pack.S, batch.max_T, pack.topology,
                                                         C.byref(nb)), "sapr_state_posteriors_workspace_bytes")
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device="cuda")
    loglik = torch.empty(N, dtype=torch.float64, device="cuda")
    post = torch.empty((N * T, S), dtype=torch.float64, device="cuda")
    path = torch.empty(N * T, dtype=torch.int32, device="cuda")

    def run(want_post, want_path):
        _lib.check(lib.sapr_state_posteriors_diag(
            _lib.ptr(batch.feats), _lib.ptr(batch.offsets), _lib.ptr(layout.slot_utt), _lib.ptr(layout.tile_model),
            layout.n_tiles, batch.D, batch.max_T, _lib.ptr(pack.blob), W, pack.S, pack.topology, S, _lib.ptr(ws),
            int(nb.value), _lib.ptr(loglik), _lib.ptr(post if want_post else None),
            _lib.ptr(path if want_path else None), _lib.current_stream()), "sapr_state_posteriors_diag")

    out = {"shape": {"N": N, "T": T, "D": D, "S": S, "W": W}, "workspace_GB": round(nb.value / 1e9, 3),
           "algorithmic_bytes_per_frame": 4 * D + 8 * S + 4}
    for cfg in args.configs:
        wp, wq = "post" in cfg, "path" in cfg
        for _ in range(2):
            run(wp, wq)
        torch.cuda.synchronize()
        t = [ev_time(lambda: run(wp, wq)) for _ in range(REPEATS)]
        out[cfg + "_ms"] = {"min": round(min(t), 4), "max": round(max(t), 4), "median": round(float(np.median(t)), 4)}
    assert torch.isfinite(loglik).all()
    if args.yardstick:
        es = EStep(batch, utt_model, W, S)
        t = []
        for i in range(2 + REPEATS):
            es._staged = False  # a one-shot call stages every time
            dt = ev_time(lambda: es.run(pack))
            if i >= 2:
                t.append(dt)
        out["estep_whole_ms"] = {"min": round(min(t), 4), "max": round(max(t), 4),
                                 "median": round(float(np.median(t)), 4)}
        del es
    print(json.dumps(out), flush=True)
    del ws, post, path, feats, batch
    torch.cuda.empty_cache()

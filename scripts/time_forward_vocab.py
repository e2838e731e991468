"""Ad-hoc timing of forward scoring over the vocabulary (dev tool):
    python scripts/time_forward_vocab.py [N]
sapr_forward_vocab (one launch: every utterance under every word model, + the arg-max / posterior epilogue) against the
only other way to the same [N, W] matrix: W consecutive sapr_forward_diag calls, one per word, every utterance assigned
to that word (tile layouts built beforehand, outside the timed region).  Bench shape: N x 101 frames x 13, S = 10,
W = 11, features from the MFCC kernel, models from bench.build_models.  Both paths are warmed, then timed alternately,
five times each, between device events; the two matrices must agree at 1e-11.  Prints one JSON line."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from _timing import ev_time
import bench
from sapr_amd.frontend import BENCH, MfccPlan
from sapr_amd.trellis import DiagModelPack, FeatureBatch, TileLayout, forward_loglik, forward_scores

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
REPEATS = 5
dev = torch.device("cuda", 0)
pcm = bench.synth_pcm(torch, N, seed=1234, device=dev)
lens = np.full(N, bench.N_SAMP, dtype=np.int64)
plan = MfccPlan(**BENCH, max_frames=bench.T_FRAMES)
feats, frames = plan(pcm, lens)
n_model = min(N, 2200)
models = bench.build_models(feats[: n_model * bench.T_FRAMES].cpu().numpy().reshape(n_model, bench.T_FRAMES, bench.D))
pack = DiagModelPack.from_params(*models, device=dev)
batch = FeatureBatch.from_packed(feats.contiguous(), np.asarray(frames, dtype=np.int64))
W = pack.W
layouts = [TileLayout.build(batch.lengths, np.full(N, w), W, dev) for w in range(W)]


def vocab():
    return forward_scores(batch, pack).loglik


def per_word():
    return torch.stack([forward_loglik(batch, pack, None, layout=layouts[w]) for w in range(W)], dim=1)


for _ in range(2):
    new, old = vocab(), per_word()
torch.cuda.synchronize()
rel = ((new - old).abs() / old.abs()).max().item()
assert torch.isfinite(old).all() and rel <= 1e-11, f"the two matrices differ: max relative difference {rel:.3e}"
t_new, t_old = [], []
for _ in range(REPEATS):
    t_new.append(ev_time(vocab))
    t_old.append(ev_time(per_word))
med_new, med_old = float(np.median(t_new)), float(np.median(t_old))
print(json.dumps({
    "shape": {"N": N, "T": bench.T_FRAMES, "D": pack.D, "S": pack.S, "W": W},
    "forward_vocab_ms": {"median": round(med_new, 4), "min": round(min(t_new), 4), "max": round(max(t_new), 4)},
    "per_word_forward_ms": {"median": round(med_old, 4), "min": round(min(t_old), 4), "max": round(max(t_old), 4)},
    "ratio_per_word_over_vocab": round(med_old / med_new, 3),
    "wins_by_more_than_the_yardsticks_spread": bool(med_old - med_new > max(t_old) - min(t_old)),
    "max_relative_difference": rel,
}))

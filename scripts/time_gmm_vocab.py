"""Ad-hoc timing of scoring over the vocabulary for the Gaussian-mixture HMMs (dev tool):
    python scripts/time_gmm_vocab.py [N] [--shapes 13,10,2 39,18,2]
sapr_gmm_vocab_diag (one launch: every utterance under every word model, + the arg-max epilogue) in FORWARD and in
VITERBI mode against the only other way to the same [N, W] matrix: W GmmBatch objects over the same features, every
utterance assigned to word w, and W estep(want_stats=False) resp. viterbi calls (tile layouts, workspaces and the device
pack built beforehand, outside the timed region).  Workload: N x 101 frames, W = 11 word models, bidiagonal
transitions, (D, S, M) = (13, 10, 2) and (39, 18, 2).  Every path is warmed twice, then the two routes are timed
alternately, five times each, between device events; the two matrices must be EQUAL (the kernels share their device
functions).  Prints one JSON line per shape, with the workspace bytes the one-launch route does without and the
float64 operations it needs from the shapes alone: W (4 S M D + ~45 per finite transition; 3 in VITERBI mode) per
frame."""
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from _timing import ev_time, summary
from sapr_amd import gmm_hmm as gh
from sapr_amd.trellis import FeatureBatch
from tests._synth import trained_like_models

F64_VECTOR_FLOPS = 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=100000)
ap.add_argument("--shapes", nargs="+", default=["13,10,2", "39,18,2"])
args = ap.parse_args()
N, T, W, REPEATS = args.N, 101, 11, 5


for shape in args.shapes:
    D, S, M = (int(v) for v in shape.split(","))
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
    rng = np.random.default_rng(0)
    prm = []
    for w in range(W):
        means = mu[w][:, None, :] + rng.normal(0, 3.0, (S, M, D))
        prm.append((sp[w], A[w], rng.dirichlet(np.full(M, 5.0), size=S), means, np.repeat(cv[w][:, None, :], M, 1)))
    pack = gh.GmmPack.from_params(prm)
    pack.device(feats.device)                                           # (the upload of the pack stays outside)
    fb = FeatureBatch.from_packed(feats, lengths)                       # offsets and the length-sorted order, once
    per_word = [gh.GmmBatch(feats, lengths, np.full(N, w), W, S, M) for w in range(W)]
    routes = {
        "forward": (lambda: gh.vocab_scores(fb, None, pack, mode="forward").score,
                    lambda: torch.stack([b.estep(pack, want_stats=False)[0] for b in per_word], dim=1)),
        "viterbi": (lambda: gh.vocab_scores(fb, None, pack, mode="viterbi").score,
                    lambda: torch.stack([b.viterbi(pack)[0] for b in per_word], dim=1)),
    }
    SP = gh.pack_layout(S, M, D)[0]
    nnz = int((A[0] > 0).sum())
    flops = {"forward": N * T * W * (4 * S * M * D + 45 * nnz), "viterbi": N * T * W * (4 * S * M * D + 3 * nnz)}
    out = {"shape": {"N": N, "T": T, "D": D, "S": S, "M": M, "W": W},
           "per_word_workspace_GB_each": round(per_word[0].ws_bytes / 1e9, 3),
           "per_word_workspace_GB_all_W": round(sum(b.ws_bytes for b in per_word) / 1e9, 3),
           "lattice_and_logb_bytes_per_frame_and_word": 2 * 8 * SP,
           "vocab_flops_ms_at_f64_vector_peak": {k: round(v / F64_VECTOR_FLOPS * 1e3, 3) for k, v in flops.items()}}
    for mode, (vocab, words) in routes.items():
        for _ in range(2):
            new, old = vocab(), words()
        torch.cuda.synchronize()
        assert torch.isfinite(old).all() and torch.equal(new, old), f"{mode}: the two matrices differ"
        t_new, t_old = [], []
        for _ in range(REPEATS):
            t_new.append(ev_time(vocab))
            t_old.append(ev_time(words))
        med_new, med_old = float(np.median(t_new)), float(np.median(t_old))
        out[f"{mode}_vocab_ms"] = summary(t_new)
        out[f"{mode}_per_word_ms"] = summary(t_old)
        out[f"{mode}_ratio_per_word_over_vocab"] = round(med_old / med_new, 3)
        out[f"{mode}_share_of_f64_vector_peak"] = round(flops[mode] / F64_VECTOR_FLOPS * 1e3 / med_new, 3)
        del new, old
    print(json.dumps(out), flush=True)
    del feats, fb, per_word, pack, routes
    torch.cuda.empty_cache()

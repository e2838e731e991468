"""Ad-hoc timing of the embedded Baum-Welch E-step against the alignment recursion (dev tool):
    python scripts/time_embedded.py [N] [--frames 505] [--shapes 11,10,13 11,18,39]
N utterances x 505 frames (five words of ~101 frames in a row, the shapes of DESIGN 6.0m), bidiagonal word models,
exits in the last state, diagonal-Gaussian emissions; in one run, on the same logb and utterances:
  align     sapr_connected_align without any path output          the yardstick: the Viterbi recursion over the chain
  forward   sapr_connected_embed, loglik only                     the forward kernel
  fb        sapr_connected_embed, statistics with D = 0           forward + backward kernel + the fold of narrow rows
  estep     sapr_connected_embed, statistics with the features    ... + the observation sums and the fold of full rows
Every route is warmed twice, then the routes are timed in turn, five times each, between device events.  Prints one
JSON line per shape: min / max / median of every route, the backward kernel as fb - forward and the reduction as
estep - fb (medians), each as a multiple of the alignment recursion, and the bytes per frame each pass moves (from the
shapes alone)."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, summary, timed_rounds, warm, word_batch

REPEATS = 5
WORDS = 5


def setup(args, W, S, D):
    import torch
    from sapr_amd import _lib, connected
    from tests._connected_ref import sample_case
    N, T = args.N, args.frames
    model, _, _ = sample_case(7, W, S, D, 0)
    net = connected.ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, None,
                                     model["means"], model["vars"], model["gconst"])
    feats, spoken = word_batch(model["means"], np.sqrt(model["vars"]), N, T, WORDS)
    total, total_words = N * T, N * WORDS
    offs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * T
    woffs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * WORDS
    words = spoken.to(torch.int32).reshape(-1).contiguous()
    lib = _lib.load()
    ls, lt, lx, ops = net.device(feats.device)
    logb = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    _lib.check(lib.sapr_connected_emit_diag(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, _lib.ptr(logb),
                                            _lib.current_stream()), "sapr_connected_emit_diag")
    ws_align = connected.align_workspace_bytes(total, N, WORDS, S)
    ws_embed = connected.embed_workspace_bytes(total, N, total_words, WORDS, S, D)
    ws = torch.empty(max(ws_align, ws_embed), dtype=torch.uint8, device="cuda")
    score = torch.empty(N, dtype=torch.float64, device="cuda")
    loglik = torch.empty(N, dtype=torch.float64, device="cuda")
    stats = {d: torch.empty((W, connected.embed_stats_width(S, d)), dtype=torch.float64, device="cuda") for d in (0, D)}

    def align():
        _lib.check(lib.sapr_connected_align(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(words), _lib.ptr(woffs),
                                            total_words, WORDS, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S,
                                            _lib.ptr(ws), ws_align, _lib.ptr(score), None, None, None, None,
                                            _lib.current_stream()), "sapr_connected_align")

    def embed(d, want_stats):
        _lib.check(lib.sapr_connected_embed(
            _lib.ptr(logb), _lib.ptr(feats) if d else None, d, _lib.ptr(offs), N, total, _lib.ptr(words),
            _lib.ptr(woffs), total_words, WORDS, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws),
            ws_embed, _lib.ptr(loglik), _lib.ptr(stats[d]) if want_stats else None, None, _lib.current_stream()),
            "sapr_connected_embed")

    routes = {"align": align, "forward": lambda: embed(0, False), "fb": lambda: embed(0, True),
              "estep": lambda: embed(D, True)}
    P = WORDS * net.SP
    facts = {"R": net.R, "chain_positions": P, "logb_GB": round(total * net.R * 8 / 1e9, 3),
             # per frame: align reads the emission values and writes a back-pointer byte per position (+ one per slot);
             # forward reads them and writes alpha and X; backward reads them, alpha (once: frame t's row is still in
             # registers from the step before) and X and writes gamma over alpha; the sums read gamma and x
             "align_bytes_per_frame": 9 * P + WORDS, "forward_bytes_per_frame": 16 * P + 8 * WORDS,
             "backward_bytes_per_frame": 24 * P + 8 * WORDS, "sums_bytes_per_frame": 8 * P + 4 * D,
             "align_workspace_GB": round(ws_align / 1e9, 3), "embed_workspace_GB": round(ws_embed / 1e9, 3)}
    return routes, facts, score, loglik, stats[D]


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, score, loglik, stats = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        warm(routes)
        torch.cuda.synchronize()
        assert torch.isfinite(score).all() and torch.isfinite(loglik).all() and bool((score <= loglik).all())
        assert float(stats[:, 0].sum()) == N * WORDS
        out["mean_loglik_minus_viterbi_score"] = round(float((loglik - score).mean()), 4)
        times = timed_rounds(routes, REPEATS)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        out["backward_ms_median"] = round(med["fb"] - med["forward"], 3)
        out["reduction_ms_median"] = round(med["estep"] - med["fb"], 3)
        for k, v in (("forward", med["forward"]), ("backward", med["fb"] - med["forward"]),
                     ("reduction", med["estep"] - med["fb"]), ("estep", med["estep"])):
            out[f"{k}_over_align"] = round(v / med["align"], 2)
        out["forward_GBps"] = round(facts["forward_bytes_per_frame"] * N * T / med["forward"] / 1e6, 1)
        out["backward_GBps"] = round(facts["backward_bytes_per_frame"] * N * T / (med["fb"] - med["forward"]) / 1e6, 1)
        print(json.dumps(out), flush=True)
        del routes, score, loglik, stats
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap, trace=False)
    measure(ap.parse_args())


if __name__ == "__main__":
    main()

"""Ad-hoc timing of connected-word decoding under a word bigram against the word loop (dev tool):
    python scripts/time_bigram.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--trace DIR]
N utterances x 505 frames (five words of ~101 frames in a row, the shapes of DESIGN 6.0j), bidiagonal word models,
exits in the last state, diagonal-Gaussian emissions, the add-one smoothed bigram of the spoken strings
(WordBigram.from_transcripts: a dense, finite lm); in one run, on the same logb and utterances:
  emit         sapr_connected_emit_diag                          the stage both recursions share
  bigram       sapr_connected_bigram without any path output     the bigram recursion alone
  bigram_path  sapr_connected_bigram with every output           (a) recursion + back-trace
  viterbi      sapr_connected_viterbi without any path output    the word-loop recursion alone (the yardstick)
  decode       sapr_connected_viterbi with every output          (b) recursion + back-trace
Every route is warmed twice, then the routes are timed in turn, five times each, between device events.  Prints one
JSON line per shape: min / max / median of every route, the ratios (a) / (b) and of the recursions alone, and the
bytes per frame each recursion moves (from the shapes alone).

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of every route per shape) and writes DIR/bigram_rocprofv3_summary.txt."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, summary, timed_rounds, trace_run, warm, word_batch, write_summary

REPEATS = 5
WORDS = 5


def setup(args, W, S, D):
    import torch
    from sapr_amd import _lib, connected
    from tests._connected_ref import sample_case
    N, T = args.N, args.frames
    model, _, _ = sample_case(7, W, S, D, 0)
    feats, spoken = word_batch(model["means"], np.sqrt(model["vars"]), N, T, WORDS)
    bigram = connected.WordBigram.from_transcripts(spoken.cpu().numpy(), W)
    net = connected.ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, None,
                                     model["means"], model["vars"], model["gconst"], bigram=bigram)
    total = N * T
    offs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * T
    lib = _lib.load()
    ls, lt, lx, ops = net.device(feats.device)
    lm, lm_start, lm_end = net._dev_lm
    logb = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    ws_loop = connected.workspace_bytes(total, N, W, S)
    ws_bigram = connected.bigram_workspace_bytes(total, N, W, S)
    ws = torch.empty(max(ws_loop, ws_bigram), dtype=torch.uint8, device="cuda")
    score = {k: torch.empty(N, dtype=torch.float64, device="cuda") for k in ("bigram", "loop")}
    n_words = {k: torch.empty(N, dtype=torch.int32, device="cuda") for k in ("bigram", "loop")}
    pw = torch.empty(total, dtype=torch.int32, device="cuda")
    ps = torch.empty(total, dtype=torch.int32, device="cuda")
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")

    def emit():
        _lib.check(lib.sapr_connected_emit_diag(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, _lib.ptr(logb),
                                                _lib.current_stream()), "sapr_connected_emit_diag")

    def bigram_route(paths):
        out = (n_words["bigram"], pw, ps, pe) if paths else (None,) * 4
        _lib.check(lib.sapr_connected_bigram(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                             _lib.ptr(lx), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), W, S,
                                             _lib.ptr(ws), ws_bigram, _lib.ptr(score["bigram"]),
                                             *(_lib.ptr(o) for o in out), _lib.current_stream()),
                   "sapr_connected_bigram")

    def viterbi(paths):
        out = (n_words["loop"], pw, ps, pe) if paths else (None,) * 4
        _lib.check(lib.sapr_connected_viterbi(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                              _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws), ws_loop, _lib.ptr(score["loop"]),
                                              *(_lib.ptr(o) for o in out), _lib.current_stream()),
                   "sapr_connected_viterbi")

    routes = {"emit": emit, "bigram": lambda: bigram_route(False), "bigram_path": lambda: bigram_route(True),
              "viterbi": lambda: viterbi(False), "decode": lambda: viterbi(True)}
    facts = {"R": net.R, "logb_GB": round(total * net.R * 8 / 1e9, 3),
             # per frame: the emission values read, one back-pointer byte per flat state, then two bytes per word / one
             # int32
             "bigram_bytes_per_frame": 9 * net.R + 2 * W, "viterbi_bytes_per_frame": 9 * net.R + 4,
             "bigram_workspace_GB": round(ws_bigram / 1e9, 3), "viterbi_workspace_GB": round(ws_loop / 1e9, 3)}
    return routes, facts, score, n_words


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, score, n_words = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        warm(routes, args.child)
        torch.cuda.synchronize()
        assert torch.isfinite(score["bigram"]).all() and torch.isfinite(score["loop"]).all()
        assert bool((score["bigram"] <= score["loop"]).all())    # (every lm entry is a log-probability: <= 0)
        out["mean_words_found"] = {k: round(float(v.float().mean()), 2) for k, v in n_words.items()}
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        out["bigram_backtrace_ms_median"] = round(med["bigram_path"] - med["bigram"], 3)
        out["ratio_bigram_over_loop"] = round(med["bigram_path"] / med["decode"], 3)
        out["ratio_recursions_alone"] = round(med["bigram"] / med["viterbi"], 3)
        out["emission_share_of_emit_plus_bigram"] = round(med["emit"] / (med["emit"] + med["bigram_path"]), 3)
        out["bigram_GBps"] = round(facts["bigram_bytes_per_frame"] * N * T / med["bigram"] / 1e6, 1)
        out["viterbi_GBps"] = round(facts["viterbi_bytes_per_frame"] * N * T / med["viterbi"] / 1e6, 1)
        print(json.dumps(out), flush=True)
        del routes, score, n_words
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap)
    args = ap.parse_args()
    measure(args)
    if args.child or not args.trace:
        return
    argv = [str(args.N), "--frames", str(args.frames), "--shapes", *args.shapes]
    header = [
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_bigram.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (emission; bigram recursion alone and with its back-trace;",
        "# word-loop recursion alone and with its back-trace) per shape; sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "bigram_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

"""Ad-hoc timing of the connected-word N-best list against the bigram loop and level building (dev tool):
    python scripts/time_nbest.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--depths 1 2 4 8] [--trace DIR]
The batch of scripts/time_levels.py: N utterances x 505 frames (five words of ~101 frames in a row), bidiagonal word
models, exits in the last state, diagonal-Gaussian emissions, the add-one smoothed bigram of the spoken strings; in one
process, on the same logb and utterances:
  bigram          sapr_connected_bigram without any path output       the loop's recursion alone (the yardstick)
  bigram_path     sapr_connected_bigram with every output             recursion + back-trace: ONE string with boundaries
  levels_8        sapr_connected_levels at L = 8                      the level recursion alone
  levels_8_path   ... + one sapr_connected_levels_backtrace           one string per count: the other source of alternatives
  nbest_n         sapr_connected_nbest at n_best = n                  the n best distinct strings, no boundaries
Every route is warmed twice, then the routes are timed in turn, five times each, between device events.  Prints one
JSON line per shape: min / max / median of every route and, per depth, the ratios to the bigram recursion and to L = 8
level building.

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own,
under a time limit: one warm-up and one timed call of every route per shape) and writes
DIR/nbest_rocprofv3_summary.txt."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, summary, timed_rounds, trace_run, warm, word_batch, write_summary

REPEATS = 5
WORDS = 5
LEVELS = 8


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
    _lib.check(lib.sapr_connected_emit_diag(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, _lib.ptr(logb),
                                            _lib.current_stream()), "sapr_connected_emit_diag")
    ws_bigram = connected.bigram_workspace_bytes(total, N, W, S)
    ws_levels = connected.levels_workspace_bytes(total, N, W, S, LEVELS)
    ws = torch.empty(max(ws_bigram, ws_levels), dtype=torch.uint8, device="cuda")
    score = {k: torch.empty(N, dtype=torch.float64, device="cuda") for k in ("bigram", "levels")}
    level = torch.empty((N, LEVELS), dtype=torch.float64, device="cuda")
    n_words = {k: torch.empty(N, dtype=torch.int32, device="cuda") for k in ("bigram", "levels")}
    pw = torch.empty(total, dtype=torch.int32, device="cuda")
    ps = torch.empty(total, dtype=torch.int32, device="cuda")
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")
    lists = {n: (torch.empty((N, n), dtype=torch.float64, device="cuda"),
                 torch.empty((N, n), dtype=torch.int64, device="cuda")) for n in args.depths}
    n_found = torch.empty(N, dtype=torch.int32, device="cuda")
    overflow = torch.empty(N, dtype=torch.uint8, device="cuda")

    def bigram_route(paths):
        out = (n_words["bigram"], pw, ps, pe) if paths else (None,) * 4
        _lib.check(lib.sapr_connected_bigram(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                             _lib.ptr(lx), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), W, S,
                                             _lib.ptr(ws), ws_bigram, _lib.ptr(score["bigram"]),
                                             *(_lib.ptr(o) for o in out), _lib.current_stream()),
                   "sapr_connected_bigram")

    def levels_route(paths):
        _lib.check(lib.sapr_connected_levels(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                             _lib.ptr(lx), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), W, S,
                                             LEVELS, _lib.ptr(ws), ws_levels, _lib.ptr(level), _lib.current_stream()),
                   "sapr_connected_levels")
        if paths:
            _lib.check(lib.sapr_connected_levels_backtrace(_lib.ptr(offs), N, total, W, S, LEVELS, _lib.ptr(ws),
                                                           ws_levels, _lib.ptr(level), None, None,
                                                           _lib.ptr(score["levels"]), _lib.ptr(n_words["levels"]),
                                                           _lib.ptr(pw), _lib.ptr(ps), _lib.ptr(pe),
                                                           _lib.current_stream()), "sapr_connected_levels_backtrace")

    def nbest_route(n):
        _lib.check(lib.sapr_connected_nbest(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                            _lib.ptr(lx), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), W, S, n,
                                            _lib.ptr(lists[n][0]), _lib.ptr(lists[n][1]), _lib.ptr(n_found),
                                            _lib.ptr(overflow), _lib.current_stream()), "sapr_connected_nbest")

    routes = {"bigram": lambda: bigram_route(False), "bigram_path": lambda: bigram_route(True),
              f"levels_{LEVELS}": lambda: levels_route(False), f"levels_{LEVELS}_path": lambda: levels_route(True)}
    for n in args.depths:
        routes[f"nbest_{n}"] = lambda n=n: nbest_route(n)
    facts = {"R": net.R, "logb_GB": round(total * net.R * 8 / 1e9, 3)}
    return routes, facts, score, lists, n_found, overflow


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, score, lists, n_found, overflow = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        warm(routes, args.child)
        torch.cuda.synchronize()
        assert torch.isfinite(score["bigram"]).all()
        for n in args.depths:   # rank 1 is the loop's score on this batch, bit for bit
            assert bool((lists[n][0][:, 0] == score["bigram"]).all())
        out["mean_strings_found"] = round(float(n_found.float().mean()), 2)     # (of the last depth run)
        out["overflowed"] = int(overflow.sum())
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        out["ratio_over_bigram_recursion"] = {n: round(med[f"nbest_{n}"] / med["bigram"], 2) for n in args.depths}
        out["ratio_over_levels_8_with_backtrace"] = {n: round(med[f"nbest_{n}"] / med[f"levels_{LEVELS}_path"], 2)
                                                     for n in args.depths}
        print(json.dumps(out), flush=True)
        del routes, score, lists
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap)
    ap.add_argument("--depths", nargs="+", type=int, default=[1, 2, 4, 8])
    args = ap.parse_args()
    measure(args)
    if args.child or not args.trace:
        return
    argv = [str(args.N), "--frames", str(args.frames), "--shapes", *args.shapes,
            "--depths", *(str(n) for n in args.depths)]
    header = [
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_nbest.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (bigram recursion alone and with its back-trace; level building",
        f"# at L = {LEVELS} alone and with one back-trace; the N-best recursion per depth) per shape; sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "nbest_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 600))


if __name__ == "__main__":
    main()

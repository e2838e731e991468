"""Ad-hoc timing of connected-word decoding with a bounded word count (level building) against the bigram loop (dev
tool):
    python scripts/time_levels.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--levels 1 2 4 8] [--trace DIR]
The batch of scripts/time_bigram.py: N utterances x 505 frames (five words of ~101 frames in a row), bidiagonal word
models, exits in the last state, diagonal-Gaussian emissions, the add-one smoothed bigram of the spoken strings; in one
run, on the same logb and utterances:
  bigram          sapr_connected_bigram without any path output       the loop's recursion alone (the yardstick)
  bigram_path     sapr_connected_bigram with every output             (b) recursion + back-trace
  levels_L        sapr_connected_levels at L levels                   the level recursion alone
  levels_L_path   ... + one sapr_connected_levels_backtrace           (a) recursion + one back-trace (default selection)
Every route is warmed twice, then the routes are timed in turn, five times each, between device events.  Prints one
JSON line per shape: min / max / median of every route, per L the ratios of the recursions alone and (a) / (b), the
back-trace's own time, and the workspace bytes (per frame and in all).

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of every route per shape) and writes DIR/levels_rocprofv3_summary.txt."""
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
    _lib.check(lib.sapr_connected_emit_diag(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, _lib.ptr(logb),
                                            _lib.current_stream()), "sapr_connected_emit_diag")
    ws_bigram = connected.bigram_workspace_bytes(total, N, W, S)
    ws_levels = {L: connected.levels_workspace_bytes(total, N, W, S, L) for L in args.levels}
    ws = torch.empty(max([ws_bigram] + list(ws_levels.values())), dtype=torch.uint8, device="cuda")
    score = {"bigram": torch.empty(N, dtype=torch.float64, device="cuda"),
             "levels": torch.empty(N, dtype=torch.float64, device="cuda")}
    level = {L: torch.empty((N, L), dtype=torch.float64, device="cuda") for L in args.levels}
    n_words = {k: torch.empty(N, dtype=torch.int32, device="cuda") for k in ("bigram", "levels")}
    pw = torch.empty(total, dtype=torch.int32, device="cuda")
    ps = torch.empty(total, dtype=torch.int32, device="cuda")
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")

    def bigram_route(paths):
        out = (n_words["bigram"], pw, ps, pe) if paths else (None,) * 4
        _lib.check(lib.sapr_connected_bigram(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                             _lib.ptr(lx), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), W, S,
                                             _lib.ptr(ws), ws_bigram, _lib.ptr(score["bigram"]),
                                             *(_lib.ptr(o) for o in out), _lib.current_stream()),
                   "sapr_connected_bigram")

    def levels_route(L, paths):
        _lib.check(lib.sapr_connected_levels(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                             _lib.ptr(lx), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), W, S, L,
                                             _lib.ptr(ws), ws_levels[L], _lib.ptr(level[L]), _lib.current_stream()),
                   "sapr_connected_levels")
        if paths:
            _lib.check(lib.sapr_connected_levels_backtrace(_lib.ptr(offs), N, total, W, S, L, _lib.ptr(ws),
                                                           ws_levels[L], _lib.ptr(level[L]), None, None,
                                                           _lib.ptr(score["levels"]), _lib.ptr(n_words["levels"]),
                                                           _lib.ptr(pw), _lib.ptr(ps), _lib.ptr(pe),
                                                           _lib.current_stream()), "sapr_connected_levels_backtrace")

    routes = {"bigram": lambda: bigram_route(False), "bigram_path": lambda: bigram_route(True)}
    for L in args.levels:
        routes[f"levels_{L}"] = lambda L=L: levels_route(L, False)
        routes[f"levels_{L}_path"] = lambda L=L: levels_route(L, True)
    facts = {"R": net.R, "logb_GB": round(total * net.R * 8 / 1e9, 3),
             "bigram_workspace_GB": round(ws_bigram / 1e9, 3),
             "levels_workspace_GB": {L: round(b / 1e9, 3) for L, b in ws_levels.items()},
             # per frame: one back-pointer byte per (level, flat state) and two bytes per (level, word)
             "levels_workspace_bytes_per_frame": {L: L * (net.R + 2 * W) for L in args.levels}}
    return routes, facts, score, level, n_words


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, score, level, n_words = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        warm(routes, args.child)
        torch.cuda.synchronize()
        assert torch.isfinite(score["bigram"]).all()
        found = n_words["bigram"].long()
        for L in args.levels:   # the loop identity on this batch: the level of the loop's own count has its score
            fits = found <= L
            got = level[L][torch.arange(N, device="cuda")[fits], found[fits] - 1]
            assert bool((got == score["bigram"][fits]).all()) and not bool((level[L] > score["bigram"][:, None]).any())
        out["mean_words_found"] = round(float(found.float().mean()), 2)
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        out["ratio_recursion_over_bigram"] = {L: round(med[f"levels_{L}"] / med["bigram"], 3) for L in args.levels}
        out["ratio_with_backtrace_over_bigram"] = {L: round(med[f"levels_{L}_path"] / med["bigram_path"], 3)
                                                   for L in args.levels}
        out["levels_backtrace_ms_median"] = {L: round(med[f"levels_{L}_path"] - med[f"levels_{L}"], 3)
                                             for L in args.levels}
        out["ms_per_level"] = {L: round(med[f"levels_{L}"] / L, 3) for L in args.levels}
        print(json.dumps(out), flush=True)
        del routes, score, level, n_words
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap)
    ap.add_argument("--levels", nargs="+", type=int, default=[1, 2, 4, 8])
    args = ap.parse_args()
    measure(args)
    if args.child or not args.trace:
        return
    argv = [str(args.N), "--frames", str(args.frames), "--shapes", *args.shapes,
            "--levels", *(str(L) for L in args.levels)]
    header = [
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_levels.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (bigram recursion alone and with its back-trace; per L the",
        "# level recursion alone and with one back-trace) per shape; sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "levels_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

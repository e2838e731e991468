"""Ad-hoc timing of the connected-word lattice against the bigram search it stands beside (dev tool):
    python scripts/time_lattice.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--trace DIR]
N utterances x 505 frames (five words of ~101 frames in a row, the shapes of DESIGN 6.0j), bidiagonal word models,
exits in the last state, diagonal-Gaussian emissions, the add-one smoothed bigram of the spoken strings; in one
process, on the same logb and utterances:
  emit         sapr_connected_emit_diag                          the stage every route shares
  bigram_path  sapr_connected_bigram with every output           the yardstick: recursion + back-trace
  lattice      sapr_connected_lattice                            the forward tables X, N, B (20 W bytes per frame)
  backward     sapr_connected_lattice_backward, own tables       beta / next / root / first: what pruning needs
  walk         sapr_connected_lattice_walk                       the best string from next
  rescore      backward under a SECOND bigram + walk             a new language-model weight and penalty, no recursion
  redecode     sapr_connected_bigram under the second bigram     what rescoring replaces: a second recursion + back-trace
The second bigram is ``bigram.scaled(1.5, -2.0)``.  Every route is warmed once, then the routes are timed in turn,
twice each, between device events.  Prints one JSON line per shape: min / max of every route, the ratios lattice /
bigram_path and rescore / redecode, and the share of utterances on which the rescored score equals the re-decode's.

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of every route per shape) and writes DIR/lattice_rocprofv3_summary.txt."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, timed_rounds, trace_run, word_batch, write_summary

REPEATS = 2
WORDS = 5


def setup(args, W, S, D):
    import torch
    from sapr_amd import _lib, connected
    from tests._connected_ref import sample_case
    N, T = args.N, args.frames
    model, _, _ = sample_case(7, W, S, D, 0)
    feats, spoken = word_batch(model["means"], np.sqrt(model["vars"]), N, T, WORDS)
    bigram = connected.WordBigram.from_transcripts(spoken.cpu().numpy(), W)
    second = bigram.scaled(1.5, -2.0)
    net = connected.ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, None,
                                     model["means"], model["vars"], model["gconst"], bigram=bigram)
    total = N * T
    offs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * T
    lib = _lib.load()
    ls, lt, lx, ops = net.device(feats.device)
    lm1 = net._dev_lm
    lm2 = tuple(torch.from_numpy(a).cuda() for a in (second.lm, second.lm_start, second.lm_end))
    logb = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    ws_bigram = connected.bigram_workspace_bytes(total, N, W, S)
    ws_lattice = connected.lattice_workspace_bytes(total, N, W, S)
    ws = torch.empty(ws_bigram, dtype=torch.uint8, device="cuda")
    tables = torch.empty(ws_lattice, dtype=torch.uint8, device="cuda")
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")   # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")     # noqa: E731
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")      # noqa: E731
    score = {k: f64(N) for k in ("bigram", "lattice", "redecode")}
    root = {k: f64(N) for k in ("own", "second")}
    first = {k: i32(N, 2) for k in ("own", "second")}
    final, n_words = i32(N), {k: i32(N) for k in ("bigram", "walk", "rescore", "redecode")}
    beta, next_end, next_word = f64(total, W), i32(total, W), u8(total, W)
    pw, ps, pe = i32(total), i32(total), u8(total)
    st = _lib.current_stream

    def emit():
        _lib.check(lib.sapr_connected_emit_diag(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, _lib.ptr(logb), st()),
                   "sapr_connected_emit_diag")

    def search(lm, key):
        _lib.check(lib.sapr_connected_bigram(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                             _lib.ptr(lx), *(_lib.ptr(a) for a in lm), W, S, _lib.ptr(ws), ws_bigram,
                                             _lib.ptr(score[key]), _lib.ptr(n_words[key]), _lib.ptr(pw), _lib.ptr(ps),
                                             _lib.ptr(pe), st()), "sapr_connected_bigram")

    def lattice():
        _lib.check(lib.sapr_connected_lattice(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                              _lib.ptr(lx), *(_lib.ptr(a) for a in lm1), W, S, _lib.ptr(tables),
                                              ws_lattice, _lib.ptr(score["lattice"]), _lib.ptr(final), st()),
                   "sapr_connected_lattice")

    def backward(lm, key):
        _lib.check(lib.sapr_connected_lattice_backward(_lib.ptr(offs), N, total, W, S, _lib.ptr(tables), ws_lattice,
                                                       _lib.ptr(lm1[1]), *(_lib.ptr(a) for a in lm), _lib.ptr(beta),
                                                       _lib.ptr(next_end), _lib.ptr(next_word), _lib.ptr(root[key]),
                                                       _lib.ptr(first[key]), st()), "sapr_connected_lattice_backward")

    def walk(key, out):
        _lib.check(lib.sapr_connected_lattice_walk(_lib.ptr(offs), N, total, W, S, _lib.ptr(next_end),
                                                   _lib.ptr(next_word), _lib.ptr(root[key]), _lib.ptr(first[key]),
                                                   _lib.ptr(n_words[out]), _lib.ptr(pw), _lib.ptr(pe), st()),
                   "sapr_connected_lattice_walk")

    def rescore():
        backward(lm2, "second")
        walk("second", "rescore")

    # (walk follows backward: it reads the next rows the own-table pass left; rescore overwrites them afterwards)
    routes = {"emit": emit, "bigram_path": lambda: search(lm1, "bigram"), "lattice": lattice,
              "backward": lambda: backward(lm1, "own"), "walk": lambda: walk("own", "walk"), "rescore": rescore,
              "redecode": lambda: search(lm2, "redecode")}
    facts = {"R": net.R, "logb_GB": round(total * net.R * 8 / 1e9, 3),
             "lattice_bytes_per_frame": 8 * net.R + 20 * W, "bigram_bytes_per_frame": 9 * net.R + 2 * W,
             "lattice_tables_GB": round(ws_lattice / 1e9, 3), "bigram_workspace_GB": round(ws_bigram / 1e9, 3),
             "backward_outputs_GB": round(13 * total * W / 1e9, 3)}
    return routes, facts, score, root, n_words


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, score, root, n_words = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        assert torch.isfinite(score["bigram"]).all()
        assert score["lattice"].cpu().numpy().tobytes() == score["bigram"].cpu().numpy().tobytes()
        slack = 4 * T * 2.0 ** -52 * float(score["bigram"].abs().max()) * 4     # (a loose eps_u: |X| <= ~|score|)
        assert bool(((root["own"] - score["bigram"]).abs() <= slack).all())
        assert bool((n_words["walk"] == n_words["bigram"]).all())
        assert bool((root["second"] <= score["redecode"] + slack).all())
        out["rescore_reaches_redecode_share"] = round(
            float(((root["second"] - score["redecode"]).abs() <= slack).float().mean()), 4)
        out["rescore_same_word_count_share"] = round(
            float((n_words["rescore"] == n_words["redecode"]).float().mean()), 4)
        out["mean_words_found"] = round(float(n_words["bigram"].float().mean()), 2)
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = {"min": round(min(t), 3), "max": round(max(t), 3)}
        best = {k: min(t) for k, t in times.items()}
        out["ratio_lattice_over_bigram_path"] = round(best["lattice"] / best["bigram_path"], 3)
        out["ratio_rescore_over_redecode"] = round(best["rescore"] / best["redecode"], 3)
        out["ratio_lattice_plus_backward_over_bigram_path"] = round(
            (best["lattice"] + best["backward"] + best["walk"]) / best["bigram_path"], 3)
        print(json.dumps(out), flush=True)
        del routes, score, root, n_words
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
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_lattice.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (emission; bigram recursion with its back-trace, under two",
        "# bigrams; the lattice's forward tables; its backward pass under two bigrams; its walk, twice) per shape;",
        "# sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "lattice_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

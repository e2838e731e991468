"""Ad-hoc timing of forward-backward over the word loop against the bigram search and the embedded kernels (dev tool):
    python scripts/time_posteriors.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--trace DIR]
The workload of scripts/time_bigram.py: N utterances x 505 frames (five words of ~101 frames in a row), bidiagonal word
models, exits in the last state, diagonal-Gaussian emissions, the add-one smoothed bigram of the spoken strings (a
dense, finite lm); in one run, on the same logb and utterances:
  bigram_path  sapr_connected_bigram with every output             the search: recursion + back-trace (the baseline)
  loop_fwd     sapr_connected_posteriors, loglik only              loop_forward_kernel alone
  loop_fb      sapr_connected_posteriors, word_post + entry_post   + loop_backward_kernel (the confidence route)
  loop_fb_post ... and post[total_frames][R]                       + 8 R bytes per frame written
  embed_fwd    sapr_connected_embed, loglik only                   embed_forward_kernel over the five spoken words
  embed_fb     sapr_connected_embed, statistics with D = 0         + embed_backward_kernel + the fold of narrow rows
Every route is warmed twice, then the routes are timed in turn, five times each, between device events.  Prints one
JSON line per shape: min / max / median of every route, the ratios to the search and to the embedded kernels, and the
bytes per frame each kernel moves (from the shapes alone).

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of every route per shape) and writes DIR/loop_posteriors_rocprofv3_summary.txt."""
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
    total, total_words = N * T, N * WORDS
    offs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * T
    woffs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * WORDS
    words = spoken.to(torch.int32).reshape(-1).contiguous()
    lib = _lib.load()
    ls, lt, lx, ops = net.device(feats.device)
    lm, lm_start, lm_end = net.device_lm(feats.device)
    logb = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    _lib.check(lib.sapr_connected_emit_diag(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, _lib.ptr(logb),
                                            _lib.current_stream()), "sapr_connected_emit_diag")
    del feats
    ws_bigram = connected.bigram_workspace_bytes(total, N, W, S)
    ws_post = connected.posteriors_workspace_bytes(total, N, W, S)
    ws_embed = connected.embed_workspace_bytes(total, N, total_words, WORDS, S, 0)
    ws = torch.empty(max(ws_bigram, ws_post, ws_embed), dtype=torch.uint8, device="cuda")
    score = torch.empty(N, dtype=torch.float64, device="cuda")
    loglik = {k: torch.empty(N, dtype=torch.float64, device="cuda") for k in ("loop", "embed")}
    n_words = torch.empty(N, dtype=torch.int32, device="cuda")
    pw = torch.empty(total, dtype=torch.int32, device="cuda")
    ps = torch.empty(total, dtype=torch.int32, device="cuda")
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")
    word_post = torch.empty((total, W), dtype=torch.float64, device="cuda")
    entry_post = torch.empty((total, W), dtype=torch.float64, device="cuda")
    post = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    stats = torch.empty((W, connected.embed_stats_width(S, 0)), dtype=torch.float64, device="cuda")

    def search():
        _lib.check(lib.sapr_connected_bigram(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                             _lib.ptr(lx), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), W, S,
                                             _lib.ptr(ws), ws_bigram, _lib.ptr(score), _lib.ptr(n_words), _lib.ptr(pw),
                                             _lib.ptr(ps), _lib.ptr(pe), _lib.current_stream()),
                   "sapr_connected_bigram")

    def loop(words_out, states_out):
        _lib.check(lib.sapr_connected_posteriors(
            _lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), _lib.ptr(lm),
            _lib.ptr(lm_start), _lib.ptr(lm_end), W, S, _lib.ptr(ws), ws_post, _lib.ptr(loglik["loop"]),
            _lib.ptr(word_post) if words_out else None, _lib.ptr(entry_post) if words_out else None,
            _lib.ptr(post) if states_out else None, _lib.current_stream()), "sapr_connected_posteriors")

    def embed(want_stats):
        _lib.check(lib.sapr_connected_embed(
            _lib.ptr(logb), None, 0, _lib.ptr(offs), N, total, _lib.ptr(words), _lib.ptr(woffs), total_words, WORDS,
            _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws), ws_embed, _lib.ptr(loglik["embed"]),
            _lib.ptr(stats) if want_stats else None, None, _lib.current_stream()), "sapr_connected_embed")

    routes = {"bigram_path": search, "loop_fwd": lambda: loop(False, False), "loop_fb": lambda: loop(True, False),
              "loop_fb_post": lambda: loop(True, True), "embed_fwd": lambda: embed(False),
              "embed_fb": lambda: embed(True)}
    R, P = net.R, WORDS * net.SP
    facts = {"R": R, "chain_positions_of_embed": P, "logb_GB": round(total * R * 8 / 1e9, 3),
             # per frame: the forward kernel reads the emission values and writes alpha and N; the backward kernel reads
             # the emission values, alpha and N and writes word_post and entry_post (and post)
             "loop_fwd_bytes_per_frame": 16 * R + 8 * W, "loop_bwd_bytes_per_frame": 16 * R + 24 * W,
             "loop_bwd_post_bytes_per_frame": 24 * R + 24 * W, "bigram_bytes_per_frame": 9 * R + 2 * W,
             "posteriors_workspace_GB": round(ws_post / 1e9, 3), "bigram_workspace_GB": round(ws_bigram / 1e9, 3)}
    return routes, facts, score, loglik, word_post


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, score, loglik, word_post = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        warm(routes, args.child)
        routes["loop_fb"]()
        torch.cuda.synchronize()
        assert torch.isfinite(score).all() and torch.isfinite(loglik["loop"]).all()
        out["min_loglik_minus_score"] = float((loglik["loop"] - score).min())
        out["max_word_post_row_sum_error"] = float((word_post.sum(dim=1) - 1.0).abs().max())
        out["mean_log_posterior_of_the_decoded_path"] = round(float((score - loglik["loop"]).mean()), 6)
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        out["loop_bwd_ms_median"] = round(med["loop_fb"] - med["loop_fwd"], 3)
        out["embed_bwd_and_fold_ms_median"] = round(med["embed_fb"] - med["embed_fwd"], 3)
        out["ratio_confidence_over_search"] = round(med["loop_fb"] / med["bigram_path"], 3)
        out["ratio_loop_fwd_over_embed_fwd"] = round(med["loop_fwd"] / med["embed_fwd"], 3)
        out["ratio_loop_bwd_over_embed_bwd"] = round((med["loop_fb"] - med["loop_fwd"]) /
                                                     (med["embed_fb"] - med["embed_fwd"]), 3)
        out["loop_fwd_GBps"] = round(facts["loop_fwd_bytes_per_frame"] * N * T / med["loop_fwd"] / 1e6, 1)
        out["loop_bwd_GBps"] = round(facts["loop_bwd_bytes_per_frame"] * N * T /
                                     (med["loop_fb"] - med["loop_fwd"]) / 1e6, 1)
        print(json.dumps(out), flush=True)
        del routes, score, loglik, word_post
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
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_posteriors.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (bigram search with its back-trace; word-loop forward kernel",
        "# alone, with the backward kernel, with post as well; embedded forward kernel alone and with its backward",
        "# kernel and fold at D = 0) per shape, plus one call of the confidence route; sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "loop_posteriors_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

"""Ad-hoc timing of the MMI E-step's denominator statistics against the numerator's reduction (dev tool):
    python scripts/time_mmi.py [N] [--frames 505] [--shapes 11,10,13 11,18,39]
N utterances x 505 frames (five words of ~101 frames in a row, the shapes of scripts/time_embedded.py), bidiagonal
word models, exits in the last state, diagonal-Gaussian emissions, the free word loop; in one run, on the same logb:
  fb          sapr_connected_embed, statistics with D = 0             the numerator's recursions and the narrow fold
  estep       sapr_connected_embed, statistics with the features      the embedded E-step: ... + embed_obs_kernel + fold
  loop_fb     sapr_connected_posteriors, loglik and post              the denominator's recursions
  den_stats   sapr_connected_loop_stats on that post                  loop_stats_accum_kernel + loop_stats_fold_kernel
  mmi         estep, loop_fb, den_stats in a row                      the whole MMI E-step on the device
Every route is warmed twice, then the routes are timed in turn, five times each, between device events.  Prints one
JSON line per shape: min / max / median of every route, the numerator's reduction as estep - fb (medians), den_stats as
a multiple of it and of the time to read post and feats once at the HBM rate bench.py uses, and the MMI E-step as a
multiple of the embedded E-step."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, summary, timed_rounds, warm, word_batch

REPEATS = 5
WORDS = 5
HBM_PEAK_GBS = 8000.0  # bench.py's


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
    lm, lm_start, lm_end = net.device_lm(feats.device)
    logb = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    _lib.check(lib.sapr_connected_emit_diag(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, _lib.ptr(logb),
                                            _lib.current_stream()), "sapr_connected_emit_diag")
    ws_embed = connected.embed_workspace_bytes(total, N, total_words, WORDS, S, D)
    ws_loop = connected.posteriors_workspace_bytes(total, N, W, S)
    ws_stats = connected.loop_stats_workspace_bytes(total, N, W, S, D)
    ws = torch.empty(max(ws_embed, ws_loop), dtype=torch.uint8, device="cuda")
    ws2 = torch.empty(max(ws_stats, 1), dtype=torch.uint8, device="cuda")
    loglik = torch.empty(N, dtype=torch.float64, device="cuda")
    den_ll = torch.empty(N, dtype=torch.float64, device="cuda")
    post = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    stats = {d: torch.empty((W, connected.embed_stats_width(S, d)), dtype=torch.float64, device="cuda") for d in (0, D)}
    den = torch.empty((W, connected.embed_stats_width(S, D)), dtype=torch.float64, device="cuda")

    def embed(d):
        _lib.check(lib.sapr_connected_embed(
            _lib.ptr(logb), _lib.ptr(feats) if d else None, d, _lib.ptr(offs), N, total, _lib.ptr(words),
            _lib.ptr(woffs), total_words, WORDS, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws),
            ws_embed, _lib.ptr(loglik), _lib.ptr(stats[d]), None, _lib.current_stream()), "sapr_connected_embed")

    def loop_fb():
        _lib.check(lib.sapr_connected_posteriors(
            _lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), _lib.ptr(lm),
            _lib.ptr(lm_start), _lib.ptr(lm_end), W, S, _lib.ptr(ws), ws_loop, _lib.ptr(den_ll), None, None,
            _lib.ptr(post), _lib.current_stream()), "sapr_connected_posteriors")

    def den_stats():
        _lib.check(lib.sapr_connected_loop_stats(
            _lib.ptr(post), _lib.ptr(feats), D, _lib.ptr(offs), N, total, None, W, S, _lib.ptr(ws2), ws_stats,
            _lib.ptr(den), _lib.current_stream()), "sapr_connected_loop_stats")

    def mmi():
        embed(D)
        loop_fb()
        den_stats()

    # (loop_fb stands before den_stats: the statistics are timed on the posteriors of this very logb)
    routes = {"fb": lambda: embed(0), "estep": lambda: embed(D), "loop_fb": loop_fb, "den_stats": den_stats,
              "mmi": mmi}
    read_bytes = total * (8 * net.R + 4 * D)
    facts = {"R": net.R, "columns": 2 * D + 1, "post_GB": round(total * net.R * 8 / 1e9, 3),
             "den_stats_read_bytes_per_frame": 8 * net.R + 4 * D,
             "read_once_at_hbm_peak_ms": round(read_bytes / HBM_PEAK_GBS / 1e6, 3),
             "partial_rows": int(ws_stats // (8 * net.R * (2 * D + 1))),
             "loop_stats_workspace_GB": round(ws_stats / 1e9, 3), "loop_workspace_GB": round(ws_loop / 1e9, 3),
             "embed_workspace_GB": round(ws_embed / 1e9, 3)}
    return routes, facts, loglik, den_ll, stats[D], den


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, loglik, den_ll, num, den = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        warm(routes)
        torch.cuda.synchronize()
        assert torch.isfinite(loglik).all() and torch.isfinite(den_ll).all() and bool((loglik <= den_ll + 1e-6).all())
        head = 2 + S + S * S
        assert float(den[0, 0]) == N and abs(float(den[:, head:head + S].sum()) / (N * T) - 1.0) < 1e-9
        assert abs(float(num[:, head:head + S].sum()) / (N * T) - 1.0) < 1e-9
        out["mean_log_posterior_of_the_transcript"] = round(float((loglik - den_ll).mean()), 4)
        times = timed_rounds(routes, REPEATS)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        reduction = med["estep"] - med["fb"]
        out["numerator_reduction_ms_median"] = round(reduction, 3)
        out["den_stats_over_numerator_reduction"] = round(med["den_stats"] / reduction, 2)
        out["den_stats_over_read_once"] = round(med["den_stats"] / facts["read_once_at_hbm_peak_ms"], 2)
        out["den_stats_GBps"] = round(facts["den_stats_read_bytes_per_frame"] * N * T / med["den_stats"] / 1e6, 1)
        out["mmi_over_estep"] = round(med["mmi"] / med["estep"], 2)
        print(json.dumps(out), flush=True)
        del routes, loglik, den_ll, num, den
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap, trace=False)
    measure(ap.parse_args())


if __name__ == "__main__":
    main()

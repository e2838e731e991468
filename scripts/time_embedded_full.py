"""Ad-hoc timing of the second-moment pass of embedded Baum-Welch (dev tool):
    python scripts/time_embedded_full.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--trace DIR]
The batch of scripts/time_embedded.py: N utterances x 505 frames (five words of ~101 frames in a row), bidiagonal word
models, exits in the last state, diagonal-Gaussian emissions; in one run, on the same logb and utterances:
  fb        sapr_connected_embed, statistics with D = 0            forward + backward kernel + the fold of narrow rows
  diag      sapr_connected_embed, statistics with the features     ... + embed_obs_kernel and the fold of {obs, obs**2}
  full      sapr_connected_embed_full                              fb + embed_full_accum_kernel + embed_full_fold_kernel
  iso       sapr_full_estep over the same frames cut into N * 5 one-word utterances under their own word model
  iso_ll    ... without the statistics (the forward kernel only)   iso - iso_ll: backward kernel + full_accum_kernel + reduction
Every route is warmed twice, then the routes are timed in turn, five times each, between device events.  Prints one
JSON line per shape: min / max / median of every route; the new pass on its own as full - fb, the diagonal observation
sums as diag - fb and the isolated-word backward + accumulation passes as iso - iso_ll (medians; full_accum_kernel on
its own is a line of the kernel trace below); the bytes of statistics each writes per word model, and the time per
byte.

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of every route per shape) and writes DIR/embedded_full_rocprofv3_summary.txt."""
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
    from sapr_amd import _lib, connected, full_cov
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
    ws_embed = connected.embed_workspace_bytes(total, N, total_words, WORDS, S, D)
    ws_full = connected.embed_full_workspace_bytes(total, N, total_words, WORDS, W, S, D)
    ws = torch.empty(max(ws_embed, ws_full), dtype=torch.uint8, device="cuda")
    loglik = torch.empty(N, dtype=torch.float64, device="cuda")
    stats = {d: torch.empty((W, connected.embed_stats_width(S, d)), dtype=torch.float64, device="cuda") for d in (0, D)}
    stats_full = torch.empty((W, connected.embed_full_stats_width(S, D)), dtype=torch.float64, device="cuda")

    def embed(d, want_stats):
        _lib.check(lib.sapr_connected_embed(
            _lib.ptr(logb), _lib.ptr(feats) if d else None, d, _lib.ptr(offs), N, total, _lib.ptr(words),
            _lib.ptr(woffs), total_words, WORDS, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws),
            ws_embed, _lib.ptr(loglik), _lib.ptr(stats[d]) if want_stats else None, None, _lib.current_stream()),
            "sapr_connected_embed")

    def full():
        _lib.check(lib.sapr_connected_embed_full(
            _lib.ptr(logb), _lib.ptr(feats), D, _lib.ptr(offs), N, total, _lib.ptr(words), _lib.ptr(woffs),
            total_words, WORDS, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws), ws_full,
            _lib.ptr(loglik), _lib.ptr(stats_full), None, _lib.current_stream()), "sapr_connected_embed_full")

    # the same frames as N * 5 one-word utterances under the full-covariance E-step of their own word model (the
    # diagonal variances as diagonal matrices: the accumulation pass does not look at them)
    with np.errstate(divide="ignore"):
        params = [(np.exp(model["log_start"][w]), np.exp(model["log_trans"][w]), model["means"][w],
                   np.array([np.diag(v) for v in model["vars"][w]])) for w in range(W)]
    pack = full_cov.FullPack.from_params(params)
    seg = np.diff(np.minimum(np.arange(WORDS + 1) * ((T + WORDS - 1) // WORDS), T))
    iso = pack.batch(feats, np.tile(seg, N), spoken.reshape(-1).cpu().numpy())
    routes = {"fb": lambda: embed(0, True), "diag": lambda: embed(D, True), "full": full,
              "iso": lambda: iso.estep(pack, want_stats=True), "iso_ll": lambda: iso.estep(pack, want_stats=False)}
    facts = {"R": net.R, "chain_positions": WORDS * net.SP, "groups": -(-N // max(8, -(-N // 96))),
             "diag_stats_bytes_per_word": 8 * 2 * S * D, "full_stats_bytes_per_word": 8 * (S * D + S * D * D),
             "embed_workspace_GB": round(ws_embed / 1e9, 3), "embed_full_workspace_GB": round(ws_full / 1e9, 3)}
    return routes, facts, loglik, stats[D], stats_full


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, loglik, stats, stats_full = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        warm(routes, args.child)
        torch.cuda.synchronize()
        assert torch.isfinite(loglik).all() and torch.isfinite(stats_full).all()
        assert float(stats[:, 0].sum()) == float(stats_full[:, 0].sum()) == N * WORDS
        head = 2 + S + S * S + S
        assert torch.equal(stats[:, :head], stats_full[:, :head])
        obs_err = float((stats[:, head:head + S * D] - stats_full[:, head:head + S * D]).abs().max())
        out["obs_max_abs_difference_diag_vs_full"] = obs_err
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        new, old, acc = med["full"] - med["fb"], med["diag"] - med["fb"], med["iso"] - med["iso_ll"]
        out["second_moment_pass_ms_median"] = round(new, 3)
        out["diag_observation_sums_ms_median"] = round(old, 3)
        out["isolated_backward_and_accumulation_ms_median"] = round(acc, 3)
        out["second_moment_pass_over_diag_sums"] = round(new / old, 2)
        out["ns_per_stat_byte_diag"] = round(old * 1e6 / (W * facts["diag_stats_bytes_per_word"]), 2)
        out["ns_per_stat_byte_full"] = round(new * 1e6 / (W * facts["full_stats_bytes_per_word"]), 2)
        print(json.dumps(out), flush=True)
        del routes, loglik, stats, stats_full
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
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_embedded_full.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (sapr_connected_embed at D = 0 and with the features,",
        "# sapr_connected_embed_full, sapr_full_estep with and without statistics over the same frames) per shape;",
        "# sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "embedded_full_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

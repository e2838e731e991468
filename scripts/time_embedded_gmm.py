"""Ad-hoc timing of the mixture-statistics pass of embedded Baum-Welch (dev tool):
    python scripts/time_embedded_gmm.py [N] [--frames 505] [--shapes 11,10,2,13 11,18,2,39] [--trace DIR]
The batch of scripts/time_embedded.py: N utterances x 505 frames (five words of ~101 frames in a row), bidiagonal word
models, exits in the last state, here with Gaussian-mixture emissions (tests/_connected_family_cases.gmm_case's
parameters); in one run, on the same logb and utterances:
  fb        sapr_connected_embed, statistics with D = 0            forward + backward kernel + the fold of narrow rows
  diag      sapr_connected_embed, statistics with the features     ... + embed_obs_kernel and the fold of {obs, obs**2}
  gmm       sapr_connected_embed_gmm                               fb + embed_gmm_accum_kernel + embed_full_fold_kernel
  iso       sapr_gmm_estep_diag over the same frames cut into N * 5 one-word utterances under their own word model
  iso_ll    ... without the statistics (emission + forward)        iso - iso_ll: backward + gmm_accum_kernel + reductions
Every route is warmed twice, then the routes are timed in turn, five times each, between device events.  Prints one
JSON line per shape: min / max / median of every route; the new pass with its fold as gmm - fb, embed_obs_kernel with
its fold on the same gamma as diag - fb and the isolated-word backward + accumulation passes as iso - iso_ll (medians;
gmm_accum_kernel on its own is a line of the kernel trace below).

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of every route per shape) and writes DIR/embedded_gmm_rocprofv3_summary.txt."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, summary, timed_rounds, trace_run, warm, write_summary

REPEATS = 5
WORDS = 5


def setup(args, W, S, M, D):
    import torch
    from sapr_amd import _lib, connected, gmm_hmm
    from tests._connected_family_cases import gmm_case
    N, T = args.N, args.frames
    model, _, _ = gmm_case(7, W, S, M, D, 0)
    pack = gmm_hmm.GmmPack.from_params([(model["startprob"][w], model["transmat"][w], model["weights"][w],
                                         model["means"][w], model["covars"][w]) for w in range(W)])
    net = connected.ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, family="gmm",
                                     pack=pack)
    # five words in a row per utterance, every frame scattered about the mean of a component (drawn by the weights) of
    # the state it walks through
    torch.manual_seed(0)
    per = (T + WORDS - 1) // WORDS
    t = torch.arange(T, device="cuda")
    spoken = torch.randint(0, W, (N, WORDS), device="cuda")
    word = spoken[:, (t // per).clamp(max=WORDS - 1)].reshape(-1)                              # [N * T]
    state = ((t % per) * S // per).expand(N, T).reshape(-1)
    comp = torch.multinomial(torch.from_numpy(model["weights"]).cuda()[word, state], 1).reshape(-1)
    mu = torch.from_numpy(model["means"]).cuda()[word, state, comp]
    sd = torch.from_numpy(np.sqrt(model["covars"])).cuda()[word, state, comp]
    feats = (mu + torch.randn(N * T, D, device="cuda", dtype=torch.float64) * sd).float().contiguous()
    del mu, sd, word, state, comp
    total, total_words = N * T, N * WORDS
    offs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * T
    woffs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * WORDS
    words = spoken.to(torch.int32).reshape(-1).contiguous()
    lib = _lib.load()
    ls, lt, lx, dpack = net.device(feats.device)
    logb = connected.emit_gmm(feats, net)
    ws_embed = connected.embed_workspace_bytes(total, N, total_words, WORDS, S, D)
    ws_gmm = connected.embed_gmm_workspace_bytes(total, N, total_words, WORDS, W, S, M, D)
    ws = torch.empty(max(ws_embed, ws_gmm), dtype=torch.uint8, device="cuda")
    loglik = torch.empty(N, dtype=torch.float64, device="cuda")
    stats = {d: torch.empty((W, connected.embed_stats_width(S, d)), dtype=torch.float64, device="cuda") for d in (0, D)}
    stats_gmm = torch.empty((W, connected.embed_gmm_stats_width(S, M, D)), dtype=torch.float64, device="cuda")

    def embed(d, want_stats):
        _lib.check(lib.sapr_connected_embed(
            _lib.ptr(logb), _lib.ptr(feats) if d else None, d, _lib.ptr(offs), N, total, _lib.ptr(words),
            _lib.ptr(woffs), total_words, WORDS, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws),
            ws_embed, _lib.ptr(loglik), _lib.ptr(stats[d]) if want_stats else None, None, _lib.current_stream()),
            "sapr_connected_embed")

    def mix():
        _lib.check(lib.sapr_connected_embed_gmm(
            _lib.ptr(logb), _lib.ptr(feats), D, _lib.ptr(dpack), M, _lib.ptr(offs), N, total, _lib.ptr(words),
            _lib.ptr(woffs), total_words, WORDS, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws),
            ws_gmm, _lib.ptr(loglik), _lib.ptr(stats_gmm), None, _lib.current_stream()), "sapr_connected_embed_gmm")

    # the same frames as N * 5 one-word utterances under the mixture E-step of their own word model
    seg = np.diff(np.minimum(np.arange(WORDS + 1) * per, T))
    iso = pack.batch(feats, np.tile(seg, N), spoken.reshape(-1).cpu().numpy())
    routes = {"fb": lambda: embed(0, True), "diag": lambda: embed(D, True), "gmm": mix,
              "iso": lambda: iso.estep(pack, want_stats=True), "iso_ll": lambda: iso.estep(pack, want_stats=False)}
    facts = {"R": net.R, "chain_positions": WORDS * net.SP, "groups": -(-N // max(8, -(-N // 96))),
             "diag_stats_bytes_per_word": 8 * 2 * S * D, "gmm_stats_bytes_per_word": 8 * S * M * (2 * D + 1),
             "embed_workspace_GB": round(ws_embed / 1e9, 3), "embed_gmm_workspace_GB": round(ws_gmm / 1e9, 3)}
    return routes, facts, loglik, stats[D], stats_gmm


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, M, D = (int(v) for v in shape.split(","))
        routes, facts, loglik, stats, stats_gmm = setup(args, W, S, M, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "M": M, "D": D, "words": WORDS}, **facts}
        warm(routes, args.child)
        torch.cuda.synchronize()
        assert torch.isfinite(loglik).all() and torch.isfinite(stats_gmm).all()
        assert float(stats[:, 0].sum()) == float(stats_gmm[:, 0].sum()) == N * WORDS
        head = 2 + S + S * S + S
        assert torch.equal(stats[:, :head], stats_gmm[:, :head])
        # the components' shares add up to the single-Gaussian sums of the same gamma
        mixed = stats_gmm[:, head + S * M:].reshape(W, 2, S, M, D).sum(dim=3).reshape(W, -1)
        rel = (mixed - stats[:, head:]).abs() / (1.0 + stats[:, head:].abs())
        out["obs_max_scaled_difference_summed_components_vs_diag"] = float(rel.max())
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        new, old, acc = med["gmm"] - med["fb"], med["diag"] - med["fb"], med["iso"] - med["iso_ll"]
        out["mixture_pass_ms_median"] = round(new, 3)
        out["diag_observation_sums_ms_median"] = round(old, 3)
        out["isolated_backward_and_accumulation_ms_median"] = round(acc, 3)
        out["mixture_pass_over_diag_sums"] = round(new / old, 2)
        out["mixture_pass_over_isolated_backward_and_accumulation"] = round(new / acc, 2)
        print(json.dumps(out), flush=True)
        del routes, loglik, stats, stats_gmm
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap, ("11,10,2,13", "11,18,2,39"), "W,S,M,D")
    args = ap.parse_args()
    measure(args)
    if args.child or not args.trace:
        return
    argv = [str(args.N), "--frames", str(args.frames), "--shapes", *args.shapes]
    header = [
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_embedded_gmm.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (sapr_connected_embed at D = 0 and with the features,",
        "# sapr_connected_embed_gmm, sapr_gmm_estep_diag with and without statistics over the same frames) per shape;",
        "# sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "embedded_gmm_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

"""Ad-hoc timing of the lattice posteriors against the word loop's forward-backward (dev tool):
    python scripts/time_lattice_posteriors.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--trace DIR]
The batch of scripts/time_lattice.py (N utterances x 505 frames, five words in a row, bidiagonal word models,
diagonal-Gaussian emissions, the add-one smoothed bigram of the spoken strings); in one process, on the same logb:
  emit            sapr_connected_emit_diag                              the stage every route shares
  search          sapr_connected_bigram with every output               the decoded path whose segments are scored
  lattice         sapr_connected_lattice                                the forward tables X, N, B
  lat_backward    sapr_connected_lattice_backward, own tables           the max-semiring pass, for comparison
  lat_post        sapr_connected_lattice_posteriors, own tables         forward + backward + posterior pass
  lat_post_second ... under bigram.scaled(1.5, -2.0)                    one more pass for another weight and penalty
  loop_post       sapr_connected_posteriors (loglik + word_post)        the exact forward-backward over the word loop
  loop_post_second ... under the second bigram                          what a second set of tables costs there
Every route is warmed once, then the routes are timed in turn, twice each, between device events.  Prints one JSON line
per shape: min / max of every route, the ratios, and how far the lattice confidence of the decoded segments (the mean
of word_post over a segment's frames) lies from the word loop's: max and mean absolute difference.

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own,
no counters: one warm-up and one timed call of every route per shape) and writes
DIR/lattice_posteriors_rocprofv3_summary.txt — the only place the three kernels behind lat_post are timed apart."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import COLUMNS, common_arguments, kernel_rows, row_lines, timed_rounds, trace_command, word_batch

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
    sizes = {"bigram": connected.bigram_workspace_bytes(total, N, W, S),
             "lattice": connected.lattice_workspace_bytes(total, N, W, S),
             "lat_post": connected.lattice_posteriors_workspace_bytes(total, N, W, S),
             "loop_post": connected.posteriors_workspace_bytes(total, N, W, S)}
    ws = {k: torch.empty(max(v, 1), dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")   # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")     # noqa: E731
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device="cuda")      # noqa: E731
    score, lat_score, root, final, n_words, first = f64(N), f64(N), f64(N), i32(N), i32(N), i32(N, 2)
    beta, next_end, next_word = f64(total, W), i32(total, W), u8(total, W)
    pw, ps, pe = i32(total), i32(total), u8(total)
    loglik = {k: f64(N) for k in ("lat", "lat_second", "loop", "loop_second")}
    record_post = f64(total, W)
    word_post = {k: f64(total, W) for k in ("lat", "loop")}
    scratch_post = f64(total, W)        # the second-table passes write here: the comparison reads the first
    st = _lib.current_stream
    p = _lib.ptr

    def emit():
        _lib.check(lib.sapr_connected_emit_diag(p(feats), total, D, p(ops), W, S, p(logb), st()),
                   "sapr_connected_emit_diag")

    def search():
        _lib.check(lib.sapr_connected_bigram(p(logb), p(offs), N, total, p(ls), p(lt), p(lx), *(p(a) for a in lm1), W,
                                             S, p(ws["bigram"]), sizes["bigram"], p(score), p(n_words), p(pw), p(ps),
                                             p(pe), st()), "sapr_connected_bigram")

    def lattice():
        _lib.check(lib.sapr_connected_lattice(p(logb), p(offs), N, total, p(ls), p(lt), p(lx), *(p(a) for a in lm1), W,
                                              S, p(ws["lattice"]), sizes["lattice"], p(lat_score), p(final), st()),
                   "sapr_connected_lattice")

    def lat_backward():
        _lib.check(lib.sapr_connected_lattice_backward(p(offs), N, total, W, S, p(ws["lattice"]), sizes["lattice"],
                                                       p(lm1[1]), *(p(a) for a in lm1), p(beta), p(next_end),
                                                       p(next_word), p(root), p(first), st()),
                   "sapr_connected_lattice_backward")

    def lat_post(lm, key, out):
        _lib.check(lib.sapr_connected_lattice_posteriors(p(offs), N, total, W, S, p(ws["lattice"]), sizes["lattice"],
                                                         p(lm1[1]), *(p(a) for a in lm), 1.0, None, p(ws["lat_post"]),
                                                         sizes["lat_post"], p(loglik[key]), p(record_post), p(out),
                                                         st()), "sapr_connected_lattice_posteriors")

    def loop_post(lm, key, out):
        _lib.check(lib.sapr_connected_posteriors(p(logb), p(offs), N, total, p(ls), p(lt), p(lx),
                                                 *(p(a) for a in lm), W, S, p(ws["loop_post"]), sizes["loop_post"],
                                                 p(loglik[key]), p(out), None, None, st()),
                   "sapr_connected_posteriors")

    routes = {"emit": emit, "search": search, "lattice": lattice, "lat_backward": lat_backward,
              "lat_post": lambda: lat_post(lm1, "lat", word_post["lat"]),
              "lat_post_second": lambda: lat_post(lm2, "lat_second", scratch_post),
              "loop_post": lambda: loop_post(lm1, "loop", word_post["loop"]),
              "loop_post_second": lambda: loop_post(lm2, "loop_second", scratch_post)}
    facts = {"R": net.R, "logb_GB": round(total * net.R * 8 / 1e9, 3),
             "lattice_tables_GB": round(sizes["lattice"] / 1e9, 3),
             "lat_post_workspace_GB": round(sizes["lat_post"] / 1e9, 3),
             "loop_post_workspace_GB": round(sizes["loop_post"] / 1e9, 3),
             "lat_post_bytes_per_frame": {"read": 20 * W, "scratch": 32 * W, "written": 16 * W}}
    state = dict(score=score, lat_score=lat_score, root=root, loglik=loglik, word_post=word_post, pw=pw, pe=pe,
                 record_post=record_post)
    return routes, facts, state


def segment_confidences(word_post, pw, pe):
    """The mean of ``word_post[f, path_word[f]]`` over every decoded segment of the batch, on the device."""
    import torch
    seg = torch.cumsum(pe.to(torch.int64), 0) - 1      # (every utterance has a path: its first frame begins a word)
    per_frame = word_post.gather(1, pw.to(torch.int64).clamp(min=0)[:, None])[:, 0]
    n = int(seg.max()) + 1
    total = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, seg, per_frame)
    count = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, seg, torch.ones_like(per_frame))
    return total / count


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, s = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, **facts}
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        assert torch.isfinite(s["score"]).all()
        assert s["lat_score"].cpu().numpy().tobytes() == s["score"].cpu().numpy().tobytes()
        ll = s["loglik"]
        assert torch.isfinite(ll["lat"]).all() and torch.isfinite(ll["loop"]).all()
        slack = 4 * T * 2.0 ** -52 * float(s["score"].abs().max()) * 4
        assert bool((ll["lat"] >= s["root"] - slack).all())          # the sum is not below the best lattice path
        assert bool((ll["loop"] >= ll["lat"] - slack).all())         # ... and the loop sums over more paths
        rows = s["word_post"]["lat"].sum(dim=1)
        out["lat_word_post_row_sum_max_error"] = float((rows - 1.0).abs().max())
        out["loglik_loop_minus_lattice"] = {"mean": round(float((ll["loop"] - ll["lat"]).mean()), 4),
                                            "max": round(float((ll["loop"] - ll["lat"]).max()), 4)}
        c_lat = segment_confidences(s["word_post"]["lat"], s["pw"], s["pe"])
        c_loop = segment_confidences(s["word_post"]["loop"], s["pw"], s["pe"])
        diff = (c_lat - c_loop).abs()
        out["segments"] = int(diff.numel())
        out["confidence_abs_difference"] = {"max": round(float(diff.max()), 6), "mean": round(float(diff.mean()), 6)}
        out["mean_confidence"] = {"lattice": round(float(c_lat.mean()), 6), "loop": round(float(c_loop.mean()), 6)}
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = {"min": round(min(t), 3), "max": round(max(t), 3)}
        best = {k: min(t) for k, t in times.items()}
        out["ratio_lattice_plus_post_over_loop_post"] = round((best["lattice"] + best["lat_post"]) / best["loop_post"], 3)
        out["ratio_lat_post_over_lat_backward"] = round(best["lat_post"] / best["lat_backward"], 3)
        out["ratio_second_lat_post_over_second_loop_post"] = round(best["lat_post_second"] / best["loop_post_second"], 3)
        print(json.dumps(out), flush=True)
        del routes, s
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap)
    args = ap.parse_args()
    measure(args)
    if args.child or not args.trace:
        return
    # (one run under rocprofv3 per shape, so that the tables of the two shapes stay apart)
    os.makedirs(args.trace, exist_ok=True)
    lines = ["# rocprofv3 --kernel-trace --stats (no counters), one run per shape of:",
             f"#   python scripts/time_lattice_posteriors.py {args.N} --frames {args.frames} --shapes W,S,D --child",
             "# one warm-up and one timed call of every route (emission; bigram search; the lattice's forward tables; its",
             "# max-semiring backward pass; the lattice posteriors under two bigrams; the word loop's forward-backward under",
             "# two bigrams); sapr kernels only"]
    for shape in args.shapes:
        trace = os.path.join(args.trace, "trace_" + shape.replace(",", "_"))
        cmd = trace_command(__file__, [str(args.N), "--frames", str(args.frames), "--shapes", shape], trace)
        with open(os.path.join(args.trace, "child.log"), "a") as log:
            subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, timeout=600)
        lines += [f"# (W, S, D) = ({shape})", COLUMNS, *row_lines(kernel_rows(trace))]
    with open(os.path.join(args.trace, "lattice_posteriors_rocprofv3_summary.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

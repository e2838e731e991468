"""Ad-hoc timing of connected-word recognition (dev tool):
    python scripts/time_connected.py [N] [--frames 505] [--families diag gmm full] [--shapes 11,10,13 11,18,39]
                                     [--gmm-shapes 11,10,2,13 11,18,2,39] [--full-shapes 11,10,13 11,18,39] [--trace DIR]
The two stages and the back-trace of sapr_amd.connected on N utterances x 505 frames (five words of ~101 frames in a
row), bidiagonal word models, exits in the last state, for every emission family: diagonal Gaussians at
(W, S, D) = (11, 10, 13) and (11, 18, 39), mixtures at (W, S, M, D) = (11, 10, 2, 13) and (11, 18, 2, 39), full
covariances (odd words tied) at (W, S, D) = (11, 10, 13) and (11, 18, 39):
  emit       sapr_connected_emit_diag / _gmm / _full            logb[total_frames][W * SP]
  viterbi    sapr_connected_viterbi without any path output    (the recursion kernel alone)
  decode     sapr_connected_viterbi with every output          (recursion + back-trace; back-trace = decode - viterbi)
and a yardstick on the same frames in the same run: for the diagonal family the all-vocabulary isolated-word scorer
sapr_viterbi_diag_scores (+ its back-trace launch, trellis.viterbi_decode without a path); for the other two the
per-model decoder (sapr_gmm_viterbi_diag / sapr_full_viterbi) of every utterance under ONE word, whose frame-parallel
emission kernel (gmm_emit_kernel / full_emit_kernel) does the arithmetic of one word of the connected emission: its
time from the kernel trace, times W, is what the connected emission kernel is compared with.  Every route is warmed
twice, then the routes are timed in turn, five times each, between device events.  Prints one JSON line per family
and shape with the bytes each stage moves and the float64 operations it needs from the shapes alone: per frame and
flat state 3 D + 2 (diag), M (4 D + 1) plus the log-sum-exp (gmm), 3 D (D + 1) / 2 + 2 D + 2 (full) for the emission, and
per finite transition distance one add and one compare in the recursion.

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of every route per shape) and writes DIR/connected_rocprofv3_summary.txt, which ends
with the yardstick comparison: connected emission kernel against W x the per-model emission kernel."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, summary, timed_rounds, trace_run, warm, word_batch, write_summary

REPEATS = 5


def setup(args, family, shape):
    import torch
    from sapr_amd import _lib, connected
    from sapr_amd.trellis import DiagModelPack, FeatureBatch, viterbi_decode
    from tests import _connected_family_cases as cases
    from tests._connected_ref import sample_case
    N, T = args.N, args.frames
    W, S, D = shape[0], shape[1], shape[-1]
    if family == "diag":
        model, _, _ = sample_case(7, W, S, D, 0)
        net = connected.ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, None,
                                         model["means"], model["vars"], model["gconst"])
        centres, spread = model["means"], np.sqrt(model["vars"])
    else:
        model, _, _ = cases.gmm_case(7, *shape, 0) if family == "gmm" else cases.full_case(7, *shape, 0)
        net = connected.ConnectedNetwork.from_models(cases.models_of(family, model))
        # (timing only: the frames lie about the first component's mean / the state's mean, a few units wide)
        centres = model["means"][:, :, 0] if family == "gmm" else model["means"]
        spread = np.sqrt(model["covars"][:, :, 0]) if family == "gmm" else np.full(centres.shape, 3.0)
    feats = word_batch(centres, spread, N, T)[0]
    lengths = np.full(N, T)
    offs = torch.from_numpy(np.r_[0, np.cumsum(lengths)].astype(np.int64)).cuda()
    total = N * T
    lib = _lib.load()
    ls, lt, lx, ops = net.device(feats.device)
    logb = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    ws_bytes = connected.workspace_bytes(total, N, W, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    score = torch.empty(N, dtype=torch.float64, device="cuda")
    n_words = torch.empty(N, dtype=torch.int32, device="cuda")
    pw = torch.empty(total, dtype=torch.int32, device="cuda")
    ps = torch.empty(total, dtype=torch.int32, device="cuda")
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")

    def emit():
        name = f"sapr_connected_emit_{family}"
        extra = (net.pack.M,) if family == "gmm" else ()
        _lib.check(getattr(lib, name)(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, *extra, _lib.ptr(logb),
                                      _lib.current_stream()), name)

    def viterbi(paths):
        out = (n_words, pw, ps, pe) if paths else (None,) * 4
        _lib.check(lib.sapr_connected_viterbi(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                              _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws), ws_bytes, _lib.ptr(score),
                                              *(_lib.ptr(o) for o in out), _lib.current_stream()),
                   "sapr_connected_viterbi")

    routes = {"emit": emit, "viterbi": lambda: viterbi(False), "decode": lambda: viterbi(True)}
    DP = net.DP
    if family == "diag":
        pack = DiagModelPack.from_params(model["startprob"], model["transmat"], model["means"], model["vars"])
        fb = FeatureBatch.from_packed(feats, lengths)
        routes["isolated_word_scores"] = lambda: viterbi_decode(fb, pack, want_path=False)
        state_flops = 3 * DP + 2
    else:
        one_word = net.pack.batch(feats, lengths, np.zeros(N, dtype=np.int64))   # every utterance under word 0
        routes["per_model_viterbi_one_word"] = lambda: one_word.viterbi(net.pack)
        MP = {1: 1, 2: 2, 3: 4, 4: 4}.get(net.pack.M, 8) if family == "gmm" else 0
        state_flops = MP * (4 * DP + 1) if family == "gmm" else 3 * DP * (DP + 1) // 2 + 2 * DP + 2
    nd = 2  # finite transition distances of a bidiagonal vocabulary
    facts = {"R": net.R, "logb_GB": round(total * net.R * 8 / 1e9, 3), "workspace_GB": round(ws_bytes / 1e9, 3),
             "emit_bytes_per_frame": 4 * D + 8 * net.R, "viterbi_bytes_per_frame": 9 * net.R + 4,
             "emit_flops_per_frame": net.R * state_flops, "viterbi_flops_per_frame": net.R * (2 * nd + 5)}
    return routes, facts, (n_words, score)


def family_shapes(args):
    given = {"diag": args.shapes, "gmm": args.gmm_shapes, "full": args.full_shapes}
    return [(f, tuple(int(v) for v in s.split(","))) for f in args.families for s in given[f]]


def measure(args):
    import torch
    N, T = args.N, args.frames
    for family, shape in family_shapes(args):
        routes, facts, (n_words, score) = setup(args, family, shape)
        names = ("W", "S", "M", "D") if family == "gmm" else ("W", "S", "D")
        out = {"family": family, "shape": {"N": N, "T": T, **dict(zip(names, shape))}, **facts}
        warm(routes, args.child)
        torch.cuda.synchronize()
        assert torch.isfinite(score).all()
        out["mean_words_found"] = round(float(n_words.float().mean()), 2)
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        out["backtrace_ms_median"] = round(med["decode"] - med["viterbi"], 3)
        out["connected_total_ms_median"] = round(med["emit"] + med["decode"], 3)
        if "isolated_word_scores" in med:
            out["ratio_connected_over_isolated"] = round((med["emit"] + med["decode"]) / med["isolated_word_scores"], 3)
        out["emit_GBps"] = round(facts["emit_bytes_per_frame"] * N * T / med["emit"] / 1e6, 1)
        out["viterbi_GBps"] = round(facts["viterbi_bytes_per_frame"] * N * T / med["viterbi"] / 1e6, 1)
        print(json.dumps(out), flush=True)
        del routes, n_words, score
        torch.cuda.empty_cache()


def kernel_avg_ms(rows, kernel, targs):
    """Average duration of the instantiation ``kernel<targs>`` (the name without its namespace and arguments)."""
    for r in rows:
        if f"{kernel}<{targs}>".replace(" ", "") in r["Name"].replace(" ", ""):
            return float(r["AverageNs"]) / 1e6
    return None


def yardstick_lines(args, rows):
    lines = ["# yardstick: connected emission kernel against W x the per-model emission kernel of the same arithmetic"]
    for family, shape in family_shapes(args):
        if family == "diag":
            continue
        DP = 13 if shape[-1] <= 13 else (26 if shape[-1] <= 26 else 39)
        targs = f"{ {1: 1, 2: 2, 3: 4, 4: 4}.get(shape[2], 8)}, {DP}" if family == "gmm" else f"{DP}"
        new = kernel_avg_ms(rows, f"connected_emit_{family}_kernel", targs)
        old = kernel_avg_ms(rows, f"{family}_emit_kernel", targs)
        if new is None or old is None:
            lines.append(f"# {family} {shape}: kernels not found in the trace")
            continue
        lines.append(f"# {family} {shape}: connected_emit_{family}_kernel<{targs}> {new:.3f} ms, "
                     f"{family}_emit_kernel<{targs}> {old:.3f} ms x W = {old * shape[0]:.3f} ms, "
                     f"ratio {new / (old * shape[0]):.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap, shapes_help="W,S,D of the diagonal family")
    ap.add_argument("--families", nargs="+", default=["diag", "gmm", "full"], choices=["diag", "gmm", "full"])
    ap.add_argument("--gmm-shapes", nargs="+", default=["11,10,2,13", "11,18,2,39"], help="W,S,M,D")
    ap.add_argument("--full-shapes", nargs="+", default=["11,10,13", "11,18,39"], help="W,S,D")
    args = ap.parse_args()
    measure(args)
    if args.child or not args.trace:
        return
    argv = [str(args.N), "--frames", str(args.frames), "--families", *args.families, "--shapes", *args.shapes,
            "--gmm-shapes", *args.gmm_shapes, "--full-shapes", *args.full_shapes]
    header = [
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_connected.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of every route (emission; recursion alone; recursion + back-trace; the",
        "# yardstick on the same frames: the all-vocabulary isolated-word scorer (diag), the per-model decoder under",
        "# one word (gmm, full)) per family and shape; sapr kernels only",
    ]
    rows = trace_run(__file__, argv, args.trace, 900)
    write_summary(os.path.join(args.trace, "connected_rocprofv3_summary.txt"), header, rows, yardstick_lines(args, rows))


if __name__ == "__main__":
    main()

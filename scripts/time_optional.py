"""Ad-hoc timing of optional transcript slots in forced alignment and the embedded E-step (dev tool):
    python scripts/time_optional.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--trace DIR]
N utterances x 505 frames (five words of ~101 frames in a row, the batch of scripts/time_align.py and
scripts/time_embedded.py), bidiagonal word models, exits in the last state, diagonal-Gaussian emissions; word 0 serves
as the silence.  In one run, on the same emitted logb, four chains:
  words5      sapr_connected_align / sapr_connected_embed over the five words           (a) the kernels without flags
  null5       the _opt entry points with optional = NULL over the five words            (b) must be (a)
  opt11       the _opt entry points over the 11 slots sil? w sil? w ... sil?            (c) the OPT kernels
  explicit11  the entry points without flags over the same 11 slots, all mandatory      (d) the yardstick for (c)
and for each of them the routes
  align       the alignment recursion alone          align_path  ... with the back-trace
  forward     the forward kernel (loglik only)       fb          forward + backward + the fold of narrow rows (D = 0)
  estep       the whole E-step with the features
(the recordings hold no pauses: opt11 steps over its silences, explicit11 has to press frames into them).  Every route
is warmed twice, then the routes are timed in turn, three times each, between device events.  Prints one JSON line
per shape: min / max / median of every route and the ratios (b) / (a), (c) / (d), (c) / (a).

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own:
one warm-up and one timed call of the opt11 routes per shape) and writes DIR/optional_rocprofv3_summary.txt."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, summary, timed_rounds, trace_run, warm, word_batch, write_summary

REPEATS = 3
WORDS = 5
SLOTS = 2 * WORDS + 1


def setup(args, W, S, D):
    import torch
    from sapr_amd import _lib, connected
    from tests._connected_ref import sample_case
    N, T = args.N, args.frames
    model, _, _ = sample_case(7, W, S, D, 0)
    net = connected.ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, None,
                                     model["means"], model["vars"], model["gconst"])
    feats, spoken = word_batch(model["means"], np.sqrt(model["vars"]), N, T, WORDS)
    total = N * T
    offs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * T
    lib = _lib.load()
    ls, lt, lx, ops = net.device(feats.device)
    logb = torch.empty((total, net.R), dtype=torch.float64, device="cuda")
    _lib.check(lib.sapr_connected_emit_diag(_lib.ptr(feats), total, D, _lib.ptr(ops), W, S, _lib.ptr(logb),
                                            _lib.current_stream()), "sapr_connected_emit_diag")
    # the two transcripts: the five words, and the 11 slots with the silence (word 0) around every word
    words5 = spoken.to(torch.int32).reshape(-1).contiguous()
    slots = torch.zeros((N, SLOTS), dtype=torch.int32, device="cuda")
    slots[:, 1::2] = spoken.to(torch.int32)
    words11 = slots.reshape(-1).contiguous()
    flags11 = torch.zeros((N, SLOTS), dtype=torch.uint8, device="cuda")
    flags11[:, 0::2] = 1
    flags11 = flags11.reshape(-1).contiguous()
    woffs = {K: torch.arange(N + 1, device="cuda", dtype=torch.int64) * K for K in (WORDS, SLOTS)}
    ws_bytes = max(connected.align_opt_workspace_bytes(total, N, SLOTS, S),
                   connected.embed_workspace_bytes(total, N, N * SLOTS, SLOTS, S, D))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    pw = torch.empty(total, dtype=torch.int32, device="cuda")
    ps = torch.empty(total, dtype=torch.int32, device="cuda")
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")
    start = torch.empty(N * SLOTS, dtype=torch.int32, device="cuda")
    stats = {d: torch.empty((W, connected.embed_stats_width(S, d)), dtype=torch.float64, device="cuda") for d in (0, D)}
    # chain: (words, slots per utterance, the _opt entry points?, flags)
    chains = {"words5": (words5, WORDS, False, None), "null5": (words5, WORDS, True, None),
              "opt11": (words11, SLOTS, True, flags11), "explicit11": (words11, SLOTS, False, None)}
    score = {c: torch.empty(N, dtype=torch.float64, device="cuda") for c in chains}
    loglik = {c: torch.empty(N, dtype=torch.float64, device="cuda") for c in chains}

    def align(chain, paths):
        wd, K, opt, flags = chains[chain]
        out = (pw, ps, pe, start) if paths else (None,) * 4
        head = (_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(wd), _lib.ptr(woffs[K]))
        tail = (N * K, K, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws), ws_bytes,
                _lib.ptr(score[chain]), *(_lib.ptr(o) for o in out), _lib.current_stream())
        if opt:
            _lib.check(lib.sapr_connected_align_opt(*head, _lib.ptr(flags), *tail), "sapr_connected_align_opt")
        else:
            _lib.check(lib.sapr_connected_align(*head, *tail), "sapr_connected_align")

    def embed(chain, d, want_stats):
        wd, K, opt, flags = chains[chain]
        head = (_lib.ptr(logb), _lib.ptr(feats) if d else None, d, _lib.ptr(offs), N, total, _lib.ptr(wd),
                _lib.ptr(woffs[K]))
        tail = (N * K, K, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), 0.0, W, S, _lib.ptr(ws), ws_bytes,
                _lib.ptr(loglik[chain]), _lib.ptr(stats[d]) if want_stats else None, None, _lib.current_stream())
        if opt:
            _lib.check(lib.sapr_connected_embed_opt(*head, _lib.ptr(flags), *tail), "sapr_connected_embed_opt")
        else:
            _lib.check(lib.sapr_connected_embed(*head, *tail), "sapr_connected_embed")

    routes = {}
    for c in (["opt11"] if args.child else chains):
        routes[f"{c}.align"] = lambda c=c: align(c, False)
        routes[f"{c}.align_path"] = lambda c=c: align(c, True)
        routes[f"{c}.forward"] = lambda c=c: embed(c, 0, False)
        routes[f"{c}.fb"] = lambda c=c: embed(c, 0, True)
        routes[f"{c}.estep"] = lambda c=c: embed(c, D, True)
    facts = {"R": net.R, "SP": net.SP, "chain_positions": {"words5": WORDS * net.SP, "slots11": SLOTS * net.SP},
             "logb_GB": round(total * net.R * 8 / 1e9, 3), "workspace_GB": round(ws_bytes / 1e9, 3)}
    return routes, facts, score, loglik, start


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        routes, facts, score, loglik, start = setup(args, W, S, D)
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS, "slots": SLOTS}, **facts}
        warm(routes, args.child)
        torch.cuda.synchronize()
        assert torch.isfinite(score["opt11"]).all() and torch.isfinite(loglik["opt11"]).all()
        if not args.child:
            assert score["words5"].cpu().numpy().tobytes() == score["null5"].cpu().numpy().tobytes()
            assert loglik["words5"].cpu().numpy().tobytes() == loglik["null5"].cpu().numpy().tobytes()
            # stepping over every silence is one of the paths of opt11; pressing frames into six silences costs
            assert bool((score["opt11"] >= score["words5"]).all()) and bool((score["opt11"] >= score["explicit11"]).all())
            out["opt11_score_equals_words5_score"] = round(float((score["opt11"] == score["words5"]).float().mean()), 4)
            out["mean_score_opt11_minus_explicit11"] = round(float((score["opt11"] - score["explicit11"]).mean()), 2)
        routes["opt11.align_path"]()
        torch.cuda.synchronize()
        out["mean_silences_taken_by_opt11"] = round(float((start.reshape(N, SLOTS)[:, 0::2] >= 0).float().sum(1).mean()), 3)
        times = timed_rounds(routes, REPEATS, args.child)
        for k, t in times.items():
            out[f"{k}_ms"] = summary(t)
        med = {k: float(np.median(t)) for k, t in times.items()}
        if not args.child:
            for r in ("align", "align_path", "forward", "fb", "estep"):
                out[f"{r}_ratios"] = {"null5_over_words5": round(med[f"null5.{r}"] / med[f"words5.{r}"], 3),
                                      "opt11_over_explicit11": round(med[f"opt11.{r}"] / med[f"explicit11.{r}"], 3),
                                      "opt11_over_words5": round(med[f"opt11.{r}"] / med[f"words5.{r}"], 3),
                                      "explicit11_over_words5": round(med[f"explicit11.{r}"] / med[f"words5.{r}"], 3)}
            for c in ("words5", "opt11", "explicit11"):
                out[f"{c}.backward_ms_median"] = round(med[f"{c}.fb"] - med[f"{c}.forward"], 3)
        print(json.dumps(out), flush=True)
        del routes, score, loglik, start
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
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_optional.py {' '.join(argv)} --child",
        "# one warm-up and one timed call of the opt11 routes (11 slots sil? w ... sil?: alignment recursion alone and",
        "# with its back-trace; forward; forward + backward + fold; whole E-step) per shape, and one more alignment with",
        "# its back-trace; sapr kernels only",
    ]
    write_summary(os.path.join(args.trace, "optional_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

"""Ad-hoc timing of online connected-word decoding against the offline decoder (dev tool):
    python scripts/time_online.py [N] [--frames 505] [--shapes 11,10,13 11,18,39] [--chunks 10 50 505] [--trace DIR]
N streams x 505 frames (five words of ~101 frames in a row, the batch of scripts/time_bigram.py), bidiagonal word
models, exits in the last state, diagonal-Gaussian emissions, the add-one smoothed bigram of the spoken strings; in one
process, on the same logb:
  offline      sapr_connected_bigram with every output           recursion + back-trace over the whole recordings
  online       per chunk size: sapr_connected_online_step and sapr_connected_online_commit for every chunk of every
               stream, then the flush — each launch timed on its own between device events and the times added up
               (the chunk rows are gathered into a packed buffer outside the timed region: a live caller emits them
               there in the first place)
The window is 256 frames, or chunk + 256 where a chunk is longer than 64 frames.  Two runs of everything; prints one JSON
line per shape with min - max of the offline time and, per chunk size, of the total step time and the total commit time,
their ratio to the offline time, and the commit latency in frames (frames consumed minus frames final, after every
commit: mean and maximum over streams and pushes) with the frames committed by force.  The first run also checks the
online scores against the offline ones by bytes and the concatenated word path where nothing was forced.

--trace DIR: afterwards the script starts itself once more under rocprofv3 --kernel-trace --stats (a run of its own,
one pass) and writes DIR/online_rocprofv3_summary.txt."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from _timing import common_arguments, ev_time, span, trace_run, word_batch, write_summary

RUNS = 2
WORDS = 5


def setup(args, W, S, D):
    """The batch of scripts/time_bigram.py and its emitted logb."""
    import torch
    from sapr_amd import connected
    from tests._connected_ref import sample_case
    N, T = args.N, args.frames
    model, _, _ = sample_case(7, W, S, D, 0)
    feats, spoken = word_batch(model["means"], np.sqrt(model["vars"]), N, T, WORDS)
    bigram = connected.WordBigram.from_transcripts(spoken.cpu().numpy(), W)
    net = connected.ConnectedNetwork(model["log_start"], model["log_trans"], model["log_exit"], 0.0, None,
                                     model["means"], model["vars"], model["gconst"], bigram=bigram)
    return net, connected.emit_diag(feats, net)


def offline(net, logb, N, T):
    """``(run, outputs)``: one sapr_connected_bigram with every output over the whole batch."""
    import torch
    from sapr_amd import _lib, connected
    lib, total = _lib.load(), N * T
    offs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * T
    ls, lt, lx, _ = net.device(logb.device)
    lm, lm_start, lm_end = net._dev_lm
    ws_bytes = connected.bigram_workspace_bytes(total, N, net.W, net.S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    score = torch.empty(N, dtype=torch.float64, device="cuda")
    n_words = torch.empty(N, dtype=torch.int32, device="cuda")
    pw, ps = (torch.empty(total, dtype=torch.int32, device="cuda") for _ in range(2))
    pe = torch.empty(total, dtype=torch.uint8, device="cuda")

    def run():
        _lib.check(lib.sapr_connected_bigram(_lib.ptr(logb), _lib.ptr(offs), N, total, _lib.ptr(ls), _lib.ptr(lt),
                                             _lib.ptr(lx), _lib.ptr(lm), _lib.ptr(lm_start), _lib.ptr(lm_end), net.W,
                                             net.S, _lib.ptr(ws), ws_bytes, _lib.ptr(score), _lib.ptr(n_words),
                                             _lib.ptr(pw), _lib.ptr(ps), _lib.ptr(pe), _lib.current_stream()),
                   "sapr_connected_bigram")
    return run, (score, n_words, pw)


def online(net, logb, N, T, chunk, want=None):
    """One pass over the batch in chunks of ``chunk`` frames: ``(step_ms, commit_ms, latency mean, max, forced)``;
    ``want``: the offline ``(score, n_words, path_word)`` to check against."""
    import torch
    from sapr_amd import _lib, connected
    lib = _lib.load()
    window = 256 if chunk <= 64 else chunk + 256
    ls, lt, lx, _ = net.device(logb.device)
    lm, lm_start, lm_end = net._dev_lm
    nbytes = connected.online_state_bytes(N, net.W, net.S, window)
    state = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    n_new, first = i32(N), torch.empty(N, dtype=torch.int64, device="cuda")
    ow, os_, oe = i32(N, window), i32(N, window), torch.empty((N, window), dtype=torch.uint8, device="cuda")
    score, n_words = torch.empty(N, dtype=torch.float64, device="cuda"), i32(N)
    forced = torch.empty(N, dtype=torch.int64, device="cuda")
    trunc = torch.empty(N, dtype=torch.uint8, device="cuda")
    flush = torch.ones(N, dtype=torch.uint8, device="cuda")
    path = torch.full((N, T), -2, dtype=torch.int32, device="cuda") if want is not None else None
    col = torch.arange(window, device="cuda")
    view = logb.view(N, T, net.R)

    def commit(fl):
        _lib.check(lib.sapr_connected_online_commit(N, net.W, net.S, window, chunk, _lib.ptr(state), nbytes, fl,
                                                    _lib.ptr(n_new), _lib.ptr(first), _lib.ptr(ow), _lib.ptr(os_),
                                                    _lib.ptr(oe), _lib.ptr(score), _lib.ptr(n_words), _lib.ptr(forced),
                                                    None, None, None, None, _lib.current_stream()),
                   "sapr_connected_online_commit")

    def keep():
        if path is not None:
            mask = col[None, :] < n_new[:, None]
            rows = torch.arange(N, device="cuda")[:, None].expand(N, window)[mask]
            path[rows, (first[:, None] + col[None, :])[mask]] = ow[mask]

    step_ms = commit_ms = 0.0
    lat_sum, lat_max, pushes = 0.0, 0, 0
    for a in range(0, T, chunk):
        n = min(chunk, T - a)
        rows = view[:, a:a + n].contiguous()                 # (outside the timed region)
        offs = torch.arange(N + 1, device="cuda", dtype=torch.int64) * n
        step_ms += ev_time(lambda: _lib.check(lib.sapr_connected_online_step(
            _lib.ptr(rows), _lib.ptr(offs), N, N * n, _lib.ptr(ls), _lib.ptr(lt), _lib.ptr(lx), _lib.ptr(lm),
            _lib.ptr(lm_start), _lib.ptr(lm_end), net.W, net.S, window, chunk, _lib.ptr(state), nbytes, None,
            _lib.ptr(trunc), _lib.current_stream()), "sapr_connected_online_step"))
        commit_ms += ev_time(lambda: commit(None))
        keep()
        lat = (a + n) - (first + n_new)
        lat_sum, lat_max, pushes = lat_sum + float(lat.float().mean()), max(lat_max, int(lat.max())), pushes + 1
    assert not bool(trunc.any())
    commit_ms += ev_time(lambda: commit(_lib.ptr(flush)))
    keep()
    if want is not None:
        assert torch.equal(score.view(torch.int64), want[0].view(torch.int64)), "online scores differ from offline"
        clean = forced == 0
        assert torch.equal(n_words[clean], want[1][clean])
        assert torch.equal(path[clean], want[2].view(N, T)[clean]), "online paths differ from offline"
    return step_ms, commit_ms, lat_sum / pushes, lat_max, int(forced.sum())


def measure(args):
    import torch
    N, T = args.N, args.frames
    for shape in args.shapes:
        W, S, D = (int(v) for v in shape.split(","))
        net, logb = setup(args, W, S, D)
        run, want = offline(net, logb, N, T)
        run()
        torch.cuda.synchronize()
        out = {"shape": {"N": N, "T": T, "W": W, "S": S, "D": D, "words": WORDS}, "R": net.R}
        runs = 1 if args.child else RUNS
        off = [ev_time(run) for _ in range(runs)]
        out["offline_ms"] = span(off)
        for chunk in args.chunks:
            res = [online(net, logb, N, T, chunk, want if k == 0 else None) for k in range(runs)]
            step, com = [r[0] for r in res], [r[1] for r in res]
            out[f"chunk_{chunk}"] = {
                "window": 256 if chunk <= 64 else chunk + 256, "pushes": (T + chunk - 1) // chunk,
                "step_ms": span(step), "commit_ms": span(com),
                "ratio_to_offline": span([(s + c) / o for s, c, o in zip(step, com, off)]),
                "latency_frames_mean": round(res[0][2], 2), "latency_frames_max": res[0][3], "forced": res[0][4]}
        print(json.dumps(out), flush=True)
        del logb, run, want
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    common_arguments(ap)
    ap.add_argument("--chunks", nargs="+", type=int, default=[10, 50, 505])
    args = ap.parse_args()
    measure(args)
    if args.child or not args.trace:
        return
    argv = [str(args.N), "--frames", str(args.frames), "--shapes", *args.shapes,
            "--chunks", *(str(c) for c in args.chunks)]
    header = [
        f"# rocprofv3 --kernel-trace --stats of: python scripts/time_online.py {' '.join(argv)} --child",
        "# one pass: emission, one offline decode (recursion + back-trace) and, per chunk size, the step and the commit of",
        "# every chunk and the flush, per shape; sapr kernels only (no counters are collected in this run)",
    ]
    write_summary(os.path.join(args.trace, "online_rocprofv3_summary.txt"), header,
                  trace_run(__file__, argv, args.trace, 900))


if __name__ == "__main__":
    main()

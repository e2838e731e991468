"""What the scripts/time_*.py route scripts share: the device-event timer, the summaries they print, the five-word
batch, the warm-up and the timed rounds, and the run of their own under rocprofv3 with its summary file.  Imported as
``from _timing import ...`` (a script's own directory is first on sys.path); torch is imported where it is used, so
that importing this module, or a script's --help, needs no device."""
import csv
import glob
import os
import statistics
import subprocess
import sys

COLUMNS = "# calls  total_ms  avg_ms  min_ms  max_ms  name"


def ev_time(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(t):
    return {"min": round(min(t), 3), "max": round(max(t), 3), "median": round(float(statistics.median(t)), 3)}


def span(t):
    return [round(min(t), 3), round(max(t), 3)]


def common_arguments(ap, shapes=("11,10,13", "11,18,39"), shapes_help="W,S,D", trace=True):
    """N, --frames and --shapes, and with ``trace`` the two flags of the run under rocprofv3."""
    ap.add_argument("N", nargs="?", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=505)
    ap.add_argument("--shapes", nargs="+", default=list(shapes), help=shapes_help)
    if trace:
        ap.add_argument("--trace", default=None, help="directory for the rocprofv3 summary (a second run of its own)")
        ap.add_argument("--child", action="store_true", help="(internal) the run under rocprofv3")


def word_batch(means, sd, N, T, words=5, device="cuda"):
    """``(feats[N * T, D] float32, spoken[N, words])``: ``words`` words in a row per utterance, the frames scattered
    about the means[W, S, D] of the states they walk through, ``sd`` wide.  (The generator is seeded here, and
    ``spoken`` is drawn before the frames: the batch is the same in every script.)"""
    import torch
    S, D = means.shape[1], means.shape[2]
    torch.manual_seed(0)
    per = (T + words - 1) // words
    t = torch.arange(T, device=device)
    spoken = torch.randint(0, means.shape[0], (N, words), device=device)
    word = spoken[:, (t // per).clamp(max=words - 1)]                                          # [N, T]
    state = ((t % per) * S // per).expand(N, T)
    mu = torch.from_numpy(means).to(device)[word.reshape(-1), state.reshape(-1)]
    sd = torch.from_numpy(sd).to(device)[word.reshape(-1), state.reshape(-1)]
    feats = (mu + torch.randn(N * T, D, device=device, dtype=torch.float64) * sd).float().contiguous()
    return feats, spoken


def warm(routes, child=False):
    """Every route in turn, twice (once in the run under rocprofv3)."""
    for _ in range(1 if child else 2):
        for fn in routes.values():
            fn()


def timed_rounds(routes, repeats, child=False, timer=ev_time):
    """``{route: [ms, ...]}``: the routes timed in turn, ``repeats`` times each (once in the run under rocprofv3)."""
    times = {k: [] for k in routes}
    for _ in range(1 if child else repeats):
        for k, fn in routes.items():
            times[k].append(timer(fn))
    return times


def trace_command(script, argv, trace_dir):
    return ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--", sys.executable,
            os.path.abspath(script), *argv, "--child"]


def kernel_rows(trace_dir):
    """The sapr kernels of the kernel statistics under ``trace_dir``, the longest total first."""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "sapr" in r["Name"]]
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    return rows


def row_lines(rows):
    return ["%5s %9.3f %8.3f %8.3f %8.3f  %s" % (r["Calls"], float(r["TotalDurationNs"]) / 1e6,
                                                 float(r["AverageNs"]) / 1e6, float(r["MinNs"]) / 1e6,
                                                 float(r["MaxNs"]) / 1e6, r["Name"]) for r in rows]


def trace_run(script, argv, out_dir, timeout):
    """Starts ``script argv --child`` as a fresh process under rocprofv3 --kernel-trace --stats (output in
    ``out_dir``/child.log, the trace in ``out_dir``/trace) and returns its ``kernel_rows``."""
    os.makedirs(out_dir, exist_ok=True)
    trace_dir = os.path.join(out_dir, "trace")
    with open(os.path.join(out_dir, "child.log"), "w") as log:
        subprocess.run(trace_command(script, argv, trace_dir), check=True, stdout=log, stderr=subprocess.STDOUT,
                       stdin=subprocess.DEVNULL, timeout=timeout)
    return kernel_rows(trace_dir)


def write_summary(path, header, rows, tail=()):
    """Writes and prints the script's ``header`` lines, the kernel table and the script's ``tail`` lines."""
    lines = [*header, COLUMNS, *row_lines(rows), *tail]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))

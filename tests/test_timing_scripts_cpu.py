"""scripts/_timing.py, the harness behind the scripts/time_*.py tools, without a device: the summaries, the order of
the warm-up and the timed rounds, the five-word batch's index arithmetic, the rocprofv3 command and the summary file;
and the scripts themselves as far as they go without one: every script compiles and imports only names the harness
has, --help of every script that has a command-line parser, and an import of the converted ones that neither parses
arguments nor loads torch."""
import ast
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)
import _timing  # noqa: E402

ALL = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(SCRIPTS, "time_*.py")))
# the scripts with a command line of their own; the one-off scripts read sys.argv[1] as a number (or nothing at all, as
# time_pipe39.py does) and go straight to the device, so "--help" means nothing to them and must not be tried here
WITH_PARSER = [n for n in ALL if "argparse" in open(os.path.join(SCRIPTS, n + ".py")).read()]
CONVERTED = ["time_align", "time_bigram", "time_connected", "time_embedded", "time_embedded_full", "time_embedded_gmm",
             "time_full_vocab", "time_fullcov", "time_lattice", "time_lattice_posteriors", "time_levels", "time_mmi",
             "time_nbest", "time_online", "time_optional", "time_posteriors"]
HELPERS_ONLY = ["time_forward_vocab", "time_gmm_vocab", "time_gmmhmm", "time_kmeans", "time_state_posteriors"]


def test_summary_and_span():
    assert _timing.summary([3.0, 1.0, 2.0]) == {"min": 1.0, "max": 3.0, "median": 2.0}
    assert list(_timing.summary([3.0, 1.0, 2.0])) == ["min", "max", "median"]
    assert _timing.summary([1.0004, 2.0006]) == {"min": 1.0, "max": 2.001, "median": 1.5}
    assert _timing.span([3.0, 1.0, 2.0]) == [1.0, 3.0]
    assert _timing.span([1.23449, 0.5]) == [0.5, 1.234]


@pytest.mark.parametrize("child", [False, True])
def test_routes_are_warmed_and_timed_in_turn(child):
    calls = []
    routes = {k: (lambda k=k: calls.append(("run", k))) for k in "ABC"}

    def timer(fn):
        calls.append("timed")
        fn()
        return float(len(calls))

    _timing.warm(routes, child)
    warm_rounds = 1 if child else 2
    assert calls == [("run", k) for k in "ABC"] * warm_rounds
    del calls[:]
    times = _timing.timed_rounds(routes, 4, child, timer=timer)
    rounds = 1 if child else 4
    assert calls == [x for k in "ABC" * rounds for x in ("timed", ("run", k))]      # A B C A B C ..., never A A A
    assert list(times) == ["A", "B", "C"] and all(len(t) == rounds for t in times.values())
    assert times["A"][0] < times["B"][0] < times["C"][0] and (child or times["C"][0] < times["A"][1])


def test_word_batch_walks_the_states_of_the_spoken_words():
    N, T, W, S, D, words = 3, 11, 3, 4, 2, 5
    means = np.arange(W * S * D, dtype=np.float64).reshape(W, S, D) * 0.5 + 1.0
    feats, spoken = _timing.word_batch(means, np.zeros((W, S, D)), N, T, words, device="cpu")
    import torch
    assert feats.dtype == torch.float32 and feats.is_contiguous() and tuple(feats.shape) == (N * T, D)
    assert tuple(spoken.shape) == (N, words) and int(spoken.min()) >= 0 and int(spoken.max()) < W
    spoken, feats = spoken.numpy(), feats.numpy().reshape(N, T, D)
    per = -(-T // words)
    for n in range(N):
        for t in range(T):
            want = means[spoken[n, min(t // per, words - 1)], (t % per) * S // per]
            np.testing.assert_array_equal(feats[n, t], want.astype(np.float32))
    again, spoken2 = _timing.word_batch(means, np.zeros((W, S, D)), N, T, words, device="cpu")     # seeded inside
    np.testing.assert_array_equal(spoken2.numpy(), spoken)
    np.testing.assert_array_equal(again.numpy().reshape(N, T, D), feats)


STATS = """"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"
"void sapr::small_kernel<13>(double const*)",4,2000000,500000,10.0,400000,600000,1.0
"at::native::vectorized_elementwise_kernel<4>",9,9000000000,1000000000,80.0,1,2,1.0
"void sapr::big_kernel(int)",12,123456789,10288065.75,10.0,9000000,20000000,1.0
"""


def test_summary_file_keeps_the_project_kernels_longest_first(tmp_path, capsys):
    sub = tmp_path / "trace" / "host" / "1234_kernel_stats.csv"
    sub.parent.mkdir(parents=True)
    sub.write_text(STATS)
    rows = _timing.kernel_rows(str(tmp_path / "trace"))
    assert [r["Name"] for r in rows] == ["void sapr::big_kernel(int)", "void sapr::small_kernel<13>(double const*)"]
    out = tmp_path / "x_rocprofv3_summary.txt"
    _timing.write_summary(str(out), ["# first", "# second"], rows, ["# after"])
    want = ["# first", "# second", "# calls  total_ms  avg_ms  min_ms  max_ms  name",
            "%5s %9.3f %8.3f %8.3f %8.3f  %s" % ("12", 123.456789, 10.28806575, 9.0, 20.0,
                                                 "void sapr::big_kernel(int)"),
            "    4     2.000    0.500    0.400    0.600  void sapr::small_kernel<13>(double const*)",
            "# after"]
    assert want[3] == "   12   123.457   10.288    9.000   20.000  void sapr::big_kernel(int)"
    assert out.read_text() == "\n".join(want) + "\n"
    assert capsys.readouterr().out == "\n".join(want) + "\n"


def test_trace_command_is_a_kernel_trace_of_a_fresh_child():
    cmd = _timing.trace_command("scripts/time_align.py", ["1000", "--frames", "505", "--shapes", "11,10,13"], "d/trace")
    assert cmd[:7] == ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", "d/trace"]
    assert cmd[7] == "--" and cmd.index("--") == 7
    assert cmd[8:10] == [sys.executable, os.path.abspath("scripts/time_align.py")]
    assert cmd[10:] == ["1000", "--frames", "505", "--shapes", "11,10,13", "--child"]
    assert [a for a in cmd[1:7] if a.startswith("-")] == ["--kernel-trace", "--stats", "--output-format", "-d"]


@pytest.mark.parametrize("name", ALL)
def test_script_compiles_and_takes_only_what_the_harness_has(name):
    """Every script, those without a parser too (time_forward_vocab.py takes ev_time from the harness and is started by
    no test: it goes straight to the device)."""
    path = os.path.join(SCRIPTS, name + ".py")
    tree = ast.parse(open(path).read(), path)
    compile(tree, path, "exec")
    taken = [a.name for node in ast.walk(tree) if isinstance(node, ast.ImportFrom) and node.module == "_timing"
             for a in node.names]
    assert all(hasattr(_timing, n) for n in taken), taken
    if name in CONVERTED + HELPERS_ONLY:
        assert "ev_time" in taken or "timed_rounds" in taken
        assert not any(isinstance(node, ast.FunctionDef) and node.name == "ev_time" for node in ast.walk(tree))


def test_every_converted_script_has_a_parser():
    assert set(CONVERTED) <= set(WITH_PARSER) and len(CONVERTED) == 16


@pytest.mark.parametrize("name", WITH_PARSER)
def test_help_exits_clean(name):
    out = subprocess.run([sys.executable, os.path.join("scripts", name + ".py"), "--help"], cwd=ROOT,
                         capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]


IMPORT_PROBE = """
import importlib, sys
sys.path.insert(0, "scripts")
sys.argv = ["probe", "--no-such-option"]
for name in %r:
    importlib.import_module(name)
    assert callable(getattr(sys.modules[name], "main")), name
    assert "torch" not in sys.modules and "sapr_amd" not in sys.modules, name
"""


def test_importing_a_converted_script_parses_nothing_and_loads_no_torch():
    out = subprocess.run([sys.executable, "-c", IMPORT_PROBE % (CONVERTED,)], cwd=ROOT, capture_output=True, text=True,
                         stdin=subprocess.DEVNULL, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]

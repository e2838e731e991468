"""Every scripts/time_*.py tool on the shared harness runs to its end at the smallest shape at which its own
assertions still mean something, and prints the JSON lines it promises: 8 utterances of 55 frames (five words of 11
frames: 5 S <= T, so that the word chain has a path), (W, S, D) = (3, 4, 2), M = 2 for the mixtures, two values for
every list option (time_mmi.py at 700 utterances, the fewest at which the fact it divides by is not rounded to zero);
the two vocabulary scripts at 64 utterances and (D, S) = (2, 4).  No run under rocprofv3 here:
time_fullcov.py, which has no run without one, is started as its own --child."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["8", "--frames", "55", "--shapes", "3,4,2"]
CASES = {
    "time_align": SMALL,
    "time_bigram": SMALL,
    "time_connected": [*SMALL, "--gmm-shapes", "3,4,2,2", "--full-shapes", "3,4,2"],
    "time_embedded": SMALL,
    "time_embedded_full": SMALL,
    "time_embedded_gmm": ["8", "--frames", "55", "--shapes", "3,4,2,2"],
    "time_full_vocab": ["64", "--shapes", "2,4"],
    "time_fullcov": ["64", "--shapes", "2,4", "--child"],
    "time_lattice": SMALL,
    "time_lattice_posteriors": SMALL,
    "time_levels": [*SMALL, "--levels", "1", "2"],
    # 700 utterances: the script divides by its fact read_once_at_hbm_peak_ms, (8 R + 4 D) N T bytes at 8 TB/s rounded
    # to a microsecond; at R = 12, D = 2, T = 55 that is 0.0 below 38 462 frames
    "time_mmi": ["700", "--frames", "55", "--shapes", "3,4,2"],
    "time_nbest": [*SMALL, "--depths", "1", "2"],
    "time_online": [*SMALL, "--chunks", "10", "55"],
    "time_optional": SMALL,
    "time_posteriors": SMALL,
}


def _in_order(v):
    """A printed time: summary's {min, max, median}, the lattice scripts' {min, max}, or span's [min, max]."""
    if isinstance(v, list):
        return len(v) == 2 and 0 < v[0] <= v[1]
    return 0 < v["min"] <= v.get("median", v["min"]) <= v["max"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_script_runs_and_prints_its_json_lines(name):
    out = subprocess.run([sys.executable, os.path.join("scripts", name + ".py"), *CASES[name]], cwd=ROOT,
                         capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines, "no output"
    for ln in lines:
        d = json.loads(ln)
        assert isinstance(d["shape"], dict) and d["shape"]["N"] == int(CASES[name][0])
        times = [v for k, v in d.items() if k.endswith("_ms") and isinstance(v, (dict, list))]
        assert times and all(_in_order(v) for v in times), ln
        if name not in ("time_lattice", "time_lattice_posteriors", "time_online"):
            assert all("median" in v for v in times), ln
    n_lines = 3 if name == "time_connected" else 1
    assert len(lines) == n_lines

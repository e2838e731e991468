"""bench.py's plain run on one GPU: it times the steps it is given, prints only the headline fields, and
--dump-outputs writes the last timed step's results, the same files from run to run and from either decoder."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_UTTS, STEPS, T = 3000, 3, 101


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--utts", str(N_UTTS), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_the_same_outputs_every_time_and_for_either_decoder(tmp_path):
    runs = {k: _bench("--dump-outputs", str(tmp_path / k), *extra)
            for k, extra in (("a", []), ("b", []), ("full", ["--decode", "full"]))}
    for d in runs.values():
        assert d["steps"] == STEPS and d["ms_per_step"] > 0 and d["higher_is_better"] is True
        assert d["unit"] == "frames/s" and d["dtype"] == "f32 (MFCC) + f64 (trellis)"
        assert d["value"] == pytest.approx(N_UTTS * T / (d["ms_per_step"] * 1e-3), rel=1e-9)
        assert not {"roofline", "cpu_baseline", "cpu_baseline_all_cores", "extra"} & set(d)
    a, b, full = (_load(tmp_path / k) for k in ("a", "b", "full"))
    assert set(a) == {"best_word", "best_score", "path", "mfcc", "mfcc_utterances"}
    assert set(full) == set(a) | {"scores"}
    for x in (*a.values(), *full.values()):
        assert x.dtype in (np.float32, np.float64)
    assert a["best_word"].shape == a["best_score"].shape == (N_UTTS,) and a["path"].shape == (N_UTTS * T,)
    assert a["mfcc"].shape == (1024 * T, 13) and full["scores"].shape == (N_UTTS, 11)
    assert a["best_word"].min() >= 0 and a["best_word"].max() < 11 and np.isfinite(a["best_score"]).all()
    for k in a:   # seeded inputs: identical from run to run; the pruned decoder returns the all-vocabulary bits
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(a[k], full[k], err_msg=k)
    np.testing.assert_array_equal(full["scores"][np.arange(N_UTTS), a["best_word"].astype(int)], a["best_score"])

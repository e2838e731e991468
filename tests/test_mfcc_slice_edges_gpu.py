"""Slice pipeline of the wave-private MFCC core on a batch whose utterance lengths sit on the edges of both kernels.

Forced slice counts (SAPR_MFCC_SLICES in {1, 2, 3, 4}, read at plan creation) on a 40-utterance batch: an utterance
without samples and one of 100 samples (one frame each), 15 / 16 / 17 frames (the 16-frame tile of the finish pass),
101 frames, and 301 frames (19 tiles: with 40 utterances the finish pass cuts every utterance over 8 wavefronts), the
rest ragged.  The yardstick is the single launch of the same build, torch.equal; rows of `out` behind total_frames keep
their contents.

The batch goes through sapr_mfcc_batch itself: MfccPlan.__call__ refuses utterances of fewer than 9 frames for the
39-dimensional preset (their delta features are not defined).  What the device computes for a one-frame utterance is
still a fixed function of the utterance's own rows (its tile repeats the last row, the edge filters read that tile),
which is all this test asks."""
import contextlib
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOP = 160
SLICES = (1, 2, 3, 4)


@contextlib.contextmanager
def _slices(value):
    """SAPR_MFCC_SLICES=value while a plan is created (it is read at plan creation)."""
    old = os.environ.get("SAPR_MFCC_SLICES")
    os.environ["SAPR_MFCC_SLICES"] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SAPR_MFCC_SLICES", None)
        else:
            os.environ["SAPR_MFCC_SLICES"] = old


def _plan(preset, slices):
    from sapr_amd.frontend import BENCH, BENCH39, MfccPlan
    with _slices(slices):
        plan = MfccPlan(**{"bench": BENCH, "bench39": BENCH39}[preset], max_frames=0)
    assert plan.two_pass
    return plan


@functools.lru_cache(maxsize=None)
def _batch():
    """(pcm, sample offsets, frame offsets) of 40 utterances: no samples, 1 frame, 15 / 16 / 17 frames (the tile edge),
    101 frames, 301 frames (19 tiles: with 40 utterances the finish pass cuts every utterance over 8 wavefronts), the
    rest ragged between 9 and 100 frames; one all silent, one half silent (the top_db clip)."""
    rng = np.random.default_rng(3)
    edge = [0, 100, 14 * HOP, 15 * HOP + 7, 16 * HOP + 159, 16000, 48000]
    lens = np.asarray([int(v) for v in rng.integers(1440, 16000, 40 - len(edge))] + edge, dtype=np.int64)
    lens = lens[rng.permutation(40)]
    frames = 1 + lens // HOP
    assert {1, 15, 16, 17, 101, 301} <= set(frames.tolist()) and 0 in lens and len(lens) == 40
    sig = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in lens]
    big = [i for i in range(40) if lens[i] > 4000]
    sig[big[0]][:] = 0.0
    sig[big[1]][: lens[big[1]] // 2] = 0.0
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    return np.concatenate(sig), so, fo


PAD_ROWS, MARK = 64, 7.0


def _run(plan):
    """[total_frames + PAD_ROWS, d_out]: the features, then rows the call must leave alone."""
    import torch
    from sapr_amd import _lib
    lib = _lib.load()
    pcm, so, fo = _batch()
    n, total = len(so) - 1, int(fo[-1])
    pcm_d, so_d, fo_d = torch.from_numpy(pcm).cuda(), torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    out = torch.full((total + PAD_ROWS, plan.d_out), MARK, device="cuda")
    ws, ws_bytes = plan.workspace(total, n, pcm_d.device)
    _lib.check(lib.sapr_mfcc_batch(plan._h, _lib.ptr(pcm_d), _lib.ptr(so_d), _lib.ptr(fo_d), n, total, _lib.ptr(out), 0,
                                   _lib.ptr(ws), ws_bytes, _lib.current_stream()), "sapr_mfcc_batch")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _single(preset):
    import torch
    want = _run(_plan(preset, 1))
    total = int(_batch()[2][-1])
    assert bool(torch.isfinite(want[:total]).all()) and bool((want[total:] == MARK).all())
    return want


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("preset", ["bench", "bench39"])
def test_forced_slices_equal_the_single_launch(preset, slices):
    import torch
    want = _single(preset)
    got = _run(_plan(preset, slices))
    total = int(_batch()[2][-1])
    assert torch.equal(got[:total], want[:total]), f"{preset}: SAPR_MFCC_SLICES={slices} differs from the single launch"
    assert bool((got[total:] == MARK).all()), f"{preset}: SAPR_MFCC_SLICES={slices} wrote behind total_frames"

"""4-frame sets of the wave-private MFCC core are cut on the launch's frame numbering through ALL utterances
(mfcc_wave.h): a set may hold the last frames of one utterance and the first of the next ones — up to four utterances
when they are shorter than a set.  Which 16-lane group or which wavefront computes a frame must not change one bit
of its row, so the yardstick is the same build run on ONE utterance at a time: such a launch numbers its frames from
the utterance's first frame and has no set that spans two utterances.  Comparisons are torch.equal.

What this yardstick does and does not see: a solo launch goes through the same kernel, and when its frame count is no
multiple of four its last set is a boundary set too (idle groups behind the launch's last frame).  It pins down that
a row does not depend on the group, set, wavefront, grid or slice that computes it; an error COMMON to every placement
would pass it.  Against that stand the oracle comparison below (a handful of utterances, tests/test_mfcc_gpu.py's
tolerance) and, outside this file, the bench outputs, which are byte-identical to those of the build that cut sets per
utterance.

The solo launches go through the C ABI with pointers into the batch's buffers (an utterance of no samples has no
tensor of its own to point at).  Presets: the plain one and the pre-emphasised one without deltas go down to
utterances of 0 samples = 1 frame, so that one set spans three and four utterances in both instantiations of the
kernel; the 39-dimensional one takes utterances of 9 frames and more (delta features are undefined below,
MfccPlan.__call__)."""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import mfcc_oracle as mo

pytestmark = pytest.mark.gpu

ATOL, RMS = 1e-3, 1.5e-4   # tests/test_mfcc_gpu.py
HOP = 160
PRESETS = ("bench", "preemph", "bench39")


def _cfg(preset):
    from sapr_amd.frontend import BENCH, BENCH39
    return {"bench": BENCH, "preemph": dict(BENCH, preemph=0.97), "bench39": BENCH39}[preset]


def _ocfg(preset):
    return {"bench": mo.BENCH, "preemph": dict(mo.BENCH, preemph=0.97),
            "bench39": dict(mo.BENCH, preemph=0.97, deltas=True)}[preset]


@contextlib.contextmanager
def _slices(value):
    """SAPR_MFCC_SLICES=value while plans are created (it is read at plan creation)."""
    old = os.environ.get("SAPR_MFCC_SLICES")
    os.environ["SAPR_MFCC_SLICES"] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SAPR_MFCC_SLICES", None)
        else:
            os.environ["SAPR_MFCC_SLICES"] = old


def _plan(preset, slices=1):
    from sapr_amd.frontend import MfccPlan
    with _slices(slices):
        plan = MfccPlan(**_cfg(preset), max_frames=0)
    assert plan.two_pass
    return plan


def _lengths(preset):
    """Sample counts of ~200 utterances; T = 1 + n // 160 covers every residue mod 4."""
    rng = np.random.default_rng(7)
    if preset != "bench39":
        # runs of utterances of 1, 2 and 3 frames: one set spans three or four utterances
        tiny = [0, 159, 160, 319, 320, 479, 1, 0, 0, 0, 0, 200, 100, 400, 330, 5, 161, 478, 0, 321]
        small = [HOP * t + int(rng.integers(0, HOP)) for t in range(0, 12)]
    else:
        tiny = [HOP * t + int(rng.integers(0, HOP)) for t in (8, 9, 10, 8, 8, 9, 11, 10, 8, 9, 8, 8)]   # 9 .. 12 frames
        small = [HOP * t + int(rng.integers(0, HOP)) for t in range(8, 20)]
    around_100 = [15840, 15999, 16000, 16001, 16160, 16319, 16320, 16480, 16000, 16000]             # T = 100 .. 104
    ragged = [int(v) for v in rng.integers(1440, 9000, 160)]
    lens = ragged[:40] + tiny + ragged[40:80] + around_100[:5] + small + ragged[80:120] + tiny[::-1] + \
        around_100[5:] + ragged[120:]
    frames = 1 + np.asarray(lens) // HOP
    assert set(frames % 4) == {0, 1, 2, 3} and {100, 101, 102, 103, 104} <= set(frames)
    if preset != "bench39":
        assert {1, 2, 3} <= set(frames)
    return lens


@functools.lru_cache(maxsize=None)
def _batch(preset):
    """(signals, sample lengths): ragged utterances, some with zeroed edges or all silent (the top_db clip is active)."""
    lens = _lengths(preset)
    base = mo.synth_utterances(len(lens), n_samples=max(lens), sr=16000, seed=41)
    sig = [b[:n].copy() for b, n in zip(base, lens)]
    for i in range(3, len(sig), 9):     # zeroed edges
        n = len(sig[i])
        sig[i][: n // 3] = 0.0
        sig[i][n - n // 4:] = 0.0
    for i in (10, 47, 131):             # digital silence
        sig[i][:] = 0.0
    return sig, np.asarray(lens, dtype=np.int64)


def _run(plan, sig, lens, grid_blocks=0):
    import torch
    pcm = torch.from_numpy(np.concatenate(sig).astype(np.float32)).cuda()
    feats, frames = plan(pcm, lens, grid_blocks=grid_blocks)
    torch.cuda.synchronize()
    return feats, frames


def _solo(plan, sig, lens):
    """Every utterance in a launch of its own: [total_frames, d_out], the rows where the batch call puts them."""
    import ctypes as C
    import torch
    from sapr_amd import _lib
    from sapr_amd.frontend import num_frames
    lib = _lib.load()
    n = len(lens)
    frames = num_frames(lens, HOP).astype(np.int64)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    pcm = torch.from_numpy(np.concatenate(sig).astype(np.float32)).cuda()
    # one [0, length] pair per utterance: the solo call's offsets
    so_pairs = torch.from_numpy(np.stack([np.zeros(n, np.int64), lens], axis=1).copy()).cuda()
    fo_pairs = torch.from_numpy(np.stack([np.zeros(n, np.int64), frames], axis=1).copy()).cuda()
    out = torch.full((int(fo[-1]), plan.d_out), float("nan"), device="cuda")
    ws, ws_bytes = plan.workspace(int(frames.max()), 1, pcm.device)
    st = _lib.current_stream()
    for i in range(n):
        _lib.check(lib.sapr_mfcc_batch(plan._h, C.c_void_p(pcm.data_ptr() + 4 * int(so[i])),
                                       C.c_void_p(so_pairs.data_ptr() + 16 * i), C.c_void_p(fo_pairs.data_ptr() + 16 * i),
                                       1, int(frames[i]), C.c_void_p(out.data_ptr() + 4 * plan.d_out * int(fo[i])), 0,
                                       _lib.ptr(ws), ws_bytes, st), "sapr_mfcc_batch")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _reference(preset):
    """The batch of _batch(preset) by solo launches and by one launch of the whole batch (computed once)."""
    import torch
    sig, lens = _batch(preset)
    plan = _plan(preset, 1)
    solo = _solo(plan, sig, lens)
    whole, frames = _run(plan, sig, lens)
    assert bool(torch.isfinite(solo).all())
    return solo, whole, frames


@pytest.mark.parametrize("preset", PRESETS)
def test_ragged_batch_equals_solo_launches(preset):
    import torch
    solo, whole, frames = _reference(preset)
    assert whole.shape == solo.shape and whole.shape[0] == int(frames.sum())
    if not torch.equal(whole, solo):
        fo = np.concatenate([[0], np.cumsum(frames)])
        rows = torch.nonzero((whole != solo).any(dim=1)).flatten().cpu().numpy()
        utts = sorted(set(int(np.searchsorted(fo, r, side="right") - 1) for r in rows))
        raise AssertionError(f"{preset}: {len(rows)} rows differ from the solo launches, utterances {utts[:20]}")


@pytest.mark.parametrize("preset", PRESETS)
def test_ragged_batch_against_the_oracle(preset):
    sig, lens = _batch(preset)
    _, whole, frames = _reference(preset)
    whole = whole.cpu().numpy()
    fo = np.concatenate([[0], np.cumsum(frames)])
    # the first utterances of the tiny run, one around T = 100, one with zeroed edges, one silent, a ragged one
    picks = [40, 41, 42, 43, 100, 3, 10, 150]
    for i in picks:
        want = mo.mfcc(sig[i], **_ocfg(preset)).T
        got = whole[fo[i]:fo[i + 1]]
        assert got.shape == want.shape
        d = got.astype(np.float64) - want.astype(np.float64)
        assert np.abs(d).max() <= ATOL, (i, np.abs(d).max())
        assert np.sqrt((d ** 2).mean()) <= RMS, (i, np.sqrt((d ** 2).mean()))


@pytest.mark.parametrize("preset", PRESETS)
def test_forced_grids(preset):
    """Few workgroups: runs end inside utterances and next to sets that span utterances."""
    import torch
    sig, lens = _batch(preset)
    _, whole, _ = _reference(preset)
    plan = _plan(preset, 1)
    for g in (1, 2, 3, 7):
        got, _ = _run(plan, sig, lens, grid_blocks=g)
        assert torch.equal(got, whole), f"{preset}: grid_blocks={g} differs from the default grid"


@pytest.mark.parametrize("preset", PRESETS)
def test_forced_slices(preset):
    """Slices number their frames from their own first utterance; a cut behind an utterance whose frame count is no
    multiple of four ends the slice in a partial set."""
    import torch
    sig, lens = _batch(preset)
    _, whole, frames = _reference(preset)
    n = len(lens)
    fo = np.concatenate([[0], np.cumsum(frames)])
    partial = 0
    for s in (2, 3, 5):
        cuts = [n * k // s for k in range(s + 1)]
        partial += sum(int(fo[b] - fo[a]) % 4 != 0 for a, b in zip(cuts[:-1], cuts[1:]))
        got, _ = _run(_plan(preset, s), sig, lens)
        assert torch.equal(got, whole), f"{preset}: SAPR_MFCC_SLICES={s} differs from the single launch"
    assert partial > 0, "no slice of this batch ends in a partial set"


@pytest.mark.parametrize("preset", PRESETS)
def test_equal_utterances_of_101_frames(preset):
    """The benchmark's shape: T = 101 = 1 mod 4, three of four utterances start inside a set."""
    import torch
    n = 64
    base = mo.synth_utterances(n, n_samples=16000, sr=16000, seed=43)
    sig = [b.copy() for b in base]
    sig[5][:] = 0.0
    sig[6][:8000] = 0.0
    lens = np.full(n, 16000, dtype=np.int64)
    plan = _plan(preset, 1)
    whole, frames = _run(plan, sig, lens)
    assert int(frames[0]) == 101
    assert torch.equal(whole, _solo(plan, sig, lens))


def test_batches_beyond_the_32_bit_frame_counter_are_refused():
    """The kernel counts a launch's frames and utterances in 32 bits: sapr_mfcc_batch returns SAPR_ERR_ARG for
    2^31 - 16 of either (include/sapr_hip.h) before it looks at the workspace or launches anything."""
    import torch
    from sapr_amd import _lib
    lib = _lib.load()
    plan = _plan("bench", 1)
    pcm = torch.zeros(16, device="cuda")
    offs = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((4, plan.d_out), 7.0, device="cuda")
    ws = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    big = (1 << 31) - 16
    for n_utts, total in ((1, big), (big, 4)):
        rc = lib.sapr_mfcc_batch(plan._h, _lib.ptr(pcm), _lib.ptr(offs), _lib.ptr(offs), n_utts, total, _lib.ptr(out),
                                 0, _lib.ptr(ws), 4096, _lib.current_stream())
        assert rc == -1, rc    # SAPR_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0x5A).all())

"""The finish pass of the wave-private MFCC core has bodies specialised on the presets' shapes (mfcc_wave.h:
mfcc_wave_finish_kernel<10, false> for 40 mels without deltas, <10, true> with them) and a generic body for every other
plan.  SAPR_FINISH_GENERIC=1 at plan creation forces the generic body, which is the yardstick here: the specialised
body holds fewer float4 pieces per lane, walks 10 DCT K-steps instead of 16 and, without deltas, has no cepstra ring —
none of which may change one bit of a feature.  Comparisons are torch.equal, for BENCH and BENCH39, under
SAPR_MFCC_SLICES = 1 (single launch sequence) and 2 (slice pipeline).

Cases:
  ragged  ~40 utterances of 1, 2, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 95, 96, 97, 101, 112, 113 frames: the
          tile edge at 16 frames, the turn of the three-tile ring at 48, the delta filters' edge rows.  BENCH39 takes
          the counts from 9 up: delta features are undefined below 9 frames and MfccPlan.__call__ refuses them.
  split   three utterances, one of 2 001 frames: the finish launch runs split > 1, a wavefront starts in the middle of
          an utterance and, with deltas, transforms its neighbour tiles itself.
Content: three sinusoids plus noise (the generator of bench.synth_pcm); every third utterance with its first and last
100 ms zeroed, so the top_db clip is active; one utterance of all zeros; one at amplitude 1e4.

The ragged batch is also held against oracle/mfcc_oracle.py within the tolerance of tests/test_mfcc_gpu.py."""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import mfcc_oracle as mo

pytestmark = pytest.mark.gpu

ATOL, RMS = 1e-3, 1.5e-4   # tests/test_mfcc_gpu.py
HOP, SR = 160, 16000
PRESETS = ("bench", "bench39")
SLICES = (1, 2)
FRAMES = (1, 2, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 95, 96, 97, 101, 112, 113)


def _cfg(preset):
    from sapr_amd.frontend import BENCH, BENCH39
    return {"bench": BENCH, "bench39": BENCH39}[preset]


def _ocfg(preset):
    return {"bench": mo.BENCH, "bench39": dict(mo.BENCH, preemph=0.97, deltas=True)}[preset]


@contextlib.contextmanager
def _env(**values):
    """Environment while a plan is created (both switches are read at plan creation); None = unset."""
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _plan(preset, slices, generic):
    from sapr_amd.frontend import MfccPlan
    with _env(SAPR_MFCC_SLICES=slices, SAPR_FINISH_GENERIC=1 if generic else None):
        plan = MfccPlan(**_cfg(preset), max_frames=0)
    assert plan.two_pass
    return plan


def _frame_counts(case, preset):
    if case == "split":
        return [50, 2001, 101]
    counts = [t for t in FRAMES if preset == "bench" or t >= 9]
    rng = np.random.default_rng(11)
    counts = counts + [int(t) for t in rng.permutation(counts)]
    return counts + [101] * (40 - len(counts))


@functools.lru_cache(maxsize=None)
def _batch(case, preset):
    """(signals, sample lengths, index of the loud utterance, index of the silent one)."""
    frames = _frame_counts(case, preset)
    rng = np.random.default_rng(5)
    lens = [HOP * (t - 1) + int(rng.integers(0, HOP)) for t in frames]   # T = 1 + n // 160
    assert [1 + n // HOP for n in lens] == frames
    base = mo.synth_utterances(len(lens), n_samples=max(lens), sr=SR, seed=23)
    sig = [b[:n].copy() for b, n in zip(base, lens)]
    for i in range(0, len(sig), 3):     # first and last 100 ms zeroed
        sig[i][: SR // 10] = 0.0
        sig[i][max(len(sig[i]) - SR // 10, 0):] = 0.0
    loud = 1 if case == "split" else max(i for i, t in enumerate(frames) if t == 113 and i % 3)
    silent = 2 if case == "split" else max(i for i, t in enumerate(frames) if t == 97)
    sig[loud] *= np.float32(1e4)
    sig[silent][:] = 0.0
    return sig, np.asarray(lens, dtype=np.int64), loud, silent


def _run(plan, sig, lens):
    import torch
    pcm = torch.from_numpy(np.concatenate(sig).astype(np.float32)).cuda()
    feats, frames = plan(pcm, lens)
    torch.cuda.synchronize()
    return feats, frames


@functools.lru_cache(maxsize=None)
def _generic(case, preset, slices):
    """The batch through the generic finish body (computed once per case)."""
    import torch
    sig, lens, _, _ = _batch(case, preset)
    feats, frames = _run(_plan(preset, slices, True), sig, lens)
    assert bool(torch.isfinite(feats).all())
    return feats, frames


def _assert_equal(got, want, frames, tag):
    import torch
    assert got.shape == want.shape and got.shape[0] == int(frames.sum())
    if not torch.equal(got, want):
        fo = np.concatenate([[0], np.cumsum(frames)])
        rows = torch.nonzero((got != want).any(dim=1)).flatten().cpu().numpy()
        where = sorted(set((int(np.searchsorted(fo, r, side="right") - 1),
                            int(r - fo[np.searchsorted(fo, r, side="right") - 1])) for r in rows))
        raise AssertionError(f"{tag}: {len(rows)} rows differ from the generic body, (utterance, frame) {where[:20]}")


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("preset", PRESETS)
def test_ragged_batch_equals_generic_body(preset, slices):
    sig, lens, _, _ = _batch("ragged", preset)
    want, frames = _generic("ragged", preset, slices)
    got, _ = _run(_plan(preset, slices, False), sig, lens)
    _assert_equal(got, want, frames, f"{preset}, SAPR_MFCC_SLICES={slices}")


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("preset", PRESETS)
def test_split_path_equals_generic_body(preset, slices):
    sig, lens, _, _ = _batch("split", preset)
    want, frames = _generic("split", preset, slices)
    assert int(frames.max()) == 2001
    got, _ = _run(_plan(preset, slices, False), sig, lens)
    _assert_equal(got, want, frames, f"{preset}, SAPR_MFCC_SLICES={slices}, split")


@pytest.mark.parametrize("preset", PRESETS)
def test_ragged_batch_against_the_oracle(preset):
    sig, lens, loud, silent = _batch("ragged", preset)
    got, frames = _run(_plan(preset, 1, False), sig, lens)
    got = got.cpu().numpy()
    fo = np.concatenate([[0], np.cumsum(frames)])
    worst = 0.0
    for i in range(len(sig)):
        want = mo.mfcc(sig[i], **_ocfg(preset)).T
        g = got[fo[i]:fo[i + 1]]
        assert g.shape == want.shape
        d = g.astype(np.float64) - want.astype(np.float64)
        worst = max(worst, float(np.abs(d).max()))
        print(f"{preset} utterance {i} T={int(frames[i])}{' loud' if i == loud else ''}{' silent' if i == silent else ''}: "
              f"max |d| {np.abs(d).max():.3e} rms {np.sqrt((d ** 2).mean()):.3e}")
        assert np.abs(d).max() <= ATOL, (i, int(frames[i]), np.abs(d).max())
        assert np.sqrt((d ** 2).mean()) <= RMS, (i, int(frames[i]), np.sqrt((d ** 2).mean()))
    print(f"{preset}: largest |d| {worst:.3e}")

"""Slice pipeline of the wave-private MFCC core (sapr_mfcc_batch, SAPR_MFCC_SLICES): cutting a batch into slices of
whole utterances, with the finish pass of slice k on the plan's side stream under the spectral kernel of slice k + 1,
must not change one bit of the features.  The yardstick is the single launch (SAPR_MFCC_SLICES=1) of the same build;
the comparison is torch.equal on the feature tensor — no tolerance (parity of the single launch with the oracle is
tests/test_mfcc_gpu.py's business).

SAPR_MFCC_SLICES is read when a plan is created, so every plan below is created under the value it is meant for.
The 39-dimensional preset goes through MfccPlan.__call__, which refuses utterances of fewer than 9 frames (delta
features are undefined there, librosa.feature.delta): its ragged lengths go down to 9 frames, the plain preset's to 0
and 1 sample."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from oracle import mfcc_oracle as mo

pytestmark = pytest.mark.gpu

FORCED = (2, 3, 7)


@contextlib.contextmanager
def _slices(value):
    """SAPR_MFCC_SLICES=value (None: unset) while plans are created."""
    old = os.environ.get("SAPR_MFCC_SLICES")
    if value is None:
        os.environ.pop("SAPR_MFCC_SLICES", None)
    else:
        os.environ["SAPR_MFCC_SLICES"] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SAPR_MFCC_SLICES", None)
        else:
            os.environ["SAPR_MFCC_SLICES"] = old


def _plan(cfg, slices):
    from sapr_amd.frontend import MfccPlan
    with _slices(slices):
        plan = MfccPlan(**cfg, max_frames=0)
    assert plan.two_pass
    return plan


def _presets():
    from sapr_amd.frontend import BENCH, BENCH39
    return {"bench": BENCH, "bench39": BENCH39}


def _ragged(preset, n_extra=0):
    """Signals with ragged lengths, an all-silent and a half-silent utterance (the top_db clip path)."""
    rng = np.random.default_rng(11)
    short = [160, 159, 1, 0] if preset == "bench" else [1440, 1599, 1441, 1440]   # 9 frames = 1440 samples
    lens = [int(v) for v in rng.integers(1500, 16000, 15 + n_extra)] + short + [15999, 16000, 3333]
    base = mo.synth_utterances(len(lens), n_samples=16000, sr=16000, seed=21)
    sig = [b[:n].copy() for b, n in zip(base, lens)]
    sig[2][:] = 0.0                       # all silent: every log-mel at the floor
    sig[5][: len(sig[5]) // 2] = 0.0      # half silent: frames below max - top_db are clipped
    return sig


def _run(plan, sig):
    import torch
    lens = np.asarray([len(s) for s in sig], dtype=np.int64)
    pcm = torch.from_numpy(np.concatenate(sig).astype(np.float32)).cuda()
    feats, frames = plan(pcm, lens)
    torch.cuda.synchronize()
    return feats, frames


@pytest.mark.parametrize("preset", ["bench", "bench39"])
def test_forced_slices_equal_the_single_launch_on_ragged_batches(preset):
    """22 utterances (not divisible by 3 or 7), ragged down to the shortest the preset takes, silence included."""
    import torch
    cfg = _presets()[preset]
    sig = _ragged(preset)
    assert len(sig) % 3 and len(sig) % 7
    want, frames = _run(_plan(cfg, 1), sig)
    assert want.shape[0] == int(frames.sum()) and bool(torch.isfinite(want).all())
    for s in FORCED:
        got, _ = _run(_plan(cfg, s), sig)
        assert torch.equal(got, want), f"{preset}: SAPR_MFCC_SLICES={s} differs from the single launch"


@pytest.mark.parametrize("preset", ["bench", "bench39"])
def test_more_slices_than_utterances(preset):
    """Five utterances, seven slices asked for: no empty launch, same features."""
    import torch
    cfg = _presets()[preset]
    sig = _ragged(preset)[:5]
    want, _ = _run(_plan(cfg, 1), sig)
    for s in (7, 32, 1000):
        got, _ = _run(_plan(cfg, s), sig)
        assert torch.equal(got, want), f"{preset}: {s} slices over {len(sig)} utterances"
    one, _ = _run(_plan(cfg, 7), sig[:1])
    assert torch.equal(one, _run(_plan(cfg, 1), sig[:1])[0])


@pytest.mark.parametrize("preset", ["bench", "bench39"])
def test_slices_on_a_non_default_stream(preset):
    import torch
    cfg = _presets()[preset]
    sig = _ragged(preset)
    want, _ = _run(_plan(cfg, 1), sig)
    st = torch.cuda.Stream()
    for s in FORCED:
        plan = _plan(cfg, s)
        lens = np.asarray([len(x) for x in sig], dtype=np.int64)
        pcm = torch.from_numpy(np.concatenate(sig).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            got, _ = plan(pcm, lens)
            # the consumer is enqueued on the same stream straight behind the call: it must see complete features
            copy = got.clone()
        st.synchronize()
        assert torch.equal(copy, want), f"{preset}: SAPR_MFCC_SLICES={s} on a side stream"
        torch.cuda.synchronize()


@pytest.mark.parametrize("preset", ["bench", "bench39"])
def test_two_calls_back_to_back_on_one_plan_and_workspace(preset):
    """The second call reuses the log-mel workspace and the utterance maxima while the first call's last finish pass
    may still run: its memset and spectral kernels must wait for it.  Different signals in the two calls, no
    synchronisation in between, outputs in separate buffers."""
    import torch
    from sapr_amd import _lib
    cfg = _presets()[preset]
    lib = _lib.load()
    sig_a = _ragged(preset, n_extra=40)
    sig_b = [s[::-1].copy() for s in sig_a]     # same lengths, other samples
    ref = _plan(cfg, 1)
    want_a, frames = _run(ref, sig_a)
    want_b, _ = _run(ref, sig_b)
    assert not torch.equal(want_a, want_b)
    lens = np.asarray([len(s) for s in sig_a], dtype=np.int64)
    so = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=so[1:])
    fo = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(frames, out=fo[1:])
    so_d, fo_d = torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    pcm_a = torch.from_numpy(np.concatenate(sig_a).astype(np.float32)).cuda()
    pcm_b = torch.from_numpy(np.concatenate(sig_b).astype(np.float32)).cuda()
    n, total = len(lens), int(fo[-1])
    for s in FORCED:
        plan = _plan(cfg, s)
        ws, ws_bytes = plan.workspace(total, n, pcm_a.device)
        out_a = torch.empty((total, plan.d_out), device="cuda")
        out_b = torch.empty((total, plan.d_out), device="cuda")
        torch.cuda.synchronize()
        for _ in range(3):   # A, B, A, B, A, B on the same workspace
            for pcm, out in ((pcm_a, out_a), (pcm_b, out_b)):
                _lib.check(lib.sapr_mfcc_batch(plan._h, _lib.ptr(pcm), _lib.ptr(so_d), _lib.ptr(fo_d), n, total,
                                               _lib.ptr(out), 0, _lib.ptr(ws), ws_bytes, _lib.current_stream()),
                           "sapr_mfcc_batch")
        torch.cuda.synchronize()
        assert torch.equal(out_a, want_a) and torch.equal(out_b, want_b), f"{preset}: SAPR_MFCC_SLICES={s}"


@pytest.mark.parametrize("preset", ["bench", "bench39"])
def test_default_slicing_equals_the_single_launch_at_100000_utterances(preset):
    """The benchmark's batch shape: 100 000 fixed-length utterances, a tenth of them digital silence; the default
    slice count (SAPR_MFCC_SLICES unset) against the single launch."""
    import torch
    cfg = _presets()[preset]
    n, n_samp = 100000, 16000
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    pcm = torch.rand(n * n_samp, device="cuda", generator=g) - 0.5
    pcm.view(n, n_samp)[::10] = 0.0
    pcm.view(n, n_samp)[1::10, : n_samp // 2] = 0.0
    lens = np.full(n, n_samp, dtype=np.int64)
    want, _ = _plan(cfg, 1)(pcm, lens)
    got, _ = _plan(cfg, None)(pcm, lens)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    forced, _ = _plan(cfg, 8)(pcm, lens)
    torch.cuda.synchronize()
    assert torch.equal(forced, want)


@pytest.mark.parametrize("slices", FORCED)
def test_frame_count_guard_with_forced_slices(slices):
    """tests/test_capi_errors_gpu.py's frame-count case under forced slices: offsets on the device that describe MORE
    frames than the caller sized the buffers for make every slice's spectral kernel return; out[0 : total_frames]
    becomes NaN and nothing is written behind `out` or behind the workspace."""
    import torch
    from sapr_amd import _lib
    from sapr_amd.frontend import BENCH, MfccPlan
    lib = _lib.load()
    with _slices(slices):
        plan = MfccPlan(**BENCH, max_frames=101)
    assert plan.two_pass
    n, T = 8, 101
    pcm = torch.randn(n * 16000, device="cuda") * 0.1
    so = (torch.arange(n + 1, dtype=torch.int64) * 16000).cuda()
    fo = (torch.arange(n + 1, dtype=torch.int64) * T).cuda()            # the device says 808 frames ...
    claimed = (n - 1) * T                                               # ... the caller sizes everything for 707
    need = C.c_size_t(0)
    assert lib.sapr_mfcc_workspace_bytes(plan._h, claimed, n, C.byref(need)) == 0 and need.value > 0
    ws = torch.full((need.value + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((n * T, 13), 7.0, device="cuda")
    rc = lib.sapr_mfcc_batch(plan._h, _lib.ptr(pcm), _lib.ptr(so), _lib.ptr(fo), n, claimed, _lib.ptr(out), 0,
                             _lib.ptr(ws), need.value, _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:claimed]).all()), "a frame-count mismatch must not pass for features"
    assert bool((out[claimed:] == 7.0).all()), "rows behind the caller's frame count were written"
    assert bool((ws[need.value:] == 0x5A).all()), "bytes behind the workspace were written"
    # the log-mel part of the workspace is untouched as well: no slice computed anything
    assert bool((ws[: claimed * 40 * 4] == 0x5A).all()), "a slice's spectral kernel ran despite the mismatch"
    # the consistent call on the same buffers still works, and equals the single launch
    rc = lib.sapr_mfcc_batch(plan._h, _lib.ptr(pcm), _lib.ptr(so[: n]), _lib.ptr(fo[: n]), n - 1, claimed, _lib.ptr(out),
                             0, _lib.ptr(ws), need.value, _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:claimed]).all()) and bool((out[claimed:] == 7.0).all())
    with _slices(1):
        single = MfccPlan(**BENCH, max_frames=101)
    want, _ = single(pcm[: (n - 1) * 16000], np.full(n - 1, 16000))
    torch.cuda.synchronize()
    assert torch.equal(out[:claimed], want)

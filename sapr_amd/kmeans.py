"""Batched k-means on the device: the k-means of hmmlearn's ``GaussianHMM._init`` (``sklearn.cluster.KMeans(n_clusters,
n_init=10)`` over all frames of a word model) for every word model and every restart at once.

The hot path is ``sapr_kmeans_step`` (``csrc/kmeans.hip``): ONE Lloyd step for G groups (k-means problems: the frames of
one word model each) and R centre sets per group, returning per (group, restart, cluster) ``{count, sum_x[D],
sqdev[D]}``.  Everything around it is small host arithmetic on ``[G, R, K, 2D+1]`` doubles: new centre = ``sum/count``,
the convergence test and the choice of the best restart (:func:`kmeans`), and the k-means++ seeding on a subsample
(:func:`kmeans_pp_seeds`).

Lloyd follows scikit-learn's rules (``KMeans(init=array, n_init=1, algorithm="lloyd")``; tests/test_kmeans_cpu.py holds
the comparison): threshold ``tol * mean_d var_d(X_g)``, stop when ``sum |c_new - c_old|^2 <= threshold``, one more step
at the final centres for the inertia, the best restart is the lowest inertia (ties: the lowest restart).  Deviations,
all deliberate:

* an EMPTY CLUSTER KEEPS ITS PREVIOUS CENTRE (scikit-learn moves it to the points farthest from their centres):
  deterministic, and it needs no second pass over frames that may live on other ranks;
* seeding is k-means++ on a uniform subsample of ``min(n_g, 256 K)`` frames of the group, one subsample per group shared
  by its restarts, drawn from numpy's ``default_rng(seed)`` — not scikit-learn's stream, not its greedy variant;
* distances are the directly squared differences in float64 (no ``|x|^2 - 2 x.c + |c|^2`` expansion, no centring pass).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

TILE = 256      # frames per tile (one workgroup)
MAX_K = 32      # clusters the kernel serves


def _torch():
    import torch
    return torch


@dataclass
class FrameTiles:
    """Frames cut into tiles of at most 256 consecutive frames that belong to one group, sorted by group.  Group g
    owns the frames ``[group_off[g], group_off[g+1])`` of the packed feature array and the tiles
    ``[group_tile_off[g], group_tile_off[g+1])``; a group without frames owns no tile."""
    tile_begin: "object"      # int64 [n_tiles]  first frame of the tile
    tile_len: "object"        # int32 [n_tiles]  1..256
    tile_group: "object"      # int32 [n_tiles]
    group_tile_off: "object"  # int32 [G+1]
    n_tiles: int
    G: int
    total_frames: int
    group_lengths: np.ndarray  # host int64 [G]
    group_off: np.ndarray      # host int64 [G+1]

    @staticmethod
    def build(group_lengths, device=None) -> "FrameTiles":
        """Host logic; ``device`` None keeps the tables on the host (CPU tensors)."""
        torch = _torch()
        gl = np.asarray(group_lengths, dtype=np.int64).reshape(-1)
        if gl.size and gl.min() < 0:
            raise ValueError("group lengths must be >= 0")
        G = int(gl.size)
        off = np.zeros(G + 1, dtype=np.int64)
        np.cumsum(gl, out=off[1:])
        n_t = (gl + TILE - 1) // TILE
        toff = np.zeros(G + 1, dtype=np.int64)
        np.cumsum(n_t, out=toff[1:])
        n_tiles = int(toff[-1])
        if n_tiles > np.iinfo(np.int32).max:
            raise ValueError("too many tiles for one launch")
        group = np.repeat(np.arange(G, dtype=np.int32), n_t)
        within = np.arange(n_tiles, dtype=np.int64) - toff[:-1][group]
        begin = off[:-1][group] + within * TILE
        length = np.minimum(off[1:][group] - begin, TILE).astype(np.int32)
        t = torch.from_numpy
        dev = device if device is not None else "cpu"
        return FrameTiles(t(begin).to(dev), t(length).to(dev), t(group).to(dev), t(toff.astype(np.int32)).to(dev),
                          n_tiles, G, int(off[-1]), gl, off)


def _pad_columns(t, D):
    """``t[..., Dm]`` zero-padded to ``[..., D]`` (the same tensor when it already has D columns)."""
    torch = _torch()
    if t.shape[-1] == D:
        return t.contiguous()
    out = torch.zeros(t.shape[:-1] + (D,), dtype=t.dtype, device=t.device)
    out[..., : t.shape[-1]] = t
    return out


class Stepper:
    """Pre-allocated ``sapr_kmeans_step`` over one feature tensor (kernel width) and one tile layout."""

    def __init__(self, feats, tiles: FrameTiles):
        torch = _torch()
        from .trellis import kernel_dims
        if feats.dim() != 2 or feats.dtype != torch.float32:
            raise ValueError("feats must be float32 [total_frames, D]")
        if feats.shape[0] != tiles.total_frames:
            raise ValueError(f"feats has {feats.shape[0]} frames, the tile layout covers {tiles.total_frames}")
        if not feats.is_cuda:
            raise _lib.SaprHipError("kmeans_step runs on the GPU only (no CPU implementation)")
        if tiles.tile_begin.device != feats.device:
            raise ValueError("the tile tables must live on the features' device (FrameTiles.build(lengths, device))")
        self.lib = _lib.load()
        self.D_model = int(feats.shape[1])
        self.D = kernel_dims(self.D_model)
        self.feats = _pad_columns(feats, self.D)
        self.tiles = tiles
        self._ws = None

    def step(self, centres, want_labels=False):
        """centres [G, R, K, D_model] (host array or device tensor) -> device stats [G, R, K, 2*D_model+1]
        (and labels [R, total_frames] int32)."""
        torch = _torch()
        dev, tl = self.feats.device, self.tiles
        if not torch.is_tensor(centres):
            centres = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float64))
        centres = centres.to(device=dev, dtype=torch.float64)
        if centres.dim() != 4 or centres.shape[0] != tl.G or centres.shape[3] != self.D_model:
            raise ValueError(f"centres must be [G={tl.G}, R, K, D={self.D_model}], got {tuple(centres.shape)}")
        R, K = int(centres.shape[1]), int(centres.shape[2])
        if R < 1 or K < 1:
            raise ValueError("centres need at least one restart and one cluster")
        cpad = _pad_columns(centres, self.D)
        nb = C.c_size_t(0)
        _lib.check(self.lib.sapr_kmeans_workspace_bytes(tl.n_tiles, R, K, self.D, C.byref(nb)),
                   "sapr_kmeans_workspace_bytes")
        if self._ws is None or self._ws.numel() < nb.value:
            self._ws = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=dev)
        W = 2 * self.D + 1
        stats = torch.empty((tl.G, R, K, W), dtype=torch.float64, device=dev)
        labels = torch.empty((R, tl.total_frames), dtype=torch.int32, device=dev) if want_labels else None
        _lib.check(self.lib.sapr_kmeans_step(
            _lib.ptr(self.feats), tl.total_frames, _lib.ptr(tl.tile_begin), _lib.ptr(tl.tile_len),
            _lib.ptr(tl.tile_group), _lib.ptr(tl.group_tile_off), tl.n_tiles, tl.G, R, K, self.D, _lib.ptr(cpad),
            _lib.ptr(self._ws), int(nb.value), _lib.ptr(stats), _lib.ptr(labels), _lib.current_stream()),
            "sapr_kmeans_step")
        if self.D_model != self.D:  # cut back to the caller's width: the padded columns hold exact zeros
            Dm = self.D_model
            stats = torch.cat([stats[..., : 1 + Dm], stats[..., 1 + self.D: 1 + self.D + Dm]], dim=-1).contiguous()
        return (stats, labels) if want_labels else stats


def kmeans_step(feats, tiles: FrameTiles, centres, want_labels=False):
    """One Lloyd step.  ``feats`` device float32 ``[total_frames, D]``, ``centres`` ``[G, R, K, D]`` float64 ->
    device ``stats[G, R, K, 2D+1]`` = ``{count, sum_x[D], sqdev[D]}`` per cluster, and with ``want_labels`` also
    ``labels[R, total_frames]`` int32.  Widths other than 13 and 39 run zero-padded (``trellis.kernel_dims``) and are
    cut back.  A cluster or group without frames gets exact zeros; a frame holding NaN gets label 0 and its NaN flows
    into the sums."""
    return Stepper(feats, tiles).step(centres, want_labels)


def kmeans_pp_seeds(X, K, rng) -> np.ndarray:
    """Plain k-means++ on a host array ``X[n, D]`` -> indices of K rows.  The first centre is drawn uniformly, each
    further one in proportion to D^2, the squared distance to the nearest centre chosen so far; when every D^2 is zero
    (all remaining rows coincide with a centre) it is drawn uniformly among the rows not chosen yet.  Rows already
    chosen have D^2 = 0, so K distinct rows come back whenever K distinct rows exist."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    if X.ndim != 2 or K < 1 or n < K:
        raise ValueError(f"kmeans_pp_seeds needs at least K={K} rows, got {X.shape}")
    chosen = np.empty(K, dtype=np.int64)
    chosen[0] = int(rng.integers(n))
    d2 = ((X - X[chosen[0]]) ** 2).sum(axis=1)
    taken = np.zeros(n, dtype=bool)
    taken[chosen[0]] = True
    for k in range(1, K):
        tot = d2.sum()
        if np.isfinite(tot) and tot > 0:
            i = int(rng.choice(n, p=d2 / tot))
        else:
            free = np.nonzero(~taken)[0]
            i = int(free[rng.integers(free.size)])
        chosen[k] = i
        taken[i] = True
        d2 = np.minimum(d2, ((X - X[i]) ** 2).sum(axis=1))
    return chosen


def _allreduce_host(a: np.ndarray, device) -> np.ndarray:
    from . import dist as sdist
    return sdist.allreduce_sum_numpy(np.ascontiguousarray(a, dtype=np.float64), device)


def column_moments(stepper: Stepper):
    """``(count[G], mean[G, D], sqdev[G, D])`` of every group over ALL ranks' frames, from two K = 1 steps: ``sum /
    count`` first, then ``sum (x - mean)^2`` about it (numpy's two-pass variance).  A group without frames has count 0
    and zeros."""
    G, D = stepper.tiles.G, stepper.D_model
    dev = stepper.feats.device
    st = _allreduce_host(stepper.step(np.zeros((G, 1, 1, D))).cpu().numpy(), dev)
    count = st[:, 0, 0, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(count[:, None] > 0, st[:, 0, 0, 1:1 + D] / count[:, None], 0.0)
    st = _allreduce_host(stepper.step(mean[:, None, None, :]).cpu().numpy(), dev)
    return count, mean, st[:, 0, 0, 1 + D:]


def _seed_centres(stepper: Stepper, K, n_init, seeds):
    """k-means++ centres [G, n_init, K, D] for every group, drawn on the lowest rank that holds at least K frames of
    the group and shared with the others by all-reducing a buffer that is zero elsewhere."""
    torch = _torch()
    from . import dist as sdist
    tl, D, dev = stepper.tiles, stepper.D_model, stepper.feats.device
    rank, world = sdist.world()
    held = np.zeros((world, tl.G))
    held[rank] = tl.group_lengths
    held = _allreduce_host(held, dev)
    short = [g for g in range(tl.G) if not (held[:, g] >= K).any()]
    if short:
        raise ValueError(f"k-means seeding: no rank holds {K} frames of group(s) {short}")
    owner = np.argmax(held >= K, axis=0)
    if seeds is None:
        seeds = np.random.SeedSequence().generate_state(tl.G)
    seeds = np.asarray(seeds).reshape(-1)
    if seeds.size != tl.G:
        raise ValueError("seeds must hold one integer per group")
    mine = [g for g in range(tl.G) if owner[g] == rank]
    rngs = {g: np.random.default_rng(int(seeds[g])) for g in mine}
    # one subsample per group, one gather from the device for all of them
    picks = {}
    for g in mine:
        n = int(tl.group_lengths[g])
        m = min(n, TILE * K)
        picks[g] = np.sort(rngs[g].choice(n, m, replace=False)) if m < n else np.arange(n)
    out = np.zeros((tl.G, n_init, K, D))
    if mine:
        rows = np.concatenate([tl.group_off[g] + picks[g] for g in mine])
        sub = stepper.feats[torch.from_numpy(rows).to(dev)][:, :D].cpu().numpy().astype(np.float64)
        at = 0
        for g in mine:
            Xg = sub[at:at + picks[g].size]
            at += picks[g].size
            for r in range(n_init):
                out[g, r] = Xg[kmeans_pp_seeds(Xg, K, rngs[g])]
    return _allreduce_host(out, dev)


def kmeans(feats, group_lengths, n_clusters, init=None, n_init=10, max_iter=300, tol=1e-4, seeds=None, moments=None):
    """Lloyd's k-means for G groups at once.  ``feats``: float32 ``[total_frames, D]`` (device tensor, or a host array
    that is uploaded), the groups' frames one after the other; ``group_lengths[G]``: THIS RANK's frames per group.

    ``init``: ``[G, R, K, D]`` explicit start centres (R restarts), or None: ``n_init`` restarts seeded by
    :func:`kmeans_pp_seeds` from ``default_rng(seeds[g])`` (``seeds`` None: fresh entropy).  ``moments``: a
    :func:`column_moments` result to reuse.  Returns host arrays ``centers[G, K, D]``, ``inertia[G]``, ``n_iter[G]``,
    ``best_init[G]`` of the best restart (lowest inertia, ties to the lowest restart).

    Every (group, restart) problem rides in every launch; converged ones keep their centres.  An empty cluster keeps
    its previous centre.  Under ``torch.distributed`` the step statistics are all-reduced every iteration, so every
    rank takes the same decisions and issues the same collectives whatever its shard holds.  A group with fewer than
    ``max(K, 2)`` frames (over all ranks) raises ``ValueError``."""
    torch = _torch()
    from . import dist as sdist
    K = int(n_clusters)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"n_clusters must lie in 1..{MAX_K}")

    def refuse_few(counts):
        few = [g for g, n in enumerate(counts) if n < max(K, 2)]
        if few:
            raise ValueError(f"k-means with {K} clusters needs at least {max(K, 2)} frames per group; group(s) {few} "
                             f"hold {[int(counts[g]) for g in few]}")
    if not sdist.is_distributed():  # (one rank holds everything: refused before anything touches the device)
        refuse_few(np.asarray(group_lengths, dtype=np.int64).reshape(-1))
    dev = _lib.require_gpu()
    if not torch.is_tensor(feats):
        feats = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32))
    feats = feats.to(dev)
    tiles = FrameTiles.build(group_lengths, dev)
    stepper = Stepper(feats, tiles)
    G, D = tiles.G, stepper.D_model
    count, _, sqdev = moments if moments is not None else column_moments(stepper)
    refuse_few(count)
    threshold = tol * (sqdev / count[:, None]).mean(axis=1)            # tol * mean_d var_d(X_g)
    if init is None:
        centres = _seed_centres(stepper, K, int(n_init), seeds)
    else:
        centres = np.array(init, dtype=np.float64)
        if centres.ndim != 4 or centres.shape[0] != G or centres.shape[2:] != (K, D):
            raise ValueError(f"init must be [G={G}, R, K={K}, D={D}], got {centres.shape}")
    R = centres.shape[1]
    active = np.ones((G, R), dtype=bool)
    n_iter = np.zeros((G, R), dtype=np.int64)

    def step_host(c):
        return sdist.allreduce_sum_(stepper.step(c)).cpu().numpy()

    for it in range(int(max_iter)):
        if not active.any():
            break
        st = step_host(centres)
        cnt = st[..., 0:1]
        with np.errstate(divide="ignore", invalid="ignore"):
            new = np.where(cnt > 0, st[..., 1:1 + D] / cnt, centres)     # an empty cluster keeps its centre
        shift = ((new - centres) ** 2).sum(axis=(2, 3))
        centres = np.where(active[:, :, None, None], new, centres)
        n_iter[active] = it + 1
        active &= ~(shift <= threshold[:, None])
    inertia_all = step_host(centres)[..., 1 + D:].sum(axis=(2, 3))     # one final step at the final centres
    best = np.argmin(inertia_all, axis=1)                              # (first lowest: ties to the lowest restart)
    gi = np.arange(G)
    return centres[gi, best], inertia_all[gi, best], n_iter[gi, best], best.astype(np.int64)

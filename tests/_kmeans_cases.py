"""Seeded inputs of tests/test_kmeans_cases_*.py: sapr_kmeans_step at the kernel branches the recipe of
tests/_kmeans_ref.py does not reach, and ``kmeans()`` with its own seeding.

The bar of the GPU file is tests/test_kmeans_gpu.py's ``_check_against_reference``: labels and counts equal to the float64
numpy reference, ``sum_x`` within 1e-11 sum|x| per column, ``sqdev`` at rtol 1e-11.  tests/test_kmeans_cases_cpu.py checks,
from the reference alone, that every case is what it claims to be (gaps above 1e-8, exact ties only between bit-identical
centre rows, the intended labels of the skewed tiles, shift against threshold, ``emptied``).

Cases:

  shape-<D>-<K>      SHAPES: the 11 recipe groups (182-484 frames) at width D, R = 3 restarts from rows of the group
                     (``_kmeans_ref.recipe_init``).  (39, 32) / (39, 26) / (13, 20): five / four / two (k, d) accumulators
                     per thread; (39, 20) a partial fourth pass (780 items); the label scan at K = 16 / 17 / 31 / 32;
                     (14, 7) and (1, 4) run padded to 39 and 13 columns.
  restarts-<D>-<K>-<R>  (13, 10) and (39, 18) at R = 1 and R = 10; at R = 10 restart 7 is a copy of restart 0.
  skewed-<D>         K = 5, R = 2, eight groups: the four PATTERNS in a group of 256 frames and in the SECOND tile of a
                     group of 512 (whose first tile is mixed).  Column 1 of frame i and of centre k carry 1000 times the
                     intended label / k, so the reference's labels are the intended ones; restart 1 holds the centres
                     in reverse order (all-in-0 becomes all-in-4, the 3 + 253 split lands on clusters 4 and 3).
                       all_first   every frame of the tile in cluster 0
                       all_last    every frame of the tile in cluster K - 1
                       one_wave    cluster 2 holds exactly the frames 64..127, the others share the rest
                       three_253   frames 5, 100 and 200 in cluster 0, the other 253 in cluster 1: its rows start at
                                   row 3 of the sorted copy and the gather's last round reads rows 255..258
  nan_centre-<D>     K = 5, R = 3 on the recipe: restart 0 has a NaN in centre 2, restart 1 in centres 1 and 3, restart 2
                     none.  np.argmin keeps the first NaN: labels 2 / 1 on every frame.
  inf_frames-<D>     K = 5, R = 2 on three recipe groups: group 0 holds +inf (column 3) and -inf (column 7) in two frames
                     of different tiles, group 1 both in column 2 (inf - inf: NaN in the sum), group 2 nothing.  Every
                     distance of such a frame is +inf: label 0.
  tables             TABLE_LENGTHS = 300, 256, 100 frames: tiles (g0: 256 + 44, g1: 256, g2: 100), D = 13, K = 4, R = 2;
                     TABLE_EDITS are applied one at a time to tile 1 / to ``group_tile_off``.
  many_tiles-<D>     D = 13: groups of 1, 7, 8, 9, 57, 64, 65, 130 tiles, D = 39: of 9 and 65, each with a partial last
                     tile (MANY_TAILS), K = 3, R = 2.  A group is ONE ``_synth.synth_utterance`` of its length (eight
                     segments, c0 at -300).  chunk = ceil(tiles / 8): 9 tiles leave the runs 5..7 empty, 65 and 130
                     tiles run the eight-wide loop once and twice with a tail of one.
  seeded-13-2        ``kmeans(n_init=4, seeds=SEEDED_SEEDS[...])`` over groups of 600 (subsampled to 512) and 300 frames;
  seeded-39-1        one group of 300 frames, K = 1 (all four restarts reach the mean: the tie branch of the bar).
  emptied            (13, 4), one restart, start centre 1 = a frame + 1e6 in every column: empty in every step.

MEASURED on the CPU from the reference (tests/test_kmeans_cases_cpu.py prints them; -s shows them):
  smallest non-zero relative gap  shapes 3.5e-7 at (39, 26), 3.5e-5 / 1.9e-5 at K = 32, 1.7e-4 at (1, 4); restarts
                                  7.7e-6 (39, 18, R = 10); skewed 0.94 (by construction); nan_centre 1.7e-5;
                                  inf_frames 2.2e-4; tables 1.5e-4; many_tiles 1.6e-6 (D = 13), 4.4e-6 (D = 39);
                                  seeded 6.3e-5; emptied 1.8e-3 — all above the 1e-8 the comparisons need
  exact ties                      only between centres drawn from the duplicated silence frames (bit-identical rows)
  seeded                          margins 13-2: 1.8e-2 (600 frames, best restart 2), 3.7e-2 (300 frames, restart 0);
                                  39-1: 0 by construction (n_iter 2 in every restart: the bar's set comparison)
  emptied                         n_iter 3; the far cluster is empty in every step
"""
import functools

import numpy as np

from tests import _kmeans_ref as ref
from tests._synth import synth_utterance

SHAPES = [(39, 32), (39, 26), (39, 20), (13, 32), (13, 31), (13, 20), (13, 17), (13, 2), (14, 7), (1, 4)]
RESTART_CASES = [(13, 10, 1), (13, 10, 10), (39, 18, 1), (39, 18, 10)]

PATTERNS = ("all_first", "all_last", "one_wave", "three_253")
SKEW_K = 5
SKEW_OFFSET = 1000.0
SKEW_COLUMN = 1
THREE = (5, 100, 200)


def _frozen(a):
    a.setflags(write=False)
    return a


def restart_init(D, K, R):
    """start centres [G, R, K, D] from rows of the group, as ``recipe_init`` draws them; at R = 10 restart 7 is restart 0."""
    groups = ref.recipe_groups(D)
    out = np.empty((len(groups), R, K, D))
    for g, X in enumerate(groups):
        for r in range(R):
            out[g, r] = X[np.random.default_rng(1000 * g + r).choice(X.shape[0], K, replace=False)]
    if R == 10:
        out[:, 7] = out[:, 0]
    return out


def pattern_labels(pattern):
    """intended labels of the 256 frames of a tile."""
    K = SKEW_K
    i = np.arange(256)
    if pattern == "all_first":
        return np.zeros(256, np.int64)
    if pattern == "all_last":
        return np.full(256, K - 1, np.int64)
    if pattern == "one_wave":
        lab = np.array([0, 1, 3, 4])[i % 4]
        lab[64:128] = 2
        return lab
    if pattern == "three_253":
        lab = np.ones(256, np.int64)
        lab[list(THREE)] = 0
        return lab
    raise ValueError(pattern)


@functools.lru_cache(maxsize=None)
def skewed(D):
    """-> (groups (tuple of float32 [n, D]), centres [G, 2, K, D], intended (tuple of int64 [n]: restart 0's labels;
    restart 1's are K - 1 - these), names)."""
    K = SKEW_K
    pool = np.concatenate(ref.recipe_groups(D), axis=0)
    rng = np.random.default_rng(4100 + D)
    groups, intended, names, centres = [], [], [], []
    at = 0
    for pattern in PATTERNS:
        for n in (256, 512):
            lab = pattern_labels(pattern)
            if n == 512:
                lab = np.concatenate([(np.arange(256) * 7) % K, lab])
            X = pool[at:at + n].astype(np.float32).copy()
            at += n
            X[:, SKEW_COLUMN] += (SKEW_OFFSET * lab).astype(np.float32)
            c = pool[rng.choice(pool.shape[0], K, replace=False)].astype(np.float64)
            c[:, SKEW_COLUMN] += SKEW_OFFSET * np.arange(K)
            groups.append(_frozen(X))
            intended.append(_frozen(lab))
            names.append(f"{pattern}-{n}")
            centres.append(np.stack([c, c[::-1]]))
    return tuple(groups), _frozen(np.stack(centres)), tuple(intended), tuple(names)


@functools.lru_cache(maxsize=None)
def nan_centre(D):
    """-> (groups, centres [G, 3, 5, D], expected label per restart (None: the reference's own))."""
    groups = ref.recipe_groups(D)
    centres = np.array(ref.recipe_init(D, 5))
    centres[:, 0, 2, D // 2] = np.nan
    centres[:, 1, 1, 0] = np.nan
    centres[:, 1, 3, D - 1] = np.nan
    return groups, _frozen(centres), (2, 1, None)


@functools.lru_cache(maxsize=None)
def inf_frames(D):
    """-> (groups (3), centres [3, 2, 5, D], rows: per group the frames that hold an infinity)."""
    src = ref.recipe_groups(D)
    pick = [g for g, X in enumerate(src) if X.shape[0] > 300][:3]
    groups = [src[g].copy() for g in pick]
    centres = np.array(ref.recipe_init(D, 5))[pick][:, :2]
    groups[0][17, 3] = np.inf
    groups[0][290, 7] = -np.inf
    groups[1][130, 2] = np.inf
    groups[1][131, 2] = -np.inf
    rows = ((17, 290), (130, 131), ())
    return tuple(_frozen(X) for X in groups), _frozen(centres), rows


# ---- tables that leave the batch -------------------------------------------------------------------------------------
TABLE_LENGTHS = (300, 256, 100)      # tiles: 0 (g0, 256), 1 (g0, 44), 2 (g1, 256), 3 (g2, 100)
TABLE_TILE = 1                       # the tile that is edited: frames 256..299 of group 0
TABLE_K, TABLE_R, TABLE_D = 4, 2, 13
# (name, table, index or "G" for the last entry, value or a function of (total_frames, tile_len, n_tiles, G))
TABLE_EDITS = (
    ("len_257", "tile_len", TABLE_TILE, lambda total, ln, nt, G: 257),
    ("len_minus_1", "tile_len", TABLE_TILE, lambda total, ln, nt, G: -1),
    ("begin_one_past", "tile_begin", TABLE_TILE, lambda total, ln, nt, G: total - ln + 1),
    ("begin_minus_1", "tile_begin", TABLE_TILE, lambda total, ln, nt, G: -1),
    ("group_G", "tile_group", TABLE_TILE, lambda total, ln, nt, G: G),
    ("group_minus_1", "tile_group", TABLE_TILE, lambda total, ln, nt, G: -1),
    ("off_last_past", "group_tile_off", "G", lambda total, ln, nt, G: nt + 5),
    ("off_first_negative", "group_tile_off", 0, lambda total, ln, nt, G: -3),
)


@functools.lru_cache(maxsize=None)
def tables():
    """-> (groups (3), centres [3, 2, 4, 13])."""
    pool = np.concatenate(ref.recipe_groups(TABLE_D), axis=0)
    cuts = np.cumsum((0,) + TABLE_LENGTHS) + 500
    groups = tuple(_frozen(pool[a:b].copy()) for a, b in zip(cuts[:-1], cuts[1:]))
    rng = np.random.default_rng(66)
    centres = np.stack([np.stack([X[rng.choice(X.shape[0], TABLE_K, replace=False)].astype(np.float64)
                                  for _ in range(TABLE_R)]) for X in groups])
    return groups, _frozen(centres)


# ---- the reduce kernel over many tiles -------------------------------------------------------------------------------
MANY_TILES = {13: (1, 7, 8, 9, 57, 64, 65, 130), 39: (9, 65)}
MANY_TAILS = {13: (200, 1, 255, 100, 17, 128, 64, 3), 39: (31, 254)}
MANY_K, MANY_R = 3, 2


def many_lengths(D):
    return tuple((t - 1) * 256 + tail for t, tail in zip(MANY_TILES[D], MANY_TAILS[D]))


@functools.lru_cache(maxsize=None)
def many_tiles(D):
    """-> (groups, centres [G, 2, 3, D])."""
    rng = np.random.default_rng(900 + D)
    groups, centres = [], []
    for n in many_lengths(D):
        proto = rng.normal(0.0, 20.0, (8, D))
        X = np.ascontiguousarray(synth_utterance(rng, proto, n).T)
        rows = [rng.choice(n, MANY_K, replace=False) if n >= MANY_K else np.arange(MANY_K) % n for _ in range(MANY_R)]
        centres.append(X[np.array(rows)].astype(np.float64))
        groups.append(_frozen(X))
    return tuple(groups), _frozen(np.stack(centres))


# ---- kmeans() with its own seeding -----------------------------------------------------------------------------------
SEEDED_N_INIT = 4
SEEDED = {(13, 2): ((600, 300), (11, 12)), (39, 1): ((300,), (5,))}     # (D, K) -> (group lengths, seeds)


@functools.lru_cache(maxsize=None)
def seeded(D, K):
    """-> (groups, seeds, reference: one ``_kmeans_ref.kmeans_seeded`` dict per group)."""
    lengths, seeds = SEEDED[(D, K)]
    pool = np.concatenate(ref.recipe_groups(D), axis=0)
    cuts = np.cumsum((0,) + lengths) + 700
    groups = tuple(_frozen(pool[a:b].copy()) for a, b in zip(cuts[:-1], cuts[1:]))
    return groups, seeds, tuple(ref.kmeans_seeded(X, K, SEEDED_N_INIT, s) for X, s in zip(groups, seeds))


EMPTIED_K, EMPTIED_FAR = 4, 1


@functools.lru_cache(maxsize=None)
def emptied():
    """-> (X float32 [n, 13], init [1, 1, 4, 13], the reference Lloyd run)."""
    X = ref.recipe_groups(13)[2]
    init = X[np.random.default_rng(31).choice(X.shape[0], EMPTIED_K, replace=False)].astype(np.float64)
    init[EMPTIED_FAR] += 1e6
    return X, _frozen(init[None, None]), ref.lloyd(X, init)

"""Two ranks (gloo, two processes sharing the box's GPU, as tests/test_multirank_gpu.py runs them): the sharded
k-means and the from-scratch ``fit_models`` — step statistics all-reduced every iteration, seeds drawn on one rank and
shared — against the single-process run, and with one rank's shard of one word empty."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
rank, world, port, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
import numpy as np, torch
if world > 1:
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
from sapr_amd import dist as sd
from sapr_amd.hmmlearn_hmm import GaussianHMM, fit_models
from sapr_amd.kmeans import kmeans
from tests import _kmeans_ref as ref
D, K = 13, 10
groups, lengths = ref.recipe_groups(D), ref.recipe_lengths(D)
res = {}
# k-means with explicit start centres, every group's frames split between the ranks
shard = []
for X in groups:
    lo, hi = sd.shard_range(X.shape[0], rank, world)
    shard.append(X[lo:hi])
c, inertia, n_iter, best = kmeans(np.concatenate(shard, axis=0), [s.shape[0] for s in shard], K,
                                  init=np.array(ref.recipe_init(D, K)))
res.update(km_centers=c, km_inertia=inertia, km_n_iter=n_iter, km_best=best)
# default-constructed models, utterances sharded; then the same with rank 1 holding nothing of word 0
for tag, starve in (("fit", False), ("starved", True)):
    models, data = [], []
    for g in range(4):
        models.append(GaussianHMM(n_components=5, random_state=g, n_iter=2))
        lo, hi = sd.shard_range(len(lengths[g]), rank, world)
        if starve and g == 0 and world > 1:
            lo, hi = (0, len(lengths[g])) if rank == 0 else (0, 0)
        offs = np.concatenate([[0], np.cumsum(lengths[g])])
        data.append((groups[g][offs[lo]:offs[hi]], list(lengths[g][lo:hi])))
    fit_models(models, data)
    for g, m in enumerate(models):
        res[f"{tag}_hist{g}"] = np.asarray(list(m.monitor_.history))
        res[f"{tag}_sp{g}"], res[f"{tag}_A{g}"] = m.startprob_, m.transmat_
        res[f"{tag}_mu{g}"], res[f"{tag}_cv{g}"] = m.means_, m._covars_
np.savez(out, **res)
if world > 1:
    dist.destroy_process_group()
print("ok", rank)
'''


def _run(tmp, world, tag):
    script = tmp / "kmeans_worker.py"
    script.write_text(WORKER)
    port = str(36500 + os.getpid() % 1000)
    outs = [str(tmp / f"{tag}_{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), str(world), port, outs[r]],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for p, o in zip(procs, logs):
        assert p.returncode == 0 and "ok" in o, o[-3000:]
    return [dict(np.load(o)) for o in outs]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kmeans_ranks")
    return _run(tmp, 1, "single")[0], _run(tmp, 2, "pair")


def test_two_rank_kmeans_equals_single_process(runs):
    single, ranks = runs
    for k in ("km_centers", "km_inertia"):
        np.testing.assert_array_equal(ranks[0][k], ranks[1][k], err_msg=k)
        np.testing.assert_allclose(ranks[0][k], single[k], rtol=1e-10, atol=0, err_msg=k)
    for k in ("km_n_iter", "km_best"):
        np.testing.assert_array_equal(ranks[0][k], ranks[1][k], err_msg=k)
        np.testing.assert_array_equal(ranks[0][k], single[k], err_msg=k)


@pytest.mark.parametrize("tag", ["fit", "starved"])
def test_two_rank_fit_from_scratch_ends_with_identical_models(runs, tag):
    single, ranks = runs
    keys = [k for k in single if k.startswith(tag + "_")]
    assert len(keys) == 4 * 5
    for k in keys:
        assert ranks[0][k].tobytes() == ranks[1][k].tobytes(), k
        assert np.isfinite(ranks[0][k]).all(), k
    for g in range(4):
        assert len(ranks[0][f"{tag}_hist{g}"]) == 2

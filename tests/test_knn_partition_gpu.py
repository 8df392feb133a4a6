"""``toolbox.knn_graph_partitioned`` on two ranks (uneven node ranges; gloo over the one GPU, as
tests/test_dist_two_ranks_gpu.py runs its ranks): each rank gathers the feature rows once and scans its own rows
against all of them; the ranks' lists, put together, are the exact kNN of the whole table, and each rank's edge list
builds its partition graph."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lattice as L
from tests.knn_dist_worker_gpu import BOUNDS, K, TABLE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_build_the_whole_tables_lists(cuda, tmp_path):
    world = len(BOUNDS) - 1
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", "29551",
           os.path.join(ROOT, "tests", "knn_dist_worker_gpu.py"), str(tmp_path)]
    res = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    ranks = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    want_idx, want_sim = L.knn_expected(*TABLE, K, True)
    idx = torch.from_numpy(np.concatenate([z["idx"] for z in ranks]))
    sim = torch.from_numpy(np.concatenate([z["sim"] for z in ranks]))
    assert torch.equal(idx, want_idx)
    assert torch.equal(sim.view(torch.int32), want_sim.view(torch.int32))
    n = BOUNDS[-1]
    for r, z in enumerate(ranks):
        r0, r1 = BOUNDS[r], BOUNDS[r + 1]
        ei, rows = z["ei"], z["idx"]
        assert rows.shape == (r1 - r0, K) and bool(z["half_refused"])
        assert ei.shape == (2, int((rows >= 0).sum())) and ei[1].min() >= r0 and ei[1].max() < r1
        assert np.array_equal(ei[0], rows[rows >= 0]) and np.array_equal(ei[1], np.repeat(np.arange(r0, r1), K))
        assert z["graph"].tolist() == [r1 - r0, n, r0, ei.shape[1]]

"""Worker of tests/test_knn_partition_gpu.py (one process per rank, launched with torch.distributed.run): the kNN
lists of the rank's node range under a ``dist.Partition`` - the feature rows gathered over gloo (the ranks share the
one GPU of the test box), the scan on the GPU - and the partition graph its edge list builds.

    knn_dist_worker_gpu.py OUT_DIR"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sngnn_amd  # noqa: E402,F401
from sngnn_amd import dist as sd, toolbox  # noqa: E402
from sngnn_amd.graph import Graph  # noqa: E402
from tests import lattice as L  # noqa: E402

TABLE, K, BOUNDS = ("lattice", 1030, 96), 16, (0, 397, 1030)


def main():
    out_dir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo")
    part = sd.Partition(rank, world, bounds=BOUNDS)
    x = L.knn_rows(*TABLE)[0]
    x_local = x[part.row_begin:part.row_end].to(dev)
    idx, sim = toolbox.knn_graph_partitioned(x_local, part, K)
    ei = toolbox.knn_edge_index_partitioned(x_local, part, K)
    g = Graph(ei, part.n_total, False, False, row_range=(part.row_begin, part.row_end))
    half_refused = False
    try:
        toolbox.knn_graph_partitioned(x_local.half(), part, K)
    except TypeError:
        half_refused = True
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), idx=idx.cpu().numpy(), sim=sim.cpu().numpy(), ei=ei.cpu().numpy(),
             graph=np.array([g.num_nodes, g.num_total_nodes, g.row_offset, g.num_edges]), half_refused=half_refused)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

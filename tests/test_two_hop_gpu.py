"""ops.two_hop_edge_index (csrc/h2gcn.hip: sngnn_two_hop_count / sngnn_two_hop_fill) exactly against the host reference
tests/h2gcn_ref.two_hop_ref: the canonical int64 [2, E2] edge list of the strict two-hop adjacency, array-equal.

The graph (h2gcn_ref.build_test_graph) has rows whose candidate bound is exactly TWO_HOP_HASH_MAX (the LDS table at its
fullest), TWO_HOP_HASH_MAX + 1 (the first bitmap row) and above, candidates that are the row itself or a direct
neighbour in both strategies, the node ids 63 and 64 as sources of both, duplicate edges, self loops, isolated nodes and
N % 64 != 0.  Actor's committed topology is the real graph; the degenerate cases are built here."""
import functools

import numpy as np
import pytest
import torch

from tests import graph_ref
from tests import h2gcn_ref as H

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _graph_cpu():
    from sngnn_amd import h2gcn
    return H.build_test_graph(h2gcn.TWO_HOP_HASH_MAX)


def _build(ei, n, cuda):
    from sngnn_amd import ops
    got = ops.two_hop_edge_index(torch.as_tensor(ei, dtype=torch.int64).to(cuda), n)
    assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 2 and got.size(0) == 2
    return got


def test_the_test_graph_is_built_exactly(cuda):
    from sngnn_amd import h2gcn
    ei, n, info = _graph_cpu()
    cb = H.candidate_bound(ei, n)
    assert cb[info["hash_row"]] == h2gcn.TWO_HOP_HASH_MAX and cb[info["above_row"]] == h2gcn.TWO_HOP_HASH_MAX + 1
    want = H.two_hop_ref(ei, n)
    got = _build(ei, n, cuda)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.shape[1] > 6000
    again = _build(ei, n, cuda)
    assert torch.equal(got, again)          # two builds are bit-identical


def test_actor_topology(cuda):
    import os
    z = np.load(os.path.join(H.HERE, "golden", "actor_topology.npz"))
    ei = np.asarray(z["edge_index"], dtype=np.int64)
    n = 7600
    want = H.two_hop_ref(ei, n)
    got = _build(ei, n, cuda)
    # (the binary pattern: 207 779 entries, largest row 1936, both from the host reference.  Counting paths instead - (A A
    # - A > 0) with the products' multiplicities - would keep 2180 direct neighbours with two or more paths: 209 959)
    assert want.shape[1] == 207779 and int(np.bincount(want[1], minlength=n).max()) == 1936
    assert np.array_equal(got.cpu().numpy(), want)


def _cases():
    path = np.stack([np.arange(0, 9), np.arange(1, 10)])
    return {
        "no edges": (np.zeros((2, 0), np.int64), 5),
        "one node": (np.zeros((2, 0), np.int64), 1),
        "one node, loops": (np.zeros((2, 3), np.int64), 1),
        "loops only": (np.stack([np.arange(7), np.arange(7)]), 7),
        "two-cycle": (np.array([[0, 1], [1, 0]]), 2),
        "path": (path, 10),
        "path with the shortcut": (np.concatenate([path, np.array([[0], [2]])], axis=1), 10),
        "duplicates": (np.concatenate([path, path, path[:, :4]], axis=1), 10),
        "ids 63 and 64": (np.array([[63, 64, 65, 62], [65, 65, 66, 66]]), 67),
        "bitmap of several chunks": _wide_fan(),
    }


def _wide_fan():
    """20 000 nodes, 1100 sources spread over all of them -> 1 -> 0 (a bitmap row whose map is read in three passes of
    256 words), with ids on both sides of the passes' boundaries (8191 | 8192, 16383 | 16384) and the last id."""
    n = 20000
    srcs = np.unique(np.concatenate([np.arange(2, n, 19), [8191, 8192, 16383, 16384, n - 1]]))[:1100]
    srcs = np.unique(np.concatenate([srcs, [8191, 8192, 16383, 16384, n - 1]]))
    ei = np.concatenate([np.stack([srcs, np.ones_like(srcs)]), np.array([[1, 8192], [0, 0]])], axis=1)
    return ei, n


@pytest.mark.parametrize("name", list(_cases()))
def test_degenerate_cases(cuda, name):
    ei, n = _cases()[name]
    want = H.two_hop_ref(ei, n)
    got = _build(ei, n, cuda)
    assert got.shape == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    if name == "path":
        assert want.shape[1] == 8
    if name == "path with the shortcut":
        pairs = set(zip(want[0].tolist(), want[1].tolist()))          # 0 -> 2 is an edge itself; 0 -> 2 -> 3 is new
        assert want.shape[1] == 8 and (0, 2) not in pairs and (0, 3) in pairs
    if name in ("two-cycle", "loops only", "no edges"):
        assert want.shape[1] == 0


def test_the_result_is_a_graph_the_build_takes(cuda):
    from sngnn_amd.graph import Graph
    ei, n, _ = _graph_cpu()
    e2 = _build(ei, n, cuda)
    g = Graph(e2, n, False, True)
    graph_ref.assert_csr(g, e2, n, False, True)
    assert g.num_edges == e2.size(1)
    # canonical: the CSR's column order is the list's own
    assert np.array_equal(g.array("col"), e2[0].cpu().numpy().astype(np.int32))


def test_refusals_return_their_codes(cuda):
    from sngnn_amd import _lib, ops
    from sngnn_amd.graph import LOOPS_REPLACE, Graph
    lib = _lib.load()
    ei, n, _ = _graph_cpu()
    eic = ei.to(cuda)
    count = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=cuda)
    stream = _lib.stream(cuda)
    with torch.cuda.device(cuda):
        for g in (Graph(eic, n, True, LOOPS_REPLACE), Graph(eic, n, False, False), Graph(eic, n, True, True),
                  Graph(eic, n, False, True, row_range=(0, n // 2))):
            assert lib.sngnn_two_hop_count(g.handle, count.data_ptr(), ws.data_ptr(), stream) == _lib.EINVAL
            assert b"loop-free" in lib.sngnn_last_error()
        assert lib.sngnn_two_hop_count(None, count.data_ptr(), ws.data_ptr(), stream) == _lib.EINVAL
        a1 = Graph(eic, n, False, True)
        offs = torch.zeros(n, dtype=torch.int64, device=cuda)
        out = torch.zeros((2, 4), dtype=torch.int64, device=cuda)
        assert lib.sngnn_two_hop_fill(a1.handle, offs.data_ptr(), 1 << 31, out.data_ptr(), ws.data_ptr(), stream) == _lib.ERANGE
        assert lib.sngnn_two_hop_fill(a1.handle, offs.data_ptr(), -1, out.data_ptr(), ws.data_ptr(), stream) == _lib.EINVAL
        assert lib.sngnn_two_hop_count(a1.handle, None, ws.data_ptr(), stream) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((count == -7).all()) and bool((out == 0).all())          # nothing was launched
    with pytest.raises(ValueError, match="GPU"):
        ops.two_hop_edge_index(ei, n)
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        ops.two_hop_edge_index(object(), n)

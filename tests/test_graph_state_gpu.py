"""Everything cached per graph lives in the ``Graph`` (``Graph.scratch`` / ``Graph.cached``): one scratch buffer per
(kind, parameters, stream) of the size the library asks for, and one copy of the CSR entries as device tensors
(``Graph.csr_entries``) shared by ``prop.prop_plain``, ``gat._plain_edges`` and GGCN's plain branch.

The graph: 300 nodes (the smallest that holds a 260-edge hub), 1200 random edges and node 3 with in-degree 260 - above
CHUNK = 128 twice over, so a split row of three tasks next to wave and small rows - loop-replaced."""
import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

_GRAPH = {}


def _graph(cuda):
    if "g" not in _GRAPH:
        from sngnn_amd.graph import LOOPS_REPLACE, Graph
        ei = helpers.random_graph(300, 1200, 11, hubs=((3, 260),))
        _GRAPH["g"] = Graph(ei.to(cuda), 300, True, LOOPS_REPLACE)
    return _GRAPH["g"]


def _cases(g):
    """(name, getter, getter with other parameters or None, the library's byte count of the first)."""
    from sngnn_amd import _lib
    from sngnn_amd.gat import gat_workspace
    from sngnn_amd.prop import prop_workspace
    lib, h = _lib.load(), g.handle
    return (("workspace", lambda: g.workspace(40), lambda: g.workspace(44), lib.sngnn_graph_workspace_bytes(h, 40)),
            ("head_workspace", g.head_workspace, None, lib.sngnn_agg_head_workspace_bytes(h)),
            ("prop_workspace", lambda: prop_workspace(g, 40, 3), lambda: prop_workspace(g, 40, 4),
             lib.sngnn_prop_workspace_bytes(h, 40, 3)),
            ("gat_workspace", lambda: gat_workspace(g, 8, 2), lambda: gat_workspace(g, 8, 4),
             lib.sngnn_gat_workspace_bytes(h, 2, 8)))


def test_one_scratch_buffer_per_kind_parameters_and_stream(cuda):
    g = _graph(cuda)
    for name, get, other, nbytes in _cases(g):
        ws = get()
        assert get() is ws, name
        assert ws.dtype == torch.uint8 and ws.device == g.device and ws.numel() == max(int(nbytes), 256), name
        if other is not None:
            assert other() is not ws and other() is other(), name
        with torch.cuda.stream(torch.cuda.Stream()):
            side = get()
            assert side is not ws and get() is side and side.numel() == ws.numel(), name
        assert get() is ws, name
    torch.cuda.synchronize()


def test_csr_entries_are_built_once_and_shared(cuda):
    from sngnn_amd import gat
    from sngnn_amd.prop import prop_plain
    g = _graph(cuda)
    entries = g.csr_entries()
    again = g.csr_entries()
    assert len(entries) == 3 and all(a is b for a, b in zip(entries, again))
    csc_eid, tgt, src = entries
    assert (csc_eid.dtype, tgt.dtype, src.dtype) == (torch.int64, torch.int32, torch.int32)
    rowptr = g.array("rowptr").astype(np.int64)
    assert int(np.diff(rowptr).max()) > 2 * 128          # (the hub: a split row of three tasks)
    want_tgt = np.repeat(np.arange(g.num_nodes, dtype=np.int32), np.diff(rowptr))
    assert np.array_equal(csc_eid.cpu().numpy(), g.array("csc_eid").astype(np.int64))
    assert np.array_equal(tgt.cpu().numpy(), want_tgt)
    assert np.array_equal(src.cpu().numpy(), g.array("col"))
    assert all(t.is_contiguous() and t.device == g.device and t.numel() == g.num_edges for t in entries)
    norm, aux = prop_plain(g)
    assert aux is entries and prop_plain(g)[1] is entries and norm.numel() == g.num_edges
    e_src, e_tgt = gat._plain_edges(g)
    assert e_src.dtype == torch.int64 and e_tgt.dtype == torch.int64
    assert torch.equal(e_src, src.long()) and torch.equal(e_tgt, tgt.long())
    assert all(a is b for a, b in zip(gat._plain_edges(g), (e_src, e_tgt)))

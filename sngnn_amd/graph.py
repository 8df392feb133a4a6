"""Device graph structure, built once per (edge_index, self-loop mode).

The reference redoes ``add_self_loops`` / ``remove_self_loops`` and the implicit
per-target grouping on every forward (models/models.py:117-120, 234-236, 323);
here the C library builds CSR-by-target / CSC-by-source once and the conv layers
look it up in a small cache keyed on the identity and version of ``edge_index``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib

_ARRAYS = {"rowptr": 0, "col": 1, "eid": 2, "cscptr": 3, "csc_eid": 4, "rperm": 5,
           "csc_dst": 6, "csc_pos": 7, "sperm": 8, "rdesc": 9, "col_s": 10, "rperm_b": 11, "rdesc_b": 12,
           "col_s_b": 13, "sdesc": 14, "fdesc": 15, "trest": 16, "task_slot": 17, "task_chunk": 18,
           "task_order": 19, "split_soff": 20, "split_task0": 21, "stask_slot": 22, "stask_chunk": 23,
           "ssplit_task0": 24, "csc_bit": 25, "inv_deg": 26}
_DESCRIPTORS = ("rdesc", "rdesc_b", "sdesc", "fdesc", "trest")          # int4 per entry

LOOPS_REPLACE = _lib.LOOPS_REPLACE


class Graph:
    """Owns a ``sngnn_graph_t`` handle."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, add_loops: bool,
                 remove_loops: bool, row_range=None):
        """``row_range=(begin, end)`` builds the node-range partition that owns the
        targets [begin, end) of a ``num_nodes``-node graph (global ids in
        ``edge_index``); ``None`` is the whole graph."""
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
        if not edge_index.is_cuda:
            raise ValueError("edge_index must live on the GPU (there is no CPU path)")
        lib = _lib.load()
        ei = edge_index.contiguous()
        self.device = ei.device
        # remove_loops: False/True as in the SNConv layers, or LOOPS_REPLACE (AGNNConv's order)
        self.add_loops, self.remove_loops = bool(add_loops), int(remove_loops)
        handle = C.c_void_p()
        r0, r1 = (0, int(num_nodes)) if row_range is None else map(int, row_range)
        # (not through _lib.call: the stream is not this entry's last argument - the handle comes after it)
        with torch.cuda.device(self.device):
            rc = lib.sngnn_graph_create_partition(ei.data_ptr(), ei.size(1), int(num_nodes), r0, r1, int(add_loops),
                                                  int(remove_loops), _lib.stream(self.device), C.byref(handle))
        _lib.check(rc, "sngnn_graph_create_partition")
        self._h = handle
        self.num_nodes = int(lib.sngnn_graph_num_nodes(handle))            # owned rows
        self.num_total_nodes = int(lib.sngnn_graph_num_total_nodes(handle))
        self.row_offset = int(lib.sngnn_graph_row_offset(handle))
        self.num_edges = int(lib.sngnn_graph_num_edges(handle))
        self.max_in_degree = int(lib.sngnn_graph_max_in_degree(handle))
        self.num_fused_nodes = int(lib.sngnn_graph_num_fused_nodes(handle))    # in- and out-degree <= 16 (node-centric backward)
        self.src_min = int(lib.sngnn_graph_src_min(handle))
        self._ws: Dict[Tuple, object] = {}          # everything cached per graph: scratch() and cached()

    @property
    def handle(self):
        return self._h

    def scratch(self, entry: str, a=None, b=None) -> torch.Tensor:
        """Scratch sized by the library's ``entry(handle[, a[, b]])``: one uint8 buffer per (entry, a, b, stream), so
        calls on the same graph from different streams never share scratch (the entry points are re-entrant per
        stream).  Allocated on first use - ``GraphedEpoch`` runs an eager pass on the very stream it then captures on,
        so the capture finds its buffers - and kept as long as the graph lives."""
        key = (entry, a, b, _lib.stream(self.device))
        ws = self._ws.get(key)
        if ws is None:
            nbytes = int(getattr(_lib.load(), entry)(self._h, *(p for p in (a, b) if p is not None)))
            ws = self._ws[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        return ws

    def cached(self, key, build):
        """Any other object kept with the graph: ``build(graph, key)`` on first use, that object from then on."""
        hit = self._ws.get(key)
        if hit is None:
            hit = self._ws[key] = build(self, key)
        return hit

    def workspace(self, channels: int) -> torch.Tensor:
        """Scratch for forward/backward at ``channels`` (one buffer per width and stream: :meth:`scratch`)."""
        return self.scratch("sngnn_graph_workspace_bytes", channels)

    def head_workspace(self) -> torch.Tensor:
        """Scratch of the classification head inside this graph's forward (``sngnn_epilogue_t.head_workspace``): a
        captured epoch that holds the graph holds the buffer its launches point into."""
        return self.scratch("sngnn_agg_head_workspace_bytes")

    def csr_entries(self):
        """(csc_eid int64 [E'], tgt int32 [E'], src int32 [E']) on the device: the CSC -> CSR map and the row and
        column of every CSR entry - the ``aux`` of ``ops.weighted_propagate``.  Built on first use (copies the
        structure arrays through the host once)."""
        return self.cached("csr_entries", _csr_entries)

    def array(self, name: str) -> np.ndarray:
        """Host copy of one of the structure arrays (tests / inspection): int32, ``[-1, 4]`` for the descriptor
        arrays, float32 for ``inv_deg``; empty for an array the build left out (``csc_bit`` of a partition)."""
        which = _ARRAYS[name]
        lib = _lib.load()
        n = int(lib.sngnn_graph_array_len(self._h, which))
        if n < 0:
            raise ValueError(f"the library knows no array {name!r} (id {which})")
        out = np.empty(max(n, 1), dtype=np.int32)[:n]       # (never a NULL destination)
        # (not through _lib.call: a blocking copy to host memory, the entry takes no stream)
        _lib.check(lib.sngnn_graph_copy_array(self._h, which, out.ctypes.data), "sngnn_graph_copy_array")
        if name in _DESCRIPTORS:
            return out.reshape(-1, 4)
        return out.view(np.float32) if name == "inv_deg" else out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().sngnn_graph_destroy(h)
            except Exception:
                pass
            self._h = None


def _csr_entries(graph: Graph, _key):
    dev = graph.device
    src = torch.from_numpy(graph.array("col")).to(dev)
    rowptr = torch.from_numpy(graph.array("rowptr").astype("int64")).to(dev)
    tgt = torch.repeat_interleave(torch.arange(graph.num_nodes, device=dev, dtype=torch.int32),
                                  rowptr[1:] - rowptr[:-1])
    csc_eid = torch.from_numpy(graph.array("csc_eid").astype("int64")).to(dev)
    return csc_eid, tgt.contiguous(), src.contiguous()


class GraphCache:
    """Per-module cache: (edge_index storage, shape, version, loop mode) -> Graph."""

    def __init__(self, max_entries: int = 4):
        self._entries: Dict[Tuple, Tuple[Graph, torch.Tensor]] = {}
        self._max = max_entries
        self._recording = None          # list of graphs handed out while record() is active

    def get(self, edge_index: torch.Tensor, num_nodes: int, add_loops: bool,
            remove_loops: bool, row_range=None) -> Graph:
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version,
               int(num_nodes), bool(add_loops), int(remove_loops), str(edge_index.device),
               None if row_range is None else tuple(map(int, row_range)))
        hit = self._entries.get(key)
        if hit is None:
            if len(self._entries) >= self._max:
                self._entries.pop(next(iter(self._entries)))
            # the entry keeps edge_index alive, so its address cannot be recycled
            # for a different tensor while the key is cached
            hit = (Graph(edge_index, num_nodes, add_loops, remove_loops, row_range), edge_index)
            self._entries[key] = hit
        if self._recording is not None and not any(g is hit[0] for g in self._recording):
            self._recording.append(hit[0])
        return hit[0]

    def note(self, graph: Graph) -> None:
        """A graph built outside this cache (the relation-sorted graph of ``ops.TypedAdjacency``) that a forward is
        about to launch on: collected by an active :meth:`record` like the graphs ``get`` hands out."""
        if self._recording is not None and not any(g is graph for g in self._recording):
            self._recording.append(graph)

    def record(self):
        """Context manager: collects the Graph objects ``get`` hands out inside it (the graphs a
        captured epoch launches on - what its owner must keep alive)."""
        cache = self

        class _Rec:
            def __enter__(self):
                cache._recording = self.graphs = []
                return self.graphs

            def __exit__(self, *exc):
                cache._recording = None
                return False
        return _Rec()

    def snapshot(self):
        """The Graph objects currently cached.  Whoever captured raw pointers of them (a HIP
        graph holds the CSR arrays and the workspaces of the graphs its kernels were launched
        on) keeps this list, so eviction from the cache cannot free them under the capture."""
        return [g for g, _ in self._entries.values()]

    def clear(self):
        self._entries.clear()


# Graphs are shared between the layers of a model (same edge_index, same mode).
GLOBAL_CACHE = GraphCache(max_entries=16)

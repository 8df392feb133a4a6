"""Host reference of the graph build: every derived array of ``sngnn_graph_t`` from the edge list, in numpy.

Written from the definitions (sort key + stability), not from the library: every order below is a
``kind="stable"`` argsort of a key, every pointer array a count, every descriptor a gather.  ``build`` returns a
dict with one entry per name of ``sngnn_amd.graph._ARRAYS`` (same dtype and shape as ``Graph.array`` returns)
plus the scalars; tests compare with ``np.array_equal`` - there is no tolerance anywhere, ``inv_deg`` included
(one correctly rounded fp32 division per row on both sides).

Definitions (thresholds: small <= 16 < wave <= 128 < split; 128 entries per task):
  E'         the original edges in order, then (add_loops and remove_loops != 1) one loop per OWNED node in node
             order; dropped: every loop (remove_loops == 1), the original loops only (== 2), every edge whose
             target is outside [row0, row1).  Targets become local (minus row0), sources stay global.
  eid        stable argsort of the local target; col = src[eid]; rowptr / cscptr counts (cscptr over N_total)
  csc_eid    stable argsort of col; csc_dst the local target of each CSC entry; csc_pos the inverse of csc_eid
  rperm      stable descending sort by in-degree;  rperm_b by (deg if deg > 16 else ceil(deg / 4) * 4)
  rdesc*[p]  {row, rowptr[row], deg, first entry of slot p in col_s*};  col_s* the rows' columns in slot order
  sperm      stable descending sort of ALL N_total sources by (out-degree if > 16, else 15 if fused, else 16);
             fused = owned, in-degree <= 16 and out-degree <= 16;  sdesc[p] = {source, cscptr, out-degree, 0}
  fdesc      the fused nodes in natural order {node, rowptr[local], cscptr[node], in-degree | out-degree << 8}
  trest      owned rows with in-degree <= 16 < out-degree, natural order {local row, rowptr, deg, 0}
  tasks      one per 128 entries of every split row (source), slot order; split_task0 / ssplit_task0 / split_soff
             the running task / task / edge counts
  csc_bit    whole graphs with edges only.  wbase = ceil(ceil(N / 2) / 4) * 4, tbase = wbase + 4 * (wave rows),
             words = tbase + 4 * n_tasks; entry t of row i: small 16 i + t; wave row at slot p
             32 wbase + 128 (p - n_split) + t; split row 32 tbase + 128 split_task0[p] + t
  task_order any permutation of the tasks is correct; ``dealt_order`` restates the placement rule separately

Outcome of the first comparison against the library (all graphs of tests/test_graph_build_gpu.py): no definition
above had to be changed to match the consumers; see that module's docstring for what was found.
"""
from __future__ import annotations

import numpy as np

SMALL, WAVE, TASK = 16, 128, 128
DEAL_GROUP, DEAL_SLICES = 4, 8             # position q of the dealing order takes from slice (q / 4) % 8

INT_ARRAYS = ("rowptr", "col", "eid", "cscptr", "csc_eid", "rperm", "csc_dst", "csc_pos", "sperm", "rdesc", "col_s",
              "rperm_b", "rdesc_b", "col_s_b", "sdesc", "fdesc", "trest", "task_slot", "task_chunk", "split_soff",
              "split_task0", "stask_slot", "stask_chunk", "ssplit_task0", "csc_bit")
ARRAYS = INT_ARRAYS + ("inv_deg", "task_order")
SCALARS = ("num_nodes", "num_total_nodes", "row_offset", "num_edges", "max_in_degree", "src_min", "num_fused_nodes")


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _desc(*cols):
    return _i32(np.stack([np.asarray(c, dtype=np.int64) for c in cols], axis=1)) if len(cols[0]) else \
        np.zeros((0, 4), np.int32)


def _ptr(ids, n):
    p = np.zeros(n + 1, np.int64)
    p[1:] = np.cumsum(np.bincount(ids, minlength=n)[:n]) if n else 0
    return p


def _desc_order(key):
    return np.argsort(-np.asarray(key, np.int64), kind="stable")


def edge_list(ei, n_total, row_range=None, add_loops=True, remove_loops=0):
    """E' as (src global, dst global) int64 arrays, in list order."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    row0, row1 = (0, n_total) if row_range is None else map(int, row_range)
    src, dst = ei[0], ei[1]
    original = np.ones(src.size, bool)
    if add_loops and remove_loops != 1:
        own = np.arange(row0, row1, dtype=np.int64)
        src, dst = np.concatenate([src, own]), np.concatenate([dst, own])
        original = np.concatenate([original, np.zeros(own.size, bool)])
    loop = src == dst
    drop = loop if remove_loops == 1 else (loop & original if remove_loops == 2 else np.zeros(src.size, bool))
    keep = ~drop & (dst >= row0) & (dst < row1)
    return src[keep], dst[keep]


def _tasks(deg_slot, n_split):
    nch = -(-deg_slot[:n_split] // TASK)
    slot = np.repeat(np.arange(n_split), nch)
    task0 = np.concatenate([[0], np.cumsum(nch)])
    chunk = np.arange(slot.size) - task0[slot]
    soff = np.concatenate([[0], np.cumsum(deg_slot[:n_split])])
    return _i32(slot), _i32(chunk), _i32(task0), _i32(soff)


def _rows_in_slot_order(perm, rowptr, deg, col):
    first = np.concatenate([[0], np.cumsum(deg[perm])])[:-1] if perm.size else np.zeros(0, np.int64)
    desc = _desc(perm, rowptr[perm], deg[perm], first)
    # entry q of the stream belongs to the slot whose range holds it
    slot = np.repeat(np.arange(perm.size), deg[perm])
    within = np.arange(col.size) - first[slot] if col.size else np.zeros(0, np.int64)
    col_s = col[rowptr[perm][slot] + within] if col.size else np.zeros(0, np.int64)
    return desc, _i32(col_s)


def build(ei, n_total, row_range=None, add_loops=True, remove_loops=0):
    row0, row1 = (0, n_total) if row_range is None else map(int, row_range)
    n = row1 - row0
    src, dst = edge_list(ei, n_total, (row0, row1), add_loops, remove_loops)
    dl = dst - row0
    r = {"ei": np.stack([src, dst])}
    eid = np.argsort(dl, kind="stable")
    col = src[eid]
    rowptr, cscptr = _ptr(dl, n), _ptr(src, n_total)
    deg, odeg = np.diff(rowptr), np.diff(cscptr)
    csc_eid = np.argsort(col, kind="stable")
    row_of_entry = dl[eid]
    csc_pos = np.empty(col.size, np.int64)
    csc_pos[csc_eid] = np.arange(col.size)
    r.update(rowptr=_i32(rowptr), col=_i32(col), eid=_i32(eid), cscptr=_i32(cscptr), csc_eid=_i32(csc_eid),
             csc_dst=_i32(row_of_entry[csc_eid]), csc_pos=_i32(csc_pos),
             inv_deg=(np.float32(1) / np.maximum(deg, 1).astype(np.float32)).astype(np.float32))

    rperm = _desc_order(deg)
    rperm_b = _desc_order(np.where(deg > SMALL, deg, -(-deg // 4) * 4))
    r["rperm"], r["rperm_b"] = _i32(rperm), _i32(rperm_b)
    r["rdesc"], r["col_s"] = _rows_in_slot_order(rperm, rowptr, deg, col)
    r["rdesc_b"], r["col_s_b"] = _rows_in_slot_order(rperm_b, rowptr, deg, col)
    if n == 0:          # the streaming order of a graph without rows is not built
        r["col_s_b"] = np.zeros(0, np.int32)

    owned = np.zeros(n_total, bool)
    owned[row0:row1] = True
    deg_g = np.full(n_total, SMALL + 1, np.int64)          # in-degree by GLOBAL id; not owned: never fused
    deg_g[row0:row1] = deg
    fused = owned & (deg_g <= SMALL) & (odeg <= SMALL)
    sperm = _desc_order(np.where(odeg > SMALL, odeg, np.where(fused, SMALL - 1, SMALL)))
    r["sperm"] = _i32(sperm)
    r["sdesc"] = _desc(sperm, cscptr[sperm], odeg[sperm], np.zeros(n_total))
    fn = np.flatnonzero(fused)
    r["fdesc"] = _desc(fn, rowptr[fn - row0], cscptr[fn], deg[fn - row0] | (odeg[fn] << 8))
    tr = np.flatnonzero((deg <= SMALL) & (odeg[row0:row1] > SMALL))
    r["trest"] = _desc(tr, rowptr[tr], deg[tr], np.zeros(tr.size))

    n_split, n_wave = int((deg > WAVE).sum()), int(((deg > SMALL) & (deg <= WAVE)).sum())
    r["task_slot"], r["task_chunk"], r["split_task0"], r["split_soff"] = _tasks(deg[rperm], n_split)
    r["stask_slot"], r["stask_chunk"], r["ssplit_task0"], _ = _tasks(odeg[sperm], int((odeg > WAVE).sum()))
    n_tasks = r["task_slot"].size

    halfwords = (n + 1) // 2                                # one halfword per row, two per word
    wbase = (halfwords + 3) // 4 * 4
    tbase = wbase + 4 * n_wave
    words = tbase + 4 * n_tasks
    r["csc_bit"] = np.zeros(0, np.int32)
    r["kept_bits_bytes"] = 0
    if n == n_total and col.size > 0:
        slot_of_row = np.empty(n, np.int64)
        slot_of_row[rperm] = np.arange(n)
        i = row_of_entry                                   # per CSR entry
        t = np.arange(col.size) - rowptr[i]
        p = slot_of_row[i]
        task0 = np.concatenate([r["split_task0"].astype(np.int64), np.zeros(n, np.int64)])[np.minimum(p, n_split)]
        bit = np.where(deg[i] <= SMALL, 16 * i + t,
                       np.where(deg[i] <= WAVE, 32 * wbase + 128 * (p - n_split) + t, 32 * tbase + 128 * task0 + t))
        assert np.unique(bit).size == bit.size and bit.min() >= 0 and bit.max() < 32 * words, \
            "kept-bit map is not injective into [0, 32 * words)"
        r["csc_bit"] = _i32(bit[csc_eid])
        r["kept_bits_bytes"] = 4 * words
    r.update(kb_wbase=wbase, kb_tbase=tbase, kb_words=words, n_tasks=n_tasks, n_split=n_split,
             num_nodes=n, num_total_nodes=n_total, row_offset=row0, num_edges=int(col.size),
             max_in_degree=int(deg.max()) if n else 0, src_min=int(col.min()) if col.size else 0,
             num_fused_nodes=int(fn.size))
    r["task_order"] = dealt_order(r)
    return r


def dealt_order(r):
    """The placement rule of ``task_order`` restated: a task's slice (of 8 equal source ranges) is the slice of
    its middle edge; position q takes the next task of slice (q / 4) % 8, or of the fullest slice (the first of
    equals) when that one is exhausted.  A mismatch here means "placement changed", not "wrong"."""
    n_tasks, n_total = int(r["n_tasks"]), int(r["num_total_nodes"])
    if n_tasks == 0:
        return np.zeros(0, np.int32)
    d = r["rdesc"][r["task_slot"]].astype(np.int64)
    e0 = r["task_chunk"].astype(np.int64) * TASK
    e1 = np.minimum(d[:, 2], e0 + TASK)
    mid = r["col"].astype(np.int64)[d[:, 1] + (e0 + e1) // 2]
    slc = np.minimum(mid * DEAL_SLICES // max(n_total, 1), DEAL_SLICES - 1)
    queues = [list(np.flatnonzero(slc == x)) for x in range(DEAL_SLICES)]
    order = []
    for q in range(n_tasks):
        x = (q // DEAL_GROUP) % DEAL_SLICES
        if not queues[x]:
            x = max(range(DEAL_SLICES), key=lambda y: (len(queues[y]), -y))
        order.append(queues[x].pop(0))
    return _i32(order)


def library_arrays(g):
    """Every array of a built ``sngnn_amd.graph.Graph`` plus its scalars, keyed like ``build``'s result."""
    from sngnn_amd import _lib
    got = {name: g.array(name) for name in ARRAYS}
    got.update({s: getattr(g, s) for s in SCALARS})
    got["kept_bits_bytes"] = int(_lib.load().sngnn_graph_kept_bits_bytes(g.handle))
    return got


def differing(got, ref, names):
    """Names among ``names`` whose library value is not exactly the reference's (dtype, shape and every element)."""
    bad = []
    for name in names:
        a, b = got[name], ref[name]
        if isinstance(b, np.ndarray):
            same = a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
        else:
            same = a == b
        if not same:
            bad.append(name)
    return bad


def assert_csr(g, ei, n_total, add_loops, remove_loops, row_range=None):
    """The built graph's CSR is EXACTLY the edge list's: ``rowptr``, ``col`` and ``eid`` (stable order inside a
    row), so an arbiter fed ``g.array("rowptr")`` / ``g.array("col")`` is fed the true graph.  Returns the
    reference (rowptr, col) as int64."""
    ref = build(np.asarray(ei.cpu() if hasattr(ei, "cpu") else ei), int(n_total), row_range, bool(add_loops),
                int(remove_loops))
    for name in ("rowptr", "col", "eid"):
        got = g.array(name)
        assert got.shape == ref[name].shape and np.array_equal(got, ref[name]), \
            f"graph build: {name} differs from the edge list's (N_total {n_total}, rows {row_range}, " \
            f"add_loops {add_loops}, remove_loops {remove_loops})"
    return ref["rowptr"].astype(np.int64), ref["col"].astype(np.int64)


# ---- the graphs both test modules use -------------------------------------------------------------------------
FIVE_NODES = 5
# a duplicated edge (1 -> 0 at positions 0 and 3), two original loops (2, 3), an isolated node (4)
FIVE_EDGES = np.array([[1, 2, 3, 1, 0, 3, 2, 0],
                       [0, 2, 1, 0, 3, 3, 0, 1]], dtype=np.int64)
# worked by hand, keyed by (add_loops, remove_loops)
FIVE_EXPECTED = {
    (0, 0): dict(rowptr=[0, 3, 5, 6, 8, 8], col=[1, 1, 2, 3, 0, 2, 0, 3], eid=[0, 3, 6, 2, 7, 1, 4, 5],
                 cscptr=[0, 2, 4, 6, 8, 8], csc_eid=[4, 6, 0, 1, 2, 5, 3, 7]),
    # E' = (1,0) (3,1) (1,0) (0,3) (2,0) (0,1) then (0,0) (1,1) (2,2) (3,3) (4,4)
    (1, 2): dict(rowptr=[0, 4, 7, 8, 10, 11], col=[1, 1, 2, 0, 3, 0, 1, 2, 0, 3, 4],
                 eid=[0, 2, 4, 6, 1, 5, 7, 8, 3, 9, 10], cscptr=[0, 3, 6, 8, 10, 11],
                 csc_eid=[3, 5, 8, 0, 1, 6, 2, 7, 4, 9, 10]),
}

BOUNDARY_NODES = 700
BOUNDARY_DEGREES = (0, 3, 4, 5, 8, 9, 12, 13, 15, 256, 257)


def boundary_graph(seed=11):
    """700 nodes whose in-degrees and out-degrees (no loop added) each hit every value of BOUNDARY_DEGREES - the
    edges of the 4-degree buckets and exact multiples of the task size.  Node i < 11 is the TARGET of degree
    BOUNDARY_DEGREES[i] with no out-edge (9, 10: large as a target, small as a source: not fused); node 20 + i the
    SOURCE of that degree with no in-edge (29, 30: small as a target, large as a source: ``trest``).  The other
    ends come from the pool 100 .. 699, which also carries 600 background edges with duplicates and 5 loops."""
    rng = np.random.default_rng(seed)
    pool = np.arange(100, BOUNDARY_NODES)
    src, dst = [], []
    for i, d in enumerate(BOUNDARY_DEGREES):
        src.append(rng.choice(pool, size=d, replace=False)), dst.append(np.full(d, i))
        src.append(np.full(d, 20 + i)), dst.append(rng.choice(pool, size=d, replace=False))
    bg = rng.choice(pool, size=(2, 560))
    loops = np.array([100, 250, 400, 401, 699])
    src += [bg[0], bg[0, :35], loops]
    dst += [bg[1], bg[1, :35], loops]
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    return ei[:, rng.permutation(ei.shape[1])], BOUNDARY_NODES


def star(n=300, inward=True):
    """Every other node points at node n - 1 (``inward``) or node n - 1 at every other node."""
    others, hub = np.arange(n - 1, dtype=np.int64), np.full(n - 1, n - 1, dtype=np.int64)
    return (np.stack([others, hub]) if inward else np.stack([hub, others])), n


def sized_graph(n, e, seed):
    """Exactly ``e`` random edges on ``n`` nodes in random order: three hub targets that take a quarter of the
    edges between them, three hub sources likewise - many equal keys in both sorts - and the last node id on
    both sides."""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, size=e), rng.integers(0, n, size=e)
    hubs_t, hubs_s = rng.choice(n, size=3, replace=False), rng.choice(n, size=3, replace=False)
    q = e // 4
    dst[:q] = hubs_t[rng.integers(0, 3, size=q)]
    src[q:2 * q] = hubs_s[rng.integers(0, 3, size=q)]
    src[-1], dst[-1] = n - 1, n - 1
    p = rng.permutation(e)
    return np.stack([src[p], dst[p]]).astype(np.int64), n

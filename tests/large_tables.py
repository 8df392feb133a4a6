"""Tables past 2 GiB and 4 GiB without a reference at size: the "blocks" construction of tests/test_large_tables_gpu.py
and tests/test_large_dense_gpu.py, and the placement arithmetic that tests/test_large_tables_cpu.py checks.

A *block* is the 3 000-node graph of tests/test_fwd_buffer_addr_gpu.py (``edges()``: in-degrees 0, 1, 2, 16, 17, 128,
129, 300 and 2 999, node 0 and node n - 1 are sources, the last table value is not zero).  A big graph of ``ntot``
nodes holds translated copies of that edge list at the offsets ``Placement.offsets`` and nothing else; its table is the
block's rows repeated with period P = 3 000 (``periodic``: built on the device), with the block's rows written once more
at every offset that is no multiple of P (a block that has to END at row ntot - 1).  A row's result does not depend on
where its block sits, so every block's results equal the near block's bit for bit, and those equal the results of the
3 000-node problem alone: no reference of the big problem is needed.

Blocks (``place``): the near block at 0; for every byte boundary B one block with the row that contains byte B strictly
inside it; a last block that ends at row ntot - 1.  Without a given ``ntot`` it is the smallest that fits them: the
block of the largest boundary is the last one.


The 32-bit quantities of the entries these tests run at such sizes, read in the sources before the first run
-------------------------------------------------------------------------------------------------------------------
(widest 32-bit quantity the kernel forms -> what keeps it in range)

sngnn_agg_forward* / _epilogue, work-item roles, buffer form (agg_fwd_src.h FwdSrc<true>): row offset
    ``(unsigned)j * 4C`` + lane term, ``(unsigned)Ntot * 4C`` as the resource size, ``(unsigned)n_edges * 4``,
    ``(unsigned)N * 16``, ``(unsigned)Ntot * filter_row_bytes`` -> taken only when fwd_plan.h: fwd_buffer_form holds:
    table_bytes < 2^31 and max(4 E', 16 N) < 2^31; filter rows have at most half a table's bytes; BUF_OOB = 2^31 is
    then beyond every resource and ``buf_off_add_sat`` keeps BUF_OOB + lane term from wrapping.
sngnn_agg_forward*, flat form (FwdSrc<false>) and every finalize (agg_fwd_fin.h), stores of out / sel_src / sel_w /
    partial rows: ``int`` row, edge and task ids (N, Ntot, E' are int32 by the graph build's own guard); every product
    with C or k is formed after a ``(size_t)`` cast.  ``cand_slot``: (n_tasks * 32) as unsigned, n_tasks <= E' / 128.
k_normalize_rows / k_filter_rows: rows are ``int64_t``, ``r * C`` is a 64-bit product, the grid is capped at
    8 192 workgroups and strides.
k_fill_sel: ``int64_t`` flat index, grid capped at 2 048.
workspace offsets (ws_layout.h): all ``int64_t``.
sngnn_agg_forward_half: the flat form only (agg_fwd.hip: ``buf`` needs dtype 0); as above.
sngnn_agg_backward_topk / _bits / _half (agg_bwd_impl.h): ``int`` node, edge and task ids; every row address is
    ``(size_t)id * a.C`` (every product with a.C in that header carries the cast); no buffer resources on this side.
sngnn_attn_forward / _backward, sngnn_signed_forward / _backward (attn_impl.h, signed_impl.h): ``int`` ids, every row
    address ``(size_t)id * a.C``; the split rows' partials ``t * stride`` with ``size_t stride = 2 C + 4``.
sngnn_adj_linear_forward / _backward, sngnn_weighted_gather_sum_rows / _scatter_sum_rows, sngnn_pair_dot_rows
    (adj_linear_impl.h on row_walk.h): gather_rows forms ``(size_t)row * ld`` with ``int64_t ld``; stores
    ``(size_t)r * a.C``; k_adj_tail counts ``(int64_t)(N - first_row) * C``; pair ids are int32 node ids.
sngnn_gcn_hop (gcn.hip on row_walk.h): five ``int64_t`` row strides, every address ``(size_t)r * ld``; the entry checks
    strides against widths and the slices against each other before it launches.
sngnn_prop_gpr_forward / _backward, sngnn_prop_appnp (prop.hip on row_walk.h): ``(size_t)r * a.C``; the element-wise
    k_prop_init runs on ``int64_t n = N * C`` with a capped grid.
sngnn_linear_forward (linear.hip): k_linear_rows forms ``(unsigned)N * F * 4``, ``(unsigned)N * C * 4`` and tile offsets
    ``(unsigned)tile * 16 * F * 4`` up to two grid strides (<= 2 048 tiles, 16 MiB at F = 128) past the table -> entered
    only when N F 4 and N C 4 are below lim = 2^31 - 64 MiB; k_linear_fwd (beyond): ``int64_t`` rows, 64-bit ``r * F``,
    grid ``(unsigned)ceil(N / 128)``.
sngnn_linear_forward_normalized: the same kernel with three more resources, ``(unsigned)N * C * 4`` for h and the unit
    rows, and BUF_OOB as the offset of the lanes beyond C (C in 36 .. 60: 16 lanes per row) ->
    sngnn_linear_normalized_supported.  FOUND WRONG: it held N F 4 and 128 N below lim but not N C 4, so at
    C > 32 and F <= 32 a table h of 2^31 bytes or more was accepted, for which BUF_OOB is IN range: the lanes beyond C
    stored zeros over the 16 bytes at byte 2^31 of h and of the unit rows.  The guard now holds N C 4 below lim too
    (test_large_dense_gpu.py: test_linear_normalized_guard).
sngnn_linear_forward_masked: k_linear_fwd only (above); ``min(rr, N - 1) * C`` is a 64-bit product.
sngnn_linear_wgrad (head.hip, linear.hip): k_wgrad_mfma forms ``(unsigned)N * C * 4``, ``(unsigned)N * F * 4`` and block
    offsets ``(unsigned)blk * 16 * F * 4`` -> wgrad_mfma_partials returns 0 unless both tables are below lim, and each
    launch takes a slab of 2^20 rows through pointers advanced in 64 bits (``g + r0 * C`` with ``int64_t r0``);
    k_wgrad_partial (beyond): ``int64_t`` rows and 64-bit ``(ib + r) * F``; its grid's z is ceil(N / 512), which the
    launch itself limits to 65 535 (N <= 33.5 M rows: beyond it the launch is refused and reported, nothing runs).
sngnn_replica_wgrad (replicas.hip): ``int64_t`` rows, ``((int64_t)rep * N + ib + r) * C``; refuses N R >= 2^31
    ("too many stacked rows").
sngnn_blend_forward / _backward, sngnn_epilogue_backward (blend.hip): flat ``int64_t`` indices and strides; grids capped
    (``blend_grid``: at most BLEND_BLOCKS workgroups; k_mask_grad: 2 048) and computed in ``int64_t`` before the cast.
sngnn_gcn2_hop (gcn2.hip on row_walk.h): ``(size_t)r * C`` through gather_rows and the store; sngnn_gcn2_map:
    ``int64_t row0 = tile * MAP_ROWS``, 64-bit ``row0 * C``.
sngnn_h2gcn_hop (h2gcn.hip on row_walk.h): ``int64_t`` strides of both slices, ``(size_t)row * ld``; the two-hop build
    refuses more than 2^31 - 1 entries (tests/test_two_hop_gpu.py).
sngnn_gat_scores / _forward / _backward (gat.hip): node * heads as ``int`` -> "N * heads must fit 31 bits"; row
    addresses ``(size_t)j * ld`` with ``int64_t ld``; head offsets ``h * C`` <= 512.
sngnn_wrgat_* (wrgat.hip): node * relations as ``int`` -> "N * relations must fit 31 bits"; k_wr_gmask runs on
    ``int64_t i`` and ``(i / C) * ldd`` with ``int64_t ldd``.
sngnn_acm_forward / _backward (acm.hip on row_walk.h): rows of P 3 C floats apart, ``(size_t)r * ld``; column offsets
    ``2 * C + c`` <= 768.
sngnn_glognn_forward / _backward (glognn.hip): the hop shares gather_rows (``(size_t)row * ld``); the C x C matrices
    are indexed ``i * C + k`` with C <= 64; the Gram kernel strides rows in ``int64_t``.
sngnn_ggcn_transition_* (ggcn.hip), sngnn_jk_max_* (jk.hip): flat ``int64_t`` element indices, capped grids.
sngnn_head_nll / _nll2 (head.hip): ``int64_t`` rows (``blk * HEAD_ROWS_PER_BLOCK``), grids capped at HEAD_MAX_BLOCKS; the
    correct count leaves as fp32: exact below 2^24 rows selected.
sngnn_replica_unpack (replicas.hip): ``int64_t`` union rows, ``i * stride + r * C`` in 64 bits.
sngnn_linkx_join_* (linkx.hip): ``int64_t row0 = tile * JOIN_ROWS``, ``row0 * H`` and ``row0 * (2 * H)`` in 64 bits.
sngnn_bn_train_* / sngnn_bn_post_* (batchnorm.hip): rows strided in ``int64_t``; the seeded dropout hashes the upper half
    of the 64-bit element index separately (device_utils.h: sn_dropout_keep).
sngnn_edge_cosine, sngnn_segment_mean, sngnn_cosine_dense (toolbox.hip): ``int64_t`` N, F, E and rows; the dense result
    is indexed through ``int64_t`` (mr, mc) and ``(size_t)split * N * N``.
sngnn_graph_create_partition (graph.hip) at 13.4 M nodes: E + N and Ntot below 2^31 - 1 by the entry's own guard.
"""
from collections import namedtuple

import torch

from tests.test_fwd_buffer_addr_gpu import N as P           # the block's node count
from tests.test_fwd_buffer_addr_gpu import edges, rows      # noqa: F401  (the block itself: reused, not copied)

Placement = namedtuple("Placement", "ntot offsets boundary_rows")


B31, B32 = 2 ** 31, 2 ** 32
LIN_LIM = 2 ** 31 - 64 * 2 ** 20        # linear.hip: lim, the buffer-addressed kernels' table limit

# every (row size, boundaries, ntot or None) the GPU tests place blocks for: name -> arguments of place()
CASES = {
    # fp32 rows of 512 channels (2 048 bytes)
    "c512_last_buffer": (2048, (), B31 // 2048 - 1),        # 2^31 - 2 048 bytes: the largest table of the buffer form
    "c512_first_flat": (2048, (), B31 // 2048),             # exactly 2^31 bytes
    "c512_past_4gib": (2048, (B31, B32), None),
    # the benchmark's width: 160-byte rows on either side of 2^31 bytes
    "c40_last_buffer": (160, (), 13421772),
    "c40_first_flat": (160, (), 13421773),
    # sngnn_gcn_hop: a 512-column slice of a table of 640 columns (2 560-byte rows)
    "gcn_slice": (2560, (B31, B32), None),
    # sngnn_acm_*: [N, 3 C] at C = 256 (3 072-byte rows); sngnn_glognn_*: 64 channels, its widest row (256 bytes)
    "acm": (3072, (B31, B32), None),
    "glognn": (256, (B31, B32), None),
    # bf16 rows of 512 channels on the fp32 case's node count: past 2^31 bytes
    "c512_bf16": (1024, (B31,), B32 // 2048 // P * P + P),
    # sngnn_linear_forward*, F = 128 (512-byte rows of x): one 16-row tile below lim, at lim, past 2^32 bytes
    "lin_below": (512, (), LIN_LIM // 512 - 16),
    "lin_at": (512, (), LIN_LIM // 512),
    "lin_past_4gib": (512, (B31, B32), None),
    # sngnn_linear_forward_normalized, F = 32, C = 40: the last N with h below lim (a partial last tile)
    "linnorm_last": (160, (), (LIN_LIM - 1) // 160),
}


def boundary_offset(row_size, boundary):
    """(T, r): the offset of a block with row r = boundary // row_size - the row that contains unit ``boundary`` of a
    table whose rows have ``row_size`` units - strictly inside, T < r < T + P - 1; a multiple of P where that holds."""
    r = boundary // row_size
    t = r // P * P
    if not t < r < t + P - 1:
        t = r - P // 2
    return t, r


def place(row_size, boundaries=(), ntot=None):
    """Blocks of a table with rows of ``row_size`` units (bytes, or elements): near, one per boundary, last."""
    marks = [boundary_offset(row_size, b) for b in sorted(boundaries)]
    if ntot is None:
        ntot = marks[-1][0] + P
    offsets = [0] + [t for t, _ in marks]
    if ntot - P not in offsets:
        offsets.append(ntot - P)
    return Placement(ntot, tuple(offsets), tuple(r for _, r in marks))


def control(placement):
    """The same number of blocks on 4 P nodes: near, (P, 2 P,) last.  A failure there is the construction's."""
    assert len(placement.offsets) <= 4
    return Placement(4 * P, tuple([0, P, 2 * P][:len(placement.offsets) - 1]) + (3 * P,), ())


def check_placement(pl, row_size, boundaries=()):
    """What the CPU test asserts of a placement (and the GPU tests before they allocate)."""
    offs = sorted(pl.offsets)
    assert offs[0] == 0 and offs[-1] + P == pl.ntot, (offs, pl.ntot)            # near block; the last one ends at ntot - 1
    for a, b in zip(offs, offs[1:]):
        assert a + P <= b, ("blocks overlap", a, b)
    assert len(pl.boundary_rows) == len(boundaries)
    for b, r in zip(sorted(boundaries), pl.boundary_rows):
        assert r * row_size <= b < (r + 1) * row_size, (b, r)                   # r is the row that contains unit b
        inside = [t for t in offs if t < r < t + P - 1]
        assert len(inside) == 1, ("boundary row not strictly inside one block", b, r, offs)
        assert b < pl.ntot * row_size                                           # the table reaches the boundary
    ids = block_edges(edges(), pl.offsets)
    assert int(ids.min()) == 0 and int(ids.max()) == pl.ntot - 1 and ids.dtype == torch.int64


def block_edges(ei, offsets):
    """Translated copies of the block's edge list [2, E] at ``offsets`` (same order inside every copy)."""
    return torch.cat([ei + t for t in offsets], dim=1)


def periodic(block_rows, ntot, offsets=()):
    """[ntot, C] on block_rows' device: the block's rows with period P, and once more at every offset off the period."""
    assert block_rows.size(0) == P
    t = block_rows.repeat((ntot + P - 1) // P, 1)[:ntot]
    for o in offsets:
        if o % P:
            t[o:o + P] = block_rows
    return t


def need_memory(cuda, gib):
    """Skip unless ``gib`` GiB are free on the device (the only skip of the large tests)."""
    import pytest
    free = torch.cuda.mem_get_info(cuda)[0]
    if free < gib * 2 ** 30:
        pytest.skip(f"needs {gib} GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")


def peak_gib():
    return torch.cuda.max_memory_allocated() / 2 ** 30

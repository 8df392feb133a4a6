"""GPU: the graph kernels on feature tables past 2 GiB and 4 GiB (tests/large_tables.py: the blocks construction).

The statement under test: a row's result does not depend on where its block sits, so every block's results equal the
near block's bit for bit - per-edge results on the blocks' CSR ranges, source ids less the block's offset - and the
near block's equal those of the 3 000-node problem alone.  Each case runs first as a *control*, the same blocks on a
graph of 4 P nodes: a failure there is the construction's, not the kernel's.

Covered: the SN aggregation forward (fp32 at 512 and 40 channels, on both sides of the buffer form's limit and past
2^32 bytes; bf16), its backward in every mode, attention, signed attention, the adjacency Linear, the weighted gather /
scatter with pair_dot_rows, the GCN hop on a column slice, GPR and APPNP, the GCN2 hop, the H2GCN hop on both sides, GAT
at 8 x 64 with the refusal of sngnn_gat_scores at N * heads = 2^31, ACM on its [N, 3C] table, GloGNN forward and
backward, WRGAT at 4 x 128.  Not asserted: wrgat's refusal "N * relations must fit 31 bits" - its accepted side
needs a graph of 2^31 / R nodes.

Out of scope: kNN and the cosine histogram (O(N^2) at this N), the two-hop build (refused above 2^31 entries and
tested at that refusal: tests/test_two_hop_gpu.py) and partitions."""
import numpy as np
import pytest
import torch

from tests import large_tables as LT
from tests.large_tables import P
from tests.test_half_gpu import bits_equal, check_contract, knobs

pytestmark = pytest.mark.gpu

WHERE = ["control", "large"]


@pytest.fixture
def lib(cuda):
    from sngnn_amd import _lib
    handle = _lib.load()
    torch.cuda.reset_peak_memory_stats()
    yield handle
    handle.sngnn_tuning_set(11, 0)
    handle.sngnn_tuning_set(3, 0)
    handle.sngnn_filter_enable(1)
    torch.cuda.empty_cache()


def placement(case, where):
    pl = LT.place(*LT.CASES[case])
    LT.check_placement(pl, LT.CASES[case][0], LT.CASES[case][1])
    return LT.control(pl) if where == "control" else pl


def build(cuda, pl, loops):
    """(graph, per-block CSR edge ranges): add_loops = loops, nothing removed; "replace" = AGNNConv's order (loops
    removed, then one added per node)."""
    from sngnn_amd.graph import LOOPS_REPLACE, Graph
    add, remove = (True, LOOPS_REPLACE) if loops == "replace" else (loops, False)
    g = Graph(LT.block_edges(LT.edges(), pl.offsets).to(cuda), pl.ntot, add, remove)
    rowptr = g.array("rowptr").astype(np.int64)
    ranges = [(int(rowptr[t]), int(rowptr[t + P])) for t in pl.offsets]
    assert len({b - a for a, b in ranges}) == 1 and ranges[0][0] == 0
    assert g.num_edges == len(ranges) * ranges[0][1] + (pl.ntot - len(ranges) * P if add else 0)
    return g, ranges


def per_edge(block_values, g, ranges):
    """A per-edge input [E']: the block's values on every block's CSR range, 1 on the loops in between."""
    t = torch.ones(g.num_edges, dtype=block_values.dtype, device=block_values.device)
    for a, b in ranges:
        t[a:b] = block_values
    return t


_ALONE = {}


def alone(cuda, loops):
    """The block by itself: the 3 000-node graph."""
    if (str(cuda), loops) not in _ALONE:
        _ALONE[str(cuda), loops] = build(cuda, LT.Placement(P, (0,), ()), loops)[0]
    return _ALONE[str(cuda), loops]


def block_slice(t, name, off, rng, n_rows):
    """Block ``off``'s part of a result: rows [off, off + P) of a per-row tensor, the CSR range of a per-edge one;
    source ids less the offset."""
    if t.size(0) == n_rows:
        s = t[off:off + P]
    else:
        s = t[rng[0]:rng[1]]
    if name == "sel_src":
        s = torch.where(s >= 0, s - off, s)
    return s


def assert_blocks(res, names, g, pl, ranges, ref, what):
    """Every block of every result equals the near block bit for bit, and the near block equals ``ref`` (the block
    alone)."""
    assert len(res) == len(names) == len(ref)
    for t, name, r in zip(res, names, ref):
        assert (t is None) == (r is None), (what, name)
        if t is None:
            continue
        assert t.size(0) in (g.num_nodes, g.num_edges) and g.num_nodes != g.num_edges
        near = block_slice(t, name, pl.offsets[0], ranges[0], g.num_nodes)
        assert bits_equal(near.contiguous(), r), f"{what}: {name} of the near block differs from the block alone"
        for off, rng in zip(pl.offsets[1:], ranges[1:]):
            got = block_slice(t, name, off, rng, g.num_nodes)
            assert bits_equal(got.contiguous(), near.contiguous()), f"{what}: {name} of the block at {off} differs from the near block"


RESULTS = ("out", "wsel", "inv_norm", "sel_src", "sel_w")


def forward_variant(lib, g, h, k, thr, variant):
    from sngnn_amd import ops
    if variant == "epilogue":
        bias = torch.linspace(-0.2, 0.2, h.size(1), device=h.device)
        return list(ops._forward_epilogue(g, h, None, k, thr, True, ops.HiddenEpilogue(True, 0.0, False), bias)), ("out", "wsel")
    lib.sngnn_filter_enable(2 if variant == "filter" else 1)
    try:
        return list(ops.aggregate_forward(g, h, k, thr, save_for_backward=True, want_selection=k is not None)), RESULTS
    finally:
        lib.sngnn_filter_enable(1)


def forward_family(cuda, lib, C, case, where, cases, both_forms):
    """plain on the graph without loops (the block's exact in-degrees), the store epilogue and the forced fp16 filter
    on the graph with a loop at every node (every row of the table is then read, as its own source)."""
    pl = placement(case, where)
    hb = LT.rows(C).to(cuda)
    h = g = None
    try:
        h = LT.periodic(hb, pl.ntot, pl.offsets)
        assert h.shape == (pl.ntot, C) and float(h[pl.ntot - 1, C - 1]) == 1.5
        for loops, variants in ((False, ("plain",)), (True, ("epilogue", "filter"))):
            g, ranges = build(cuda, pl, loops)
            ga = alone(cuda, loops)
            for variant in variants:
                for k, thr in cases:
                    what = f"{case} {where} C={C} loops={loops} {variant} k={k} thr={thr}"
                    ref, names = forward_variant(lib, ga, hb, k, thr, variant)
                    res, _ = forward_variant(lib, g, h, k, thr, variant)
                    assert_blocks(res, names, g, pl, ranges, ref, what)
                    assert float(ref[0].abs().max()) > 0.0
                    if k is not None:
                        share = float((ref[1] > -3.0).float().mean())
                        assert 0.0 < share < 1.0, (what, share)           # the case keeps some edges and drops some
                    if both_forms:
                        # the largest table the buffer form takes: the flat form computes the same bits
                        lib.sngnn_tuning_set(11, 1)
                        flat, _ = forward_variant(lib, g, h, k, thr, variant)
                        lib.sngnn_tuning_set(11, 0)
                        for a, b, name in zip(flat, res, names):
                            assert bits_equal(a, b), f"{what}: {name} of the buffer form differs from the flat form"
                        del flat
                    del res
            del g
            g = None
            torch.cuda.empty_cache()
        print(f"{case} {where}: ntot {pl.ntot}, table {pl.ntot * C * 4 / 2 ** 30:.3f} GiB, blocks at {pl.offsets}, "
              f"peak {LT.peak_gib():.1f} GiB")
    finally:
        del h, g
        torch.cuda.empty_cache()


K_THR = [(16, 0.0), (16, 0.9), (None, 0.0), (None, 0.9)]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("case", ["c512_last_buffer", "c512_first_flat", "c512_past_4gib"])
def test_forward_fp32_c512(cuda, lib, case, where):
    LT.need_memory(cuda, 30)
    forward_family(cuda, lib, 512, case, where, K_THR, both_forms=case == "c512_last_buffer")


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("case", ["c40_last_buffer", "c40_first_flat"])
def test_forward_fp32_c40(cuda, lib, case, where):
    LT.need_memory(cuda, 16)
    forward_family(cuda, lib, 40, case, where, [(16, 0.0)], both_forms=case == "c40_last_buffer")


@pytest.mark.parametrize("where", WHERE)
def test_half_forward_and_backward_bf16_c512(cuda, lib, where):
    """tests/test_half_gpu.py's contract on the whole big problem (the half forward and backward against the fp32 ones
    on the widened rows, bit for bit), then the blocks of the half results against the near block and the block alone."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 40)
    case, C = "c512_bf16", 512
    pl = placement(case, where)
    hb = LT.rows(C).to(cuda).to(torch.bfloat16)
    h = g = None
    try:
        h = LT.periodic(hb, pl.ntot, pl.offsets)
        g, ranges = build(cuda, pl, True)
        ga = alone(cuda, True)
        for k, thr in ((16, 0.0),):          # (one case: with top_k None beside it the test outlasted the products-size one)
            what = f"{case} {where} k={k} thr={thr}"
            torch.manual_seed(7)
            got = check_contract(g, h, k, thr, what, bwd_modes=(0,))
            ref = ops.aggregate_forward(ga, hb, k, thr, save_for_backward=True, want_selection=k is not None)
            assert_blocks(list(got), RESULTS, g, pl, ranges, list(ref), what)
            del got
        print(f"{case} {where}: ntot {pl.ntot}, table {pl.ntot * C * 2 / 2 ** 30:.3f} GiB, peak {LT.peak_gib():.1f} GiB")
    finally:
        del h, g
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_backward_fp32_c512(cuda, lib, where):
    """sngnn_agg_backward_topk under knob 3 = 0, 1, 2 and sngnn_agg_backward_bits on the forward's own weights and kept
    bits, past 2^32 bytes of h, grad_out and grad_h."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 40)
    case, C, k, thr = "c512_past_4gib", 512, 16, 0.0
    pl = placement(case, where)
    hb = LT.rows(C).to(cuda)
    gob = torch.randn(P, C, generator=torch.Generator().manual_seed(3)).to(cuda)
    h = go = g = None
    try:
        h = LT.periodic(hb, pl.ntot, pl.offsets)
        go = LT.periodic(gob, pl.ntot, pl.offsets)
        for loops in (False, True):
            g, ranges = build(cuda, pl, loops)
            ga = alone(cuda, loops)
            wsel = ops.aggregate_forward(g, h, k, thr, save_for_backward=True)[1]
            wsel_a = ops.aggregate_forward(ga, hb, k, thr, save_for_backward=True)[1]
            for mode in (0, 1, 2):
                with knobs(k3=mode):
                    gh = ops.aggregate_backward(g, h, go, wsel, k)
                    ref = ops.aggregate_backward(ga, hb, gob, wsel_a, k)
                assert_blocks([gh], ("grad_h",), g, pl, ranges, [ref], f"{case} {where} loops={loops} knob 3 = {mode}")
                assert float(ref.abs().max()) > 0.0
                del gh
            if ops.kept_bits_supported(g, k, C):
                assert ops.kept_bits_supported(ga, k, C)
                kb = ops._forward_epilogue(g, h, None, k, thr, True, None, None, True)[1]
                kb_a = ops._forward_epilogue(ga, hb, None, k, thr, True, None, None, True)[1]
                gh = ops.aggregate_backward_bits(g, h, go, kb, k)
                ref = ops.aggregate_backward_bits(ga, hb, gob, kb_a, k)
                assert_blocks([gh], ("grad_h",), g, pl, ranges, [ref], f"{case} {where} loops={loops} kept bits")
                del gh, kb
            else:
                print(f"{case} {where} loops={loops}: no kept-bit path on this graph")
            del g, wsel
            g = None
            torch.cuda.empty_cache()
        print(f"{case} {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del h, go, g
        torch.cuda.empty_cache()


def big_case(cuda, where, C=512):
    pl = placement("c512_past_4gib", where)
    hb = LT.rows(C).to(cuda)
    gob = torch.randn(P, C, generator=torch.Generator().manual_seed(3)).to(cuda)
    return pl, hb, gob


@pytest.mark.parametrize("where", WHERE)
def test_attention_fp32_c512(cuda, lib, where):
    """sngnn_attn_forward / _backward past 2^32 bytes, on the loop mode of AGNNConv (every row holds its own loop)."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 36)
    pl, hb, gob = big_case(cuda, where)
    h = go = g = None
    try:
        h, go = LT.periodic(hb, pl.ntot, pl.offsets), LT.periodic(gob, pl.ntot, pl.offsets)
        g, ranges = build(cuda, pl, "replace")
        ga = alone(cuda, "replace")
        res = ops.attention_forward(g, h)
        ref = ops.attention_forward(ga, hb)
        assert_blocks(list(res), ("out", "alpha"), g, pl, ranges, list(ref), f"attention forward {where}")
        assert float(ref[0].abs().max()) > 0.0
        gh = ops.attention_backward(g, h, go, res[1])
        gref = ops.attention_backward(ga, hb, gob, ref[1])
        assert_blocks([gh], ("grad_h",), g, pl, ranges, [gref], f"attention backward {where}")
        assert float(gref.abs().max()) > 0.0
        print(f"attention {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del h, go, g
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_signed_fp32_c512(cuda, lib, where):
    """sngnn_signed_forward / _backward past 2^32 bytes: per-edge coefficients of both signs on every block's edges."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 36)
    pl, hb, gob = big_case(cuda, where)
    c2 = torch.tensor([0.7, -0.4], device=cuda)
    h = go = g = None
    try:
        h, go = LT.periodic(hb, pl.ntot, pl.offsets), LT.periodic(gob, pl.ntot, pl.offsets)
        g, ranges = build(cuda, pl, False)
        ga = alone(cuda, False)
        coef_b = torch.randn(ga.num_edges, generator=torch.Generator().manual_seed(9)).to(cuda)
        coef = per_edge(coef_b, g, ranges)
        res = ops.signed_forward(g, h, coef, c2)
        ref = ops.signed_forward(ga, hb, coef_b, c2)
        assert_blocks(list(res), ("out", "s"), g, pl, ranges, list(ref), f"signed forward {where}")
        assert float(ref[0].abs().max()) > 0.0 and bool((ref[1] > 0).any()) and bool((ref[1] < 0).any())
        back = ops.signed_backward(g, h, go, coef, res[1], c2)
        bref = ops.signed_backward(ga, hb, gob, coef_b, ref[1], c2)
        assert_blocks(list(back), ("grad_wh", "u"), g, pl, ranges, list(bref), f"signed backward {where}")
        assert float(bref[0].abs().max()) > 0.0
        print(f"signed {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del h, go, g
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_adj_linear_fp32_c512(cuda, lib, where):
    """sngnn_adj_linear_forward / _backward (the adjacency as a Linear's input: a gather-sum and its transpose) past
    2^32 bytes of the weight table."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 30)
    pl, hb, gob = big_case(cuda, where)
    bias = torch.linspace(-0.2, 0.2, 512, device=cuda)
    wt = go = g = None
    try:
        wt, go = LT.periodic(hb, pl.ntot, pl.offsets), LT.periodic(gob, pl.ntot, pl.offsets)
        g, ranges = build(cuda, pl, False)
        ga = alone(cuda, False)
        for b in (bias, None):
            out = ops.adj_linear_forward(g, wt, b)
            ref = ops.adj_linear_forward(ga, hb, b)
            assert_blocks([out], ("out0",), g, pl, ranges, [ref], f"adj_linear forward {where} bias={b is not None}")
            assert float(ref.abs().max()) > 0.0
            del out
        dwt = ops.adj_linear_backward(g, go)
        dref = ops.adj_linear_backward(ga, gob)
        assert_blocks([dwt], ("dwt",), g, pl, ranges, [dref], f"adj_linear backward {where}")
        assert float(dref.abs().max()) > 0.0
        print(f"adj_linear {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del wt, go, g
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_weighted_gather_scatter_and_pair_dot_c512(cuda, lib, where):
    """sngnn_weighted_gather_sum_rows, its transpose sngnn_weighted_scatter_sum_rows and sngnn_pair_dot_rows (the three
    launches of ops.weighted_propagate and its backward) past 2^32 bytes of x, grad_out and grad_x."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 36)
    pl, hb, gob = big_case(cuda, where)
    x = go = g = out = None
    try:
        g, ranges = build(cuda, pl, False)
        ga = alone(cuda, False)
        w_b = torch.randn(ga.num_edges, generator=torch.Generator().manual_seed(4)).to(cuda)
        xa, wa = hb.clone().requires_grad_(True), w_b.clone().requires_grad_(True)
        ref = ops.weighted_propagate(xa, wa, ga, ga.csr_entries())
        ref.backward(gob)
        x = LT.periodic(hb, pl.ntot, pl.offsets).requires_grad_(True)
        go = LT.periodic(gob, pl.ntot, pl.offsets)
        w = per_edge(w_b, g, ranges).requires_grad_(True)
        out = ops.weighted_propagate(x, w, g, g.csr_entries())
        out.backward(go)
        assert_blocks([out.detach(), x.grad, w.grad], ("out", "grad_x", "grad_w"), g, pl, ranges,
                      [ref.detach(), xa.grad, wa.grad], f"weighted propagate {where}")
        assert float(ref.detach().abs().max()) > 0.0 and float(xa.grad.abs().max()) > 0.0 and float(wa.grad.abs().max()) > 0.0
        print(f"weighted propagate {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del x, go, g, out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_gcn_hop_on_a_column_slice(cuda, lib, where):
    """sngnn_gcn_hop at its widest row, 512 columns, gathered from the interior columns [64, 576) of a table of 640
    (2 560-byte rows: the table passes 2^32 bytes, and so does the contiguous destination), A^ and its transpose."""
    from sngnn_amd import gcn
    LT.need_memory(cuda, 24)
    pl = placement("gcn_slice", where)
    gen = torch.Generator().manual_seed(21)
    tb = torch.randn(P, 640, generator=gen).to(cuda)
    table = dst = g = None
    try:
        table = LT.periodic(tb, pl.ntot, pl.offsets)
        g, ranges = build(cuda, pl, "replace")
        ga = alone(cuda, "replace")
        dst = torch.full((pl.ntot, 512), float("nan"), device=cuda)
        ref = torch.full((P, 512), float("nan"), device=cuda)
        for transpose in (False, True):
            gcn.hop(g, table[:, 64:576], dst, transpose=transpose)
            gcn.hop(ga, tb[:, 64:576], ref, transpose=transpose)
            assert_blocks([dst], ("dst0",), g, pl, ranges, [ref], f"gcn hop {where} transpose={transpose}")
            assert float(ref.abs().max()) > 0.0 and bool(torch.isfinite(ref).all())
        print(f"gcn hop {where}: ntot {pl.ntot}, table {pl.ntot * 2560 / 2 ** 30:.3f} GiB, peak {LT.peak_gib():.1f} GiB")
    finally:
        del table, dst, g
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name", ["gpr", "appnp"])
def test_prop_gpr_and_appnp_c512(cuda, lib, name, where):
    """sngnn_prop_gpr_forward / _backward (the gradient of x) and sngnn_prop_appnp with its transpose, K = 2, past 2^32
    bytes.  The blocks are closed under the adjacency, so two hops stay inside a block."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 40)
    pl, hb, gob = big_case(cuda, where)
    gamma = torch.tensor([0.5, 0.3, 0.2], device=cuda)
    x = go = g = out = None
    try:
        g, ranges = build(cuda, pl, "replace")
        ga = alone(cuda, "replace")
        go = LT.periodic(gob, pl.ntot, pl.offsets)
        run = {"gpr": lambda t, gr: ops.gpr_propagate(t, gamma, gr),
               "appnp": lambda t, gr: ops.appnp_propagate(t, gr, 2, 0.1)}[name]
        xa = hb.clone().requires_grad_(True)
        ref = run(xa, ga)
        ref.backward(gob)
        x = LT.periodic(hb, pl.ntot, pl.offsets).requires_grad_(True)
        out = run(x, g)
        out.backward(go)
        assert_blocks([out.detach(), x.grad], ("out", "grad_x"), g, pl, ranges, [ref.detach(), xa.grad],
                      f"{name} {where}")
        assert float(ref.detach().abs().max()) > 0.0 and float(xa.grad.abs().max()) > 0.0
        print(f"{name} {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del x, go, g, out
        torch.cuda.empty_cache()


def no_ranges(pl):
    return [(0, 0)] * len(pl.offsets)


@pytest.mark.parametrize("where", WHERE)
def test_gcn2_hop_c512(cuda, lib, where):
    """sngnn_gcn2_hop, a A^ x + b x0 and its transpose, 512 channels, past 2^32 bytes."""
    from sngnn_amd import gcn2
    LT.need_memory(cuda, 24)
    pl, hb, gob = big_case(cuda, where)
    x = x0 = g = None
    try:
        x, x0 = LT.periodic(hb, pl.ntot, pl.offsets), LT.periodic(gob, pl.ntot, pl.offsets)
        g, ranges = build(cuda, pl, "replace")
        ga = alone(cuda, "replace")
        for transpose in (False, True):
            out = gcn2._hop(g, x, x0, 0.9, 0.1, transpose)
            ref = gcn2._hop(ga, hb, gob, 0.9, 0.1, transpose)
            assert_blocks([out], ("out",), g, pl, ranges, [ref], f"gcn2 hop {where} transpose={transpose}")
            assert float(ref.abs().max()) > 0.0
            del out
        print(f"gcn2 hop {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del x, x0, g
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_gat_h8_c64(cuda, lib, where):
    """gat_propagate at heads x C = 8 x 64 = 512, forward and the gradient of xp, past 2^32 bytes (the attention
    vectors' gradients are sums over all nodes, not a block's: not compared)."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 36)
    pl, hb, gob = big_case(cuda, where)
    gen = torch.Generator().manual_seed(31)
    att_s, att_d = (torch.randn(1, 8, 64, generator=gen).to(cuda) for _ in range(2))
    x = go = g = out = None
    try:
        g, ranges = build(cuda, pl, "replace")
        ga = alone(cuda, "replace")
        xa = hb.clone().requires_grad_(True)
        ref = ops.gat_propagate(xa, att_s, att_d, ga, 8)
        ref.backward(gob)
        x = LT.periodic(hb, pl.ntot, pl.offsets).requires_grad_(True)
        go = LT.periodic(gob, pl.ntot, pl.offsets)
        out = ops.gat_propagate(x, att_s, att_d, g, 8)
        out.backward(go)
        assert_blocks([out.detach(), x.grad], ("out", "grad_xp"), g, pl, ranges, [ref.detach(), xa.grad], f"gat {where}")
        assert float(ref.detach().abs().max()) > 0.0 and float(xa.grad.abs().max()) > 0.0
        print(f"gat {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del x, go, g, out
        torch.cuda.empty_cache()


def test_gat_scores_guard_n_times_heads(cuda, lib):
    """sngnn_gat_scores refuses N * heads >= 2^31 ("N * heads must fit 31 bits"): N = 2^31 - 1 at one head of one channel
    runs (and every score is the product it should be), N = 2^31 is refused before anything is launched."""
    from sngnn_amd import _lib
    LT.need_memory(cuda, 30)
    n = 2 ** 31 - 1
    xb = torch.randn(P, 1, generator=torch.Generator().manual_seed(32)).to(cuda)
    att = torch.tensor([0.75, -1.5], device=cuda)
    xp = a = b = None
    try:
        xp = LT.periodic(xb, n)
        a, b = (torch.full((n,), float("nan"), device=cuda) for _ in range(2))
        with pytest.raises(ValueError, match="N \\* heads must fit 31 bits"):
            _lib.call("sngnn_gat_scores", cuda, xp, att[:1], att[1:], n + 1, 1, 1, a, b)
        assert bool(torch.isnan(a[:P]).all())
        _lib.call("sngnn_gat_scores", cuda, xp, att[:1], att[1:], n, 1, 1, a, b)
        assert torch.equal(a[:P], xb[:, 0] * 0.75) and torch.equal(b[:P], xb[:, 0] * -1.5)
        for t in (a, b):
            whole = t[:n // P * P].view(-1, P)
            assert bool((whole.view(torch.int32) == t[:P].view(torch.int32)).all())
            assert torch.equal(t[n // P * P:], t[:n % P])
    finally:
        del xp, a, b
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_h2gcn_hop_both_sides(cuda, lib, where):
    """sngnn_h2gcn_hop: [A1 src | A2 src] from 256 to 512 columns and the transpose back, the destination past 2^32
    bytes; A2 is the two-hop build's result on the big graph (27 M entries: far below its own limit)."""
    from sngnn_amd import h2gcn
    LT.need_memory(cuda, 24)
    pl, hb, gob = big_case(cuda, where)
    src = dst = adj = back = None
    try:
        ei = LT.edges()
        adj = h2gcn.H2Adjacency(LT.block_edges(ei, pl.offsets).to(cuda), pl.ntot)
        adj_a = h2gcn.H2Adjacency(ei.to(cuda), P)
        assert adj.a2.num_edges == len(pl.offsets) * adj_a.a2.num_edges
        src = LT.periodic(hb[:, :256].contiguous(), pl.ntot, pl.offsets)
        dst = torch.full((pl.ntot, 512), float("nan"), device=cuda)
        ref = torch.full((P, 512), float("nan"), device=cuda)
        h2gcn.hop(adj, src, dst)
        h2gcn.hop(adj_a, hb[:, :256].contiguous(), ref)
        assert_blocks([dst], ("dst",), adj.a1, pl, no_ranges(pl), [ref], f"h2gcn hop {where}")
        assert float(ref.abs().max()) > 0.0 and bool(torch.isfinite(ref).all())
        back = torch.full((pl.ntot, 256), float("nan"), device=cuda)
        ref_b = torch.full((P, 256), float("nan"), device=cuda)
        h2gcn.hop(adj, dst, back, transpose=True)
        h2gcn.hop(adj_a, ref, ref_b, transpose=True)
        assert_blocks([back], ("dst",), adj.a1, pl, no_ranges(pl), [ref_b], f"h2gcn hop {where}, transpose")
        print(f"h2gcn hop {where}: ntot {pl.ntot}, A2 {adj.a2.num_edges} entries, peak {LT.peak_gib():.1f} GiB")
    finally:
        del src, dst, adj, back
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_acm_c256(cuda, lib, where):
    """sngnn_acm_forward / _backward at C = 256, its widest: the [N, 3 C] table past 2^32 bytes (3 072-byte rows); out,
    the saved [L | H] and the six scalars a row, and the gradient of the table (the parameters' gradients are sums over
    all rows: not compared)."""
    from sngnn_amd import acm
    LT.need_memory(cuda, 30)
    pl = placement("acm", where)
    c = 256
    gen = torch.Generator().manual_seed(41)
    pb = torch.randn(P, 3 * c, generator=gen).to(cuda)
    gob = torch.randn(P, c, generator=gen).to(cuda)
    al, ah, am = (torch.randn(c, generator=gen).to(cuda) / 16.0 for _ in range(3))
    av = torch.randn(9, generator=gen).to(cuda)
    p = go = g = res = None
    try:
        g, ranges = build(cuda, pl, True)
        ga = alone(cuda, True)
        pa = pb.clone().requires_grad_(True)
        ref = acm.acm_filterbank_fused(pa, al, ah, am, av, ga, True)
        ref[0].backward(gob)
        p = LT.periodic(pb, pl.ntot, pl.offsets).requires_grad_(True)
        go = LT.periodic(gob, pl.ntot, pl.offsets)
        res = acm.acm_filterbank_fused(p, al, ah, am, av, g, True)
        res[0].backward(go)
        assert_blocks([t.detach() for t in res] + [p.grad], ("out", "LH", "datt", "grad_P"), g, pl, ranges,
                      [t.detach() for t in ref] + [pa.grad], f"acm {where}")
        assert float(ref[0].detach().abs().max()) > 0.0 and float(pa.grad.abs().max()) > 0.0
        print(f"acm {where}: ntot {pl.ntot}, table {pl.ntot * 3072 / 2 ** 30:.3f} GiB, peak {LT.peak_gib():.1f} GiB")
    finally:
        del p, go, g, res
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_glognn_forward_and_backward_c64(cuda, lib, where):
    """sngnn_glognn_forward / _backward at 64 channels, the layer's widest, x past 2^32 bytes.  The C x C matrices come
    from the Gram matrix of ALL rows, so the entries are called with the block's own matrices on both graphs: the
    row-local pass and the hops are then a block's own."""
    from sngnn_amd import _lib, glognn
    LT.need_memory(cuda, 36)
    pl = placement("glognn", where)
    c, orders, alpha, beta, gamma = 64, 2, 0.0, 1.0, 0.6
    gen = torch.Generator().manual_seed(51)
    xb, hb, gb = (torch.randn(P, c, generator=gen).to(cuda) for _ in range(3))
    w32 = torch.tensor([0.7, 0.3], device=cuda)
    x = h0 = go = g = None
    try:
        g, ranges = build(cuda, pl, False)
        ga = alone(cuda, False)
        ws_a = glognn.glognn_workspace(ga, c, orders)
        G = glognn._gram(xb, xb, ws_a)[0]
        small, mt32 = glognn._solve(G, None, alpha, beta, gamma)

        def forward(gr, xx, hh):
            S, out = torch.full_like(xx, float("nan")), torch.full_like(xx, float("nan"))
            _lib.call("sngnn_glognn_forward", cuda, gr.handle, xx, hh, mt32, w32, orders, beta, gamma, c, S, out,
                      glognn.glognn_workspace(gr, c, orders))
            return S, out

        S_a, out_a = forward(ga, xb, hb)
        gtm = glognn._gram(xb, gb, ws_a, a_sub=hb, sub=gamma, a2=S_a)
        gg2, _ = glognn._solve_backward(gtm[1], gtm[0], beta, 1.0 - gamma, G, small[2], small[3], None, alpha, beta, gamma)

        def backward(gr, gg, xx):
            gx, gh0 = torch.full_like(xx, float("nan")), torch.full_like(xx, float("nan"))
            _lib.call("sngnn_glognn_backward", cuda, gr.handle, gg, xx, mt32, gg2, w32, orders, beta, gamma, c, gx, gh0,
                      None, glognn.glognn_workspace(gr, c, orders))
            return gx, gh0

        ref_b = backward(ga, gb, xb)
        x, h0, go = (LT.periodic(t, pl.ntot, pl.offsets) for t in (xb, hb, gb))
        res = forward(g, x, h0)
        assert_blocks(list(res), ("S", "out"), g, pl, ranges, [S_a, out_a], f"glognn forward {where}")
        assert bool(torch.isfinite(out_a).all()) and float(out_a.abs().max()) > 0.0
        del res
        back = backward(g, go, x)
        assert_blocks(list(back), ("grad_x", "grad_h0"), g, pl, ranges, list(ref_b), f"glognn backward {where}")
        assert bool(torch.isfinite(ref_b[0]).all()) and float(ref_b[0].abs().max()) > 0.0
        print(f"glognn {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del x, h0, go, g
        torch.cuda.empty_cache()


@pytest.mark.parametrize("where", WHERE)
def test_wrgat_r4_c128(cuda, lib, where):
    """wrgat_conv at relations x C = 4 x 128 = 512, the table past 2^32 bytes: out and the gradient of P (the attention
    vectors' gradients are sums over all nodes: not compared).  Its refusal "N * relations must fit 31 bits" is not
    asserted: the accepted side needs a graph of 2^31 / R nodes."""
    from sngnn_amd import ops
    LT.need_memory(cuda, 30)
    pl, hb, _ = big_case(cuda, where)
    gen = torch.Generator().manual_seed(71)
    atten = torch.randn(4, 256, generator=gen).to(cuda) / 16.0
    gob = torch.randn(P, 128, generator=gen).to(cuda)
    ei = LT.edges()
    types = torch.arange(ei.size(1)) % 4
    x = go = adj = out = None
    try:
        adj_a = ops.TypedAdjacency(ei.to(cuda), types.to(cuda), None, P, 4)
        adj = ops.TypedAdjacency(LT.block_edges(ei, pl.offsets).to(cuda), types.repeat(len(pl.offsets)).to(cuda), None,
                                 pl.ntot, 4)
        xa = hb.clone().requires_grad_(True)
        ref = ops.wrgat_conv(xa, atten, None, None, adj_a)
        ref.backward(gob)
        x = LT.periodic(hb, pl.ntot, pl.offsets).requires_grad_(True)
        go = LT.periodic(gob, pl.ntot, pl.offsets)
        out = ops.wrgat_conv(x, atten, None, None, adj)
        out.backward(go)
        assert_blocks([out.detach(), x.grad], ("out", "grad_P"), adj.graph, pl, no_ranges(pl), [ref.detach(), xa.grad],
                      f"wrgat {where}")
        assert float(ref.detach().abs().max()) > 0.0 and float(xa.grad.abs().max()) > 0.0
        print(f"wrgat {where}: ntot {pl.ntot}, peak {LT.peak_gib():.1f} GiB")
    finally:
        del x, go, adj, out
        torch.cuda.empty_cache()

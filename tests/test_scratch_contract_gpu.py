"""The memory around the results: every entry of include/sngnn_hip.h that takes a ``workspace`` is run through the
Python layer, forward and backward, three times - unguarded, then twice on guarded scratch (tests/guarded_scratch.py:
payloads of EXACTLY the bytes the entry's size function returned, between two 4 096-byte canary guards) whose payload
is pre-filled with the words 0x7FC12345 (a NaN) and then with 0xFF bytes (a negative NaN, -1 in an integer region, all
ones in a bitmap).  The payloads are poisoned again between a case's forward and its backward.

Asserted, with no tolerance anywhere (the library is deterministic and free of floating-point atomics):
  * no guard byte changed - a call writes only inside the bytes its size function promised;
  * every output of both guarded runs equals the unguarded run's bit for bit - no result depends on what the scratch
    held before the call, and no size function returns too little (production pads to 256 bytes; the harness does not).

Spin-wait safety, by reading csrc/: the only kernels that wait on a workspace word are the three in-launch finalize
forms of agg_fwd_fin.h; they wait for ``fin_done[t] == fin_nonce`` with the nonce 0xF1A0000000000000 + counter, which
neither poison equals, and give up after FIN_SPIN_MAX = 2^19 polls.  Every other ``while`` / ``for (;;)`` in csrc/ is
host code, a binary search, a bit scan or a probe of an LDS table the block has just cleared.

No region is exempt: nothing in the library was found to depend on a workspace's contents on entry.

Which widths run where.  The 600-node degree graph (every row class) and the 40-node ring (no split and no wave rows:
the size functions at their floors) run every graph entry at all of 1, 5, 40, 64 and 130 channels - the lane layouts
of ``row_cfg``; the 2 400-node hub graph and the edgeless graph add their row classes at 40 (the epilogue, prepared
and gather_floor families also at 64): the lane layout is chosen by the width alone, so the other widths would repeat
the degree graph's kernels on more tasks.  Entries that do
not take every width, and why:
  * the store epilogue (``HiddenEpilogue``: ``sngnn_agg_forward_epilogue`` / ``_prepared_epilogue`` with bias, relu or
    dropout) is refused unless C % 4 == 0 - it stores 16-byte rows - so it runs at 40 and 64; the same two entries
    WITHOUT store flags (a training forward that writes its kept bits) and ``sngnn_agg_backward_bits``,
    ``sngnn_agg_forward_prepared``, ``_rows``, ``_normalized`` and ``sngnn_agg_backward`` take any width and run at
    all five (``agg_prepared``);
  * the head epilogue, ``sngnn_head_nll2`` and ``sngnn_head_nll_blend`` need C <= 64 (the last two also C % 4 == 0
    for the blend): 40 and 64, resp. 1, 5, 40, 64; ``sngnn_head_nll`` alone also runs at 130, its wide kernel;
  * ``gcn2_conv`` stops at 128 channels (130 becomes 128), the GloGNN norm layer and ``gram`` at 64.
``test_the_table_enters_every_entry_with_a_workspace_parameter`` holds this against the names that went through
``_lib.call`` while the scratch was guarded, per width.

The lifetime half: ``test_a_captured_epoch_keeps_its_scratch`` - a buffer ``_lib.workspace`` handed out once stays
alive for the process's life, whatever a later, larger model asks for.
"""
import functools
import gc
import math
import os
import re
import weakref

import pytest
import torch

from tests import guarded_scratch as GS
from tests import glognn_ref
from tests import gpr_ref as R
from tests.test_half_gpu import knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = {"deg": (1, 5, 40, 64, 130), "hub": (40,), "ring": (1, 5, 40, 64, 130), "empty": (40,)}
GRAPHS = tuple(WIDTHS)


# ------------------------------------------------------------------ graphs (edge lists on the CPU, device graphs once)

@functools.lru_cache(maxsize=None)
def _edges(kind):
    if kind == "deg":          # 600 nodes, every row class on both sides
        return R.degree_graph()
    if kind == "hub":          # 2 400 nodes, 18 tasks on either side
        return R.hub_graph()
    if kind == "ring":         # no split and no wave rows: n_tasks == n_stasks == 0, the size functions at their floors
        i = torch.arange(40)
        return torch.cat([torch.stack([i, (i + 1) % 40]), torch.stack([(i + 1) % 40, i])], dim=1).contiguous(), 40
    assert kind == "empty"     # nodes but no edges
    return torch.empty((2, 0), dtype=torch.int64), 50


@functools.lru_cache(maxsize=None)
def _edges_unique(kind):
    """ACM's reading: unique loop-free edges plus the diagonal."""
    ei, n = _edges(kind)
    ei = torch.unique(ei[:, ei[0] != ei[1]], dim=1)
    return torch.cat([ei, torch.arange(n).repeat(2, 1)], dim=1).contiguous(), n


_DEV = {}


def _graph(dev, kind, mode, row_range=None):
    """mode: 'sn' (loops added then all removed: the SN layers'), 'loops' (replaced: gcn_norm's), 'noloop' (removed),
    'raw' (as listed), 'acm' (unique + diagonal, as listed)."""
    from sngnn_amd.graph import LOOPS_REPLACE, Graph
    key = (kind, mode, row_range)
    if key not in _DEV:
        ei, n = _edges_unique(kind) if mode == "acm" else _edges(kind)
        add, rem = {"sn": (True, True), "loops": (True, LOOPS_REPLACE), "noloop": (False, True), "raw": (False, False),
                    "acm": (False, False)}[mode]
        _DEV[key] = Graph(ei.to(dev), n, add, rem, row_range)
    return _DEV[key]


def _seed_of(*key):
    s = 0
    for ch in "/".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def _cpu_gen(*key):
    return torch.Generator().manual_seed(_seed_of(*key))


def _leaf(t, dev):
    return t.to(dev).requires_grad_(True)


# ------------------------------------------------------------------ the table of cases

CASES = {}          # name -> (make() -> CPU inputs, run(dev, inputs, mark) -> dict of tensors, labels that must be handed out)


def _add(name, expects, make, run):
    assert name not in CASES, name
    CASES[name] = (make, run, tuple(expects))


G_WS = "sngnn_graph_workspace_bytes"


# ---- the aggregation, forward and backward ----------------------------------------------------------------------------

# (knob 9, filter mode, knob 3): knob 9 at 0 and 2, the fp16 filter at its default and forced, knob 3 at 0, 1 and 2
AGG_VARIANTS = ((0, 1, 0), (2, 1, 1), (0, 2, 2), (2, 2, 0))
AGG_SELECT = ((None, 0.0), (16, 0.0), (16, 0.9))


def _agg_run(kind, top_k, thr, k9, filt, k3, dtype, ranges):
    def run(dev, inp, mark):
        from sngnn_amd import _lib, ops
        lib = _lib.load()
        out = {}
        lib.sngnn_filter_enable(filt)
        try:
            for r in ranges:
                g = _graph(dev, kind, "sn", r)
                h = inp["h"].to(dev).to(dtype)
                lo, hi = (0, g.num_total_nodes) if r is None else r
                go = inp["go"][lo:hi].to(dev).to(dtype).contiguous()
                with knobs(k9=k9):
                    res = ops.aggregate_forward(g, h, top_k, thr, save_for_backward=True, want_selection=top_k is not None)
                mark()
                with knobs(k3=k3):
                    gh = ops.aggregate_backward(g, h, go, res[1], top_k)
                for q, t in zip(("out", "wsel", "inv", "sel_src", "sel_w", "grad_h"), (*res, gh)):
                    if t is not None:
                        out[f"{q}{'' if r is None else r}"] = t
        finally:
            lib.sngnn_filter_enable(1)
        return out
    return run


def _agg_make(kind, c):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("agg", kind, c)
        return dict(h=R.rows("gaussian", n, c, gen), go=torch.randn(n, c, generator=gen))
    return make


for _kind in GRAPHS:
    for _c in WIDTHS[_kind]:
        for _top_k, _thr in AGG_SELECT:
            for _k9, _filt, _k3 in AGG_VARIANTS:
                _add(f"agg/{_kind}/C{_c}/k{_top_k}/thr{_thr}/k9={_k9},filter={_filt},k3={_k3}", [G_WS],
                     _agg_make(_kind, _c), _agg_run(_kind, _top_k, _thr, _k9, _filt, _k3, torch.float32, (None,)))
        _add(f"agg_bf16/{_kind}/C{_c}", [G_WS], _agg_make(_kind, _c),
             _agg_run(_kind, 16, 0.0, 0, 1, 0, torch.bfloat16, (None,)))
for _c in WIDTHS["deg"]:          # the 600-node graph as two node-range partitions
    for _top_k, _thr in AGG_SELECT:
        _add(f"agg_partitions/deg/C{_c}/k{_top_k}/thr{_thr}", [G_WS], _agg_make("deg", _c),
             _agg_run("deg", _top_k, _thr, 0, 1, 0, torch.float32, ((0, 300), (300, 600))))


def _prepared_case(kind, c, top_k, thr):
    """The forms on unit rows the caller holds: ``sngnn_agg_forward_prepared`` (with the caller's filter rows),
    ``_prepared_epilogue`` (unit rows; with the hidden epilogue where C % 4 == 0 lets the store epilogue in), the
    training forward without store flags, on raw and on unit rows (``sngnn_agg_forward_epilogue`` /
    ``_prepared_epilogue`` writing kept bits and ``sngnn_agg_backward_bits`` where the graph has that path, the plain
    entries otherwise), ``_rows`` (two complementary row sets), and the two entries the Python layer does not call -
    ``sngnn_agg_forward_normalized`` and ``sngnn_agg_backward`` - entered as the header declares them."""
    def run(dev, inp, mark):
        from sngnn_amd import _lib, ops
        g = _graph(dev, kind, "sn")
        n_rows, e = g.num_nodes, g.num_edges
        h, go = inp["h"].to(dev), inp["go"].to(dev)
        n, nrm, filt = ops.normalize_rows_filter(h)
        res = {}
        out, sel_src, sel_w = ops.aggregate_forward_normalized(g, n, nrm, top_k, thr, want_selection=True, filt=filt)
        res.update(prepared_out=out, prepared_sel_src=sel_src, prepared_sel_w=sel_w)
        mark()
        unit = ops.UnitRows()
        unit.n, unit.nrm, unit.filt = n, nrm, filt
        if c % 4 == 0:          # (the store epilogue: 16-byte rows)
            hl = h.clone().requires_grad_(True)
            epi = ops.HiddenEpilogue(True, 0.5, True, torch.tensor([4242], dtype=torch.int64, device=dev))
            epi.applied = True
            act = ops.aggregate(hl, g, top_k, thr, unit=unit, epilogue=epi, bias=None)
            mark()
            act.backward(go)
            res.update(prepared_epilogue_out=act.detach(), prepared_epilogue_grad_h=hl.grad)
            mark()
        # a training forward without store flags, on raw and on unit rows: at knob 3 = 0 the library chooses between the
        # kept-bits pair and the plain entries by the graph; knob 3 = 2 (the node-centric backward) gives every graph that
        # has the bit layout the kept-bits pair, at any width
        for tag, rows, k3 in (("train", None, 0), ("train_unit", unit, 0), ("train_bits", None, 2), ("train_unit_bits", unit, 2)):
            hl = h.clone().requires_grad_(True)
            with knobs(k3=k3):
                act = ops.aggregate(hl, g, top_k, thr, unit=rows)
                mark()
                act.backward(go)
            res.update({f"{tag}_out": act.detach(), f"{tag}_grad_h": hl.grad})
            mark()
        flag = (torch.arange(n_rows, device=dev) % 3 == 0).to(torch.uint8)
        rows_out = torch.empty((n_rows, c), device=dev)
        rows_wsel, rows_inv = torch.empty(e, device=dev), torch.empty(n_rows, device=dev)
        for want in (1, 0):
            ops.aggregate_forward_rows(g, n, nrm, filt, top_k, thr, flag, want, rows_out, rows_wsel, rows_inv)
            mark()
        res.update(rows_out=rows_out, rows_wsel=rows_wsel, rows_inv=rows_inv)
        norm_out, wsel, inv = torch.empty((n_rows, c), device=dev), torch.empty(e, device=dev), torch.empty(n_rows, device=dev)
        _lib.call("sngnn_agg_forward_normalized", dev, g.handle, n, nrm, c, top_k, float(thr), norm_out, wsel, inv, None, None,
                  g.workspace(c))
        mark()
        grad_h = torch.empty_like(h)
        _lib.call("sngnn_agg_backward", dev, g.handle, h, c, go, wsel, grad_h, g.workspace(c))
        res.update(normalized_out=norm_out, normalized_wsel=wsel, normalized_inv=inv, backward_grad_h=grad_h)
        return res
    return _agg_make(kind, c), run


for _kind in GRAPHS:
    for _c in sorted(set(WIDTHS[_kind] + (40, 64))):
        _add(f"agg_prepared/{_kind}/C{_c}", [G_WS], *_prepared_case(_kind, _c, 16, 0.9))


def _epilogue_case(kind, c, top_k, thr):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("epi", kind, c)
        return dict(h=R.rows("gaussian", n, c, gen), go=torch.randn(n, c, generator=gen), bias=0.3 * torch.randn(c, generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        g = _graph(dev, kind, "sn")
        h, bias = _leaf(inp["h"], dev), _leaf(inp["bias"], dev)
        epi = ops.HiddenEpilogue(True, 0.5, True, torch.tensor([20240], dtype=torch.int64, device=dev))
        epi.applied = True
        out = ops.aggregate(h, g, top_k, thr, epilogue=epi, bias=bias)
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_h=h.grad, grad_bias=bias.grad)
    return make, run


def _head_case(kind, c, top_k, thr):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("head", kind, c)
        r = torch.rand(n, generator=gen)
        return dict(h=R.rows("gaussian", n, c, gen), bias=0.3 * torch.randn(c, generator=gen),
                    y=torch.randint(0, c, (n,), generator=gen), train=(r < 0.6).to(torch.uint8),
                    sets=((r >= 0.6) & (r < 0.8)).to(torch.uint8) + 2 * (r >= 0.8).to(torch.uint8))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        g = _graph(dev, kind, "sn")
        assert ops.head_supported(g, c, top_k), "the head epilogue must apply to this case"
        y, train, sets = inp["y"].to(dev), inp["train"].to(dev), inp["sets"].to(dev)
        h, bias = _leaf(inp["h"], dev), _leaf(inp["bias"], dev)
        met, met4 = torch.zeros(2, device=dev), torch.zeros(4, device=dev)
        out = ops.aggregate(h, g, top_k, thr, None, None, bias, ops.HeadEpilogue(y, train, met, int(inp["train"].sum()), grad=True))
        mark()
        out.backward(out.detach())
        mark()
        with torch.no_grad():
            logits = ops.aggregate(h.detach(), g, top_k, thr, None, None, bias.detach(),
                                   ops.HeadEpilogue(y, sets, met4, int((inp["sets"] & 1).ne(0).sum()),
                                                    int((inp["sets"] & 2).ne(0).sum())))
        return dict(grad_logits=out.detach(), metrics=met, grad_h=h.grad, grad_bias=bias.grad, logits=logits, metrics4=met4)
    return make, run


for _kind in GRAPHS:
    for _c in (40, 64):          # the store epilogue needs C % 4 == 0, the head epilogue also C <= 64
        for _top_k, _thr in ((16, 0.0), (None, 0.0)):
            _add(f"agg_hidden_epilogue/{_kind}/C{_c}/k{_top_k}", [G_WS], *_epilogue_case(_kind, _c, _top_k, _thr))
            _add(f"agg_head_epilogue/{_kind}/C{_c}/k{_top_k}", [G_WS, "sngnn_agg_head_workspace_bytes"],
                 *_head_case(_kind, _c, _top_k, _thr))


# ---- attention and signed attention -------------------------------------------------------------------------------------

def _attn_case(kind, c, dtype):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("attn", kind, c)
        return dict(h=R.rows("gaussian", n, c, gen), go=torch.randn(n, c, generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        g = _graph(dev, kind, "loops")
        h = _leaf(inp["h"].to(dtype), dev)
        out = ops.attention(h, g)
        mark()
        out.backward(inp["go"].to(dev).to(dtype))
        return dict(out=out.detach(), grad_h=h.grad)
    return make, run


def _signed_case(kind, c, dtype):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("signed", kind, c)
        return dict(wh=R.rows("gaussian", n, c, gen), go=torch.randn(n, c, generator=gen), gen_seed=_seed_of("coef", kind, c))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        g = _graph(dev, kind, "noloop")
        coef = _leaf(torch.randn(g.num_edges, generator=torch.Generator().manual_seed(inp["gen_seed"])), dev)
        c2 = _leaf(torch.tensor([0.5, -0.3]), dev)
        wh = _leaf(inp["wh"].to(dtype), dev)
        out = ops.signed_propagate(wh, coef, c2, g)
        mark()
        out.backward(inp["go"].to(dev).to(dtype))
        return dict(out=out.detach(), grad_wh=wh.grad, grad_coef=coef.grad, grad_c2=c2.grad)
    return make, run


for _kind in GRAPHS:
    for _c in WIDTHS[_kind]:
        for _dt, _tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            _add(f"attention/{_kind}/C{_c}/{_tag}", [G_WS], *_attn_case(_kind, _c, _dt))
            _add(f"signed/{_kind}/C{_c}/{_tag}", [G_WS], *_signed_case(_kind, _c, _dt))


# ---- the gather-sums: adj_linear, gather / scatter, plain and weighted ------------------------------------------------

def _adj_linear_case(kind, c):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("adj", kind, c)
        return dict(W=torch.randn(c, n, generator=gen), b=torch.randn(c, generator=gen), go=torch.randn(n, c, generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        g = _graph(dev, kind, "sn")
        w = inp["W"].t().contiguous().to(dev).t().requires_grad_(True)          # the reference-shaped column-major parameter
        b = _leaf(inp["b"], dev)
        out = ops.adj_linear(w, b, g)
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_W=w.grad, grad_b=b.grad)
    return make, run


def _gather_case(kind, c, weighted):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("gather", kind, c, weighted)
        return dict(table=R.rows("gaussian", n, c, gen), b=torch.randn(c, generator=gen), go=torch.randn(n, c, generator=gen),
                    gen_seed=_seed_of("w", kind, c))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        g = _graph(dev, kind, "raw")
        table = _leaf(inp["table"], dev)
        if weighted:
            w = _leaf(torch.randn(g.num_edges, generator=torch.Generator().manual_seed(inp["gen_seed"])), dev)
            out = ops.weighted_propagate(table, w, g, g.csr_entries())
        else:
            b = _leaf(inp["b"], dev)
            out = ops.gather_sum(table, b, g)
        mark()
        out.backward(inp["go"].to(dev))
        res = dict(out=out.detach(), grad_table=table.grad)
        res["grad_w" if weighted else "grad_b"] = (w if weighted else b).grad
        return res
    return make, run


for _kind in GRAPHS:
    for _c in WIDTHS[_kind]:
        _add(f"adj_linear/{_kind}/C{_c}", [G_WS], *_adj_linear_case(_kind, _c))
        _add(f"gather_scatter_sum_rows/{_kind}/C{_c}", [G_WS], *_gather_case(_kind, _c, False))
        _add(f"weighted_gather_scatter_sum_rows/{_kind}/C{_c}", [G_WS], *_gather_case(_kind, _c, True))


# ---- the hop families ----------------------------------------------------------------------------------------------------

def _rows_case(tag, kind, c, out_c=None):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen(tag, kind, c)
        return dict(x=R.rows("gaussian", n, c, gen), x0=R.rows("gaussian", n, c, gen),
                    go=torch.randn(n, out_c or c, generator=gen))
    return make


def _gpr_run(kind, c):
    def run(dev, inp, mark):
        from sngnn_amd import ops
        g = _graph(dev, kind, "loops")
        x, gamma = _leaf(inp["x"], dev), _leaf(torch.tensor(R.ppr(0.1, 3)), dev)
        out = ops.gpr_propagate(x, gamma, g)
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_x=x.grad, grad_gamma=gamma.grad)
    return run


def _appnp_run(kind, c):
    def run(dev, inp, mark):
        from sngnn_amd import ops
        x = _leaf(inp["x"], dev)
        out = ops.appnp_propagate(x, _graph(dev, kind, "loops"), 3, 0.1)
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_x=x.grad)
    return run


def _gcn_run(kind, c):
    def run(dev, inp, mark):
        from sngnn_amd import ops
        x, b = _leaf(inp["x"], dev), _leaf(inp["x0"][0].clone(), dev)
        out = ops.gcn_conv(x, b, _graph(dev, kind, "loops"))
        assert type(out.grad_fn).__name__.startswith("_GCNConv"), "the fused arm"
        mark()
        out.backward(inp["go"].to(dev))          # (the backward ends in sngnn_gcn_bias_grad)
        return dict(out=out.detach(), grad_xp=x.grad, grad_bias=b.grad)
    return run


def _gcn2_run(kind, c):
    def make_w():
        return torch.randn(c, c, generator=_cpu_gen("gcn2w", c)) / math.sqrt(c)

    def run(dev, inp, mark):
        from sngnn_amd import ops
        x, x0, w = _leaf(inp["x"], dev), _leaf(inp["x0"], dev), _leaf(make_w(), dev)
        out = ops.gcn2_conv(x, x0, w, _graph(dev, kind, "loops"), 0.1, math.log(1.5))
        assert type(out.grad_fn).__name__.startswith("_GCN2Conv"), "the fused arm"
        mark()
        out.backward(inp["go"].to(dev))          # (with its sngnn_linear_wgrad)
        return dict(out=out.detach(), grad_x=x.grad, grad_x0=x0.grad, grad_weight1=w.grad)
    return run


def _h2gcn_run(kind, c):
    def run(dev, inp, mark):
        from sngnn_amd import ops
        ei, n = _edges(kind)
        adj = ops.H2Adjacency(ei.to(dev), n)          # the two-hop build runs on the guarded scratch too
        x = _leaf(inp["x"], dev)
        out = ops.h2gcn_conv(x, adj)
        assert type(out.grad_fn).__name__.startswith("_H2GCNConv"), "the fused arm"
        mark()
        out.backward(inp["go"].to(dev))
        return dict(edge_index2=adj.edge_index2, out=out.detach(), grad_x=x.grad)
    return run


def _glognn_run(kind, c):
    orders = 2

    def run(dev, inp, mark):
        from sngnn_amd import glognn, ops
        ei, n = _edges(kind)
        key = (kind, "glognn_raw")
        if key not in _DEV:
            _DEV[key] = glognn.raw_graph(ei.to(dev), n)
        gen = _cpu_gen("glognn_w", kind, c)
        ow = _leaf((0.6 + 0.8 * torch.rand(orders, 1, generator=gen)) / orders, dev)
        dw = _leaf((0.6 + 0.8 * torch.rand(c, 1, generator=gen)) / c, dev)
        x, h0 = _leaf(inp["x"], dev), _leaf(inp["x0"], dev)
        out = ops.glognn_norm(x, h0, ow, dw, _DEV[key], *glognn_ref.SCALARS[1], orders, 2, 2)
        assert type(out.grad_fn).__name__.startswith("_GloGNNNorm"), "the fused arm"
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_x=x.grad, grad_h0=h0.grad, grad_orders_weight=ow.grad, grad_diag_weight=dw.grad)
    return run


def _mlpnorm_bias_run(kind, c):
    def run(dev, inp, mark):
        from sngnn_amd import mlpnorm
        rows, bias = _leaf(inp["x"], dev), _leaf(inp["x0"][0].clone(), dev)
        out = mlpnorm._AddBias.apply(rows, bias, _graph(dev, kind, "raw"))
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_rows=rows.grad, grad_bias=bias.grad)
    return run


def _gat_case(kind, c, heads=2):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("gat", kind, c)
        return dict(xp=R.rows("gaussian", n, heads * c, gen), a_src=torch.randn(1, heads, c, generator=gen),
                    a_dst=torch.randn(1, heads, c, generator=gen), go=torch.randn(n, heads * c, generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        xp, a_src, a_dst = _leaf(inp["xp"], dev), _leaf(inp["a_src"], dev), _leaf(inp["a_dst"], dev)
        out = ops.gat_propagate(xp, a_src, a_dst, _graph(dev, kind, "loops"), heads)
        assert type(out.grad_fn).__name__.startswith("_GATPropagate"), "the fused arm"
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_xp=xp.grad, grad_att_src=a_src.grad, grad_att_dst=a_dst.grad)
    return make, run


def _wrgat_case(kind, c, rel=3):
    def make():
        ei, n = _edges(kind)
        gen = _cpu_gen("wrgat", kind, c)
        return dict(P=R.rows("gaussian", n, rel * c, gen), atten=torch.randn(rel, 2 * c, generator=gen),
                    self_rows=torch.randn(n, c, generator=gen), bias=torch.randn(c, generator=gen),
                    go=torch.randn(n, c, generator=gen), et=torch.randint(0, rel, (ei.size(1),), generator=gen),
                    ew=0.5 + torch.rand(ei.size(1), generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        ei, n = _edges(kind)
        key = (kind, "typed", rel)
        if key not in _DEV:
            _DEV[key] = ops.TypedAdjacency(ei.to(dev), inp["et"].to(dev), inp["ew"].to(dev), n, rel)
        leaves = [_leaf(inp[q], dev) for q in ("P", "atten", "self_rows", "bias")]
        out = ops.wrgat_conv(*leaves, _DEV[key], relu=True)
        assert type(out.grad_fn).__name__.startswith("_WRGATConv"), "the fused arm"
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_P=leaves[0].grad, grad_atten=leaves[1].grad, grad_self=leaves[2].grad,
                    grad_bias=leaves[3].grad)
    return make, run


def _acm_case(kind, c):
    def make():
        _, n = _edges(kind)
        gen = _cpu_gen("acm", kind, c)
        return dict(p=R.rows("gaussian", n, 3 * c, gen), go=torch.randn(n, c, generator=gen),
                    par=[torch.rand(c, 1, generator=gen) * 2 - 1 for _ in range(3)] +
                        [(torch.rand(3, 3, generator=gen) * 2 - 1) / math.sqrt(3.0)])

    def run(dev, inp, mark):
        from sngnn_amd import ops
        p = _leaf(inp["p"], dev)
        par = [_leaf(t, dev) for t in inp["par"]]
        out, lh, datt = ops.acm_filterbank_fused(p, *par, _graph(dev, kind, "acm"), True)
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), lh=lh, datt=datt, grad_P=p.grad, **{f"grad_par{i}": t.grad for i, t in enumerate(par)})
    return make, run


for _kind in GRAPHS:
    for _c in WIDTHS[_kind]:
        _add(f"gpr_propagate/{_kind}/C{_c}", ["sngnn_prop_workspace_bytes"], _rows_case("gpr", _kind, _c), _gpr_run(_kind, _c))
        _add(f"appnp/{_kind}/C{_c}", ["sngnn_prop_workspace_bytes"], _rows_case("appnp", _kind, _c), _appnp_run(_kind, _c))
        _add(f"gat_propagate/{_kind}/C{_c}", ["sngnn_gat_workspace_bytes"], *_gat_case(_kind, _c))
        _add(f"wrgat_conv/{_kind}/C{_c}", ["sngnn_wrgat_workspace_bytes"], *_wrgat_case(_kind, _c))
        _add(f"acm_filterbank/{_kind}/C{_c}", ["sngnn_acm_workspace_bytes"], *_acm_case(_kind, _c))
        _add(f"gcn_conv/{_kind}/C{_c}", ["sngnn_gcn_workspace_bytes"], _rows_case("gcn", _kind, _c), _gcn_run(_kind, _c))
        _add(f"h2gcn/{_kind}/C{_c}", ["sngnn_two_hop_workspace_bytes", "sngnn_h2gcn_workspace_bytes"],
             _rows_case("h2gcn", _kind, _c, 2 * _c), _h2gcn_run(_kind, _c))
        _add(f"mlpnorm_bias_grad/{_kind}/C{_c}", ["sngnn_gcn_workspace_bytes"], _rows_case("mlpnorm", _kind, _c),
             _mlpnorm_bias_run(_kind, _c))
        _c2 = min(_c, 128)          # GCN2's widest fused layer
        _add(f"gcn2_conv/{_kind}/C{_c2}", ["sngnn_gcn2_workspace_bytes", "wgrad"], _rows_case("gcn2", _kind, _c2),
             _gcn2_run(_kind, _c2))
        if _c <= 64:                # the GloGNN norm layer's widest fused layer
            _add(f"glognn_norm/{_kind}/C{_c}", ["sngnn_glognn_workspace_bytes"], _rows_case("glognn", _kind, _c),
                 _glognn_run(_kind, _c))


# ---- the dense entries ---------------------------------------------------------------------------------------------------

DENSE_N = (700, 1100)


def _gram_case(n, c):
    def make():
        gen = _cpu_gen("gram", n, c)
        return dict(a=torch.randn(n, c, generator=gen), b=torch.randn(n, c, generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        a, b = inp["a"].to(dev), inp["b"].to(dev)
        first = ops.gram(a)
        mark()
        return dict(aa=first, ab=ops.gram(a, b))
    return make, run


def _bn_case(n, c, post):
    def make():
        gen = _cpu_gen("bn", n, c, post)
        return dict(x=torch.randn(n, c, generator=gen), bias=torch.randn(c, generator=gen), go=torch.randn(n, c, generator=gen),
                    gamma=1.0 + 0.2 * torch.randn(c, generator=gen), beta=0.2 * torch.randn(c, generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        bn = torch.nn.BatchNorm1d(c).to(dev)
        with torch.no_grad():
            bn.weight.copy_(inp["gamma"])
            bn.bias.copy_(inp["beta"])
        seed = torch.tensor([77], dtype=torch.int64, device=dev)
        x, bias = _leaf(inp["x"], dev), _leaf(inp["bias"], dev)
        out = ops.batch_norm_post_act(x, bn, 0.5, seed) if post else ops.batch_norm_act(x, bn, bias, 0.5, seed=seed)
        mark()
        out.backward(inp["go"].to(dev))
        res = dict(out=out.detach(), grad_x=x.grad, grad_gamma=bn.weight.grad, grad_beta=bn.bias.grad,
                   running_mean=bn.running_mean, running_var=bn.running_var)
        if not post:
            res["grad_bias"] = bias.grad
        return res
    return make, run


def _blend_case(n, c, with_epilogue):
    def make():
        gen = _cpu_gen("blend", n, c)
        return dict(out0=torch.randn(n, c, generator=gen), out1=torch.randn(n, c, generator=gen), go=torch.randn(n, c, generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        out0, out1, beta = _leaf(inp["out0"], dev), _leaf(inp["out1"], dev), _leaf(torch.tensor([0.3]), dev)
        epi = None
        if with_epilogue:
            epi = ops.HiddenEpilogue(True, 0.5, True, torch.tensor([99], dtype=torch.int64, device=dev))
        out = ops.blend(out0, out1, beta, epi)
        assert type(out.grad_fn).__name__.startswith("_Blend"), "the fused arm"
        assert epi is None or epi.applied
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad0=out0.grad, grad1=out1.grad, grad_beta=beta.grad)
    return make, run


def _head_nll_case(n, c):
    def make():
        gen = _cpu_gen("head_nll", n, c)
        r = torch.rand(n, generator=gen)
        return dict(z=torch.randn(n, c, generator=gen), z1=torch.randn(n, c, generator=gen), y=torch.randint(0, c, (n,), generator=gen),
                    train=(r < 0.6).to(torch.uint8),
                    sets=((r >= 0.6) & (r < 0.8)).to(torch.uint8) + 2 * (r >= 0.8).to(torch.uint8))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        y, train, sets = inp["y"].to(dev), inp["train"].to(dev), inp["sets"].to(dev)
        n_tr, n_a, n_b = int(inp["train"].sum()), int((inp["sets"] & 1).ne(0).sum()), int((inp["sets"] & 2).ne(0).sum())
        z = _leaf(inp["z"], dev)
        loss, correct = ops.head_nll(z, y, train, n_tr)
        loss.backward()
        res = dict(loss=loss.detach(), correct=correct, grad_z=z.grad)
        if c <= 64:               # (sngnn_head_nll2's limit; sngnn_head_nll alone runs its wide kernel above it)
            mark()
            res["metrics4"] = ops.head_nll2(z.detach(), y, sets, n_a, n_b)
        if c % 4 == 0 and c <= 64:          # the blended head: rows of 16-byte vectors
            mark()
            out0, out1, beta = _leaf(inp["z"], dev), _leaf(inp["z1"], dev), _leaf(torch.tensor([0.3]), dev)
            met = torch.zeros(2, device=dev)
            head = ops.HeadEpilogue(y, train, met, n_tr, grad=True)
            g = ops.blend_head(out0, out1, beta, head)
            assert head.applied and g is not None
            mark()
            g.backward(g.detach())
            res.update(blend_head_grad=g.detach(), blend_head_metrics=met, blend_head_grad0=out0.grad,
                       blend_head_grad1=out1.grad, blend_head_grad_beta=beta.grad)
        return res
    return make, run


def _ggcn_case(n, c, prev_elu):
    def make():
        gen = _cpu_gen("ggcn", n, c)
        return {q: torch.randn(n, c, generator=gen) for q in ("prop", "wh", "prev", "go")}

    def run(dev, inp, mark):
        from sngnn_amd import ops
        prop, wh, prev, cs = (_leaf(inp["prop"], dev), _leaf(inp["wh"], dev), _leaf(inp["prev"], dev),
                              _leaf(torch.tensor([0.4, 1.3]), dev))
        out = ops.ggcn_transition(prop, wh, cs, prev, 0.7, prev_elu)
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_prop=prop.grad, grad_wh=wh.grad, grad_prev=prev.grad, grad_cs=cs.grad)
    return make, run


def _linear_wgrad_case(n, c, f):
    def make():
        gen = _cpu_gen("wgrad", n, c, f)
        return dict(x=torch.randn(n, f, generator=gen), w=torch.randn(c, f, generator=gen) / math.sqrt(f),
                    b=torch.randn(c, generator=gen), go=torch.randn(n, c, generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import ops
        lin = torch.nn.Linear(f, c).to(dev)
        with torch.no_grad():
            lin.weight.copy_(inp["w"])
            lin.bias.copy_(inp["b"])
        out = ops.linear(inp["x"].to(dev), lin)
        mark()
        out.backward(inp["go"].to(dev))
        return dict(out=out.detach(), grad_weight=lin.weight.grad, grad_bias=lin.bias.grad)
    return make, run


def _replica_case(n, r, c, f):
    def make():
        gen = _cpu_gen("replica", n, r, c, f)
        rnd = torch.rand(r, n, generator=gen)
        return dict(g=torch.randn(r * n, c, generator=gen), x=torch.randn(n, f, generator=gen),
                    out0=torch.randn(r * n, c, generator=gen), out1=torch.randn(r * n, c, generator=gen),
                    beta=torch.rand(r, generator=gen), y=torch.randint(0, c, (n,), generator=gen),
                    sel=(rnd < 0.6).to(torch.uint8))

    def run(dev, inp, mark):
        from sngnn_amd import splits
        d = {k: v.to(dev) for k, v in inp.items()}
        gw, gb = splits.replica_wgrad(d["g"], d["x"], r)
        mark()
        g0, g1, gbeta = splits.replica_blend_backward(d["g"], d["out0"], d["out1"], d["beta"])
        mark()
        counts = inp["sel"].sum(dim=1).to(torch.int64).clamp_min(1).to(dev)
        met, met_b = torch.zeros((r, 2), device=dev), torch.zeros((r, 2), device=dev)
        gl = splits.replica_head(d["out0"], d["y"], d["sel"], counts, met, grad=True)
        mark()
        gl_b = splits.replica_head(d["out0"], d["y"], d["sel"], counts, met_b, logits1=d["out1"], beta=d["beta"], grad=True)
        return dict(grad_W=gw, grad_b=gb, g0=g0, g1=g1, grad_beta=gbeta, head_grad=gl, head_metrics=met,
                    blend_head_grad=gl_b, blend_head_metrics=met_b)
    return make, run


def _toolbox_case(n, f):
    def make():
        gen = _cpu_gen("toolbox", n, f)
        return dict(x=torch.randn(n, f, generator=gen), y=torch.randint(0, 4, (n,), generator=gen))

    def run(dev, inp, mark):
        from sngnn_amd import toolbox
        x, y = inp["x"].to(dev), inp["y"].to(dev)
        hist = toolbox.node_similarity_histogram(x, bins=50, y=y, clamp=False)
        mark()
        hist1 = toolbox.node_similarity_histogram(x, bins=200)
        mark()
        idx, sim = toolbox.knn_graph(x, 8)
        res = dict(knn_idx=idx, knn_sim=sim)
        res.update({f"hist2_{q}": t for q, t in hist._asdict().items()})
        res.update({f"hist1_{q}": t for q, t in hist1._asdict().items()})
        return res
    return make, run


def _gather_floor_case(kind, c):
    def make():
        _, n = _edges(kind)
        return dict(table=torch.randn(n, c, generator=_cpu_gen("floor", kind, c)))

    def run(dev, inp, mark):
        from sngnn_amd import _lib
        g = _graph(dev, kind, "sn")
        table = inp["table"].to(dev)
        out = torch.zeros((g.num_nodes, c), dtype=torch.float32, device=dev)
        for mode in (0, 1):
            ws = _lib.workspace("gather_floor", _lib.load().sngnn_gather_floor_workspace_bytes(), dev)
            _lib.call("sngnn_gather_floor", dev, g.handle, table, c, mode, out if mode else None, ws)
            mark()
        return dict(out=out)
    return make, run


for _n in DENSE_N:
    for _c in (1, 5, 40, 64):
        _add(f"gram/N{_n}/C{_c}", ["glognn_gram"], *_gram_case(_n, _c))
    for _c in (1, 5, 40, 64, 130):
        _add(f"bn_train/N{_n}/C{_c}", ["bn_train"], *_bn_case(_n, _c, False))
        _add(f"bn_post/N{_n}/C{_c}", ["bn_train"], *_bn_case(_n, _c, True))
        _add(f"blend_backward/N{_n}/C{_c}", ["blend"], *_blend_case(_n, _c, False))
        _add(f"blend_backward_epilogue/N{_n}/C{_c}", ["blend"], *_blend_case(_n, _c, True))
        _add(f"ggcn_transition/N{_n}/C{_c}", ["ggcn_transition"], *_ggcn_case(_n, _c, False))
        _add(f"ggcn_transition_prev_elu/N{_n}/C{_c}", ["ggcn_transition"], *_ggcn_case(_n, _c, True))
    for _c in (1, 5, 40, 64, 130):
        _add(f"head_nll/N{_n}/C{_c}", ["head"], *_head_nll_case(_n, _c))
    for _c, _f in ((40, 33), (40, 64), (5, 16), (64, 128), (130, 5)):      # N = 1 100 with F in {16, 64, 128}: the MFMA path
        _add(f"linear_wgrad/N{_n}/C{_c}/F{_f}", ["wgrad"], *_linear_wgrad_case(_n, _c, _f))
    for _r, _c in ((3, 5), (3, 8), (5, 8), (6, 8), (10, 5)):                # R C = 15, 24, 40, 48, 50: every KACC arm
        _add(f"replica/N{_n}/R{_r}/C{_c}", ["replica_wgrad", "replica_head", "replica_blend"], *_replica_case(_n, _r, _c, 33))
    _add(f"toolbox/N{_n}", ["cosine_hist", "knn"], *_toolbox_case(_n, 33))
for _kind in GRAPHS:
    for _c in (40, 64):
        _add(f"gather_floor/{_kind}/C{_c}", ["gather_floor"], *_gather_floor_case(_kind, _c))


# ------------------------------------------------------------------ running a case

PURPOSES = {"wgrad": "sngnn_linear_wgrad_workspace_bytes", "bn_train": "sngnn_bn_train_workspace_bytes",
            "head": "sngnn_head_workspace_bytes", "blend": "sngnn_blend_workspace_bytes",
            "ggcn_transition": "sngnn_ggcn_transition_workspace_bytes", "glognn_gram": "sngnn_glognn_gram_workspace_bytes",
            "replica_wgrad": "sngnn_replica_wgrad_workspace_bytes", "replica_head": "sngnn_replica_head_workspace_bytes",
            "replica_blend": "sngnn_replica_blend_workspace_bytes", "cosine_hist": "sngnn_cosine_hist_workspace_bytes",
            "knn": "sngnn_knn_workspace_bytes", "gather_floor": "sngnn_gather_floor_workspace_bytes"}
_SEEN = set()          # size entries / purposes the harness handed out, over all cases run in this session
_RAN = set()
_ENTERED = {}          # library entry -> the cases in which it went through ``_lib.call`` while the scratch was guarded


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.uint8) if t.numel() else t


def _force_fused(monkeypatch):
    from sngnn_amd import acm, gat, gcn, gcn2, glognn, h2gcn, prop, wrgat
    for mod, flag in ((prop, "FUSE_GPR"), (gat, "FUSE_GAT"), (wrgat, "FUSE_WRGAT"), (acm, "FUSE_ACM"), (gcn, "FUSE_GCN"),
                      (gcn2, "FUSE_GCN2"), (h2gcn, "FUSE_H2GCN"), (glognn, "FUSE_GLOGNN")):
        monkeypatch.setattr(mod, flag, True)


def _run_case(name, dev, monkeypatch):
    from sngnn_amd import _lib
    make, run, expects = CASES[name]
    _force_fused(monkeypatch)
    real_call = _lib.call

    def spy(entry, *args):
        _ENTERED.setdefault(entry, set()).add(name)
        return real_call(entry, *args)
    inp = make()
    want = run(dev, inp, lambda: None)
    torch.cuda.synchronize()
    assert want, "a case returns its outputs"
    failures = []
    for poison, tag in ((GS.POISON_NAN, "0x7FC12345 words"), (GS.POISON_ONES, "0xFF bytes")):
        with monkeypatch.context() as m:
            harness = GS.GuardedScratch(poison).install(m)
            m.setattr(_lib, "call", spy)
            got = run(dev, inp, harness.repoison)
            torch.cuda.synchronize()
            _SEEN.update(harness.labels())
            missing = [e for e in expects if e not in harness.labels()]
            assert not missing, f"{name}: the case did not reach {missing} (handed out: {sorted(harness.labels())})"
            failures += [f"poison {tag}: {line}" for line in harness.damage()]
            assert got.keys() == want.keys()
            for q in want:
                a, b = want[q], got[q]
                assert a.dtype == b.dtype and a.shape == b.shape, (name, q)
                if not torch.equal(_bits(a), _bits(b)):
                    bad = (_bits(a) != _bits(b)).nonzero().flatten()
                    first = int(bad[0]) // max(a.element_size(), 1)
                    failures.append(f"poison {tag}: output {q} differs from the unguarded run in {bad.numel()} bytes, first "
                                    f"at element {first} of {a.numel()} (unguarded {a.reshape(-1)[first].item()!r}, guarded "
                                    f"{b.reshape(-1)[first].item()!r}); scratch handed out: "
                                    f"{[(r.label, r.args, r.nbytes) for r in harness.records]}")
    _RAN.add(name)
    assert not failures, f"{name}:\n  " + "\n  ".join(failures)


@pytest.mark.parametrize("name", sorted(CASES))
def test_scratch_contract(cuda, monkeypatch, name):
    _run_case(name, cuda, monkeypatch)


def _header_workspace_entries():
    with open(os.path.join(ROOT, "include", "sngnn_hip.h")) as fh:
        text = fh.read()
    return sorted(set(re.findall(r"\bint64_t\s+(sngnn_\w*workspace_bytes)\s*\(", text)))


def test_every_size_function_of_the_header_was_handed_out(cuda, monkeypatch):
    """The header's ``*_workspace_bytes`` names, each handed out by the harness at least once.  (Runs whatever case of
    the table this session has not run yet - it passes alone too - and ignores their own verdicts: those belong to
    ``test_scratch_contract``.)"""
    names = _header_workspace_entries()
    assert len(names) >= 23 and "sngnn_graph_workspace_bytes" in names and "sngnn_knn_workspace_bytes" in names
    first_of = {}
    for name in sorted(CASES):
        first_of.setdefault(name.split("/")[0], name)
    for name in first_of.values():          # one case per family is enough to see its size entries
        if name.split("/")[0] not in {r.split("/")[0] for r in _RAN}:
            try:
                _run_case(name, cuda, monkeypatch)
            except AssertionError:
                pass
    seen = {PURPOSES.get(label, label) for label in _SEEN}
    assert not [n for n in names if n not in seen], (sorted(seen), names)


ALL = (1, 5, 40, 64, 130)
VEC4 = (40, 64)             # the store epilogue's and the head epilogue's widths (C % 4 == 0; the head also C <= 64)
UPTO64 = (1, 5, 40, 64)
ON_GRAPHS = ("deg", "ring")          # where a graph family runs every width it takes
# entry -> (family of the table, the widths at which a case of that family must ENTER it, on both of ON_GRAPHS or, a
# dense family, at both of DENSE_N; None: the family has no width - one case must enter it)
COVERED_BY = {
    "sngnn_agg_forward": ("agg", ALL), "sngnn_agg_backward_topk": ("agg", ALL),
    "sngnn_agg_forward_half": ("agg_bf16", ALL), "sngnn_agg_backward_half": ("agg_bf16", ALL),
    "sngnn_agg_forward_prepared": ("agg_prepared", ALL), "sngnn_agg_forward_rows": ("agg_prepared", ALL),
    "sngnn_agg_forward_normalized": ("agg_prepared", ALL), "sngnn_agg_backward": ("agg_prepared", ALL),
    "sngnn_agg_forward_epilogue": ("agg_prepared", ALL), "sngnn_agg_forward_prepared_epilogue": ("agg_prepared", ALL),
    "sngnn_agg_backward_bits": ("agg_prepared", ALL),
    "sngnn_attn_forward": ("attention", ALL), "sngnn_attn_backward": ("attention", ALL),
    "sngnn_attn_forward_half": ("attention", ALL), "sngnn_attn_backward_half": ("attention", ALL),
    "sngnn_signed_forward": ("signed", ALL), "sngnn_signed_backward": ("signed", ALL),
    "sngnn_signed_forward_half": ("signed", ALL), "sngnn_signed_backward_half": ("signed", ALL),
    "sngnn_adj_linear_forward": ("adj_linear", ALL), "sngnn_adj_linear_backward": ("adj_linear", ALL),
    "sngnn_gather_sum_rows": ("gather_scatter_sum_rows", ALL), "sngnn_scatter_sum_rows": ("gather_scatter_sum_rows", ALL),
    "sngnn_weighted_gather_sum_rows": ("weighted_gather_scatter_sum_rows", ALL),
    "sngnn_weighted_scatter_sum_rows": ("weighted_gather_scatter_sum_rows", ALL),
    "sngnn_prop_gpr_forward": ("gpr_propagate", ALL), "sngnn_prop_gpr_backward": ("gpr_propagate", ALL),
    "sngnn_prop_appnp": ("appnp", ALL), "sngnn_gat_forward": ("gat_propagate", ALL), "sngnn_gat_backward": ("gat_propagate", ALL),
    "sngnn_wrgat_forward": ("wrgat_conv", ALL), "sngnn_wrgat_backward": ("wrgat_conv", ALL),
    "sngnn_acm_forward": ("acm_filterbank", ALL), "sngnn_acm_backward": ("acm_filterbank", ALL),
    "sngnn_gcn_hop": ("gcn_conv", ALL), "sngnn_gcn_bias_grad": ("gcn_conv", ALL),
    "sngnn_gcn2_hop": ("gcn2_conv", (1, 5, 40, 64, 128)),
    "sngnn_two_hop_count": ("h2gcn", ALL), "sngnn_two_hop_fill": ("h2gcn", ALL), "sngnn_h2gcn_hop": ("h2gcn", ALL),
    "sngnn_glognn_forward": ("glognn_norm", UPTO64), "sngnn_glognn_backward": ("glognn_norm", UPTO64),
    "sngnn_gather_floor": ("gather_floor", VEC4),
    "sngnn_glognn_gram": ("gram", UPTO64),
    "sngnn_bn_train_forward": ("bn_train", ALL), "sngnn_bn_train_backward": ("bn_train", ALL),
    "sngnn_bn_post_forward": ("bn_post", ALL), "sngnn_bn_post_backward": ("bn_post", ALL),
    "sngnn_blend_backward": ("blend_backward", ALL), "sngnn_blend_backward_epilogue": ("blend_backward_epilogue", ALL),
    "sngnn_ggcn_transition_backward": ("ggcn_transition", ALL),
    "sngnn_head_nll": ("head_nll", ALL), "sngnn_head_nll2": ("head_nll", UPTO64), "sngnn_head_nll_blend": ("head_nll", VEC4),
    "sngnn_linear_wgrad": ("linear_wgrad", (5, 40, 64, 130)),
    "sngnn_replica_wgrad": ("replica", (5, 8)), "sngnn_replica_head_nll": ("replica", (5, 8)),
    "sngnn_replica_blend_backward": ("replica", (5, 8)),
    "sngnn_cosine_hist": ("toolbox", None), "sngnn_knn_graph": ("toolbox", None),
}
# the store epilogue proper (bias / relu / dropout in the stores) and the head epilogue are flags of entries counted
# above; their cases are agg_hidden_epilogue and agg_head_epilogue at VEC4, which assert their own arm
# (``head_supported``, ``epi.applied``) when they run.


def _width_of(name):
    m = re.search(r"/C(\d+)(/|$)", name)
    return int(m.group(1)) if m else None


def _needed_cases():
    """For every entry of COVERED_BY, the (family, place, width) triples it is promised at, each with the table's first
    case there."""
    need = {}
    for entry, (family, widths) in COVERED_BY.items():
        for name in sorted(CASES):
            parts = name.split("/")
            if parts[0] != family:
                continue
            if widths is None:
                need.setdefault((family, None, None), name)
            elif parts[1] in ON_GRAPHS + tuple(f"N{n}" for n in DENSE_N) and _width_of(name) in widths:
                need.setdefault((family, parts[1], _width_of(name)), name)
    return need


def test_the_table_enters_every_entry_with_a_workspace_parameter(cuda, monkeypatch):
    """Every function of the header with a ``workspace`` (or ``head_workspace``) parameter went through ``_lib.call``
    while the scratch was guarded and poisoned, at every width COVERED_BY promises, on the degree graph and on the ring
    (a dense family: at both row counts).  Taken from the calls the guarded runs recorded, not from the table's names: a
    case that is in the table but takes another arm (no kept-bits path on its graph, say) does not count.  (Runs the
    cases it needs that this session has not run yet - it passes alone too - and ignores their own verdicts: those
    belong to ``test_scratch_contract``.)"""
    with open(os.path.join(ROOT, "include", "sngnn_hip.h")) as fh:
        text = fh.read()
    entries = sorted(set(m.group(1) for m in re.finditer(r"\bint\s+(sngnn_\w+)\s*\(([^;{]*?)\)\s*;", text, re.S)
                         if re.search(r"\bvoid\s*\*\s*workspace\b", m.group(2))))
    assert len(entries) >= 59          # (the header's count when this was written: the pattern still finds them)
    assert not [e for e in entries if e not in COVERED_BY], [e for e in entries if e not in COVERED_BY]
    need = _needed_cases()
    for name in sorted(set(need.values()) - _RAN):
        try:
            _run_case(name, cuda, monkeypatch)
        except AssertionError:
            pass
    missing = []
    for entry, (family, widths) in sorted(COVERED_BY.items()):
        entered = {n for n in _ENTERED.get(entry, ()) if n.split("/")[0] == family}
        if widths is None:
            if not entered:
                missing.append(f"{entry}: entered by no case of {family}")
            continue
        places = sorted({place for fam, place, _ in need if fam == family})
        assert places, (entry, family)
        for place in places:
            lacking = [c for c in widths if (family, place, c) in need
                       and not any(n.split("/")[1] == place and _width_of(n) == c for n in entered)]
            absent = [c for c in widths if (family, place, c) not in need]
            if lacking or absent:
                missing.append(f"{entry}: {family}/{place} does not enter it at C = {lacking}, has no case at C = {absent}")
    assert not missing, "\n  ".join(["the guarded runs did not enter:"] + missing)


# ------------------------------------------------------------------ lifetime

def _plus_model(dev, data, hidden, seed):
    from sngnn_amd import SNGNN_Plus
    torch.manual_seed(seed)
    n, f = data.x.shape
    model = SNGNN_Plus(f, hidden, 4, n, 2, 16, 0.0, 1, 0.5, True).to(dev)
    return model, torch.optim.Adam(model.parameters(), lr=0.01)


def _lifetime_data(dev, features, seed=5):
    from sngnn_amd.synth import Data
    ei, n = _edges("deg")
    gen = torch.Generator().manual_seed(seed)
    r = torch.rand(n, generator=gen)
    return Data(x=torch.randn(n, features, generator=gen), edge_index=ei.clone(), y=torch.randint(0, 4, (n,), generator=gen),
                train_mask=r < 0.6, val_mask=(r >= 0.6) & (r < 0.8), test_mask=r >= 0.8).to(dev)


def _two_replays(epoch):
    epoch.graph.replay()
    epoch.graph.replay()
    torch.cuda.synchronize()
    return epoch.metrics.clone()


def test_a_captured_epoch_keeps_its_scratch(cuda, monkeypatch):
    """A ``GraphedEpoch`` has the addresses of the ``_lib.workspace`` buffers its eager warm-up and its capture were
    handed baked into its launches.  Training a second, larger model afterwards must not release them: every one of
    them is still alive (the deterministic, host-side gate) after each of their slots was made to grow; and the
    captured epoch's replays still equal those of an undisturbed twin built from the same seed, bit for bit.

    The epoch's buffers are taken from the hand-outs while it is built - (purpose, stream, buffer) - not from the
    process-wide cache: which pool stream the epoch captures on, and what an earlier test left there, do not matter."""
    from sngnn_amd import _lib, ops
    from sngnn_amd.train import GraphedEpoch, train_step
    data = _lifetime_data(cuda, 16)
    twin_model, twin_opt = _plus_model(cuda, data, 32, 31)
    want = _two_replays(GraphedEpoch(twin_model, data, twin_opt, warmup=1))

    handed, real = {}, _lib.workspace

    def spy(key, nbytes, device):
        ws = real(key, nbytes, device)
        handed[(key, _lib.stream(device), ws.data_ptr())] = ws
        return ws

    model, opt = _plus_model(cuda, data, 32, 31)
    with monkeypatch.context() as m:
        m.setattr(_lib, "workspace", spy)
        m.setattr(ops, "_workspace", spy)
        epoch = GraphedEpoch(model, data, opt, warmup=1)
    assert _lib.workspace is real and ops._workspace is real
    assert {"wgrad", "bn_train"} <= {k[0] for k in handed}, sorted(map(str, handed))
    streams = sorted({k[1] for k in handed})          # (its side stream, and the current one for what precedes the warm-up)
    assert any(st != _lib.stream(cuda) for st in streams), f"the epoch warms up and captures on a side stream, not on {streams}"
    refs = {k: weakref.ref(ws) for k, ws in handed.items()}
    ranges = {k: (ws.data_ptr(), ws.numel()) for k, ws in handed.items()}
    handed.clear()

    def on(stream_id, fn):
        if stream_id == _lib.stream(cuda):
            return fn()
        side = torch.cuda.ExternalStream(stream_id, device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            out = fn()
        torch.cuda.current_stream(cuda).wait_stream(side)
        return out

    # a second model with a wider hidden layer and more input features: one eager step on the current stream and on
    # the epoch's; then every slot that step did not outgrow (an earlier test may have left it larger) is asked for
    # more than it holds, so that EVERY buffer of the epoch has been outgrown whatever ran before
    big_data = _lifetime_data(cuda, 48)
    big_model, big_opt = _plus_model(cuda, big_data, 96, 32)
    for st in sorted(set(streams) | {_lib.stream(cuda)}):
        on(st, lambda: train_step(big_model, big_data, big_opt))
    by_model = sorted(str(k[:2]) for k, (ptr, _) in ranges.items()
                      if on(k[1], lambda k=k: _lib.workspace(k[0], 1, cuda)).data_ptr() != ptr)
    for k, (ptr, size) in ranges.items():
        on(k[1], lambda k=k, size=size: _lib.workspace(k[0], 2 * size + 1, cuda))
    torch.cuda.synchronize()
    gc.collect()
    print(f"lifetime: {len(refs)} buffers handed to the epoch on streams {streams}; outgrown by the larger model: {by_model}")
    stuck = sorted(str(k[:2]) for k, (ptr, _) in ranges.items()
                   if on(k[1], lambda k=k: _lib.workspace(k[0], 1, cuda)).data_ptr() == ptr)
    assert not stuck, f"these buffers of the epoch are still the live ones of their slots: {stuck}"
    dead = sorted(str(k[:2]) for k, ref in refs.items() if ref() is None)
    assert not dead, f"buffers a captured epoch points into were released when a later call asked for more: {dead}"

    # where the allocator hands a recorded range to someone else, that tensor must survive the replays (after the fix a
    # recorded buffer is alive, so nothing can overlap it and only the gate above holds)
    canaries = []
    for _, (_, size) in list(ranges.items()) * 8:
        if len(canaries) < 64:
            canaries.append(torch.full((size,), GS.CANARY, dtype=torch.uint8, device=cuda))
    overlapping = [t for t in canaries for base, size in ranges.values()
                   if t.data_ptr() < base + size and base < t.data_ptr() + t.numel()]
    print(f"lifetime: {len(overlapping)} of {len(canaries)} canary tensors overlap a recorded scratch range")
    got = _two_replays(epoch)
    for t in overlapping:
        assert bool((t == GS.CANARY).all()), "a replay wrote its partial sums into a tensor allocated after the capture"
    assert torch.equal(_bits(got), _bits(want)), (got.tolist(), want.tolist())

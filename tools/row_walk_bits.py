#!/usr/bin/env python3
"""The bits of the kernels on csrc/row_walk.h - the seven gather-sum hop kernels on walk_rows and the nine edge-softmax
kernels of GAT and WRGAT on row_unit: one line per case - the case's
name, then the sha256 of each output's bytes, forward and backward where the operator has one.  Inputs come from seeded
CPU generators, so two builds of the library can be compared line for line:

    python tools/row_walk_bits.py > a.txt
    SNGNN_LIB_PATH=/path/to/other/libsngnn_hip.so python tools/row_walk_bits.py > b.txt
    cmp a.txt b.txt

Graphs: tests/gpr_ref.degree_graph (in- and out-degrees 1, 2, 16, 17, 128, 129, 400: every row class, four tasks) and
tests/gpr_ref.hub_graph (a row of 18 tasks on either side: the finalize's four-chain loop), each built the way a family
needs it (loops replaced, raw, unique and loop-free).  Cases: gpr_propagate / appnp_propagate at C = 5, 6, 40, 512
(K = 2), gcn_conv at the same widths, mixhop_propagate at (47, 3) and (64, 2) (narrow-vector slices), GCN2Conv at 40 and
47, h2gcn_conv at 6 and 40, glognn_norm at 5 and 40 (two orders), the ACM layer at 5 and 40 with and without relu,
adj_linear forward and backward with bias at 40 (the lowest source id of either graph's SN edge list is above 0: the
shifted rows and the bias-only tail run), once more without the sources below 3, and a weighted gather-sum (GGCN's
plain propagation) at 40.  The softmax families, on every lane layout their tests reach: gat_propagate at GAT_SHAPES
(out, the saved m | l, grad_xp, grad_att_src, grad_att_dst), and wrgat_conv at WRGAT_SHAPES on the graph with one
explicit loop per node but the last seven (relations wrgat_ref.scattered; TypedAdjacency sorts by relation), with and
without edge weights, the root slice (and bias) and the fused relu (out, the saved m | l, grad_P, grad_atten, grad_self,
grad_bias).  The hub's 18 tasks on either side run the three families' task-order merges."""
import hashlib
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import acm_ref, glognn_ref, wrgat_ref       # noqa: E402
from tests import gpr_ref as R              # noqa: E402


def sha(t):
    if t is None:
        return "none"
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def emit(name, *tensors):
    print(name, *[sha(t) for t in tensors], flush=True)


def gen_for(name):
    return torch.Generator().manual_seed(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def saved(out, function, index):
    """A tensor the fused autograd function saved for its backward (the softmax's m and l [2, N, H]); read before
    ``backward`` frees it.  The plain op sequence has no such node: the tool is about the kernels."""
    assert type(out.grad_fn).__name__.startswith(function), "the fused arm"
    return out.grad_fn.saved_tensors[index]


# the (heads, C) and (R, C) pairs of tests/test_gat_gpu.py and tests/test_wrgat_gpu.py: SHAPES, then the other lane layouts
GAT_SHAPES = ((1, 1), (1, 40), (2, 5), (2, 64), (3, 7), (4, 33), (8, 8), (1, 130), (2, 96), (1, 257), (1, 512), (16, 32))
WRGAT_SHAPES = ((1, 1), (1, 40), (2, 5), (3, 7), (4, 33), (5, 8), (4, 64), (16, 32), (1, 130), (2, 96), (1, 257), (1, 512))


def main():
    from sngnn_amd import acmgcn, glognn, ops, prop
    from sngnn_amd.gcnii import GCN2Conv
    from sngnn_amd.graph import LOOPS_REPLACE, Graph
    dev = torch.device("cuda:0")
    for gname, (ei, n) in (("degree", R.degree_graph()), ("hub", R.hub_graph())):
        eid = ei.to(dev)
        loops = Graph(eid, n, True, LOOPS_REPLACE)
        for c in (5, 6, 40, 512):
            name = f"{gname} gpr C={c}"
            gen = gen_for(name)
            x, g = randn(gen, n, c).to(dev).requires_grad_(True), randn(gen, n, c).to(dev)
            gamma = torch.tensor(R.ppr(0.1, 2)).to(dev).requires_grad_(True)
            out = ops.gpr_propagate(x, gamma, loops)
            out.backward(g)
            emit(name, out, x.grad, gamma.grad)
            name = f"{gname} appnp C={c}"
            x = randn(gen, n, c).to(dev).requires_grad_(True)
            out = ops.appnp_propagate(x, loops, 2, 0.1)
            out.backward(g)
            emit(name, out, x.grad)
            name = f"{gname} gcn_conv C={c}"
            xp, b = randn(gen, n, c).to(dev).requires_grad_(True), randn(gen, c).to(dev).requires_grad_(True)
            out = ops.gcn_conv(xp, b, loops)
            out.backward(g)
            emit(name, out, xp.grad, b.grad)
        for c, hops in ((47, 3), (64, 2)):
            name = f"{gname} mixhop C={c} hops={hops}"
            gen = gen_for(name)
            p, g = randn(gen, n, (hops + 1) * c).to(dev).requires_grad_(True), randn(gen, n, (hops + 1) * c).to(dev)
            out = ops.mixhop_propagate(p, loops, hops)
            out.backward(g)
            emit(name, out, p.grad)
        for c in (40, 47):
            name = f"{gname} gcn2conv C={c}"
            gen = gen_for(name)
            conv = GCN2Conv(c, 0.1, 0.5, 1).to(dev)
            with torch.no_grad():
                conv.weight1.copy_((randn(gen, c, c) / math.sqrt(c)).to(dev))
            x, x0 = (randn(gen, n, c).to(dev).requires_grad_(True) for _ in range(2))
            out = conv(x, x0, loops)
            assert conv.last_path == "fused"
            out.backward(randn(gen, n, c).to(dev))
            emit(name, out, x.grad, x0.grad, conv.weight1.grad)
        adj2 = ops.H2Adjacency(eid, n)
        for c in (6, 40):
            name = f"{gname} h2gcn C={c}"
            gen = gen_for(name)
            x = randn(gen, n, c).to(dev).requires_grad_(True)
            out = ops.h2gcn_conv(x, adj2)
            out.backward(randn(gen, n, 2 * c).to(dev))
            emit(name, out, x.grad)
        raw = glognn.raw_graph(eid, n)
        for c in (5, 40):
            name = f"{gname} glognn C={c}"
            gen = gen_for(name)
            x, h0 = (randn(gen, n, c).to(dev).requires_grad_(True) for _ in range(2))
            ow = ((0.6 + 0.8 * torch.rand(2, 1, generator=gen)) / 2).to(dev).requires_grad_(True)
            dw = ((0.6 + 0.8 * torch.rand(c, 1, generator=gen)) / c).to(dev).requires_grad_(True)
            out = ops.glognn_norm(x, h0, ow, dw, raw, *glognn_ref.SCALARS[1], 2, 2, 2)
            assert type(out.grad_fn).__name__.startswith("_GloGNNNorm")
            out.backward(randn(gen, n, c).to(dev))
            emit(name, out, x.grad, h0.grad, ow.grad, dw.grad)
        uniq = torch.unique(ei[:, ei[0] != ei[1]], dim=1)
        (li, lv), (hi, hv) = acm_ref.row_normalized_adjacency_np(uniq.numpy(), n)
        pair = acmgcn._AdjPair(acm_ref.coo(li, lv, n).to(dev), acm_ref.coo(hi, hv, n).to(dev))
        assert pair.uniform
        for c in (5, 40):
            for relu in (True, False):
                name = f"{gname} acm C={c} relu={int(relu)}"
                gen = gen_for(name)
                p = randn(gen, n, 3 * c)
                par = [t.to(dev).requires_grad_(True) for t in acm_ref.attention_parameters(c, "init", p, gen)]
                p = p.to(dev).requires_grad_(True)
                out, lh, datt = ops.acm_filterbank_fused(p, *par, pair.graph, relu)
                out.backward(randn(gen, n, c).to(dev))
                emit(name, out, lh, datt, p.grad, *[t.grad for t in par])
        c = 40
        for tag, e in (("", ei), (" sources>=3", ei[:, ei[0] >= 3])):
            name = f"{gname} adj_linear C={c}{tag}"
            gen = gen_for(name)
            sn = Graph(e.to(dev), n, True, True)
            assert sn.src_min > 0, "the shifted rows and the bias-only tail run"
            name += f" src_min={sn.src_min}"
            w = torch.nn.Parameter(randn(gen, c, n).t().contiguous().to(dev).t())
            b = randn(gen, c).to(dev).requires_grad_(True)
            out = ops.adj_linear(w, b, sn)
            out.backward(randn(gen, n, c).to(dev))
            emit(name, out, w.grad, b.grad)
        name = f"{gname} weighted gather C={c}"
        gen = gen_for(name)
        norm, aux = prop.prop_plain(loops)
        x = randn(gen, n, c).to(dev).requires_grad_(True)
        wq = randn(gen, norm.numel()).to(dev).requires_grad_(True)
        out = ops.weighted_propagate(x, wq, loops, aux)
        out.backward(randn(gen, n, c).to(dev))
        emit(name, out, x.grad, wq.grad)
        for heads, c in GAT_SHAPES:
            name = f"{gname} gat H={heads} C={c}"
            gen = gen_for(name)
            xp, g = randn(gen, n, heads * c).to(dev).requires_grad_(True), randn(gen, n, heads * c).to(dev)
            ws, wd = (randn(gen, 1, heads, c).to(dev).requires_grad_(True) for _ in range(2))
            out = ops.gat_propagate(xp, ws, wd, loops, heads)
            ml = saved(out, "_GATPropagate", 4)
            out.backward(g)
            emit(name, out, ml, xp.grad, ws.grad, wd.grad)
        # the typed graph of tests/test_wrgat_gpu.py: one explicit loop per node but the last seven (the build adds none)
        nl = torch.arange(n - 7, dtype=torch.int64)
        typed = torch.cat([ei, torch.stack([nl, nl])], dim=1).contiguous()
        ew = wrgat_ref.weights(typed.size(1), gen_for(f"{gname} wrgat weights"))
        for r, c in WRGAT_SHAPES:
            et = wrgat_ref.scattered(typed, r)
            for weighted in (True, False):
                adj = ops.TypedAdjacency(typed.to(dev), et.to(dev), ew.to(dev) if weighted else None, n, r)
                for root in (True, False):
                    for relu in (True, False):
                        name = f"{gname} wrgat R={r} C={c} w={int(weighted)} root={int(root)} relu={int(relu)}"
                        gen = gen_for(name)
                        p, atten = randn(gen, n, r * c), randn(gen, r, 2 * c) / math.sqrt(c)
                        extras = (randn(gen, n, c), randn(gen, c)) if root else (None, None)
                        ins = [None if t is None else t.to(dev).requires_grad_(True) for t in (p, atten) + extras]
                        out = ops.wrgat_conv(*ins, adj, relu)
                        ml = saved(out, "_WRGATConv", 3)
                        out.backward(randn(gen, n, c).to(dev))
                        emit(name, out, ml, *[None if t is None else t.grad for t in ins])
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()

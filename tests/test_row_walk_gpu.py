"""The seven gather-sum hop kernels on csrc/row_walk.h (gpr_propagate, gcn_conv, the GCN2 hop, h2gcn_conv, glognn_norm,
the ACM layer, the adjacency-linear forward) on a graph whose split rows have 18 tasks on either side
(gpr_ref.hub_graph): the finalize's four-chain loop over the tasks' partial rows (``t + 12 < t1``) first runs at 13
tasks, a degree above 1 536, which the 400-entry rows of the degree graph never reach.

One width per family (C = 40, Gaussian rows, the fused arm), each output per element against the family's float64
arbiter under the project's gate (tests/arbiter.py: |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG, exactly 0 where MAG
is 0, no exemptions), K_ref measured here from the reference's own fp32 op sequence on the same inputs.  The graph,
the arbiters and K_ref are computed on the CPU (``test_references_on_the_cpu`` builds them without a GPU)."""
import functools
import math

import pytest
import torch

from oracle import sngnn_oracle as O
from tests import acm_ref
from tests import arbiter as A
from tests import gcn2_ref, gcn_ref, glognn_ref, h2gcn_ref
from tests import gpr_ref as R
from tests import helpers

C = 40
MIN_TASKS = 13            # the fewest tasks at which sum_task_partials' unrolled loop runs


@functools.lru_cache(maxsize=None)
def _hub():
    return R.hub_graph()


@functools.lru_cache(maxsize=None)
def _hub_unique():
    """ACM's reading: unique, loop-free edges (row_normalized_adjacency adds the diagonal)."""
    ei, n = _hub()
    ei = ei[:, ei[0] != ei[1]]
    return torch.unique(ei, dim=1), n


def _k_ref(ref, arb, outputs):
    return {q: A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 restatement {q}")[0] for q in outputs}


def _rows(n, c, gen):
    return R.rows("gaussian", n, c, gen)


# ------------------------------------------------------------------ the cases: inputs, arbiter, K_ref (CPU, built once)

@functools.lru_cache(maxsize=None)
def _gpr_case():
    ei, n = _hub()
    gen = torch.Generator().manual_seed(11)
    x, g = _rows(n, C, gen), _rows(n, C, gen)
    gamma = torch.tensor(R.ppr(0.1, 2))
    arb = R.gpr_arbiter(ei, n, x, gamma.float().double(), g)
    x32, t = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    out = R.gpr_prop(x32, ei, t)
    out.backward(g)
    ref = dict(out=out.detach(), grad_x=x32.grad, grad_gamma=t.grad)
    return (x, gamma, g), arb, _k_ref(ref, arb, ("out", "grad_x", "grad_gamma"))


@functools.lru_cache(maxsize=None)
def _gcn_case():
    ei, n = _hub()
    gen = torch.Generator().manual_seed(12)
    xp, g, bias = _rows(n, C, gen), _rows(n, C, gen), torch.randn(C, generator=gen)
    arb = gcn_ref.gcn_conv_arbiter(ei, n, xp, bias, g)
    return (xp, bias, g), arb, _k_ref(gcn_ref.gcn_conv_torch(ei, n, xp, bias, g), arb, ("out", "grad_xp", "grad_bias"))


GCN2_SCALARS = (0.1, math.log(1.5))


@functools.lru_cache(maxsize=None)
def _gcn2_case():
    ei, n = _hub()
    gen = torch.Generator().manual_seed(13)
    x, x0, g = _rows(n, C, gen), _rows(n, C, gen), _rows(n, C, gen)
    w = torch.randn(C, C, generator=gen) / math.sqrt(C)
    arb = gcn2_ref.gcn2_arbiter(ei, n, x, x0, w, *GCN2_SCALARS, g)
    ref = gcn2_ref.gcn2_conv_torch(ei, n, x, x0, w, *GCN2_SCALARS, g)
    return (x, x0, w, g), arb, _k_ref(ref, arb, ("out", "grad_x", "grad_x0", "grad_weight1"))


@functools.lru_cache(maxsize=None)
def _h2gcn_case():
    ei, n = _hub()
    gen = torch.Generator().manual_seed(14)
    x, g = _rows(n, C, gen), _rows(n, 2 * C, gen)
    arb = h2gcn_ref.conv_arbiter(ei, n, x, g)
    return (x, g), arb, _k_ref(h2gcn_ref.conv_torch(ei, n, x, g), arb, ("out", "grad_x"))


GLO_SCALARS, GLO_ORDERS = glognn_ref.SCALARS[1], 2


@functools.lru_cache(maxsize=None)
def _glognn_case():
    """norm_func2 with order_func2: both parameter gradients exist."""
    ei, n = _hub()
    gen = torch.Generator().manual_seed(15)
    x, h0, g = _rows(n, C, gen), _rows(n, C, gen), torch.randn(n, C, generator=gen)
    ow = (0.6 + 0.8 * torch.rand(GLO_ORDERS, 1, generator=gen)) / GLO_ORDERS
    dw = (0.6 + 0.8 * torch.rand(C, 1, generator=gen)) / C * torch.where(torch.rand(C, 1, generator=gen) < 0.25, -1.0, 1.0)
    adj = glognn_ref.dense_adj(ei, n, torch.float32)
    arb = glognn_ref.arbiter(adj, x, h0, ow, dw, GLO_SCALARS, GLO_ORDERS, 2, 2, g)
    ref = glognn_ref.reference_run(x, h0, ow, dw, adj, GLO_SCALARS, GLO_ORDERS, 2, 2, g, torch.float32)
    outputs = ("out", "grad_x", "grad_h0", "grad_orders_weight", "grad_diag_weight")
    return (x, h0, ow, dw, g), arb, _k_ref(ref, arb, outputs)


@functools.lru_cache(maxsize=None)
def _acm_pair():
    ei, n = _hub_unique()
    (li, lv), (hi, hv) = acm_ref.row_normalized_adjacency_np(ei.numpy(), n)
    return acm_ref.coo(li, lv, n), acm_ref.coo(hi, hv, n)


@functools.lru_cache(maxsize=None)
def _acm_case():
    """acm_ref.case's steps on the hub graph's pair (relu on, the reference's init scale): the arbiter is evaluated on
    the relu masks of whoever it judges, so it is built per run (``_acm_arbiter``); K_ref on the fp32 sequence's own."""
    _, n = _hub_unique()
    low, high = _acm_pair()
    gen = torch.Generator().manual_seed(16)
    p, gout = _rows(n, 3 * C, gen), _rows(n, C, gen)
    par = acm_ref.attention_parameters(C, "init", p, gen)
    ref = acm_ref.run_layer_ops(p, low, high, *par, gout, True, torch.float32)
    arb64 = acm_ref.arbiter(p, low, high, *par, gout, None, True)
    k_pre = [A.reference_units(ref[q] if q != "M" else p[:, 2 * C:], arb64[q], arb64["MAG_" + q], "fp32 " + q)[0]
             for q in ("L", "H", "M")]
    arb = _acm_arbiter(p, par, gout, acm_ref.pre_masks(ref["L"], ref["H"], p[:, 2 * C:]))
    return (p, par, gout), (arb64, k_pre), _k_ref(ref, arb, acm_ref.QUANTITIES)


def _acm_arbiter(p, par, gout, masks):
    low, high = _acm_pair()
    return acm_ref.arbiter(p, low, high, *par, gout, masks, True)


@functools.lru_cache(maxsize=None)
def _adj_case():
    """out_0 = Linear(num_nodes, C)(adj) of models.py:124-130 on the SN edge list (loops replaced).  The arbiter is the
    expression in float64, once as written and once on |weight|, |bias| (the adjacency has no negative entry)."""
    ei, n = _hub()
    gen = torch.Generator().manual_seed(17)
    W, b = torch.randn(C, n, generator=gen), torch.randn(C, generator=gen)
    ei_p = O.sn_edge_list(ei, n, True, True)
    row, col = ei_p[0] - ei_p[0].min(), ei_p[1]

    def out64(w, bias):
        return bias[None, :] + torch.zeros(n, C, dtype=torch.float64).index_add_(0, row, w.t()[col])

    arb = dict(out=out64(W.double(), b.double()), MAG_out=out64(W.double().abs(), b.double().abs()))
    ref = dict(out=O.adj_linear_reference(W, b, ei_p, n))
    return (W, b), arb, _k_ref(ref, arb, ("out",))


CASES = dict(gpr=_gpr_case, gcn=_gcn_case, gcn2=_gcn2_case, h2gcn=_h2gcn_case, glognn=_glognn_case, acm=_acm_case,
             adj=_adj_case)


# ------------------------------------------------------------------ the CPU half

def test_hub_graph_reaches_the_unrolled_finalize_loop():
    """Both sides of every family's reading of the graph have a row of at least 13 tasks (18 as built); one isolated
    node, duplicates and original self loops are there."""
    ei, n = _hub()
    loops_replaced, _, _ = R.gcn_norm(ei, n)
    unique, _ = _hub_unique()
    with_diagonal = torch.cat([unique, torch.arange(n).repeat(2, 1)], dim=1)
    a1 = torch.from_numpy(h2gcn_ref.a1_entries(ei)[0]), torch.from_numpy(h2gcn_ref.a1_entries(ei)[1])
    for what, e in (("raw", ei), ("loops replaced", loops_replaced), ("unique + diagonal", with_diagonal),
                    ("loop-free", torch.stack(a1))):
        t_in, t_out = R.split_tasks(e, n)
        assert t_in >= MIN_TASKS and t_out >= MIN_TASKS, (what, t_in, t_out)
        assert (t_in, t_out) == (18, 18), (what, t_in, t_out)
    ind, outd = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert int(ind[0]) == R.HUB_DEGREE and int(outd[1]) == R.HUB_DEGREE
    assert int(((ind == 0) & (outd == 0)).sum()) >= 1 and int(ind[n - 1] + outd[n - 1]) == 0, "an isolated node"
    assert int((ei[0] == ei[1]).sum()) >= 4, "original self loops"
    assert torch.unique(ei, dim=1).size(1) < ei.size(1), "duplicate edges"


@pytest.mark.parametrize("family", sorted(CASES))
def test_references_on_the_cpu(family):
    """The arbiter and the fp32 op sequence of every case: K_ref is finite and the reference is exactly 0 wherever the
    magnitude is (reference_units asserts it) - the premise of holding the kernels to the gate."""
    _, _, k_ref = CASES[family]()
    for q, k in k_ref.items():
        assert math.isfinite(k), (family, q, k)


# ------------------------------------------------------------------ the GPU half

_DEV = {}


def _loops_graph(cuda):
    if "loops" not in _DEV:
        from sngnn_amd.graph import LOOPS_REPLACE, Graph
        ei, n = _hub()
        _DEV["loops"] = Graph(ei.to(cuda), n, True, LOOPS_REPLACE)
    return _DEV["loops"]


def _gate(family, got, arb, k_ref):
    failures, parts = [], []
    for q, k in k_ref.items():
        assert got[q].dtype in (torch.float32, torch.float64), q
        print(f"row walk {family} {q}: K_ref {k:.2f}", end="")
        try:
            u, _ = A.check(got[q], arb[q], arb["MAG_" + q], k, f"row walk {family} {q}")
            print(f", kernel {u:.2f}")
            parts.append(f"{q} K_ref {k:.2f} / kernel {u:.2f}")
        except AssertionError as ex:
            print(" FAILED")
            failures.append(str(ex))
    helpers.REPORT_LINES.append(f"row walk hub graph {family} C={C}: " + ", ".join(parts) +
                                " (worst element, units of 2^-24 x MAG)")
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_gpr_propagate_on_the_hub_graph(cuda, monkeypatch):
    from sngnn_amd import ops, prop
    monkeypatch.setattr(prop, "FUSE_GPR", True)
    (x, gamma, g), arb, k_ref = _gpr_case()
    xg, tg = x.to(cuda).requires_grad_(True), gamma.to(cuda).requires_grad_(True)
    out = ops.gpr_propagate(xg, tg, _loops_graph(cuda))
    out.backward(g.to(cuda))
    _gate("gpr_propagate", dict(out=out.detach(), grad_x=xg.grad, grad_gamma=tg.grad), arb, k_ref)


@pytest.mark.gpu
def test_gcn_conv_on_the_hub_graph(cuda, monkeypatch):
    from sngnn_amd import gcn, ops
    monkeypatch.setattr(gcn, "FUSE_GCN", True)
    (xp, bias, g), arb, k_ref = _gcn_case()
    xg, bg = xp.to(cuda).requires_grad_(True), bias.to(cuda).requires_grad_(True)
    out = ops.gcn_conv(xg, bg, _loops_graph(cuda))
    out.backward(g.to(cuda))
    _gate("gcn_conv", dict(out=out.detach(), grad_xp=xg.grad, grad_bias=bg.grad), arb, k_ref)


@pytest.mark.gpu
def test_gcn2_hop_on_the_hub_graph(cuda, monkeypatch):
    from sngnn_amd import gcn2, ops
    monkeypatch.setattr(gcn2, "FUSE_GCN2", True)
    (x, x0, w, g), arb, k_ref = _gcn2_case()
    xg, x0g, wg = (t.to(cuda).requires_grad_(True) for t in (x, x0, w))
    out = ops.gcn2_conv(xg, x0g, wg, _loops_graph(cuda), *GCN2_SCALARS)
    out.backward(g.to(cuda))
    _gate("gcn2_conv", dict(out=out.detach(), grad_x=xg.grad, grad_x0=x0g.grad, grad_weight1=wg.grad), arb, k_ref)


@pytest.mark.gpu
def test_h2gcn_conv_on_the_hub_graph(cuda, monkeypatch):
    from sngnn_amd import h2gcn, ops
    monkeypatch.setattr(h2gcn, "FUSE_H2GCN", True)
    ei, n = _hub()
    (x, g), arb, k_ref = _h2gcn_case()
    xg = x.to(cuda).requires_grad_(True)
    out = ops.h2gcn_conv(xg, ops.H2Adjacency(ei.to(cuda), n))
    out.backward(g.to(cuda))
    _gate("h2gcn_conv", dict(out=out.detach(), grad_x=xg.grad), arb, k_ref)


@pytest.mark.gpu
def test_glognn_norm_on_the_hub_graph(cuda, monkeypatch):
    from sngnn_amd import glognn, ops
    monkeypatch.setattr(glognn, "FUSE_GLOGNN", True)
    ei, n = _hub()
    tensors, arb, k_ref = _glognn_case()
    leaves = [t.to(cuda).requires_grad_(True) for t in tensors[:4]]
    out = ops.glognn_norm(*leaves, glognn.raw_graph(ei.to(cuda), n), *GLO_SCALARS, GLO_ORDERS, 2, 2)
    assert type(out.grad_fn).__name__.startswith("_GloGNNNorm"), "the fused arm"
    out.backward(tensors[4].to(cuda))
    got = dict(out=out.detach(), grad_x=leaves[0].grad, grad_h0=leaves[1].grad, grad_orders_weight=leaves[2].grad,
               grad_diag_weight=leaves[3].grad)
    _gate("glognn_norm", got, arb, k_ref)


@pytest.mark.gpu
def test_acm_layer_on_the_hub_graph(cuda):
    from sngnn_amd import acmgcn, ops
    (p, par, gout), (arb64, k_pre), k_ref = _acm_case()
    low, high = _acm_pair()
    pair = acmgcn._AdjPair(low.to(cuda), high.to(cuda))
    assert pair.uniform, "the hub graph's pair is the kernel's case"
    pg = p.to(cuda).requires_grad_(True)
    parg = [t.to(cuda).requires_grad_(True) for t in par]
    out, lh, _ = ops.acm_filterbank_fused(pg, *parg, pair.graph, True)
    out.backward(gout.to(cuda))
    masks = acm_ref.pre_masks(lh[:, :C], lh[:, C:], pg.detach()[:, 2 * C:])
    acm_ref.check_masks(masks, arb64, k_pre, "row walk acm")
    got = dict(out=out.detach(), grad_P=pg.grad, grad_a_low=parg[0].grad.reshape(-1), grad_a_high=parg[1].grad.reshape(-1),
               grad_a_mlp=parg[2].grad.reshape(-1), grad_att_vec=parg[3].grad)
    _gate("acm layer", got, _acm_arbiter(p, par, gout, tuple(m.cpu() for m in masks)), k_ref)


@pytest.mark.gpu
def test_adj_linear_forward_on_the_hub_graph(cuda):
    from sngnn_amd import ops
    from sngnn_amd.graph import Graph
    ei, n = _hub()
    (W, b), arb, k_ref = _adj_case()
    graph = Graph(ei.to(cuda), n, True, True)
    out = ops.adj_linear(W.t().contiguous().to(cuda).t(), b.to(cuda), graph)
    _gate("adj_linear forward", dict(out=out.detach()), arb, k_ref)

"""GPU: R replicas of one 1-layer model in one job (sngnn_amd/splits.py, replicas.hip) against the single
model's path - the union graph's aggregation and every new kernel bit for bit on each replica's slice, the
batch's log-probs and gradients against ``replica(r)``, and ``train_splits`` on the real Actor data with the
published hyper-parameters against ten sequential ``train.train_graphed`` runs."""
import os

import numpy as np
import pytest
import torch

import sngnn_amd
from sngnn_amd import _lib, ops
from sngnn_amd import splits as S
from sngnn_amd import train as T
from sngnn_amd.graph import Graph
from sngnn_amd.synth import Data

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _graph(n, e, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=gen)
    dst = torch.cat([torch.randint(0, n, (e - 40,), generator=gen), torch.full((40,), 3)])   # one long row
    return torch.stack([src, dst]).to(dev)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---------------------------------------------------------------------------------------------
# aggregation on the union graph
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["SNGNN", "SNGNN_Plus", "SNGNN_Plus_Plus"])
@pytest.mark.parametrize("rem", [0, 1])
@pytest.mark.parametrize("k,thr", [(1, 0.99), (16, 0.0)])
def test_union_aggregation_equals_the_single_graph(cuda, kind, rem, k, thr):
    if kind == "SNGNN" and (rem == 1 or k != 1):
        pytest.skip("SNGNN keeps its loops and selects nothing: one configuration")
    n, e, c, R = 300, 2400, 8, 3
    ei = _graph(n, e, 7, cuda)
    top_k, remove = (None, False) if kind == "SNGNN" else (k, bool(rem))
    gen = torch.Generator().manual_seed(11)
    hs = [torch.randn(n, c, generator=gen).to(cuda) for _ in range(R)]
    hs[1] = hs[0].clone()                     # identical h in two replicas, a different one in the third
    single = Graph(ei, n, True, remove)
    ug = S.union_graph(ei, n, R, True, remove)
    assert ug.num_nodes == R * n and ug.num_edges == R * single.num_edges
    hu = torch.cat(hs).requires_grad_(True)
    out_u, wsel_u = ops.aggregate_forward(ug, hu.detach(), top_k, thr, save_for_backward=True)[:2]
    gout = torch.randn(R * n, c, generator=gen).to(cuda)
    yu = ops.aggregate(hu, ug, top_k, thr)
    yu.backward(gout)
    ep = single.num_edges
    for r in range(R):
        h = hs[r].clone().requires_grad_(True)
        out_s, wsel_s = ops.aggregate_forward(single, h.detach(), top_k, thr, save_for_backward=True)[:2]
        assert torch.equal(out_u[r * n:(r + 1) * n], out_s), r
        assert torch.equal(wsel_u[r * ep:(r + 1) * ep], wsel_s), r         # kept weights (CSR order, block r)
        y = ops.aggregate(h, single, top_k, thr)
        assert torch.equal(yu[r * n:(r + 1) * n].detach(), y.detach()), r
        y.backward(gout[r * n:(r + 1) * n])
        assert torch.equal(hu.grad[r * n:(r + 1) * n], h.grad), r
    if kind == "SNGNN_Plus_Plus" and single.src_min == 0:
        wt = [torch.randn(n, c, generator=gen).to(cuda) for _ in range(R)]
        o_u = ops.adj_linear_forward(ug, torch.cat(wt), None)
        g0 = torch.randn(R * n, c, generator=gen).to(cuda)
        d_u = ops.adj_linear_backward(ug, g0)
        for r in range(R):
            assert torch.equal(o_u[r * n:(r + 1) * n], ops.adj_linear_forward(single, wt[r], None)), r
            assert torch.equal(d_u[r * n:(r + 1) * n], ops.adj_linear_backward(single, g0[r * n:(r + 1) * n])), r


# ---------------------------------------------------------------------------------------------
# the new kernels against the single-model entries on each replica's slice
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [5, 6, 8, 40, 64])
def test_unpack_equals_normalize_rows_filter(cuda, c):
    n, R = 1000, 4
    gen = torch.Generator().manual_seed(c)
    hs = torch.randn(n, R * c, generator=gen).to(cuda)
    hs[17, :] = 0.0                                              # a zero row: the clamped norm
    bias = torch.randn(R, c, generator=gen).to(cuda)
    unit = ops.UnitRows(want_filter=ops.filter_row_bytes(c) > 0)
    h = S.replica_unpack(hs, bias, R, unit)
    assert (unit.filt is not None) == (ops.filter_row_bytes(c) > 0)
    for r in range(R):
        want_h = hs[:, r * c:(r + 1) * c] + bias[r]
        assert torch.equal(h[r * n:(r + 1) * n], want_h), r
        nn_, nrm, filt = ops.normalize_rows_filter(want_h.contiguous())
        assert torch.equal(unit.n[r * n:(r + 1) * n], nn_), r
        assert torch.equal(unit.nrm[r * n:(r + 1) * n], nrm), r
        if filt is not None:
            assert torch.equal(unit.filt[r * n:(r + 1) * n], filt), r
    h2 = S.replica_unpack(hs, None, R, None)
    assert torch.equal(h2[n:2 * n], hs[:, c:2 * c])


@pytest.mark.parametrize("c", [5, 8, 40])
def test_replica_head_equals_head_nll(cuda, c):
    n, R = 3000, 5
    gen = torch.Generator().manual_seed(100 + c)
    z = torch.randn(R * n, c, generator=gen).to(cuda)
    y = torch.randint(0, c, (n,), generator=gen).to(cuda)
    r_ = torch.rand(R, n, generator=gen)
    tr, va, te = (r_ < 0.6), (r_ >= 0.6) & (r_ < 0.8), r_ >= 0.8
    sel_t = tr.to(torch.uint8).to(cuda)
    sel_e = (va.to(torch.uint8) | (te.to(torch.uint8) << 1)).to(cuda)
    cnt = torch.stack([tr.sum(1), va.sum(1), te.sum(1)], 1).clamp_min(1)
    metrics = torch.zeros(R, 6, device=cuda)
    g = S.replica_head(z, y, sel_t, cnt[:, 0].contiguous().to(cuda), metrics[:, 0:2], grad=True)
    S.replica_head(z, y, sel_e, cnt[:, 1:].contiguous().to(cuda), metrics[:, 2:6])
    for r in range(R):
        zr = z[r * n:(r + 1) * n].clone()
        (loss, corr), gr = ops.head_nll_with_grad(zr, y, sel_t[r].contiguous(), int(cnt[r, 0]))
        assert torch.equal(metrics[r, 0], loss) and torch.equal(metrics[r, 1], corr), r
        assert torch.equal(g[r * n:(r + 1) * n], gr), r
        m2 = ops.head_nll2(zr, y, sel_e[r].contiguous(), int(cnt[r, 1]), int(cnt[r, 2]))
        assert torch.equal(metrics[r, 2:6], m2), r
    # the blend with a per-replica beta in the head's pass
    z1 = torch.randn(R * n, c, generator=gen).to(cuda)
    beta = torch.rand(R, generator=gen).to(cuda)
    metrics.zero_()
    g = S.replica_head(z, y, sel_t, cnt[:, 0].contiguous().to(cuda), metrics[:, 0:2], logits1=z1, beta=beta, grad=True)
    S.replica_head(z, y, sel_e, cnt[:, 1:].contiguous().to(cuda), metrics[:, 2:6], logits1=z1, beta=beta)
    for r in range(R):
        o0, o1, b = z[r * n:(r + 1) * n].clone(), z1[r * n:(r + 1) * n].clone(), beta[r:r + 1].clone()
        m_t, m_e = torch.zeros(2, device=cuda), torch.zeros(4, device=cuda)
        if c % 4 == 0:
            head = ops.HeadEpilogue(y, sel_t[r].contiguous(), m_t, int(cnt[r, 0]), grad=True)
            gr = ops.blend_head(o0, o1, b, head)
            ops.blend_head(o0, o1, b, ops.HeadEpilogue(y, sel_e[r].contiguous(), m_e, int(cnt[r, 1]), int(cnt[r, 2])))
        else:
            zb = ops.blend(o0, o1, b)
            (_, _), gr = ops.head_nll_with_grad(zb, y, sel_t[r].contiguous(), int(cnt[r, 0]), out=m_t)
            ops.head_nll2(zb, y, sel_e[r].contiguous(), int(cnt[r, 1]), int(cnt[r, 2]), out=m_e)
        assert torch.equal(metrics[r, 0:2], m_t), (r, metrics[r], m_t)
        assert torch.equal(metrics[r, 2:6], m_e), (r, metrics[r], m_e)
        assert torch.equal(g[r * n:(r + 1) * n], gr.detach()), r


@pytest.mark.parametrize("n,c", [(7600, 5), (2277, 8), (1000, 3)])
def test_replica_blend_equals_the_single_blend(cuda, n, c):
    R = 4
    gen = torch.Generator().manual_seed(n)
    o0, o1, g = (torch.randn(R * n, c, generator=gen).to(cuda) for _ in range(3))
    beta = torch.rand(R, generator=gen).to(cuda)
    out = S.replica_blend_forward(o0, o1, beta)
    g0, g1, gb = S.replica_blend_backward(g, o0, o1, beta)
    lib = _lib.load()
    ws = torch.empty(int(lib.sngnn_blend_workspace_bytes()), dtype=torch.uint8, device=cuda)
    for r in range(R):
        a, b_, gr = (t[r * n:(r + 1) * n].clone() for t in (o0, o1, g))
        br = beta[r:r + 1].clone()
        o = torch.empty_like(a)
        _lib.check(lib.sngnn_blend_forward(a.data_ptr(), b_.data_ptr(), br.data_ptr(), a.numel(), o.data_ptr(),
                                           _stream(cuda)), "blend_forward")
        s0, s1, sb = torch.empty_like(a), torch.empty_like(a), torch.empty(1, device=cuda)
        _lib.check(lib.sngnn_blend_backward(gr.data_ptr(), a.data_ptr(), b_.data_ptr(), br.data_ptr(), a.numel(),
                                            s0.data_ptr(), s1.data_ptr(), sb.data_ptr(), ws.data_ptr(), _stream(cuda)),
                   "blend_backward")
        assert torch.equal(out[r * n:(r + 1) * n], o), r
        assert torch.equal(g0[r * n:(r + 1) * n], s0) and torch.equal(g1[r * n:(r + 1) * n], s1), r
        if (n * c) % 4 == 0:
            assert torch.equal(gb[r:r + 1], sb), (r, gb[r].item(), sb.item())
        else:          # (slices not 16-byte aligned: the single call's vector loads differ; documented)
            assert abs(gb[r].item() - sb.item()) <= 1e-5 * max(1.0, abs(sb.item())), r


def _single_wgrad(g, x):
    lib = _lib.load()
    n, f = x.shape
    c = g.size(1)
    gw, gb = torch.empty(c, f, device=g.device), torch.empty(c, device=g.device)
    ws = torch.empty(int(lib.sngnn_linear_wgrad_workspace_bytes(n, c, f)), dtype=torch.uint8, device=g.device)
    _lib.check(lib.sngnn_linear_wgrad(g.data_ptr(), x.data_ptr(), n, c, f, gw.data_ptr(), gb.data_ptr(), ws.data_ptr(),
                                      _stream(g.device)), "wgrad")
    return gw, gb


@pytest.mark.parametrize("n,f,c,R", [(7600, 932, 5, 10), (2277, 2325, 5, 3), (700, 300, 40, 2), (5000, 64, 8, 3)])
def test_replica_wgrad_equals_linear_wgrad(cuda, n, f, c, R):
    gen = torch.Generator().manual_seed(f)
    x = torch.randn(n, f, generator=gen).to(cuda)
    g = torch.randn(R * n, c, generator=gen).to(cuda)
    gw, gb = S.replica_wgrad(g, x, R)
    mfma = f in (16, 32, 64, 128) and n >= 1024          # sngnn_linear_wgrad's matrix-core path
    for r in range(R):
        sw, sb = _single_wgrad(g[r * n:(r + 1) * n].clone(), x)
        if not mfma:
            assert torch.equal(gw[r * c:(r + 1) * c], sw), r
            assert torch.equal(gb[r * c:(r + 1) * c], sb), r
        else:
            # the single call's MFMA path sums in another order: the replica kernel keeps the FMA path's
            dw = (gw[r * c:(r + 1) * c] - sw).abs().max().item() / sw.abs().max().item()
            db = (gb[r * c:(r + 1) * c] - sb).abs().max().item() / sb.abs().max().item()
            print(f"wgrad N={n} F={f} C={c} replica {r}: MFMA single path differs by {dw:.3e} (weight) "
                  f"{db:.3e} (bias) of the max-norm")
            assert dw <= 1e-5 and db <= 1e-5


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
def _models(kind, R, f, c, n, dev, k=1, thr=0.99, rem=0, betas=None):
    ms = []
    for r in range(R):
        torch.manual_seed(1234 + r)
        if kind == "SNGNN":
            m = sngnn_amd.SNGNN(f, 16, c, 1)
            with torch.no_grad():
                m.lins[0].bias.uniform_(-0.3, 0.3)
        elif kind == "SNGNN_Plus":
            m = sngnn_amd.SNGNN_Plus(f, 16, c, n, 1, k, thr, rem, 0.0)
        else:
            m = sngnn_amd.SNGNN_Plus_Plus(f, 16, c, n, 1, k, thr, betas[r] if betas else 0.5, rem, 0.0)
        ms.append(m.to(dev))
    return ms


@pytest.mark.parametrize("kind,c,k,thr,rem", [("SNGNN", 5, 1, 0.0, 0), ("SNGNN_Plus", 5, 1, 0.99, 0),
                                               ("SNGNN_Plus", 20, 16, 0.0, 1), ("SNGNN_Plus_Plus", 5, 1, 0.99, 0),
                                               ("SNGNN_Plus_Plus", 8, 16, 0.0, 1)])
def test_batch_logprobs_and_gradients_equal_each_replica(cuda, kind, c, k, thr, rem):
    d = sngnn_amd.synth.make_dataset("chameleon", scale=0.2, seed=5)
    n, f, R = d.x.size(0), d.x.size(1), 3
    data = Data(x=d.x.to(cuda), edge_index=d.edge_index.to(cuda), y=(d.y % c).to(cuda))
    ms = _models(kind, R, f, c, n, cuda, k, thr, rem, betas=[0.0, 0.3, 1.0])
    batch = S.ReplicaBatch.from_models(ms)
    gen = torch.Generator().manual_seed(9)
    masks = (torch.rand(R, n, generator=gen) < 0.6).to(cuda)
    lp = batch(data)
    loss = sum(torch.nn.functional.nll_loss(lp[r * n:(r + 1) * n][masks[r]], data.y[masks[r]]) for r in range(R))
    loss.backward()
    worst_lp = worst_g = 0.0
    for r in range(R):
        m = batch.replica(r)
        want = m(data)
        got = lp[r * n:(r + 1) * n].detach()
        assert torch.allclose(got, want.detach(), rtol=1e-4, atol=2e-5), r
        worst_lp = max(worst_lp, (got - want.detach()).abs().max().item())
        torch.nn.functional.nll_loss(want[masks[r]], data.y[masks[r]]).backward()
        blocks = batch._blocks(r)
        for name, p in m.named_parameters():
            gb_ = blocks[name]
            grad_b = {"lins.0.lin.weight": batch.lin_weight.grad[r * batch.Cp:r * batch.Cp + c],
                      "lins.0.lin.bias": batch.lin_bias.grad[r * batch.Cp:r * batch.Cp + c]}.get(name)
            if grad_b is None:
                full = {"lins.0.bias": lambda: batch.bias.grad[r], "lins.0.w.bias": lambda: batch.w_bias.grad[r],
                        "lins.0.w.weight": lambda: batch.w_weight.grad[:, r * n:(r + 1) * n],
                        "lins.0.beta": lambda: batch.beta.grad[r:r + 1]}[name]
                grad_b = full()
            assert gb_.shape == p.shape
            scale = max(p.grad.abs().max().item(), 1e-30)
            err = (grad_b.reshape(p.shape) - p.grad).abs().max().item()
            worst_g = max(worst_g, err / scale)
            assert err <= 2e-5 * scale, (r, name, err, scale)
    print(f"{kind} C={c} top_k={k} thr={thr}: max |d log-prob| {worst_lp:.3e}, max grad error / max-norm {worst_g:.3e}")


# ---------------------------------------------------------------------------------------------
# end to end on the real Actor data
# ---------------------------------------------------------------------------------------------
def _actor(dev):
    topo, feat = np.load(os.path.join(GOLDEN, "actor_topology.npz")), np.load(os.path.join(GOLDEN, "actor_features.npz"))
    n, f = (int(v) for v in feat["shape"])
    x = torch.zeros(n, f)
    x[torch.from_numpy(feat["row"].astype(np.int64)), torch.from_numpy(feat["col"].astype(np.int64))] = \
        torch.from_numpy(feat["val"])
    masks = {k: [] for k in ("train_mask", "val_mask", "test_mask")}
    for i in range(10):
        z = np.load(os.path.join(GOLDEN, "actor_raw", f"film_split_0.6_0.2_{i}.npz"))
        for k in masks:
            masks[k].append(torch.from_numpy(z[k].astype(bool)))
    stacked = [torch.stack(masks[k]).to(dev) for k in ("train_mask", "val_mask", "test_mask")]
    assert np.array_equal(stacked[0][0].cpu().numpy(), topo["train_mask0"].astype(bool))   # the same node order
    data = Data(x=x.to(dev), edge_index=torch.from_numpy(topo["edge_index"].astype(np.int64)).to(dev),
                y=torch.from_numpy(topo["y"].astype(np.int64)).to(dev))
    return data, stacked


def _published(kind, f, n, beta):
    torch.manual_seed(1234)                         # the sweep's seed: every run starts from the same init
    if kind == "SNGNN_Plus":
        return sngnn_amd.SNGNN_Plus(f, 64, 5, n, 1, 1, 0.99, 0, 0.0)
    return sngnn_amd.SNGNN_Plus_Plus(f, 64, 5, n, 1, 1, 0.99, beta, 0, 0.0)


@pytest.mark.parametrize("kind", ["SNGNN_Plus", "SNGNN_Plus_Plus"])
def test_train_splits_on_real_actor_matches_sequential_runs(cuda, kind):
    data, (tr, va, te) = _actor(cuda)
    n, f = data.x.shape
    epochs = 20
    if kind == "SNGNN_Plus":
        masks, betas = (tr, va, te), [None] * 10
    else:
        masks, betas = S.repeat_for_betas([tr[:2], va[:2], te[:2]], [0.0, 0.3, 0.5, 0.8, 1.0])
    R = masks[0].size(0)
    assert R == 10
    ms = [_published(kind, f, n, b).to(cuda) for b in betas]
    batch = S.ReplicaBatch.from_models(ms)
    opt = torch.optim.Adam(batch.parameters(), lr=0.1, weight_decay=5e-4)
    res = S.train_splits(batch, data, masks, opt, epochs=epochs, patience=300)
    assert res["epochs_run"] == epochs
    worst_loss = worst_acc = 0.0
    for r in range(R):
        single = _published(kind, f, n, betas[r]).to(cuda)
        d = Data(x=data.x, edge_index=data.edge_index, y=data.y, train_mask=masks[0][r], val_mask=masks[1][r],
                 test_mask=masks[2][r])
        o = torch.optim.Adam(single.parameters(), lr=0.1, weight_decay=5e-4)
        ref = T.train_graphed(single, d, o, epochs=epochs, patience=300)
        got = res["results"][r]["history"]
        assert len(got) == len(ref["history"]) == epochs
        g = np.array([[h["train_loss"], h["val_loss"], h["test_loss"], h["train_acc"], h["val_acc"], h["test_acc"]]
                      for h in got])
        w = np.array([[h["train_loss"], h["val_loss"], h["test_loss"], h["train_acc"], h["val_acc"], h["test_acc"]]
                      for h in ref["history"]])
        assert np.allclose(g[:, :3], w[:, :3], rtol=1e-4, atol=1e-5), (r, g[:, :3], w[:, :3])
        rows = [int(masks[0][r].sum()), int(masks[1][r].sum()), int(masks[2][r].sum())]
        for j in range(3):
            assert np.abs(g[:, 3 + j] - w[:, 3 + j]).max() <= 3.0 / rows[j] + 1e-12, (r, j)
        worst_loss = max(worst_loss, float(np.abs(g[:, :3] - w[:, :3]).max()))
        worst_acc = max(worst_acc, float((np.abs(g[:, 3:] - w[:, 3:]) * np.array(rows)).max()))
    m, s = S.mean_std([r_["final_test_acc"] for r_ in res["results"]])
    print(f"{kind} R={R}: max |d loss| {worst_loss:.3e}, max accuracy difference {worst_acc:.0f} rows; "
          f"final test accuracy {m:.2f}±{s:.2f} after {epochs} epochs")

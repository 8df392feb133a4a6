#!/usr/bin/env python3
"""Fixtures of the ACMGCN model (models/models.py:1742-1893), made by running the REFERENCE classes themselves.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names; nothing of the reference travels: the
outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_acm_model.py            # check + write tests/golden/acm_model_*.npz, acm_adj_*.npz
    python tests/golden/pin_acm_model.py --check    # check only

GraphConvolution2 and ACMGCN are core torch, so under pin_reference.py's stubs every line of the model runs verbatim
on the CPU, forward and backward.  Both adjacencies come from the reference's own utils/data_transform.py
(``row_normalized_adjacency``, ``get_adj_high``, ``sparse_mx_to_torch_sparse_tensor``) with the real scipy and
scikit-learn; train.py:290's ``to_scipy_sparse_matrix`` is PyG's and is restated here as
``scipy.sparse.coo_matrix((ones, edge_index))``, whose conversion adds duplicate edges up as PyG's does.  If
data_transform.py does not import, the l1 normalisation is restated in numpy (tests/acm_ref.py) and the note says so.

The reference never initialises ``low_param`` / ``high_param`` / ``mlp_param`` (``torch.FloatTensor(1, 1)``) and never
reads them; they are zeroed here so that a fixture does not hold whatever the allocator returned.

A model file holds: ``edge_index``, both adjacencies as COO arrays (``low_indices`` / ``low_values``, ``high_*``), ``x``,
the labels ``y``, every entry of the ``state_dict`` (``param.<key>``, their order in ``keys``), the log-probabilities
``out`` in training mode with dropout 0, every parameter's gradient of ``F.nll_loss(out, y)`` (``grad.<key>``),
``hyper`` = (nfeat, nhid, nclass), ``model_type`` and a ``note``.  An ``acm_adj_*`` file holds an ``edge_index``, ``n`` and
the pair.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from pin_ggcn_model import import_reference_data_transform, quiet  # noqa: E402
from pin_reference import REFERENCE, ROOT, import_reference_models  # noqa: E402

sys.path.insert(0, ROOT)
from tests import acm_ref as M  # noqa: E402

# name -> (model_type, n, edges, nfeat, nhid, nclass, seed, dirty edge list)
CASES = {
    "acm_model_a": ("acmgcn", 300, 1200, 24, 16, 5, 61, False),
    "acm_model_b": ("acmsgc", 300, 1200, 24, 16, 5, 62, False),
    "acm_model_c": ("acmgcn", 300, 1200, 24, 16, 5, 63, True),
}


def edges(n, e, seed, dirty):
    """A directed edge list without duplicates and self loops whose last two nodes have no out-edge and whose node 0 has
    150; ``dirty``: with 40 duplicate edges (7 of them tripled) and 5 self loops on top."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n - 2, (e,), generator=gen)
    dst = torch.randint(0, n, (e,), generator=gen)
    hub = torch.randperm(n - 1, generator=gen)[:150] + 1
    ei = torch.cat([torch.stack([src, dst]), torch.stack([torch.zeros_like(hub), hub])], dim=1)
    ei = torch.unique(ei[:, ei[0] != ei[1]], dim=1)
    if dirty:
        ei = torch.cat([ei, ei[:, :40], ei[:, :7], torch.arange(5).repeat(2, 1)], dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous()


def adjacency_pair(T, ei, n):
    """((idx, val), (idx, val)) of adj_low and adj_high as train.py:289-294 builds them, coalesced; and a note."""
    mine = M.row_normalized_adjacency_np(ei.numpy(), n)
    if T is None:
        return mine, "adjacencies restated in numpy (tests/acm_ref.py): utils/data_transform.py does not import"
    import scipy.sparse as sp
    a = sp.coo_matrix((np.ones(ei.size(1), np.float32), (ei[0].numpy(), ei[1].numpy())), (n, n))
    with quiet():
        low = T.row_normalized_adjacency(a)
        high = T.get_adj_high(low)
        low, high = T.sparse_mx_to_torch_sparse_tensor(low).coalesce(), T.sparse_mx_to_torch_sparse_tensor(high).coalesce()
    pair = tuple((t.indices().numpy(), t.values().numpy()) for t in (low, high))
    for (ia, va), (ib, vb), what in zip(pair, mine, ("adj_low", "adj_high")):
        assert np.array_equal(ia, ib), what + ": the numpy restatement has other entries"
        d = float(np.abs(va.astype(np.float64) - vb).max())
        print(f"  {what}: {va.size} entries, numpy restatement {'bit for bit' if d == 0 else f'within {d:.1e}'}")
        assert d <= 2.0 ** -24, (what, d)
    return pair, ("adjacencies made by the reference's own row_normalized_adjacency / get_adj_high / "
                  "sparse_mx_to_torch_sparse_tensor (utils/data_transform.py:68-80, 11-18) with scipy and scikit-learn")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    R = import_reference_models()
    T = import_reference_data_transform()
    for name, (mt, n, e, nfeat, nhid, nclass, seed, dirty) in CASES.items():
        ei = edges(n, e, seed, dirty)
        ((li, lv), (hi, hv)), note = adjacency_pair(T, ei, n)
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(n, nfeat, generator=gen)
        y = torch.randint(0, nclass, (n,), generator=gen)
        torch.manual_seed(seed)
        with quiet():
            ref = R.ACMGCN(nfeat, nhid, nclass, 0.0, mt)
        with torch.no_grad():
            for k, p in ref.named_parameters():
                if k.endswith("_param"):
                    p.zero_()
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train()
        adj_low, adj_high = M.coo(li, lv, n), M.coo(hi, hv, n)
        out = ref(types.SimpleNamespace(x=x), {"adj_low": adj_low, "adj_high": adj_high})
        F.nll_loss(out, y).backward()
        grads = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        z = dict(edge_index=ei.numpy(), low_indices=li, low_values=lv, high_indices=hi, high_values=hv, x=x.numpy(),
                 y=y.numpy(), out=out.detach().numpy(), hyper=np.array([nfeat, nhid, nclass], np.int64),
                 model_type=np.array(mt), keys=np.array(list(state)), note=np.array(note),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()})
        # the restatement the tests use reproduces the run
        fx = M.Fixture(z)
        res = M.run(fx, torch.float32)
        worst = float((res["out"] - out.detach()).abs().max()) / float(out.detach().abs().max())
        for k, g in grads.items():
            worst = max(worst, float((res["grads"][k] - g).abs().max()) / max(float(g.abs().max()), 1e-30))
        print(f"  {name}: reference ACMGCN({mt}) == restatement within {worst:.1e} x max-norm over log-probabilities and "
              f"{len(grads)} gradients (n = {n}, nnz = {lv.size} / {hv.size}, {len(state)} state entries)")
        assert worst <= 2e-6, worst
        if not args.check:
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **z)
            adj = os.path.join(HERE, name.replace("model", "adj") + ".npz")
            np.savez_compressed(adj, edge_index=ei.numpy(), n=np.array(n), low_indices=li, low_values=lv,
                                high_indices=hi, high_values=hv, note=np.array(note))
            for f in (path, adj):
                assert os.path.getsize(f) < 200 * 1024, f
                print(f"    wrote {os.path.relpath(f, ROOT)} ({os.path.getsize(f)} bytes)")


if __name__ == "__main__":
    main()

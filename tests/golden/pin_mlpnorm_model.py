#!/usr/bin/env python3
"""Fixtures of the MLPNORM model (GloGNN, models/models.py:1307-1450), made by running the REFERENCE class itself.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names; nothing of the reference travels: the
outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_mlpnorm_model.py            # check + write tests/golden/mlpnorm_model_*.npz
    python tests/golden/pin_mlpnorm_model.py --check    # check only

``MLPNORM.__init__``, ``reset_parameters`` and ``forward`` run verbatim on the CPU under pin_reference.py's stubs: the
class touches torch names only, so nothing is restated.  The adjacency is ``to_dense_adj(edge_index)`` as train.py:284
makes it - ``[1, N, N]``, entry (i, j) the number of edges i -> j - written out here with ``index_put_`` (PyG is absent).
``reset_parameters()`` is called (the reference's ``__init__`` leaves the two float64 matrices uninitialised),
``orders_weight`` and ``diag_weight`` are perturbed away from their constants, dropout is 0.

The three cases:
  a  train.py:350's configuration (alpha 0, beta 1, gamma 0.5, delta 0.5, norm_func1, 2 norm layers, 2 orders,
     order_func2) at nhid = 32
  b  norm_func1, order_func1, alpha 0.3, 3 orders, 3 norm layers; beta 0.02 and gamma 0.6 keep it well conditioned
     (at beta 1 the hub's A^3 terms put the reference's own fp32 log-probabilities 17.6 off their float64 values:
     a gate of 4 x that holds nothing)
  c  norm_func2 with the 2-D adjacency ``adj_dense[0]`` (with the 3-D one its missing squeeze makes ``mm`` raise at the
     second norm layer), 2 norm layers, order_func2

A file holds: ``edge_index``, ``x``, the labels ``y``, every entry of the ``state_dict`` before the run (``param.<key>``,
their order in ``keys``), the log-probabilities ``out`` in training mode, every parameter's gradient of
``F.nll_loss(out, y)`` (``grad.<key>``), ``hyper`` = the constructor's arguments in order (without the device) and the
``note``.
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
from pin_acm_model import edges  # noqa: E402
from pin_reference import REFERENCE, ROOT, import_reference_models  # noqa: E402

NOTE = ("out and grads by the reference's own MLPNORM class (models/models.py:1307-1450) on the CPU after "
        "reset_parameters(), orders_weight and diag_weight perturbed, dropout 0; adjacency = to_dense_adj(edge_index) "
        "written out with index_put_ ({dims}-D)")

# name -> (n, edges, nfeat, nhid, nclass, alpha, beta, gamma, delta, norm_func_id, norm_layers, orders, orders_func_id,
#          seed, adjacency dims)
CASES = {
    "mlpnorm_model_a": (300, 1200, 24, 32, 5, 0, 1, 0.5, 0.5, 1, 2, 2, 2, 81, 3),
    "mlpnorm_model_b": (300, 1200, 24, 32, 7, 0.3, 0.02, 0.6, 0.6, 1, 3, 3, 1, 82, 3),
    "mlpnorm_model_c": (300, 1200, 24, 32, 5, 0.0, 0.9, 0.4, 0.5, 2, 2, 2, 2, 83, 2),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    R = import_reference_models()
    for name, (n, e, fin, hid, ncls, alpha, beta, gamma, delta, nfid, layers, orders, ofid, seed, dims) in CASES.items():
        ei = edges(n, e, seed, True)
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(n, fin, generator=gen)
        y = torch.randint(0, ncls, (n,), generator=gen)
        torch.manual_seed(seed)
        ref = R.MLPNORM(n, fin, hid, ncls, 0.0, alpha, beta, gamma, delta, nfid, layers, orders, ofid, "cpu")
        ref.reset_parameters()
        with torch.no_grad():
            ref.orders_weight.mul_(0.6 + 0.8 * torch.rand(orders, 1, generator=gen))
            ref.diag_weight.mul_(0.6 + 0.8 * torch.rand(ncls, 1, generator=gen))
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        adj = torch.zeros(n, n).index_put_((ei[0], ei[1]), torch.ones(ei.size(1)), accumulate=True)
        ref.train()
        out = ref(types.SimpleNamespace(x=x, num_nodes=n, edge_index=ei), {"adj_dense": adj[None] if dims == 3 else adj})
        assert out.shape == (n, ncls), out.shape
        F.nll_loss(out, y).backward()
        grads = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert all(float(g.abs().max()) > 0 for g in grads.values()), "a zero gradient compares nothing"
        want = {"fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias", "fc4.weight", "fc4.bias"}
        want |= {"orders_weight"} if ofid == 2 else set()
        want |= {"diag_weight"} if nfid == 2 else set()
        assert set(grads) == want, sorted(grads)
        z = dict(edge_index=ei.numpy(), x=x.numpy(), y=y.numpy(), out=out.detach().numpy(),
                 hyper=np.array([n, fin, hid, ncls, 0.0, alpha, beta, gamma, delta, nfid, layers, orders, ofid], np.float64),
                 keys=np.array(list(state)), note=np.array(NOTE.format(dims=dims)),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()})
        print(f"  {name}: reference MLPNORM ran (n = {n}, {ei.size(1)} edges, {layers} norm layers, {orders} orders, "
              f"norm_func{nfid}, order_func{ofid}, {len(state)} state entries, {len(grads)} gradients); "
              f"max |log-prob| {float(out.detach().abs().max()):.3f}")
        if not args.check:
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **z)
            assert os.path.getsize(path) < 200 * 1024, path
            print(f"    wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Fixtures of the WRGAT model (models/models.py:1896-2041), made by running the REFERENCE class itself.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names; nothing of the reference travels: the
outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_wrgat_model.py            # check + write tests/golden/wrgat_model_{a,b,c}.npz
    python tests/golden/pin_wrgat_model.py --check    # check only (against the committed files too)

``WeightedRGATConv.__init__`` / ``forward`` / ``message``, ``masked_edge_index`` and ``WRGAT`` run verbatim on the CPU
under pin_reference.py's stubs.  Two PyG names they touch are absent here and are RESTATED (tests/wrgat_ref.py), put in
place of the stubs: ``MessagePassing.propagate`` called with ``size=(N, N)`` (gathers by the message's argument names,
aggr='mean' as sum / max(count, 1)) and ``inits.glorot``; ``utils.softmax`` is pin_reference.py's own stand-in (the
oracle's segment_softmax).  The fixture's ``note`` says so.

Cases: R = 1, 3 and 5; with and without ``root``; ``edge_weight`` given and None; in (c) relation 4 carries no edge; drop 0.
About 300 nodes, duplicates, self loops, an in-degree hub beyond 128 and nodes without in-edges.

A file holds: ``edge_index``, ``edge_color``, ``edge_weight`` (where given), ``x``, the labels ``y``, every entry of the
``state_dict`` before the run (``param.<key>``, their order in ``keys``), the log-probabilities ``out`` in training mode,
every parameter's gradient of ``F.nll_loss(out, y)`` (``grad.<key>``), ``hyper`` = (features, classes, relations, dims,
drop, root, weighted) and the ``note``.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from pin_reference import REFERENCE, ROOT  # noqa: E402

sys.path.insert(0, ROOT)
from tests import wrgat_ref as W  # noqa: E402

NOTE = ("out and grads by the reference's own WRGAT / WeightedRGATConv classes (models/models.py:1896-2041) on the CPU; "
        "MessagePassing.propagate with size=(N, N) and aggr='mean', and inits.glorot, are absent here and restated "
        "(tests/wrgat_ref.py: propagate_sized, glorot); utils.softmax is tests/golden/pin_reference.py's stand-in")

# name -> (n, edges, features, classes, relations, empty last relation, dims, root, weighted, seed)
CASES = {
    "wrgat_model_a": (300, 1500, 24, 5, 1, False, 16, True, True, 101),
    "wrgat_model_b": (300, 1500, 24, 5, 3, False, 12, False, False, 102),
    "wrgat_model_c": (310, 1600, 20, 4, 5, True, 8, True, True, 103),
}


def typed_edges(n, e, r, empty_last, weighted, seed):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.stack([torch.randint(0, n - 2, (e,), generator=gen), torch.randint(4, n, (e,), generator=gen)])
    hub = torch.randperm(n - 2, generator=gen)[:170]
    ei = torch.cat([ei, torch.stack([hub, torch.full_like(hub, 5)]), ei[:, :40], ei[:, :7],
                    torch.arange(6, 16).repeat(2, 1)], dim=1)
    ei = ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous()
    et = torch.randint(0, r - 1 if empty_last else r, (ei.size(1),), generator=gen)
    ew = W.weights(ei.size(1), gen) if weighted else None
    return ei, et, ew


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    _, WRGAT = W.reference_classes(HERE)
    for name, (n, e, fin, cls, r, empty_last, dims, root, weighted, seed) in CASES.items():
        ei, et, ew = typed_edges(n, e, r, empty_last, weighted, seed)
        indeg = torch.bincount(ei[1], minlength=n)
        assert int(indeg.max()) > 128 and int((indeg == 0).sum()) >= 1
        assert not empty_last or int((et == r - 1).sum()) == 0
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(n, fin, generator=gen)
        y = torch.randint(0, cls, (n,), generator=gen)
        torch.manual_seed(seed)
        ref = WRGAT(fin, cls, r, dims=dims, drop=0, root=root)
        with torch.no_grad():           # a bias that is not the initial zero
            ref.conv1.bias.copy_(0.2 * torch.randn(dims, generator=gen))
            ref.conv2.bias.copy_(0.2 * torch.randn(cls, generator=gen))
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train()
        out = ref(x, ei, ew, et)
        F.nll_loss(out, y).backward()
        grads = {k: p.grad for k, p in ref.named_parameters()}
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
        for k, g in grads.items():      # a zero gradient compares nothing (the empty relation's slices are exactly 0)
            live = g[:r - 1] if empty_last and k.endswith(("weight", "atten")) else g
            assert float(live.abs().max()) > 0, k
            if empty_last and k.endswith(("weight", "atten")):
                assert float(g[r - 1].abs().max()) == 0.0, k
        z = dict(edge_index=ei.numpy(), edge_color=et.numpy(), x=x.numpy(), y=y.numpy(), out=out.detach().numpy(),
                 hyper=np.array([fin, cls, r, dims, 0.0, float(root), float(weighted)], np.float64),
                 keys=np.array(list(state)), note=np.array(NOTE),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()})
        if weighted:
            z["edge_weight"] = ew.numpy()
        # the restatement (tests/wrgat_ref.py) reproduces the reference on the fixture
        mine = W.WRGATRef(fin, cls, r, dims=dims, root=root)
        mine.load_state_dict(state)
        res = mine(x, ei, ew, et)
        mg = torch.autograd.grad(F.nll_loss(res, y), list(mine.parameters()))
        worst = float((res - out).detach().abs().max()) / float(out.detach().abs().max())
        for (k, _), g in zip(mine.named_parameters(), mg):
            worst = max(worst, float((g - grads[k]).abs().max()) / float(grads[k].abs().max()))
        print(f"  {name}: reference WRGAT == restatement within {worst:.1e} x max-norm over log-probabilities and "
              f"{len(grads)} gradients (n = {n}, {ei.size(1)} edges, R = {r}, max in-degree {int(indeg.max())})")
        assert worst <= 5e-6, worst
        path = os.path.join(HERE, name + ".npz")
        if args.check:
            if os.path.exists(path):
                with np.load(path) as old:
                    assert sorted(old.files) == sorted(z), name
                    for k in z:
                        if z[k].dtype.kind in "fc":
                            assert np.allclose(old[k], z[k], rtol=1e-5, atol=1e-7), (name, k)
                        else:
                            assert np.array_equal(old[k], z[k]), (name, k)
                print(f"    {os.path.relpath(path, ROOT)} holds this run")
        else:
            np.savez_compressed(path, **z)
            assert os.path.getsize(path) < 200 * 1024, path
            print(f"    wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Fixtures of the GCNII model (models/models.py:1247-1303), made by running the REFERENCE class itself.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names; nothing of the reference travels: the
outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_gcnii_model.py            # check + write tests/golden/gcnii_model_*.npz
    python tests/golden/pin_gcnii_model.py --check    # check only

``GCNII.__init__``, ``reset_parameters`` and ``forward`` run verbatim on the CPU under pin_reference.py's stubs.  The
three PyG / torch_sparse names its forward touches are absent here and are RESTATED (tests/gcn2_ref.py), put in place
of the stubs: ``GCN2Conv`` (PyG 2.0.4, normalize=False: propagate, mul by 1 - alpha, alpha x_0, addmm; glorot init),
``gcn_norm`` (self loops added: the reference passes ``False`` as ``improved``) and ``SparseTensor`` (a holder of row,
col, value).  The fixture's ``note`` says so.

A file holds: ``edge_index``, ``x``, the labels ``y``, every entry of the ``state_dict`` before the run
(``param.<key>``, their order in ``keys``), the log-probabilities ``out`` in training mode with dropout 0, every
parameter's gradient of ``F.nll_loss(out, y)`` (``grad.<key>``), the running statistics after the run
(``after.<key>``), ``hyper`` = (in, hidden, out, num_layers, alpha, theta, shared_weights, dropout) and the ``note``.
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

sys.path.insert(0, ROOT)
from tests import gcn2_ref as M  # noqa: E402

NOTE = ("out, grads and running statistics by the reference's own GCNII class (models/models.py:1247-1303) on the CPU; "
        "GCN2Conv, gcn_norm and SparseTensor are absent here and restated (tests/gcn2_ref.py: GCN2ConvRef, gcn_norm_ref, "
        "SparseTensorRef)")

# name -> (n, edges, in, hidden, out, num_layers, alpha, theta, shared_weights, seed, dirty edge list)
CASES = {
    "gcnii_model_a": (300, 1200, 24, 16, 5, 4, 0.1, 0.5, True, 71, False),
    "gcnii_model_b": (300, 1200, 24, 16, 5, 8, 0.0, 1.0, True, 72, False),
    "gcnii_model_c": (300, 1200, 24, 16, 5, 3, 0.2, 0.5, False, 73, True),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    R = import_reference_models()
    R.GCN2Conv, R.gcn_norm, R.SparseTensor = M.GCN2ConvRef, M.gcn_norm_ref, M.SparseTensorRef
    for name, (n, e, fin, hid, fout, layers, alpha, theta, shared, seed, dirty) in CASES.items():
        ei = edges(n, e, seed, dirty)
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(n, fin, generator=gen)
        y = torch.randint(0, fout, (n,), generator=gen)
        torch.manual_seed(seed)
        ref = R.GCNII(fin, hid, fout, layers, alpha, theta, shared, 0.0)
        with torch.no_grad():           # norms that are not the identity, running statistics that are not (0, 1)
            for bn in ref.bns:
                bn.weight.copy_(1.0 + 0.3 * torch.randn(hid, generator=gen))
                bn.bias.copy_(0.2 * torch.randn(hid, generator=gen))
                bn.running_mean.copy_(0.1 * torch.randn(hid, generator=gen))
                bn.running_var.copy_(0.5 + torch.rand(hid, generator=gen))
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train()
        out = ref(types.SimpleNamespace(x=x, num_nodes=n, edge_index=ei))
        F.nll_loss(out, y).backward()
        grads = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert all(float(g.abs().max()) > 0 for g in grads.values()), "a zero gradient compares nothing"
        after = {k: v.clone() for k, v in ref.state_dict().items() if "running_" in k}
        z = dict(edge_index=ei.numpy(), x=x.numpy(), y=y.numpy(), out=out.detach().numpy(),
                 hyper=np.array([fin, hid, fout, layers, alpha, theta, float(shared), 0.0], np.float64),
                 keys=np.array(list(state)), note=np.array(NOTE),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()},
                 **{"after." + k: v.numpy() for k, v in after.items()})
        fx = M.Fixture(z)
        res = M.run(fx, torch.float32)
        worst = float((res["out"] - out.detach()).abs().max()) / float(out.detach().abs().max())
        for k, g in grads.items():
            worst = max(worst, float((res["grads"][k] - g).abs().max()) / max(float(g.abs().max()), 1e-30))
        for k, v in after.items():
            worst = max(worst, float((res["after"][k] - v).abs().max()) / max(float(v.abs().max()), 1e-30))
        print(f"  {name}: reference GCNII == restatement within {worst:.1e} x max-norm over log-probabilities, "
              f"{len(grads)} gradients and {len(after)} running statistics (n = {n}, {ei.size(1)} edges, {layers} layers, "
              f"{len(state)} state entries)")
        assert worst <= 2e-6, worst
        if not args.check:
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **z)
            assert os.path.getsize(path) < 200 * 1024, path
            print(f"    wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

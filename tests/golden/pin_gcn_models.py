#!/usr/bin/env python3
"""Fixtures of the GCN, GCNJK and MixHop models (models/models.py:539-580, 788-843, 693-786), made by running the
REFERENCE classes themselves.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names; nothing of the reference travels: the
outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_gcn_models.py            # check + write tests/golden/{gcn,gcnjk,mixhop}_model_*.npz
    python tests/golden/pin_gcn_models.py --check    # check only

``GCN``, ``GCNJK``, ``MixHopLayer`` and ``MixHop`` - ``__init__``, ``reset_parameters`` and ``forward`` - run verbatim on
the CPU under pin_reference.py's stubs.  The PyG / torch_sparse names their forwards touch are absent here and are
RESTATED (tests/gcn_ref.py), put in place of the stubs: ``GCNConv`` (PyG 2.0.4: a bias-free glorot linear, gcn_norm,
propagate, + bias), ``JumpingKnowledge`` ('max' / 'cat'), ``gcn_norm`` (self loops added: MixHop passes ``False`` as
``improved``), ``SparseTensor`` (a holder of row, col, value) and ``matmul`` (the sum over a row's entries).  The
fixture's ``note`` says so.

A file holds: ``edge_index``, ``x``, the labels ``y``, every entry of the ``state_dict`` before the run
(``param.<key>``, their order in ``keys``), the log-probabilities ``out`` in training mode with dropout 0, every
parameter's gradient of ``F.nll_loss(out, y)`` (``grad.<key>``), the running statistics after the run
(``after.<key>``), ``hyper`` = (kind, in, hidden, out, num_layers, dropout, use_bn | jk_type is 'cat' | hops) with kind
0 = GCN, 1 = GCNJK, 2 = MixHop, and the ``note``.
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
from tests import gcn_ref as M  # noqa: E402

NOTE = ("out, grads and running statistics by the reference's own {cls} class (models/models.py) on the CPU; GCNConv, "
        "JumpingKnowledge, gcn_norm, SparseTensor and matmul are absent here and restated (tests/gcn_ref.py: GCNConvRef, "
        "JumpingKnowledgeRef, gcn_norm_ref, SparseTensorRef, matmul)")

# name -> (kind, n, edges, in, hidden, out, num_layers, kind's own, seed, dirty edge list)
CASES = {
    "gcn_model_a": (0, 300, 1200, 24, 16, 5, 2, 1, 81, False),          # use_bn
    "gcn_model_b": (0, 300, 1200, 24, 12, 5, 3, 1, 82, True),
    "gcnjk_model_a": (1, 300, 1200, 24, 16, 5, 3, 0, 83, False),        # max
    "gcnjk_model_b": (1, 300, 1200, 24, 12, 5, 3, 1, 84, True),         # cat
    "mixhop_model_a": (2, 300, 1200, 24, 8, 5, 2, 2, 85, False),        # hops
    "mixhop_model_b": (2, 300, 1200, 24, 6, 5, 3, 3, 86, True),
}


def build(R, kind, fin, hid, fout, layers, own):
    if kind == 0:
        return R.GCN(fin, hid, fout, layers, 0.0, False, bool(own))
    if kind == 1:
        return R.GCNJK(fin, hid, fout, layers, 0.0, False, "cat" if own else "max")
    return R.MixHop(fin, hid, fout, layers, 0.0, own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    R = import_reference_models()
    R.GCNConv, R.JumpingKnowledge, R.gcn_norm = M.GCNConvRef, M.JumpingKnowledgeRef, M.gcn_norm_ref
    R.SparseTensor, R.matmul = M.SparseTensorRef, M.matmul
    for name, (kind, n, e, fin, hid, fout, layers, own, seed, dirty) in CASES.items():
        ei = edges(n, e, seed, dirty)
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(n, fin, generator=gen)
        y = torch.randint(0, fout, (n,), generator=gen)
        torch.manual_seed(seed)
        ref = build(R, kind, fin, hid, fout, layers, own)
        with torch.no_grad():           # norms that are not the identity, running statistics that are not (0, 1)
            for bn in ref.bns:
                w = bn.num_features
                bn.weight.copy_(1.0 + 0.3 * torch.randn(w, generator=gen))
                bn.bias.copy_(0.2 * torch.randn(w, generator=gen))
                bn.running_mean.copy_(0.1 * torch.randn(w, generator=gen))
                bn.running_var.copy_(0.5 + torch.rand(w, generator=gen))
            for k, p in ref.named_parameters():          # (GCNConv's bias starts at zero: it would compare nothing)
                if k.startswith("convs.") and k.endswith(".bias") and ".lins." not in k:
                    p.copy_(0.1 * torch.randn(p.shape, generator=gen))
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train()
        out = ref(types.SimpleNamespace(x=x, num_nodes=n, edge_index=ei))
        F.nll_loss(out, y).backward()
        grads = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert all(float(g.abs().max()) > 0 for g in grads.values()), "a zero gradient compares nothing"
        after = {k: v.clone() for k, v in ref.state_dict().items() if "running_" in k}
        cls = type(ref).__name__
        z = dict(edge_index=ei.numpy(), x=x.numpy(), y=y.numpy(), out=out.detach().numpy(),
                 hyper=np.array([kind, fin, hid, fout, layers, 0.0, float(own)], np.float64),
                 keys=np.array(list(state)), note=np.array(NOTE.format(cls=cls)),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()},
                 **{"after." + k: v.numpy() for k, v in after.items()})
        fx = M.Fixture(z)
        res = M.run(fx, torch.float32)
        worst = float((res["out"] - out.detach()).abs().max()) / float(out.detach().abs().max())
        for k, g in grads.items():
            worst = max(worst, float((res["grads"][k] - g).abs().max()) / max(float(g.abs().max()), 1e-30))
        for k, v in after.items():
            worst = max(worst, float((res["after"][k] - v).abs().max()) / max(float(v.abs().max()), 1e-30))
        print(f"  {name}: reference {cls} == restatement within {worst:.1e} x max-norm over log-probabilities, "
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

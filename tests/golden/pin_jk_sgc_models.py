#!/usr/bin/env python3
"""Fixtures of the GATJK, SGC, SGCMem and MultiLP models (models/models.py:846-900, 479-493, 496-536, 636-690), made by
running the REFERENCE classes themselves.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names; nothing of the reference travels: the
outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_jk_sgc_models.py            # check + write tests/golden/{gatjk,sgc,sgcmem}_model_*.npz, multilp_case_*.npz
    python tests/golden/pin_jk_sgc_models.py --check    # check only

``GATJK``, ``SGC``, ``SGCMem`` and ``MultiLP`` - ``__init__``, ``reset_parameters`` and ``forward`` - run verbatim on the
CPU under pin_reference.py's stubs.  The PyG / torch_sparse names their forwards touch are absent here and are RESTATED,
put in place of the stubs: ``GATConv`` (tests/gat_ref.py's GATConvRef with ``reset_parameters``: tests/jk_sgc_ref.py
GATConvJK), ``JumpingKnowledge`` ('max' / 'cat'), ``gcn_norm``, ``matmul`` (tests/gcn_ref.py), ``SparseTensor`` (the holder
of tests/gcn2_ref.py with ``device()``: SparseTensorDev) and ``SGConv`` (PyG 2.0.4's layer restated from memory of that
release: SGConvRef).  The fixture's ``note`` says so.

A model file holds the fields of gcn_model_*.npz: ``edge_index``, ``x``, the labels ``y``, every entry of the
``state_dict`` before the run (``param.<key>``, their order in ``keys``), the output ``out`` in training mode with dropout
0 (GATJK: log-probabilities; SGC / SGCMem: the linear's output), every parameter's gradient of ``F.nll_loss`` of the
log-probabilities (``grad.<key>``), the running statistics after the run (``after.<key>``), ``hyper`` (tests/jk_sgc_ref.py:
Fixture) and the ``note``.  A MultiLP file holds ``edge_index``, ``n``, ``label``, ``train_idx``, ``out``, ``hyper`` =
(out_channels, alpha, hops, num_iters, mult_bin), empty ``keys`` and the ``note``.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from pin_acm_model import edges  # noqa: E402
from pin_reference import REFERENCE, ROOT, import_reference_models  # noqa: E402

sys.path.insert(0, ROOT)
from tests import gcn_ref as G  # noqa: E402
from tests import jk_sgc_ref as M  # noqa: E402

NOTE = ("out{rest} by the reference's own {cls} class (models/models.py) on the CPU; the third-party layers are absent "
        "here and restated: GATConv (tests/gat_ref.py GATConvRef + reset_parameters), JumpingKnowledge, gcn_norm, matmul "
        "(tests/gcn_ref.py), SparseTensor (tests/gcn2_ref.py + device()), and SGConv - PyG 2.0.4's layer RESTATED from "
        "memory of that release (tests/jk_sgc_ref.py SGConvRef), not run")

# name -> (kind, n, edges, in, hidden, out, num_layers, heads, cat, seed, dirty edge list); SGC / SGCMem: hidden = hops
MODEL_CASES = {
    "gatjk_model_a": (0, 300, 1200, 24, 8, 5, 3, 2, 0, 91, False),          # max
    "gatjk_model_b": (0, 300, 1200, 24, 4, 5, 2, 3, 1, 92, True),           # cat
    "gatjk_model_c": (0, 300, 1200, 24, 8, 5, 4, 1, 0, 93, False),          # max, one head
    "sgc_model_a": (1, 300, 1200, 24, 2, 5, 0, 0, 0, 94, False),
    "sgcmem_model_a": (2, 300, 1200, 24, 3, 5, 0, 0, 0, 95, True),
}
# name -> (n, edges, out_channels, alpha, hops, num_iters, mult_bin, label form, seed, dirty)
LP_CASES = {
    "multilp_case_a": (300, 1200, 5, 0.1, 1, 50, False, "class", 96, False),
    "multilp_case_b": (300, 1200, 3, 0.5, 2, 10, True, "tasks", 97, True),
    "multilp_case_c": (300, 1200, 4, 0.3, 1, 20, False, "rows", 98, False),
}


def _write(args, name, z):
    if not args.check:
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **z)
        assert os.path.getsize(path) < M.MAX_BYTES, path
        print(f"    wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


def pin_models(R, args):
    for name, (kind, n, e, fin, hid, fout, layers, heads, cat, seed, dirty) in MODEL_CASES.items():
        ei = edges(n, e, seed, dirty)
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(n, fin, generator=gen)
        y = torch.randint(0, fout, (n,), generator=gen)
        torch.manual_seed(seed)
        if kind == 0:
            ref = R.GATJK(fin, hid, fout, layers, 0.0, heads, "cat" if cat else "max")
            hyper = [0, fin, hid, fout, layers, 0.0, heads, float(cat)]
        else:
            ref = (R.SGC if kind == 1 else R.SGCMem)(fin, fout, hid)
            hyper = [kind, fin, fout, hid]
        ref.reset_parameters()          # (the reference's own, through the restated layers')
        with torch.no_grad():           # norms that are not the identity, running statistics that are not (0, 1)
            for bn in getattr(ref, "bns", []):
                w = bn.num_features
                bn.weight.copy_(1.0 + 0.3 * torch.randn(w, generator=gen))
                bn.bias.copy_(0.2 * torch.randn(w, generator=gen))
                bn.running_mean.copy_(0.1 * torch.randn(w, generator=gen))
                bn.running_var.copy_(0.5 + torch.rand(w, generator=gen))
            for k, p in ref.named_parameters():          # (GATConv's bias starts at zero: it would compare nothing)
                if k.startswith("convs.") and k.endswith(".bias"):
                    p.copy_(0.1 * torch.randn(p.shape, generator=gen))
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train()
        out = ref(types.SimpleNamespace(x=x, num_nodes=n, edge_index=ei, graph=dict(num_nodes=n, edge_index=ei)))
        logp = out if kind == 0 else torch.log_softmax(out, dim=1)
        M.loss_of(logp, y).backward()
        grads = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert all(float(g.abs().max()) > 0 for g in grads.values()), "a zero gradient compares nothing"
        after = {k: v.clone() for k, v in ref.state_dict().items() if "running_" in k}
        cls = type(ref).__name__
        z = dict(edge_index=ei.numpy(), x=x.numpy(), y=y.numpy(), out=out.detach().numpy(),
                 hyper=np.array(hyper, np.float64), keys=np.array(list(state)),
                 note=np.array(NOTE.format(cls=cls, rest=", grads and running statistics")),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()},
                 **{"after." + k: v.numpy() for k, v in after.items()})
        fx = M.Fixture(z)
        res = M.run(fx, torch.float32)
        worst = float((res["out"] - out.detach()).abs().max()) / float(out.detach().abs().max())
        assert set(res["grads"]) == set(grads)
        for k, g in grads.items():
            worst = max(worst, float((res["grads"][k] - g).abs().max()) / max(float(g.abs().max()), 1e-30))
        for k, v in after.items():
            worst = max(worst, float((res["after"][k] - v).abs().max()) / max(float(v.abs().max()), 1e-30))
        print(f"  {name}: reference {cls} == restatement within {worst:.1e} x max-norm over the output, {len(grads)} "
              f"gradients and {len(after)} running statistics (n = {n}, {ei.size(1)} edges, {len(state)} state entries)")
        assert worst <= 2e-6, worst
        _write(args, name, z)


def pin_label_propagation(R, args):
    for name, (n, e, c, alpha, hops, iters, mult_bin, form, seed, dirty) in LP_CASES.items():
        ei = edges(n, e, seed, dirty)
        gen = torch.Generator().manual_seed(seed + 1)
        if form == "class":
            label = torch.randint(0, c, (n, 1), generator=gen)
        elif form == "tasks":
            label = torch.randint(0, 2, (n, c), generator=gen)
        else:          # multi-label float rows, negative entries among them
            label = torch.randn(n, c, generator=gen) * (torch.rand(n, c, generator=gen) < 0.4)
        train_idx = torch.randperm(n, generator=gen)[:n // 2].sort().values
        ref = R.MultiLP(c, alpha, hops, iters, mult_bin)
        out = ref(types.SimpleNamespace(label=label, graph=dict(num_nodes=n, edge_index=ei)), train_idx)
        assert out.shape == (n, c) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        z = dict(edge_index=ei.numpy(), n=np.array(n, np.int64), label=label.numpy(), train_idx=train_idx.numpy(),
                 out=out.numpy(), hyper=np.array([c, alpha, hops, iters, float(mult_bin)], np.float64),
                 keys=np.array([], dtype="<U1"), note=np.array(NOTE.format(cls="MultiLP", rest="")))
        fx = M.LPFixture(z)
        worst = float((fx.run(torch.float32) - out).abs().max()) / float(out.abs().max())
        print(f"  {name}: reference MultiLP == restatement within {worst:.1e} x max-norm (n = {n}, {ei.size(1)} edges, "
              f"{form} labels, alpha {alpha}, hops {hops}, {iters} iterations)")
        assert worst <= 2e-6, worst
        _write(args, name, z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    R = import_reference_models()
    R.GATConv, R.SGConv, R.JumpingKnowledge = M.GATConvJK, M.SGConvRef, G.JumpingKnowledgeRef
    R.gcn_norm, R.SparseTensor, R.matmul = G.gcn_norm_ref, M.SparseTensorDev, G.matmul
    pin_models(R, args)
    pin_label_propagation(R, args)


if __name__ == "__main__":
    main()

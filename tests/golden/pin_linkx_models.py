#!/usr/bin/env python3
"""Fixtures of LINK (models/models.py:409-434), LINK_Concat (:1057-1095) and LINKX (:1098-1146), made by running the
REFERENCE classes themselves.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names; nothing of the reference travels: the
outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_linkx_models.py            # check + write tests/golden/link*_model_*.npz
    python tests/golden/pin_linkx_models.py --check    # check only

The three classes, ``MLP`` included, run verbatim on the CPU under pin_reference.py's stubs, forward and backward:
``nn.Linear`` takes the sparse COO adjacency as its input in this torch.  The one torch_sparse name their forwards touch
is RESTATED here: ``SparseTensor(row, col, sparse_sizes).to_torch_sparse_coo_tensor()`` - entries sorted by (row, col),
duplicates kept, value 1.0 each, any shape (pin_reference.py's stub is square only).  It takes no values, as LINK_Concat
hands it none.  The fixture's ``note`` says so.

A file holds, in the format pin_gcnii_model.py documents: ``edge_index``, ``x``, the labels ``y``, every entry of the
``state_dict`` before the run (``param.<key>``, their order in ``keys``), the log-probabilities ``out`` in training mode
with dropout 0, every parameter's gradient of ``F.nll_loss(out, y)`` (``grad.<key>``), the running statistics after the
run (``after.<key>``; LINKX's ``W.bias`` is moved so that about half of the join's relu is live), ``model`` (the class name), ``hyper`` (its positional constructor arguments, tests/linkx_ref.py:
HYPER) and the ``note``.
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
from tests import linkx_ref as M  # noqa: E402

NOTE = ("out, grads and running statistics by the reference's own {kind} class (models/models.py) on the CPU, nn.Linear "
        "on the sparse COO adjacency; torch_sparse's SparseTensor(row, col, sparse_sizes).to_torch_sparse_coo_tensor() is "
        "absent here and restated (entries sorted by (row, col), duplicates kept, value 1)")


class SparseTensorRect:
    """torch_sparse.SparseTensor(row, col, sparse_sizes) as models.py:428, 1085 and 1131 build it."""

    def __init__(self, row=None, col=None, sparse_sizes=None):
        self.row, self.col, self.sizes = row, col, tuple(int(s) for s in sparse_sizes)

    def to_torch_sparse_coo_tensor(self):
        perm = torch.argsort(self.row * self.sizes[1] + self.col, stable=True)
        idx = torch.stack([self.row[perm], self.col[perm]], dim=0)
        return torch.sparse_coo_tensor(idx, torch.ones(idx.size(1), dtype=torch.float32), self.sizes)


def _dirty_bn(model, gen):
    """Norms that are not the identity, running statistics that are not (0, 1)."""
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                c = m.num_features
                m.weight.copy_(1.0 + 0.3 * torch.randn(c, generator=gen))
                m.bias.copy_(0.2 * torch.randn(c, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(c, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(c, generator=gen))


# name -> (class, seed, edit of the edge list / features / norms, the positional constructor arguments)
N, E, FIN, FOUT = 300, 1200, 24, 5
CASES = {
    "link_model_a": ("LINK", 81, "shift", lambda n: (n, FOUT)),
    "linkx_model_a": ("LINKX", 82, None, lambda n: (FIN, 16, FOUT, 2, n, 0.0, False, False, False, 1, 1)),
    "linkx_model_b": ("LINKX", 83, "bn", lambda n: (FIN, 40, FOUT, 3, n, 0.0, False, False, False, 2, 2)),
    "linkx_model_c": ("LINKX", 84, "shift", lambda n: (FIN, 130, FOUT, 2, n, 0.0, False, False, False, 1, 1)),
    "link_concat_model_a": ("LINK_Concat", 85, None, lambda n: (FIN, 16, FOUT, 1, n, 0.0, True)),
    "link_concat_model_b": ("LINK_Concat", 86, "sparse_x", lambda n: (FIN, 16, FOUT, 2, n, 0.0, True)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    R = import_reference_models()
    R.SparseTensor = SparseTensorRect
    for name, (kind, seed, edit, ctor) in CASES.items():
        ei = edges(N, E, seed, True)                      # duplicates and self loops on top
        if edit == "shift":                               # the lowest source id above 0: row - row.min() shows
            ei = ei[:, ei[0] >= 3]
            ei = torch.cat([ei, ei[:, :40], ei[:, :7], torch.arange(5, 10).repeat(2, 1)], dim=1).contiguous()
            assert int(ei[0].min()) == 3
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(N, FIN, generator=gen)
        if edit == "sparse_x":                            # zeros and non-binary values: the binarisation shows
            x = x * (torch.rand(N, FIN, generator=gen) < 0.3) * torch.randint(1, 4, (N, FIN), generator=gen)
        y = torch.randint(0, FOUT, (N,), generator=gen)
        hyper = ctor(N)
        torch.manual_seed(seed)
        ref = getattr(R, kind)(*hyper)
        if edit == "bn":
            _dirty_bn(ref, gen)
        if kind == "LINKX":
            # the join adds two rows of log-probabilities, about -2 ln(hidden) an element, in front of its relu: as
            # initialised nearly every element is dead and mlpA, mlpX and W get zero gradients.  A bias that centres
            # the pre-activations leaves about half of them live, so that the fixture compares something.
            with torch.no_grad():
                ref.W.bias.add_(2.0 * float(np.log(hyper[1])))
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train()
        out = ref(types.SimpleNamespace(x=x, num_nodes=N, edge_index=ei))
        F.nll_loss(out, y).backward()
        grads = {k: (p.grad.to_dense() if p.grad.is_sparse else p.grad) for k, p in ref.named_parameters()
                 if p.grad is not None}
        assert set(grads) == {k for k, _ in ref.named_parameters()}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        assert all(float(g.abs().max()) > 0 for g in grads.values()), "a zero gradient compares nothing"
        after = {k: v.clone() for k, v in ref.state_dict().items() if "running_" in k}
        z = dict(edge_index=ei.numpy(), x=x.numpy(), y=y.numpy(), out=out.detach().numpy(), model=np.array(kind),
                 hyper=np.array([float(v) for v in hyper], np.float64), keys=np.array(list(state)),
                 note=np.array(NOTE.format(kind=kind)),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()},
                 **{"after." + k: v.numpy() for k, v in after.items()})
        fx = M.Fixture(z)
        res = M.run(fx, torch.float32)
        worst = float((res["out"] - out.detach()).abs().max()) / float(out.detach().abs().max())
        for k, g in grads.items():
            worst = max(worst, float((res["grads"][k] - g).abs().max()) / max(float(g.abs().max()), 1e-30))
        for k, v in after.items():
            worst = max(worst, float((res["after"][k] - v).abs().max()) / max(float(v.abs().max()), 1e-30))
        print(f"  {name}: reference {kind} == restatement within {worst:.1e} x max-norm over log-probabilities, "
              f"{len(grads)} gradients and {len(after)} running statistics (n = {N}, {ei.size(1)} edges, lowest source "
              f"{int(ei[0].min())}, {len(state)} state entries)")
        assert worst <= 2e-6, worst
        if not args.check:
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **z)
            assert os.path.getsize(path) < 1024 * 1024, path
            print(f"    wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

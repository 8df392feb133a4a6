#!/usr/bin/env python3
"""Fixtures of the H2GCN model (models/models.py:903-1024), made by running the REFERENCE class itself.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names, and scipy, which ``init_adj`` calls;
nothing of the reference travels: the outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_h2gcn_model.py            # check + write tests/golden/h2gcn_model_{a,b,c}.npz
    python tests/golden/pin_h2gcn_model.py --check    # check only

``H2GCN.__init__``, ``init_adj`` and ``forward`` (and ``H2GCNConv``, and the reference's ``MLP``) run verbatim on the CPU
under pin_reference.py's stubs.  The torch_sparse / PyG names they touch are absent here and are RESTATED
(tests/h2gcn_ref.py, tests/gcn_ref.py), put in place of the stubs: ``SparseTensor`` (row, col, value; ``remove_diag``,
which drops the diagonal of the object it is called on as ``init_adj`` expects, ``to_scipy``, ``from_scipy``),
``matmul`` (sparse x sparse: the pattern of the product, without values where neither operand has any; sparse x dense:
the sum over a row's entries), ``gcn_norm`` on a SparseTensor without self loops (deg = the row sum, dinv 0 for an empty
row) and ``JumpingKnowledge`` ('cat').  The fixture's ``note`` says so.

Fixture (a) is the reference as it is: ``relu(feature_embed(data))`` is exactly 0 (the MLP ends in log_softmax), so the
log-probabilities do not depend on ``x`` and every ``feature_embed`` gradient is pinned as exactly 0.  Fixtures (b) and
(c) swap ``feature_embed`` for an MLP of the same parameters that returns its logits (the package's
``embed_logits=True``): 3 layers, norms on / off, conv_dropout off / on.  Dropout 0 everywhere.

A file holds: ``edge_index``, ``x``, the labels ``y``, every entry of the ``state_dict`` before the run
(``param.<key>``, their order in ``keys``), the log-probabilities ``out`` in training mode, every parameter's gradient
of ``F.nll_loss(out, y)`` (``grad.<key>``), the running statistics after the run (``after.<key>``), ``hyper`` = (in,
hidden, out, num_layers, dropout, num_mlp_layers, use_bn, conv_dropout, embed_logits) and the ``note``.
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
from tests import gcn_ref as G  # noqa: E402
from tests import h2gcn_ref as H  # noqa: E402

NOTE = ("out, grads and running statistics by the reference's own H2GCN class (models/models.py: __init__, init_adj, "
        "forward, H2GCNConv{embed}) on the CPU; SparseTensor (with remove_diag acting on the object, to_scipy, "
        "from_scipy), the sparse-sparse and sparse-dense matmul, gcn_norm without self loops and JumpingKnowledge are "
        "absent here and restated (tests/h2gcn_ref.py: SparseTensorRef, matmul, gcn_norm_ref; tests/gcn_ref.py: "
        "JumpingKnowledgeRef)")
EMBED = {False: ", MLP", True: "; feature_embed swapped for an MLP of the same parameters that returns its logits "
                               "(tests/h2gcn_ref.py: LogitsMLP) - the package's embed_logits=True"}

# name -> (n, edges, in, hidden, out, num_layers, num_mlp_layers, use_bn, conv_dropout, embed_logits, seed)
CASES = {
    "h2gcn_model_a": (300, 900, 24, 16, 5, 2, 2, True, True, False, 91),
    "h2gcn_model_b": (300, 900, 24, 12, 5, 3, 2, True, False, True, 92),
    "h2gcn_model_c": (300, 900, 24, 8, 5, 3, 1, False, True, True, 93),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    R = import_reference_models()
    R.SparseTensor, R.matmul, R.gcn_norm, R.JumpingKnowledge = H.SparseTensorRef, H.matmul, H.gcn_norm_ref, G.JumpingKnowledgeRef
    for name, (n, e, fin, hid, fout, layers, mlp_layers, use_bn, conv_dropout, logits, seed) in CASES.items():
        ei = edges(n, e, seed, True)
        gen = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(n, fin, generator=gen)
        y = torch.randint(0, fout, (n,), generator=gen)
        torch.manual_seed(seed)
        ref = R.H2GCN(fin, hid, fout, ei, n, layers, 0.0, False, mlp_layers, use_bn, conv_dropout)
        if logits:
            emb = H.LogitsMLP(fin, hid, hid, mlp_layers, 0.0)
            emb.load_state_dict(ref.feature_embed.state_dict(), strict=True)
            ref.feature_embed = emb
        with torch.no_grad():           # norms that are not the identity, running statistics that are not (0, 1)
            for bn in list(ref.bns) + list(ref.feature_embed.bns):
                w = bn.num_features
                bn.weight.copy_(1.0 + 0.3 * torch.randn(w, generator=gen))
                bn.bias.copy_(0.2 * torch.randn(w, generator=gen))
                bn.running_mean.copy_(0.1 * torch.randn(w, generator=gen))
                bn.running_var.copy_(0.5 + torch.rand(w, generator=gen))
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train()
        out = ref(types.SimpleNamespace(x=x, num_nodes=n, edge_index=ei))
        F.nll_loss(out, y).backward()
        grads = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        embed = [k for k in grads if k.startswith("feature_embed.")]
        assert embed
        if logits:
            assert all(float(grads[k].abs().max()) > 0 for k in embed), "a zero gradient compares nothing"
        else:           # the quirk: relu(log_softmax(.)) == 0
            assert all(float(grads[k].abs().max()) == 0.0 for k in embed)
        assert float(grads["final_project.weight"].abs().max()) > 0
        after = {k: v.clone() for k, v in ref.state_dict().items() if "running_" in k}
        if not logits:          # nothing of x arrives: another x, the same bits
            with torch.no_grad():
                other = ref(types.SimpleNamespace(x=torch.randn(n, fin, generator=gen), num_nodes=n, edge_index=ei))
            assert torch.equal(other, out.detach())
        z = dict(edge_index=ei.numpy(), x=x.numpy(), y=y.numpy(), out=out.detach().numpy(),
                 hyper=np.array([fin, hid, fout, layers, 0.0, mlp_layers, float(use_bn), float(conv_dropout), float(logits)],
                                np.float64),
                 keys=np.array(list(state)), note=np.array(NOTE.format(embed=EMBED[logits])),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()},
                 **{"after." + k: v.numpy() for k, v in after.items()})
        fx = H.Fixture(z)
        # the adjacencies the reference cached are the restatement's, entry for entry
        (ei1, n1), (ei2, n2) = H.adjacencies(ei, n, torch.float32)
        for adj, (eir, nr) in ((ref.adj_t, (ei1, n1)), (ref.adj_t2, (ei2, n2))):
            dense = torch.zeros(n, n).index_put_((eir[1], eir[0]), nr, accumulate=True)
            theirs = torch.zeros(n, n).index_put_((adj.row, adj.col), adj.value, accumulate=True)
            assert bool(((dense != 0) == (theirs != 0)).all()) and float((dense - theirs).abs().max()) <= 1e-6
        res = H.run(fx, torch.float32)
        assert set(res["grads"]) == set(grads)
        worst = float((res["out"] - out.detach()).abs().max()) / float(out.detach().abs().max())
        for k, g in grads.items():
            worst = max(worst, float((res["grads"][k] - g).abs().max()) / max(float(g.abs().max()), 1e-30))
        for k, v in after.items():
            worst = max(worst, float((res["after"][k] - v).abs().max()) / max(float(v.abs().max()), 1e-30))
        print(f"  {name}: reference H2GCN == restatement within {worst:.1e} x max-norm over log-probabilities, "
              f"{len(grads)} gradients and {len(after)} running statistics (n = {n}, {ei.size(1)} edges, "
              f"{int(ei2.size(1))} two-hop entries, {layers} layers, {len(state)} state entries)")
        assert worst <= 2e-6, worst
        if not args.check:
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **z)
            assert os.path.getsize(path) < 200 * 1024, path
            print(f"    wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

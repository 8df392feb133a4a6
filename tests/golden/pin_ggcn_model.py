#!/usr/bin/env python3
"""Fixtures of the whole GGCN model (models/models.py:1640-1739), made by running the REFERENCE class itself.

BUILD CONTAINER ONLY (needs the reference checkout that pin_reference.py names; nothing of the reference
travels: the outputs are plain .npz data under tests/golden/).  Run from the repo root:

    python tests/golden/pin_ggcn_model.py            # check + write tests/golden/ggcn_model_*.npz
    python tests/golden/pin_ggcn_model.py --check    # check only

GGCN and GGCNlayer_SP are core torch, so under pin_reference.py's stubs (which only make the reference's import
block succeed) every line of the model runs verbatim on the CPU, forward and backward.  Each case is run in
training mode with dropout 0, away from the symmetric initial point (``coeff`` = 0) as pin_ggcn does, and is
compared with the restatement the tests use (tests/ggcn_model_ref.py) before it is written.

A file holds: the adjacency's indices and values, the degree values (use_degree), ``x``, an output gradient
``gout`` (the loss is <log-probabilities, gout>), every entry of the initial ``state_dict`` (``param.<key>``, their
order in ``keys``), the log-probabilities, every parameter's gradient (``grad.<key>``), ``hyper`` = (nfeat, nlayers,
nhidden, nclass, dropout, decay_rate, exponent), ``flags`` = (use_degree, use_sign, use_decay, use_bn, use_ln) and a
``note``.
"""
from __future__ import annotations

import os

# row_normalize's np.power(rowsum, -1) is a float32 power, which numpy dispatches by CPU feature: its AVX512 form is
# one ulp off the reciprocal for many integers (7, 11, 13, 14, 15, 22 ...; 992 of 1 .. 4999), the baseline form for
# none below 953.  A fixture must not depend on the CPU that made it, so numpy runs its baseline form here (set
# before numpy is imported).  With the AVX512 form 24 of case (b)'s 1099 values - its rows of sum 7 - come out
# one ulp lower.
os.environ["NPY_DISABLE_CPU_FEATURES"] = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"

import argparse
import contextlib
import importlib.util
import io
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from pin_reference import REFERENCE, ROOT, ggcn_case, import_reference_models  # noqa: E402

sys.path.insert(0, ROOT)
from tests import ggcn_model_ref as M  # noqa: E402

FLAGS = ("use_degree", "use_sign", "use_decay", "use_bn", "use_ln")

# name -> (constructor keywords, graph)
CASES = {
    "ggcn_model_a_l3": dict(kw=dict(nlayers=3, nhidden=16, dropout=0.0, decay_rate=1.0, exponent=3.0, use_degree=True),
                            graph=("ggcn_case", 300, 1200, 20, 5, 51)),
    # train.py:357-360's literal keyword values
    "ggcn_model_b_l4_train_py": dict(kw=dict(nlayers=4, nhidden=24, dropout=0.0, decay_rate=1e-7, exponent=2,
                                             use_degree=False, use_sign=True, use_decay=True, scale_init=0.5,
                                             deg_intercept_init=0.5, use_bn=False, use_ln=False),
                                     graph=("row_normalised", 250, 1100, 16, 6, 52)),
    "ggcn_model_c_l2_nosign": dict(kw=dict(nlayers=2, nhidden=16, dropout=0.0, decay_rate=1.0, exponent=3.0,
                                           use_sign=False),
                                   graph=("ggcn_case", 200, 800, 12, 4, 53)),
    "ggcn_model_d_l3_bn": dict(kw=dict(nlayers=3, nhidden=16, dropout=0.0, decay_rate=1.0, exponent=3.0, use_bn=True),
                               graph=("ggcn_case", 200, 800, 12, 4, 54)),
}


@contextlib.contextmanager
def quiet():
    """(tqdm's bar and the deprecated sparse constructor's warning)"""
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        yield


def import_reference_data_transform():
    """utils/data_transform.py itself under the stubs (scipy and scikit-learn are the real packages), or None."""
    try:
        spec = importlib.util.spec_from_file_location("sngnn_reference_data_transform",
                                                      os.path.join(REFERENCE, "utils", "data_transform.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    except Exception as exc:          # noqa: BLE001 - any import failure means: build the adjacency by hand
        print("  utils/data_transform.py does not import under the stubs:", repr(exc))
        return None


def directed_edges(n, e, seed):
    """A directed edge list with duplicate edges, a few self-loops and two nodes without out-edges."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n - 2, (e,), generator=gen)
    dst = torch.randint(0, n, (e,), generator=gen)
    ei = torch.stack([src, dst])
    ei = torch.cat([ei, ei[:, :40], ei[:, :7], torch.arange(5).repeat(2, 1)], dim=1)      # duplicates (x2, x3), loops
    return ei[:, torch.randperm(ei.size(1), generator=gen)]


def make_graph(spec, T):
    kind, n, e, f, c, seed = spec
    if kind == "ggcn_case":
        adj, x, gout = ggcn_case(n, e, f, c, seed)
        return adj, x, gout, None, "symmetric normalised adjacency with self-loops (pin_reference.ggcn_case)"
    ei = directed_edges(n, e, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(n, f, generator=gen)
    gout = torch.randn(n, c, generator=gen)
    from sngnn_amd.ggcn import edge_index_to_torch_coo_tensor as ours
    mine = ours(x, ei)
    if T is not None:
        with quiet():
            adj = T.edge_index_to_torch_coo_tensor(x, ei)
        note = ("adjacency made by the reference's own edge_index_to_torch_coo_tensor (utils/data_transform.py:58-65), "
                "numpy's float32 power in its baseline (non-AVX512) form; coalesced")
        adj = adj.coalesce()          # (the reference's entries are unique; its rows list their columns downwards)
        idx, val = adj._indices(), adj._values()
        assert torch.equal(idx, mine._indices())
        same = torch.equal(val, mine._values())
        print(f"  edge_index_to_torch_coo_tensor: {idx.size(1)} entries, values "
              f"{'bit for bit' if same else 'DIFFER'} (max |d| {float((val - mine._values()).abs().max()):.2e})")
        assert same
        adj = torch.sparse_coo_tensor(idx, val, adj.size()).coalesce()
    else:
        adj = mine
        note = "adjacency built by hand (sngnn_amd.ggcn.edge_index_to_torch_coo_tensor): the reference's module does not import"
    return adj, x, gout, ei, note


def perturb(model):
    """Away from the symmetric initial point, a little differently in every layer."""
    with torch.no_grad():
        for i, conv in enumerate(model.convs):
            if hasattr(conv, "coeff"):
                conv.coeff.copy_(torch.tensor([0.3, -0.4, 0.1]) * (1.0 + 0.25 * i))
                conv.scale.add_(-0.1 * i)
            if hasattr(conv, "deg_coeff"):
                conv.deg_coeff.copy_(torch.tensor([0.7 - 0.1 * i, 0.2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare only, write nothing")
    args = ap.parse_args()
    if not os.path.isdir(REFERENCE):
        sys.exit("needs the reference checkout (build container only)")
    R = import_reference_models()
    T = import_reference_data_transform()
    for name, case in CASES.items():
        kw = dict(case["kw"])
        adj, x, gout, ei, note = make_graph(case["graph"], T)
        n, f, c = x.size(0), x.size(1), gout.size(1)
        torch.manual_seed(case["graph"][-1])
        ref = R.GGCN(nfeat=f, nclass=c, device="cpu", use_sparse=True, **kw)
        perturb(ref)
        dp = None
        if ref.use_degree:
            with quiet():
                ref.precompute_degree_s(adj)
            dp = ref.degree_precompute
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.train()
        with quiet():
            out = ref(types.SimpleNamespace(x=x), {"adj_coo_tensor": adj})
        (out * gout).sum().backward()
        grads = {k: p.grad for k, p in ref.named_parameters()}
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())

        flags = {k: bool(kw.get(k, k in ("use_degree", "use_sign", "use_decay"))) for k in FLAGS}
        hyper = np.array([f, kw["nlayers"], kw["nhidden"], c, kw["dropout"], kw["decay_rate"], kw["exponent"]], np.float64)
        z = dict(adj_indices=adj._indices().numpy(), adj_values=adj._values().numpy(), x=x.numpy(), gout=gout.numpy(),
                 out=out.detach().numpy(), hyper=hyper, flags=np.array([int(flags[k]) for k in FLAGS], np.int64),
                 keys=np.array(list(state)), note=np.array(note),
                 **{"param." + k: v.numpy() for k, v in state.items()}, **{"grad." + k: g.numpy() for k, g in grads.items()})
        if dp is not None:
            z["degree_values"] = dp._values().numpy()
        if ei is not None:
            z["edge_index"] = ei.numpy()

        # the restatement the tests use reproduces the run (same host: to the last bits of the sparse products)
        fx = M.Fixture(z)
        res = M.run(fx, torch.float32)
        worst = float((res["out"] - out.detach()).abs().max()) / float(out.detach().abs().max())
        for k, g in grads.items():
            worst = max(worst, float((res["grads"][k] - g).abs().max()) / max(float(g.abs().max()), 1e-30))
        print(f"  {name}: reference GGCN == restatement within {worst:.1e} x max-norm over log-probabilities and "
              f"{len(grads)} gradients (n = {n}, nnz = {adj._nnz()}, {len(state)} state entries)")
        assert worst <= 2e-6, worst
        if not args.check:
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **z)
            size = os.path.getsize(path)
            assert size < 200 * 1024, (name, size)
            print(f"    wrote {os.path.relpath(path, ROOT)} ({size} bytes)")


if __name__ == "__main__":
    main()

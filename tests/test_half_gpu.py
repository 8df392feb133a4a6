"""GPU: the half path - the aggregation on float16 / bfloat16 rows, forward and backward, and the layers and
models cast to those types.

The contract (include/sngnn_hip.h, "Half-width feature rows"): with hf = h.float(), gf = grad_out.float(),
  1. the half forward IS the fp32 on-the-fly forward (knob 2 = 2) on hf, under the same knob 9 setting:
     wsel / inv_norm / sel_src / sel_w equal bit for bit (ties included), out == ref.out.to(D) bit for bit;
  2. its kept edges are those of the default (table-path) fp32 forward on hf;
  3. grad_h == sngnn_agg_backward_topk(hf, gf, same wsel, same top_k).to(D) bit for bit, under the same knob 3;
  4. deterministic, no host synchronisation.
"""
import glob
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sngnn_amd import _lib, ops, synth
from sngnn_amd.graph import Graph
from tests.helpers import REGIMES, check_selection, oracle_aggregate, random_graph, regime_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.bfloat16, torch.float16)
KNOB_DEFAULTS = {2: 0, 3: 0, 9: 1}


class knobs:
    """sngnn_tuning_set for the duration of a block; restores the library's defaults."""

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            _lib.load().sngnn_tuning_set(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            _lib.load().sngnn_tuning_set(k, KNOB_DEFAULTS[k])


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}.get(a.dtype)
    return torch.equal(a.view(view), b.view(view)) if view else torch.equal(a, b)


def fwd(g, h, k, thr, sel=True):
    return ops.aggregate_forward(g, h, k, thr, save_for_backward=True, want_selection=sel and k is not None)


def check_contract(g, h, k, thr, what, bwd_modes=(0,)):
    """Contract items 1-3 for one graph / rows / top_k / thr; returns the half forward's results."""
    D = h.dtype
    hf = h.float()
    for fin in (0, 2):                                       # split rows finalized by a launch / in-launch (forced)
        with knobs(k9=fin):
            got = fwd(g, h, k, thr)
            with knobs(k2=2):
                ref = fwd(g, hf, k, thr)
        tag = f"{what} k9={fin}"
        assert got[0].dtype == D, tag
        assert bits_equal(got[0], ref[0].to(D)), f"{tag}: out != ref.out.to({D})"
        for name, a, b in zip(("wsel", "inv_norm", "sel_src", "sel_w"), got[1:], ref[1:]):
            assert bits_equal(a, b), f"{tag}: {name} differs from the fp32 on-the-fly forward"
    # 2. the same kept edges as the default (table-path) fp32 forward
    dflt = fwd(g, hf, k, thr)
    assert torch.equal(got[1] != _lib.UNSELECTED, dflt[1] != _lib.UNSELECTED), f"{what}: kept set != default path"
    if k is not None:
        assert torch.equal(got[3], dflt[3]), f"{what}: sel_src != default path"
    # 3. the gradient
    go = torch.randn(g.num_nodes, h.size(1), device=h.device).to(D)
    for mode in bwd_modes:
        with knobs(k3=mode):
            gh = ops.aggregate_backward(g, h, go, got[1], k)
            want = ops.aggregate_backward(g, hf, go.float(), got[1], k)
        assert gh.dtype == D
        assert bits_equal(gh, want.to(D)), f"{what} k3={mode}: grad_h != fp32 backward .to({D})"
    return got


@pytest.fixture(scope="module")
def graphs(cuda):
    """One graph per loop mode with every row class: split rows (> 128 in-edges: 700 and 300), wave rows
    (17 .. 128) and small rows."""
    n = 3000
    ei = random_graph(n, 15000, 11, hubs=((5, 700), (17, 300), (40, 90), (41, 60), (42, 33), (43, 20)))
    # a block of wave rows
    rng = np.random.default_rng(3)
    extra = [(int(s), int(t)) for t in range(100, 160) for s in rng.choice(n, size=int(rng.integers(17, 128)),
                                                                          replace=False)]
    ei = torch.unique(torch.cat([ei, torch.tensor(extra).t()], dim=1), dim=1)
    return {rem: Graph(ei.to(cuda), n, True, rem) for rem in (False, True)}, ei, n


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [5, 7, 40, 47, 64, 129])
def test_contract_grid(cuda, graphs, D, C):
    gs, _, n = graphs
    torch.manual_seed(C)
    h = torch.randn(n, C, device=cuda).to(D)
    h[200:260] = h[300:360]                                  # exact duplicate rows: exact ties
    cases = 0
    for rem, g in gs.items():
        for k in (None, 0, 1, 16, 200):
            for thr in (-1.5, 0.0, 0.9):
                if k is None and thr != 0.0:
                    continue                                 # (no selection: the threshold is not read)
                check_contract(g, h, k, thr, f"{D} C={C} rem={rem} k={k} thr={thr}",
                               bwd_modes=(0, 1, 2) if (k == 16 and thr == 0.0) else (0,))
                cases += 1
    print(f"{D} C={C}: {cases} cases bit for bit")


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [7, 40])
@pytest.mark.parametrize("kind", REGIMES)
def test_contract_on_the_regimes(cuda, graphs, D, C, kind):
    """The contract is bit for bit against the fp32 path, so it inherits that path's checks against the float64
    arbiter (tests/test_backward_regimes_gpu.py) only on the rows those checks ran on: the same five regimes,
    rounded to D.  In fp16 the ``tiny`` and ``near_eps`` rows become subnormals and zeros, and a row of out or
    grad_h may overflow: "the fp32 result rounded once" holds there as well (+-inf equals +-inf), so nothing
    is filtered out."""
    gs, _, n = graphs
    h = regime_inputs(n, C, kind)[0].to(cuda).to(D)
    for rem, g in gs.items():
        for k, thr in ((16, 0.0), (3, 0.3), (None, 0.0)):
            check_contract(g, h, k, thr, f"{D} {kind} C={C} rem={rem} k={k} thr={thr}", bwd_modes=(0, 1, 2))
    hf = h.float()
    print(f"{D} {kind} C={C}: {int((hf.abs().sum(1) == 0).sum())} zero rows, "
          f"{int(((hf != 0) & (hf.abs() < torch.finfo(D).tiny)).sum())} subnormal elements after rounding")


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
def test_tie_fixtures(cuda, D):
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "agg_ties_*.npz")))
    assert files
    for f in files:
        z = np.load(f)
        add, rem, k = (int(v) for v in z["params"])
        thr = float(z["thr"][0])
        h = torch.from_numpy(z["h"]).to(cuda).to(D)
        g = Graph(torch.from_numpy(z["edge_index"]).to(cuda), h.size(0), bool(add), bool(rem))
        hf = h.float()
        dup = h.size(0) - torch.unique(hf, dim=0).size(0)
        got = check_contract(g, h, k, thr, os.path.basename(f), bwd_modes=(0, 1))
        res = oracle_aggregate(hf.cpu(), torch.from_numpy(z["edge_index"]), bool(add), bool(rem), k, thr)
        near = check_selection(res, got[3], got[4], k, thr, strict=False, h=hf.cpu())
        print(f"{os.path.basename(f)} {D}: {dup} duplicate rows after rounding, {near} near-tie rows vs oracle")


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C,k,thr", [(40, 16, 0.0), (40, 16, 0.9), (5, 1, 0.0), (47, 3, -1.5)])
def test_selection_against_oracle(cuda, graphs, D, C, k, thr):
    gs, ei, n = graphs
    torch.manual_seed(100 + C)
    h = torch.randn(n, C, device=cuda).to(D)
    got = fwd(gs[True], h, k, thr)
    res = oracle_aggregate(h.float().cpu(), ei, True, True, k, thr)
    near = check_selection(res, got[3], got[4], k, thr, strict=False, h=h.float().cpu())
    assert near <= max(1, n // 100), near
    print(f"{D} C={C} k={k} thr={thr}: {near} near-tie rows vs oracle")


def test_config4_full_size_bf16(cuda):
    d = synth.make_dataset("arxiv")
    n = d.x.size(0)
    g = Graph(d.edge_index.to(cuda), n, True, True)
    torch.manual_seed(4)
    h = torch.randn(n, 40, device=cuda).to(torch.bfloat16)
    for thr in (0.0, 0.9):
        check_contract(g, h, 16, thr, f"config 4 thr={thr}", bwd_modes=(0,))
        for _ in range(3):
            fwd(g, h, 16, thr, sel=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fwd(g, h, 16, thr, sel=False)
        torch.cuda.synchronize()
        print(f"config 4 bf16 forward (top_k 16, thr {thr}): {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms "
              "per call (wall clock, 20 calls)")


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
def test_deterministic_and_no_sync(cuda, graphs, D):
    gs, _, n = graphs
    g = gs[True]
    h = torch.randn(n, 40, device=cuda).to(D)
    go = torch.randn(n, 40, device=cuda).to(D)
    a = fwd(g, h, 16, 0.0)
    ga = ops.aggregate_backward(g, h, go, a[1], 16)
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = fwd(g, h, 16, 0.0)
        gb = ops.aggregate_backward(g, h, go, b[1], 16)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for x, y in zip(a, b):
        assert bits_equal(x, y)
    assert bits_equal(ga, gb)


def test_half_refuses_fused_arguments(cuda, graphs):
    gs, _, n = graphs
    h = torch.randn(n, 40, device=cuda, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bfloat16"):
        ops.aggregate(h, gs[True], 16, 0.0, None, ops.HiddenEpilogue(True, 0.0, False),
                      torch.zeros(40, device=cuda, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="float32"):
        ops.aggregate_forward(gs[True], h.double(), 16, 0.0)


def _models(f, c, n):
    from sngnn_amd import SNGNN, SNGNN_Plus, SNGNN_Plus_Plus
    for layers in (1, 2):
        for bn in (False, True):
            yield f"SNGNN L{layers} bn={bn}", lambda: SNGNN(f, 32, c, layers, bn)
            yield (f"SNGNN_Plus L{layers} bn={bn}",
                   lambda: SNGNN_Plus(f, 32, c, n, layers, 16, 0.0, 1, 0.5, bn))
            yield (f"SNGNN_Plus_Plus L{layers} bn={bn}",
                   lambda: SNGNN_Plus_Plus(f, 32, c, n, layers, 16, 0.0, 0.3, 1, 0.5, bn))


@pytest.mark.parametrize("D", DTYPES, ids=["bf16", "fp16"])
def test_models_cast_to_half(cuda, D):
    """Each model trained 200 steps in fp32 (logits with the margins of a model in use: a fresh model's are
    nearly tied), then cast to D: output and gradients in D; in eval mode its arg-max against the same
    parameters upcast to fp32, on the same (rounded) features."""
    import copy
    from sngnn_amd import conv
    from sngnn_amd.train import train_step
    data = synth.make_dataset("chameleon")
    n, f, c = data.x.size(0), data.x.size(1), synth.num_classes("chameleon")
    dh = data.to(cuda)
    dh.x = dh.x.to(D)
    d32 = data.to(cuda)
    d32.x = dh.x.float()
    for name, make in _models(f, c, n):
        torch.manual_seed(7)
        m32 = make().to(cuda)
        opt = torch.optim.Adam(m32.parameters(), lr=0.01)
        for _ in range(200):
            train_step(m32, d32, opt)
        m = copy.deepcopy(m32).to(D)
        m32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
        m.train()
        out = m(dh)
        assert out.dtype == D, name
        loss = F.nll_loss(out[dh.train_mask].float(), dh.y[dh.train_mask])
        loss.backward()
        for pn, p in m.named_parameters():
            assert p.grad is not None and p.grad.dtype == D, (name, pn)
            assert bool(torch.isfinite(p.grad).all()), (name, pn)
        m.eval()
        m32.eval()
        with torch.no_grad():
            a = m(dh).float().argmax(1)
            b = m32(d32).argmax(1)
            agree = int((a == b).sum())
            if conv.HALF_PAD:                              # the padded rows give the unpadded form's bits
                conv.HALF_PAD = False
                try:
                    ref = m(dh)
                finally:
                    conv.HALF_PAD = True
                assert bits_equal(m(dh), ref), name
        print(f"{name} {D}: arg-max agrees with fp32 on {agree} of {n} nodes")
        assert agree >= 0.99 * n, (name, agree)


def test_training_bf16_matches_fp32(cuda):
    from sngnn_amd import SNGNN_Plus
    from sngnn_amd.train import train
    data = synth.make_dataset("chameleon")
    n, f, c = data.x.size(0), data.x.size(1), synth.num_classes("chameleon")
    torch.manual_seed(21)
    init = SNGNN_Plus(f, 64, c, n, 1, 10, 0.0, 1, 0.5).state_dict()
    accs = {}
    for D in (torch.float32, torch.bfloat16):
        torch.manual_seed(21)
        m = SNGNN_Plus(f, 64, c, n, 1, 10, 0.0, 1, 0.5)
        m.load_state_dict(init)
        m = m.to(cuda).to(D)
        d = data.to(cuda)
        d.x = d.x.to(D)
        opt = torch.optim.Adam(m.parameters(), lr=0.01, weight_decay=5e-4)
        accs[D] = train(m, d, opt, 100, 1000)["final_test_acc"]
    print(f"100 epochs, chameleon: final test accuracy fp32 {accs[torch.float32]:.4f}, "
          f"bf16 {accs[torch.bfloat16]:.4f}")
    assert abs(accs[torch.float32] - accs[torch.bfloat16]) <= 0.03


def test_refusals(cuda):
    from sngnn_amd import SNGNN_Plus, dist, splits
    from sngnn_amd.train import GraphedEpoch, train_graphed
    data = synth.make_dataset("chameleon", scale=0.25)
    n, f, c = data.x.size(0), data.x.size(1), synth.num_classes("chameleon")
    m = SNGNN_Plus(f, 32, c, n, 1, 10, 0.0, 1, 0.5).to(cuda).to(torch.bfloat16)
    d = data.to(cuda)
    d.x = d.x.to(torch.bfloat16)
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    with pytest.raises(TypeError, match="bfloat16"):
        GraphedEpoch(m, d, opt)
    with pytest.raises(TypeError, match="bfloat16"):
        train_graphed(m, d, opt, 2, 2)
    with pytest.raises(TypeError, match="bfloat16"):
        splits.ReplicaBatch(m, 2)
    with pytest.raises(TypeError, match="bfloat16"):
        splits.train_splits(None, d, None, None, 1, 1)
    with pytest.raises(TypeError, match="float16"):
        dist.check_features(torch.zeros(4, 4, dtype=torch.float16))

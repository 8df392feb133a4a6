"""GPU: the selections of the forward aggregation and of the kNN builder on lattice inputs (tests/lattice.py), against
the oracle with NO tolerance: either the selection is the reference's or it is not.

On lattice rows every cosine is an integer over the support in any summation order, so ties are plentiful - across
the cut, at cos == thr - and the right answer is fixed by the tie rule alone (the earlier edge position; the lower
node id).  tests/test_lattice_cpu.py asserts those premises, and that the cases below contain such rows in every
row class, without a GPU.  The Gaussian tests and their near-tie rule keep guarding the rounding behaviour, which
these inputs by construction do not exercise.

Nothing here uses a numeric tolerance.  Bit equality is relaxed in one place only:
  * a cosine of -0.0 (tests/lattice.py: the underflow rows, the all -0.0 row).  It orders like +0.0 and the kernels
    return +0.0 for it; the oracle's own zero carries whatever sign its summation leaves (a sum of -0.0 products
    is -0.0 in a serial loop and +0.0 from an accumulator that starts at +0.0).  The expected cosines are therefore
    canonicalised with ``+ 0.0`` before the bitwise comparison, and ``out`` is compared with ``torch.equal`` (-0.0 ==
    +0.0; every other value bit for bit).  No rounding step is involved.
"""
import numpy as np
import pytest
import torch

from tests import lattice as L
from tests.helpers import check_selection

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = {2: 0, 5: 0, 6: 0, 9: 1}


class knobs:
    """sngnn_tuning_set for the duration of a block; restores the library's defaults."""

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        from sngnn_amd import _lib
        for k, v in self.kv.items():
            assert _lib.load().sngnn_tuning_set(k, v) == 0, (k, v)

    def __exit__(self, *exc):
        from sngnn_amd import _lib
        for k in self.kv:
            _lib.load().sngnn_tuning_set(k, KNOB_DEFAULTS[k])


def same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def expected_sel_w(res):
    """[N, k] fp32: the oracle's cosine of every selected edge in rank order, +0.0 padded (and -0.0 -> +0.0)."""
    pos = res["sel_pos"]
    return torch.where(pos >= 0, res["s"][pos.clamp_min(0)], torch.zeros(())) + 0.0


def assert_forward_is_the_oracles(g, got, case, h, what, storage=torch.float32):
    """One launch's (out, wsel, inv_norm, sel_src, sel_w) against the oracle of ``case``, nothing tolerated."""
    from sngnn_amd import _lib
    name, n, c, k, t, rem, flags = case
    res, thr = L.forward_oracle(case), L.forward_inputs(case)[2]
    out, wsel, inv, sel_src, sel_w = (None if v is None else v.cpu() for v in got)
    assert g.num_edges == res["ei"].size(1), what
    assert check_selection(res, sel_src, sel_w, k, thr, strict=True) == 0, what
    assert same_bits(sel_w, expected_sel_w(res)), f"{what}: sel_w is not the oracle's cosine"
    # the saved weights mark exactly the oracle's kept edges, with their cosines
    eid = torch.from_numpy(g.array("eid").astype(np.int64))
    w_list = torch.full((g.num_edges,), float("nan"))
    w_list[eid] = wsel
    kept = torch.zeros(g.num_edges, dtype=torch.bool)
    kept[res["sel_pos"][res["sel_pos"] >= 0]] = True
    assert torch.equal(w_list != _lib.UNSELECTED, kept), f"{what}: wsel marks other edges than the oracle kept"
    assert same_bits(w_list[kept], res["s"][kept] + 0.0), f"{what}: wsel is not the oracle's cosine"
    assert out.dtype == storage and torch.equal(out, res["out"].to(storage)), f"{what}: out"
    assert same_bits(inv, 1.0 / h.float().norm(dim=1).clamp_min(1e-12)), f"{what}: inv_norm is not the exact reciprocal"


@pytest.mark.parametrize("case", L.FORWARD_CASES, ids=L.FORWARD_IDS)
def test_forward_fp32_selection_is_exactly_the_oracles(cuda, case):
    """Every lane layout (C), top_k regime, lattice threshold and loop mode; the default launch, the split rows'
    finalize as a launch of its own / inside the main launch (knob 9), and the on-the-fly scoring (knob 2 = 2)."""
    from sngnn_amd import ops
    from sngnn_amd.graph import Graph
    name, n, c, k, t, rem, flags = case
    h, ei, thr = L.forward_inputs(case)
    g = Graph(ei.to(cuda), n, True, rem)
    hg = h.to(cuda)
    for what, kv in (("default", {}), ("k9=0", dict(k9=0)), ("k9=2", dict(k9=2)), ("k2=2", dict(k2=2))):
        with knobs(**kv):
            got = ops.aggregate_forward(g, hg, k, thr, save_for_backward=True, want_selection=True)
            lean = ops.aggregate_forward(g, hg, k, thr)[0]
            torch.cuda.synchronize()
        assert_forward_is_the_oracles(g, got, case, h, f"{name} {what}")
        # the launch without the optional outputs gives the same bits
        assert same_bits(lean.cpu(), got[0].cpu()), f"{name} {what}: out without the optional outputs"
    assert same_bits(ops.aggregate(hg, g, k, thr).cpu(), got[0].cpu()), f"{name}: ops.aggregate"


@pytest.mark.parametrize("D", (torch.bfloat16, torch.float16), ids=("bf16", "fp16"))
@pytest.mark.parametrize("case", L.HALF_CASES, ids=L.HALF_IDS)
def test_forward_half_selection_is_exactly_the_fp32_oracles(cuda, case, D):
    """The half path on the same lattice rows (exact in bf16 and fp16): the fp32 oracle's selection and cosines, its
    ``out`` rounded to the storage type."""
    from sngnn_amd import ops
    from sngnn_amd.graph import Graph
    name, n, c, k, t, rem, flags = case
    h, ei, thr = L.forward_inputs(case)
    assert torch.equal(h.to(D).float(), h)
    g = Graph(ei.to(cuda), n, True, rem)
    hg = h.to(cuda).to(D)
    for what, kv in (("default", {}), ("k9=0", dict(k9=0)), ("k9=2", dict(k9=2))):
        with knobs(**kv):
            got = ops.aggregate_forward(g, hg, k, thr, save_for_backward=True, want_selection=True)
            torch.cuda.synchronize()
        assert_forward_is_the_oracles(g, got, case, h, f"{name} {D} {what}", storage=D)


def offset4(t, dev):
    """``t`` on the device with its base 4 bytes past a 16-byte boundary (tests/test_dense_regimes_gpu.py)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("case", L.KNN_CASES, ids=L.KNN_IDS)
def test_knn_graph_is_exactly_the_tie_rules(cuda, case):
    """``toolbox.knn_graph`` on staircases (one big tie group per level; ascending ids: every later column tile beats the
    list - park overflow, compaction and merges), lattice rows, identical rows, zero rows and the -0.0 pairs; every
    route (knob 6), both MFMA kinds on the fused route (knob 5), the unaligned base: ids and cosines exactly those
    of (cosine descending, node id ascending), the padding included."""
    from sngnn_amd import toolbox
    name, kind, n, f, k, excl, route, knob5, off = case
    x, _ = L.knn_rows(kind, n, f)
    want_idx, want_sim = L.knn_expected(kind, n, f, k, excl)
    xd = offset4(x, cuda) if off else x.to(cuda)
    assert xd.data_ptr() % 16 == off
    with knobs(k6=route, k5=knob5):
        idx, sim = toolbox.knn_graph(xd, k, exclude_self=excl)
        torch.cuda.synchronize()
    idx, sim = idx.cpu(), sim.cpu()
    bad = torch.nonzero((idx != want_idx).any(1)).flatten()
    assert bad.numel() == 0, (f"{name}: {bad.numel()} rows differ, first {int(bad[0])}: got {idx[bad[0]].tolist()} "
                              f"want {want_idx[bad[0]].tolist()}")
    assert torch.equal(idx, want_idx)
    assert same_bits(sim, want_sim), f"{name}: sim"

"""ops.h2gcn_conv (csrc/h2gcn.hip: sngnn_h2gcn_hop) per element against the float64 arbiter of tests/h2gcn_ref.py, with the
project's own gate (tests/arbiter.py): |got - float64| <= 4 max(K_ref, 2) 2^-24 MAG element by element, exactly 0 where MAG
is 0, no exemptions.  K_ref is the worst element of the reference's own op sequence in fp32 (two propagates with the
per-edge norm and a cat: h2gcn_ref.conv_torch on the CPU), measured here on the same inputs and printed in the summary.

The graph (h2gcn_ref.build_test_graph) is directed and asymmetric - a dinv taken from the out-degree, or a backward hop
on the CSR side, fails -, the in- and out-degrees of BOTH adjacencies each hit 1, 2, 16, 17, 128, 129 and 400 (every row
class on both sides of both), rows of A2 are empty, sources of its rows have dinv 0, and N % 64 != 0.  W = 1, 5, 6, 40, 47,
64, 128, 256, 512 and 514 (which the same call runs as the plain op sequence); fused and FUSE_H2GCN=False pass the same
gate.  The hop itself on interior column slices of wider tables: nothing outside the slice changes, and the result is
the dense call's bit for bit at every vector width."""
import ctypes
import functools

import pytest
import torch

from tests import arbiter as A
from tests import gpr_ref as R
from tests import h2gcn_ref as H
from tests import helpers

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 6, 40, 47, 64, 128, 256, 512, 514)
ROWS = ("gaussian", "logprob", "heavy")
OUTPUTS = ("out", "grad_x")


@functools.lru_cache(maxsize=None)
def _graph_cpu():
    ei, n, _ = H.build_test_graph()
    return ei, n


_ADJ = {}


def _adj(cuda):
    if "a" not in _ADJ:
        from sngnn_amd import ops
        ei, n = _graph_cpu()
        _ADJ["a"] = ops.H2Adjacency(ei.to(cuda), n)
    return _ADJ["a"]


@functools.lru_cache(maxsize=None)
def _case(w, rows):
    """Inputs, the float64 arbiter and the fp32 restatement's K_ref of one case (computed once, shared by the fused and
    the plain path)."""
    ei, n = _graph_cpu()
    gen = torch.Generator().manual_seed(1000 * w + len(rows))
    x, g = R.rows(rows, n, w, gen), R.rows(rows, n, 2 * w, gen)
    arb = H.conv_arbiter(ei, n, x, g)
    ref = H.conv_torch(ei, n, x, g)
    k_ref = {q: A.reference_units(ref[q], arb[q], arb["MAG_" + q], f"fp32 restatement {q}")[0] for q in OUTPUTS}
    return x, g, arb, k_ref


def _run(ops, adj, x, g):
    xg = x.clone().requires_grad_(True)
    out = ops.h2gcn_conv(xg, adj)
    out.backward(g)
    return dict(out=out.detach(), grad_x=xg.grad)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("w", WIDTHS)
def test_h2gcn_conv_against_float64(cuda, monkeypatch, w, fused):
    from sngnn_amd import h2gcn, ops
    monkeypatch.setattr(h2gcn, "FUSE_H2GCN", fused)
    adj = _adj(cuda)
    launches = []
    real_hop = h2gcn.hop
    monkeypatch.setattr(h2gcn, "hop", lambda *a, **k: (launches.append(1), real_hop(*a, **k))[1])
    worst_ref = {q: 0.0 for q in OUTPUTS}
    worst = dict(worst_ref)
    failures = []
    label = "fused" if fused else "plain"
    for rows in ROWS:
        x, g, arb, k_ref = _case(w, rows)
        del launches[:]
        got = _run(ops, adj, x.to(cuda), g.to(cuda))
        assert len(launches) == (2 if fused and w <= 512 else 0), (w, len(launches))
        assert got["out"].shape == (x.size(0), 2 * w) and got["grad_x"].shape == x.shape
        for q in OUTPUTS:
            assert got[q].dtype == torch.float32
            print(f"{label} W={w} {rows} {q}: K_ref {k_ref[q]:.2f}", end="")
            try:
                u, _ = A.check(got[q], arb[q], arb["MAG_" + q], k_ref[q], f"{label} W={w} {rows} {q}")
                print(f", kernel {u:.2f}")
                if u >= worst[q]:
                    worst[q], worst_ref[q] = u, k_ref[q]
            except AssertionError as ex:
                print(" FAILED")
                failures.append(str(ex))
    line = f"h2gcn conv {label} W={w}: " + ", ".join(f"{q} K_ref {worst_ref[q]:.2f} / kernel {worst[q]:.2f}" for q in worst) + \
        " (worst element, units of 2^-24 x MAG)"
    print(line)
    helpers.REPORT_LINES.append(line)
    assert not failures, "\n".join(failures)


def test_empty_rows_store_exact_zeros(cuda):
    """Rows without an entry (isolated nodes; rows of A2 emptied by the subtraction) are exact zeros on their side."""
    from sngnn_amd import ops
    import numpy as np
    adj = _adj(cuda)
    ei, n = _graph_cpu()
    x = torch.randn(n, 24, device=cuda)
    out = ops.h2gcn_conv(x, adj).cpu()
    src, tgt = H.a1_entries(ei)
    e2 = H.two_hop_ref(ei, n)
    empty1 = torch.from_numpy(np.bincount(tgt, minlength=n) == 0)
    empty2 = torch.from_numpy(np.bincount(e2[1], minlength=n) == 0)
    assert int(empty1.sum()) > 0 and int((empty2 & ~empty1).sum()) > 0
    assert bool((out[empty1][:, :24] == 0).all()) and bool((out[empty2][:, 24:] == 0).all())
    assert bool((out[~empty1][:, :24] != 0).any()) and bool((out[~empty2][:, 24:] != 0).any())


def _eval_norm(c, gen):
    """(running_mean, invstd, gamma, beta_bn) with running_var log-uniform over 1e-6 .. 1e4 (as test_gcn_gpu.py)."""
    rv = 10.0 ** (torch.rand(c, generator=gen) * 10.0 - 6.0)
    rv[0], rv[-1] = 1e-6, 1e4
    invstd = 1.0 / torch.sqrt(rv + 1e-5)
    return (torch.randn(c, generator=gen), invstd, 1.0 + 0.5 * torch.randn(c, generator=gen), 0.3 * torch.randn(c, generator=gen))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
def test_evaluation_epilogue(cuda, monkeypatch, fused):
    """(out - running_mean) * invstd * gamma + beta_bn on all 2W columns in the hop's stores (no relu), running_var from
    1e-6 to 1e4: against float64, and bit for bit against torch's arithmetic on the kernel's own hop."""
    from sngnn_amd import h2gcn, ops
    monkeypatch.setattr(h2gcn, "FUSE_H2GCN", fused)
    adj = _adj(cuda)
    ei, n = _graph_cpu()
    failures = []
    for w in (47, 64):
        x, _, _, _ = _case(w, "gaussian")
        en = _eval_norm(2 * w, torch.Generator().manual_seed(w))
        arb = H.conv_arbiter(ei, n, x, None, en)
        ref = H.eval_epilogue(H.conv_torch(ei, n, x)["out"], en)
        k_ref = A.reference_units(ref, arb["y"], arb["MAG_y"], "fp32 restatement y")[0]
        enc = tuple(t.to(cuda) for t in en)
        with torch.no_grad():
            got = ops.h2gcn_conv(x.to(cuda), adj, enc)
            bare = ops.h2gcn_conv(x.to(cuda), adj)
        assert float(got.min()) < 0.0          # no relu
        if fused:
            assert torch.equal(got, ((bare - enc[0]) * enc[1]) * enc[2] + enc[3])
        what = f"eval epilogue {'fused' if fused else 'plain'} W={w}"
        try:
            u, _ = A.check(got, arb["y"], arb["MAG_y"], k_ref, what)
            line = f"h2gcn {what}: K_ref {k_ref:.2f} / kernel {u:.2f}"
            print(line)
            helpers.REPORT_LINES.append(line)
        except AssertionError as ex:
            failures.append(str(ex))
    assert not failures, "\n".join(failures)
    xg = torch.randn(n, 8, device=cuda, requires_grad=True)
    v = torch.ones(16, device=cuda)
    with pytest.raises(ValueError, match="evaluation"):
        ops.h2gcn_conv(xg, adj, (v, v, v, v))
    with pytest.raises(ValueError, match="eval_norm"):
        ops.h2gcn_conv(xg.detach(), adj, (v, v, v))
    with pytest.raises(ValueError, match="eval_norm"):
        ops.h2gcn_conv(xg.detach(), adj, (v[:8], v[:8], v[:8], v[:8]))          # W elements, not 2W


SENTINEL = 0x7FC12345          # a NaN pattern: any read of it would poison a result, any write over it shows
SRC_SENTINEL = 3.0e38          # finite (lanes beyond the width load column 0 of the slice, never this)


def _wide(n, ld, cuda, value=None):
    t = torch.empty((n, ld), dtype=torch.float32, device=cuda)
    if value is None:
        t.view(torch.int32).fill_(SENTINEL)
    else:
        t.fill_(value)
    return t


def _outside_untouched(t, c0, c1):
    bits = t.view(torch.int32)
    return bool((bits[:, :c0] == SENTINEL).all()) and bool((bits[:, c1:] == SENTINEL).all())


@pytest.mark.parametrize("transpose", [False, True], ids=["csr", "csc"])
@pytest.mark.parametrize("off", [8, 6, 5], ids=["vec4", "vec2", "vec1"])
def test_slices_are_exact(cuda, off, transpose):
    """The hop on an interior column slice of wider source and destination tables whose other columns hold a sentinel:
    every destination column outside the slice keeps its bits, and the slice equals the dense-table call bit for bit -
    at offsets 8, 6 and 5 floats, which force vector widths 4, 2 and 1 on a 64-column hop."""
    from sngnn_amd import h2gcn
    adj = _adj(cuda)
    _, n = _graph_cpu()
    for w in (64, 47, 128):
        ws, wd = (2 * w, w) if transpose else (w, 2 * w)
        ld = 2 * w + 16
        gen = torch.Generator().manual_seed(w + off)
        x = R.rows("heavy", n, ws, gen).to(cuda)
        dense = torch.empty((n, wd), device=cuda)
        h2gcn.hop(adj, x, dense, transpose=transpose)
        src, dst = _wide(n, ld, cuda, SRC_SENTINEL), _wide(n, ld, cuda)
        src[:, off:off + ws] = x
        h2gcn.hop(adj, src[:, off:off + ws], dst[:, off:off + wd], transpose=transpose)
        assert _outside_untouched(dst, off, off + wd), (w, off)
        assert torch.equal(dst[:, off:off + wd], dense), (w, off)
        assert float(dense.abs().max()) > 0 and bool(torch.isfinite(dense).all())


def _raw_hop(lib, g1, g2, args, d1, d2, transpose, ws, stream):
    return lib.sngnn_h2gcn_hop(g1.handle, g2.handle, ctypes.byref(args), d1.data_ptr(), d2.data_ptr(), transpose,
                               ws.data_ptr(), ws.data_ptr(), stream)


def _args(src, dst, w):
    from sngnn_amd import _lib
    a = _lib.H2gcnHop()
    a.src, a.ld_src, a.dst, a.ld_dst, a.W = src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), w
    return a


def test_refusals_return_their_codes_and_launch_nothing(cuda):
    from sngnn_amd import _lib, ops
    from sngnn_amd.graph import LOOPS_REPLACE, Graph
    from sngnn_amd.prop import prop_dinv
    lib = _lib.load()
    adj = _adj(cuda)
    ei, n = _graph_cpu()
    x = torch.randn(n, 16, device=cuda)
    out = _wide(n, 32, cuda)
    table = _wide(n, 64, cuda)
    table[:, :16] = x
    before = table.clone()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=cuda)
    stream = _lib.stream(cuda)
    d1, d2 = adj.dinv1, adj.dinv2
    looped = Graph(ei.to(cuda), n, True, LOOPS_REPLACE)
    small = Graph(ei[:, (ei < n - 1).all(0)].to(cuda), n - 1, False, True)
    part = Graph(ei.to(cuda), n, False, True, row_range=(0, n // 2))
    with torch.cuda.device(cuda):
        ok = _args(x, out, 16)
        assert _raw_hop(lib, looped, adj.a2, ok, d1, d2, 0, ws, stream) == _lib.EINVAL
        assert b"loop-free" in lib.sngnn_last_error()
        assert _raw_hop(lib, adj.a1, looped, ok, d1, d2, 0, ws, stream) == _lib.EINVAL
        assert _raw_hop(lib, adj.a1, small, ok, d1, d2, 0, ws, stream) == _lib.EINVAL          # mismatched N
        assert _raw_hop(lib, part, adj.a2, ok, d1, d2, 0, ws, stream) == _lib.EINVAL           # a partition
        assert lib.sngnn_h2gcn_hop(None, adj.a2.handle, ctypes.byref(ok), d1.data_ptr(), d2.data_ptr(), 0, ws.data_ptr(),
                                   ws.data_ptr(), stream) == _lib.EINVAL
        assert lib.sngnn_h2gcn_hop(adj.a1.handle, adj.a2.handle, ctypes.byref(ok), None, d2.data_ptr(), 0, ws.data_ptr(),
                                   ws.data_ptr(), stream) == _lib.EINVAL
        for w in (0, 513):
            bad = _args(x, out, 16)
            bad.W = w
            assert _raw_hop(lib, adj.a1, adj.a2, bad, d1, d2, 0, ws, stream) == _lib.ERANGE
        # source and destination columns of one table overlap (0..16 and 8..40 of the same rows); in place
        assert _raw_hop(lib, adj.a1, adj.a2, _args(table[:, :16], table[:, 8:40], 16), d1, d2, 0, ws, stream) == _lib.EINVAL
        assert b"overlaps" in lib.sngnn_last_error()
        assert _raw_hop(lib, adj.a1, adj.a2, _args(table[:, :32], table[:, 16:32], 16), d1, d2, 1, ws, stream) == _lib.EINVAL
        one = _args(x, out, 16)
        one.rm = d1.data_ptr()
        assert _raw_hop(lib, adj.a1, adj.a2, one, d1, d2, 0, ws, stream) == _lib.EINVAL          # one norm pointer alone
        full = _args(table[:, :32], out[:, :16], 16)
        full.rm = full.invstd = full.gamma = full.beta_bn = d1.data_ptr()
        assert _raw_hop(lib, adj.a1, adj.a2, full, d1, d2, 1, ws, stream) == _lib.EINVAL         # a norm on the transpose
        # sngnn_h2gcn_dinv takes loop-free graphs only; sngnn_prop_dinv keeps refusing them
        assert lib.sngnn_h2gcn_dinv(looped.handle, d1.data_ptr(), stream) == _lib.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(table.view(torch.int32), before.view(torch.int32))
    assert bool((out.view(torch.int32) == SENTINEL).all())          # nothing was launched
    with pytest.raises(ValueError):
        prop_dinv(adj.a1)
    with pytest.raises(ValueError, match="GPU"):
        ops.h2gcn_conv(x.cpu(), adj)
    with pytest.raises(ValueError, match="shape"):
        ops.h2gcn_conv(x[:-1], adj)
    with pytest.raises(ValueError, match="GPU"):
        ops.H2Adjacency(ei, n)
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        ops.H2Adjacency(object(), n)
    # half rows run the plain op sequence (the gathers in fp32)
    h = ops.h2gcn_conv(x.half(), adj)
    assert h.dtype == torch.float16 and torch.allclose(h.float(), ops.h2gcn_conv(x, adj), atol=2e-2, rtol=2e-2)


def test_dinv_is_the_row_degree_on_both_sides(cuda):
    """dinv = in-degree^-1/2 of each adjacency, 0 for an empty row (never the out-degree)."""
    import numpy as np
    adj = _adj(cuda)
    ei, n = _graph_cpu()
    _, tgt = H.a1_entries(ei)
    e2 = H.two_hop_ref(ei, n)
    for dinv, t in ((adj.dinv1, tgt), (adj.dinv2, e2[1])):
        deg = np.bincount(t, minlength=n).astype(np.float64)
        want = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
        got = dinv.cpu().numpy().astype(np.float64)
        assert np.array_equal(got == 0, deg == 0)
        assert float(np.abs(got - want).max()) <= 2.0 ** -24


def test_two_calls_are_bit_identical_and_nothing_synchronises(cuda, monkeypatch):
    from sngnn_amd import h2gcn, ops
    monkeypatch.setattr(h2gcn, "FUSE_H2GCN", True)
    adj = _adj(cuda)
    x, g, _, _ = _case(47, "heavy")
    xc, gc = x.to(cuda), g.to(cuda)
    a = _run(ops, adj, xc, gc)          # (builds the workspaces)
    scratch = torch.full((300_000,), 3.0, device=cuda)          # other work in between
    del scratch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = _run(ops, adj, xc, gc)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for q in OUTPUTS:
        assert torch.equal(a[q], b[q]), q
        assert float(a[q].abs().max()) > 0

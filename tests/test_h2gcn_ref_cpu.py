"""CPU: the H2GCN references of tests/h2gcn_ref.py against independent restatements - the two-hop pattern against a
brute-force triple loop, dense boolean matrices and (where scipy imports) the reference's own A @ A route; the float64
arbiter against dense normalised matrices; the test graph's degree classes and strategy rows; the reference-default
embed's exact zeros; the constants the Python side exports against the header."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import h2gcn_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(ei, n):
    src, tgt = H.a1_entries(ei)
    a = [[False] * n for _ in range(n)]
    for s, t in zip(src, tgt):
        a[t][s] = True
    out = []
    for i in range(n):
        for k in range(n):
            if k == i or a[i][k]:
                continue
            if any(a[i][j] and a[j][k] for j in range(n)):
                out.append((k, i))
    return np.array(out, np.int64).reshape(-1, 2).T


def _tiny(seed, n, e):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=gen)
    return torch.cat([ei, ei[:, :e // 4]], dim=1)          # duplicates; loops come with the draw


@pytest.mark.parametrize("seed,n,e", [(1, 7, 12), (2, 13, 40), (3, 20, 30), (4, 5, 25), (5, 9, 0)])
def test_two_hop_ref_against_a_triple_loop(seed, n, e):
    ei = _tiny(seed, n, e)
    want = _brute(ei, n)
    got = H.two_hop_ref(ei, n)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(H.two_hop_dense(ei, n), want)


def test_two_hop_ref_small_cases():
    assert H.two_hop_ref(torch.tensor([[0, 1], [1, 0]]), 2).shape == (2, 0)                    # diagonal candidates only
    assert H.two_hop_ref(torch.tensor([[0, 1, 0], [1, 2, 2]]), 3).shape == (2, 0)              # the candidate is an edge
    assert np.array_equal(H.two_hop_ref(torch.tensor([[0, 1], [1, 2]]), 3), np.array([[0], [2]]))
    assert H.two_hop_ref(torch.tensor([[0, 1, 2], [0, 1, 2]]), 3).shape == (2, 0)              # loops only


def test_two_hop_ref_against_the_scipy_route():
    sp = pytest.importorskip("scipy.sparse")
    ei, n, _ = H.build_test_graph()
    src, tgt = H.a1_entries(ei)
    a = sp.csr_matrix((np.ones(src.size), (tgt, src)), shape=(n, n))          # duplicates summed, as to_scipy does
    a2 = sp.csr_matrix(a @ a)
    a2.data[:] = 1.0          # (torch_sparse's product of two value-less tensors is a pattern: to_scipy fills in ones)
    a2.setdiag(0)
    a2 = a2 - a
    a2.data[:] = np.where(a2.data > 0, 1.0, 0.0)
    a2.eliminate_zeros()
    coo = a2.tocoo()
    order = np.lexsort((coo.col, coo.row))
    want = np.stack([coo.col[order], coo.row[order]]).astype(np.int64)
    assert np.array_equal(H.two_hop_ref(ei, n), want)


def test_the_arbiter_against_dense_matrices():
    ei, n, _ = H.build_test_graph(hash_max=40)
    src, tgt = H.a1_entries(ei)
    e2 = H.two_hop_ref(ei, n)
    m1, m2 = H.dense_normalised(src, tgt, n), H.dense_normalised(e2[0], e2[1], n)
    gen = torch.Generator().manual_seed(3)
    x, g = torch.randn(n, 5, generator=gen), torch.randn(n, 10, generator=gen)
    arb = H.conv_arbiter(ei, n, x, g)
    xd, gd = x.double().numpy(), g.double().numpy()
    want = np.concatenate([m1 @ xd, m2 @ xd], axis=1)
    mag = np.concatenate([m1 @ np.abs(xd), m2 @ np.abs(xd)], axis=1)
    gx = m1.T @ gd[:, :5] + m2.T @ gd[:, 5:]
    assert np.allclose(arb["out"].numpy(), want, rtol=1e-12, atol=1e-13)
    assert np.allclose(arb["MAG_out"].numpy(), mag, rtol=1e-12, atol=1e-13)
    assert np.allclose(arb["grad_x"].numpy(), gx, rtol=1e-12, atol=1e-13)
    # the fp32 op sequence through autograd says the same to fp32 accuracy, and its gradient is the transpose
    ref = H.conv_torch(ei, n, x, g)
    assert np.allclose(ref["out"].numpy(), want, rtol=1e-4, atol=1e-5)
    assert np.allclose(ref["grad_x"].numpy(), gx, rtol=1e-4, atol=1e-5)
    # the graph is directed: the out-degree normalisation is a different matrix
    assert not np.allclose(m1, m1.T)


def test_the_test_graph_hits_every_class():
    from sngnn_amd import h2gcn
    ei, n, info = H.build_test_graph(h2gcn.TWO_HOP_HASH_MAX)
    assert n % 64 != 0 and n < 4000
    src, tgt = H.a1_entries(ei)
    e2 = H.two_hop_ref(ei, n)
    in1, out1 = np.bincount(tgt, minlength=n), np.bincount(src, minlength=n)
    in2, out2 = np.bincount(e2[1], minlength=n), np.bincount(e2[0], minlength=n)
    for d in H.GADGET_DEGREES:
        assert in2[info["a2_in"][d]] == d and out2[info["a2_out"][d]] == d
        assert in1[info["a1_in"][d]] == d and out1[info["a1_out"][d]] == d
    cb = H.candidate_bound(ei, n)
    hm = h2gcn.TWO_HOP_HASH_MAX
    assert cb[info["hash_row"]] == hm and cb[info["above_row"]] == hm + 1 and cb[info["bitmap_row"]] == hm + 2
    assert in2[info["hash_row"]] == hm - 2          # the pool's h - 1 less the direct neighbour K_1 (the row itself never counts)
    assert in2[info["above_row"]] == hm + 1
    assert in2[info["bitmap_row"]] == hm            # h - 1 + {63, 64} less K_0
    rows_b = set(e2[0][e2[1] == info["bitmap_row"]].tolist())
    assert {63, 64} <= rows_b and info["bitmap_row"] not in rows_b and info["pool"][0] not in rows_b
    assert set(e2[0][e2[1] == info["table_63_64"]].tolist()) == {63, 64}
    a, b = info["two_cycle"]
    assert in2[a] == 0 and in2[b] == 0 and in1[a] == 1
    assert in2[info["triangle"][2]] == 0
    # rows of A2 emptied by the subtraction although A1's row is not; isolated nodes; duplicates and loops in the list
    assert int(((in2 == 0) & (cb > 0)).sum()) > 0 and int(((in1 == 0) & (out1 == 0)).sum()) > 0
    assert int((ei[0] == ei[1]).sum()) > 0
    assert np.unique(tgt * n + src).size < src.size
    # sources of dinv 0 inside rows of both adjacencies (multiplied, never skipped)
    assert int((in1[src] == 0).sum()) > 0 and int((in2[e2[0]] == 0).sum()) > 0


def test_relu_of_log_softmax_is_exactly_zero():
    """The reference-default embed: MLP.forward ends in log_softmax, H2GCN.forward applies relu next - exact zeros, and
    exactly zero gradients into the embed."""
    gen = torch.Generator().manual_seed(0)
    for scale in (1e-3, 1.0, 50.0):
        z = (scale * torch.randn(300, 7, generator=gen)).requires_grad_(True)
        y = F.relu(F.log_softmax(z, dim=1))
        assert bool((y == 0).all())
        (y * torch.randn(300, 7, generator=gen)).sum().backward()
        assert bool((z.grad == 0).all())
    one = torch.zeros(4, 1, requires_grad=True)          # a single class: log_softmax is exactly 0, relu'(0) = 0
    y = F.relu(F.log_softmax(one, dim=1))
    y.sum().backward()
    assert bool((y == 0).all()) and bool((one.grad == 0).all())


def test_constants_match_the_header():
    from sngnn_amd import _lib, h2gcn
    text = open(os.path.join(ROOT, "include", "sngnn_hip.h")).read()
    m = re.search(r"#define SNGNN_TWO_HOP_HASH_MAX (\d+)", text)
    assert m and int(m.group(1)) == _lib.TWO_HOP_HASH_MAX == h2gcn.TWO_HOP_HASH_MAX
    assert h2gcn.MAX_WIDTH == _lib.MAX_CHANNELS


def test_hop_struct_layout_matches_the_header(tmp_path):
    import ctypes as C
    import shutil
    import subprocess
    from sngnn_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [name for name, _ in _lib.H2gcnHop._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sngnn_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(sngnn_h2gcn_hop_t));']
    lines += [f'  printf("{f} %zu\\n", offsetof(sngnn_h2gcn_hop_t, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(_lib.H2gcnHop)
    for f in fields:
        assert int(out[f]) == getattr(_lib.H2gcnHop, f).offset, f


def test_no_cpu_path_and_the_constructor_contract():
    from sngnn_amd import H2GCN, H2GCNConv, ops
    ei = torch.randint(0, 10, (2, 20))
    with pytest.raises(ValueError, match="GPU"):
        H2GCN(4, 8, 3, ei, 10)
    with pytest.raises(ValueError, match="GPU"):
        ops.two_hop_edge_index(ei, 10)
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        H2GCN(4, 8, 3, object(), 10)
    assert list(H2GCNConv().state_dict()) == []

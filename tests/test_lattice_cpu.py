"""CPU: the premises of the exact selection tests (tests/test_exact_selection_gpu.py), asserted for every case that
file runs - so that "bit-equal to the oracle" there is a statement about the kernels and not about the inputs.

  * Exactness: every oracle cosine of a forward case is an integer over the support (the underflow rows' edges: an
    integer times 2^-80 / sqrt(s), or +-0.0), and the oracle's ``out`` is bit-equal to the exact sum divided once.
  * Oracle agreement: the Python oracle (torch's amax restatement of scatter_max) and the serial-loop C oracle agree
    exactly - sel_src, sel_pos, the cosines and out - on every case.  That includes both kinds of -0.0 rows: torch's
    ``src == out[index]`` compares floats, so -0.0 and +0.0 tie and the earlier position wins, as in the C loop's
    strict ``>``.  No row had to be left out of the forward cases.
  * Coverage: every case has a row with a tie ACROSS the cut and a row with an in-edge at cos == thr; each row class
    (small / wave / split) has a cut-tie row; a split row of >= 13 tasks of 128 edges exists; the planted -0.0
    edges sit in front of +0.0 ones with the cut between them.
  * kNN: ``knn_exact`` against a brute-force float64 ranking, and the -0.0 pairs really are -0.0 in fp32.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lattice as L


def test_lattice_rows_are_lattice_rows():
    for c in (1, 3, 4, 7, 16, 47, 64, 130, 512):
        h = L.lattice_rows(360, c, seed=c)
        s = L.support(c)
        live = [r for r in range(360) if r not in L.ZERO_ROWS]
        assert ((h[live] != 0).sum(1) == s).all() and (h[list(L.ZERO_ROWS)] == 0).all()
        mag = h[live].abs().amax(1)
        assert ((h[live] == 0) | (h[live].abs() == mag[:, None])).all()
        assert set(torch.log2(mag).tolist()) <= set(range(-3, 4)) and len(set(mag.tolist())) > 1
        # the reciprocal norm is exact
        assert torch.equal(1.0 / h[live].norm(dim=1), 1.0 / (s ** 0.5 * mag))
        for D in (torch.bfloat16, torch.float16):
            assert torch.equal(h.to(D).float(), h)
    assert (L.lattice_rows(50, 7, 1, scale=False).abs().amax(1)[:40] == 1).all()
    assert np.float32(L.TINY) / np.float32(1e-12) == np.float32(2.0 ** -80) and np.float32(L.TINY) ** 2 == 0


@pytest.mark.parametrize("case", L.FORWARD_CASES, ids=L.FORWARD_IDS)
def test_forward_case_is_exact_and_the_oracles_agree(case):
    from oracle import c_oracle as CO
    name, n, c, k, t, rem, flags = case
    h, ei, thr = L.forward_inputs(case)
    res = L.forward_oracle(case)
    s_sup = L.support(c)
    # cosines on the lattice
    tiny = torch.zeros(n, dtype=torch.bool)
    if "u" in flags:
        tiny[[L.TINY_NEG] + list(L.TINY_POS)] = True
    on_tiny = tiny[res["ei"][0]] | tiny[res["ei"][1]]
    d = res["s"].double() * s_sup
    assert (d[~on_tiny] == d[~on_tiny].round()).all() and d[~on_tiny].abs().max() <= s_sup
    both = tiny[res["ei"][0]] & tiny[res["ei"][1]]
    assert (res["s"][both] == 0).all()
    dt = res["s"][on_tiny & ~both].double() * 2.0 ** 80 * s_sup ** 0.5
    assert (dt == dt.round()).all()
    # out: the exact sum, divided once
    assert torch.equal(res["out"], L.exact_out(h, res))
    want_inv = 1.0 / h.norm(dim=1).clamp_min(1e-12)
    assert torch.equal(want_inv, (1.0 / h.double().norm(dim=1).clamp_min(float(np.float32(1e-12)))).float())
    # the C oracle: the same bits
    cres = CO.aggregate(h.numpy(), ei.numpy(), add_loops=True, remove_loops=rem, top_k=k, thr=thr)
    assert np.array_equal(cres["ei"], res["ei"].numpy())
    assert np.array_equal(cres["s"], res["s"].numpy())                      # (-0.0 == +0.0)
    assert np.array_equal(cres["sel_src"], res["sel_src"].numpy())
    assert np.array_equal(cres["sel_pos"], res["sel_pos"].numpy())
    assert np.array_equal(cres["out"], res["out"].numpy())
    # coverage: a tie across the cut and an edge at cos == thr
    cut_tie, at_thr = L.cut_facts(res, n, k, thr)
    assert cut_tie.any(), f"{name}: no row with a tie across the cut"
    assert at_thr.any(), f"{name}: no in-edge with cos == thr"
    if "u" in flags:
        # the planted rows: the edge from TINY_NEG comes first, scores a zero (the oracle's sum of -0.0 products) and
        # is kept; the cut falls among the zeros behind it
        for tgt in L.TINY_POS[:2]:
            pos = torch.nonzero(res["ei"][1] == tgt).flatten()
            assert int(res["ei"][0][pos[0]]) == L.TINY_NEG and (res["s"][pos] == 0).all() and pos.numel() > k
            assert res["sel_pos"][tgt].tolist()[:k] == pos[:k].tolist() and cut_tie[tgt]
        unit = F.normalize(h, dim=-1)
        prod = unit[L.TINY_NEG] * unit[L.TINY_POS[0]]
        assert (prod == 0).all() and torch.signbit(prod).all()               # every product is -0.0


def test_forward_cases_cover_every_row_class():
    seen = {"small": 0, "wave": 0, "split": 0}
    neg_zero_classes = set()
    tasks = 0
    for case in L.FORWARD_CASES:
        name, n, c, k, t, rem, flags = case
        res = L.forward_oracle(case)
        deg, classes = L.row_classes_of(res, n)
        cut_tie, _ = L.cut_facts(res, n, k, L.forward_inputs(case)[2])
        for cls, m in classes.items():
            seen[cls] += int((m & cut_tie).sum())
        split_tie = classes["split"] & cut_tie
        if split_tie.any():
            tasks = max(tasks, int(-(-deg[split_tie].max() // 128)))
        if "u" in flags:
            neg_zero_classes |= {cls for cls, m in classes.items() for tgt in L.TINY_POS[:2] if m[tgt]}
    assert all(v > 0 for v in seen.values()), seen
    assert tasks >= 13, f"largest split row with a cut tie has {tasks} tasks"
    assert neg_zero_classes == {"small", "wave"}
    # every case of the half path is a forward case of its own: the premises above hold for it
    assert set(L.HALF_CASES) <= set(L.FORWARD_CASES)
    assert not any("u" in c[6] for c in L.HALF_CASES)


def _brute_knn(x, k, excl):
    xn = F.normalize(x.double(), dim=1)
    S = xn @ xn.t()
    n = x.size(0)
    rows = []
    for i in range(n):
        cand = [j for j in range(n) if not (excl and j == i)]
        cand.sort(key=lambda j: (-round(float(S[i, j]) * 64), j))            # cosines are multiples of 1/64 at most
        rows.append(cand[:k] + [-1] * (k - len(cand[:k])))
    return torch.tensor(rows)


@pytest.mark.parametrize("kind,n,f", [("asc", 60, 16), ("desc", 60, 20), ("shuffled", 75, 33), ("lattice", 70, 40),
                                      ("identical", 9, 16), ("zero", 6, 16), ("negzero", 40, 32), ("zeropair", 40, 16),
                                      ("lattice", 5, 64)])
def test_knn_exact_against_brute_force(kind, n, f):
    x, lat = L.knn_rows(kind, n, f)
    for k, excl in ((1, True), (7, True), (7, False)):
        idx, sim = L.knn_exact(lat, k, excl)
        assert torch.equal(idx, _brute_knn(lat, k, excl))
        S32 = F.normalize(lat, dim=1) @ F.normalize(lat, dim=1).t()
        got = torch.where(idx >= 0, S32.gather(1, idx.clamp_min(0)), torch.zeros(()))
        assert torch.equal(sim, got)
        # the rows the kernel sees score the same floats as the lattice they stand for (-0.0 == +0.0)
        Sx = F.normalize(x, dim=1) @ F.normalize(x, dim=1).t()
        assert torch.equal(Sx, S32)


def test_knn_staircase_dot_products():
    x = L.staircase_rows(170, 16).double()
    a = (torch.arange(170) * 17) // 170
    assert torch.equal(x @ x.t(), (16 - 2 * (a[:, None] - a[None, :]).abs()).double())
    assert set(a.tolist()) == set(range(17))
    d = L.staircase_rows(170, 16, False)
    assert torch.equal(d, L.staircase_rows(170, 16).flip(0))
    sh = L.staircase_rows(170, 16, "shuffled", seed=3)
    assert not torch.equal(sh, x.float()) and torch.equal(sh.sum(1).sort().values, x.float().sum(1).sort().values)


def test_the_negative_zero_pairs_are_negative_zero():
    """What the kernels compute: the kNN builder's scaled dot product and the forward's unit-row products."""
    x, _ = L.underflow_pair_rows(40, 32, 1)
    acc = (x[0] * x[1]).sum()
    inv = 1.0 / x.norm(dim=1)
    assert float(acc) == -(2.0 ** -80) and float(inv[0]) == 2.0 ** -40 == float(inv[1])
    cos = acc * (inv[0] * inv[1])
    assert float(cos) == 0.0 and bool(torch.signbit(cos))
    assert ((x[:2] @ x[2:].t()) == 0).all()
    h = L.lattice_rows(360, 64, 1, neg_zero_rows=True)
    prod = F.normalize(h, dim=-1)[L.NEG_ZERO_PAIR[0]] * F.normalize(h, dim=-1)[L.NEG_ZERO_PAIR[1]]
    assert (prod == 0).all() and torch.signbit(prod).all()


def test_knn_cases_reach_the_branches():
    """Shapes of the kNN cases against the builder's launch arithmetic (csrc/knn.hip): column splits so that
    k_knn_merge takes several rounds at k = 32 ((128 - k) / k = 3 splits per round), every feature width class, every
    route, both MFMA kinds, the unaligned base."""
    def splits(n, rows):
        nrb = -(-n // rows)
        ns = max(1, min(nrb, -(-320 // nrb)))
        nct = -(-n // (64 if rows == 256 else 128))
        tps = -(-nct // ns)
        return -(-nct // tps)
    assert splits(2304, 256) > 2 * 3 and splits(2304, 128) > 2 * 3
    kinds = {c[1] for c in L.KNN_CASES}
    assert kinds == {"asc", "desc", "shuffled", "lattice", "identical", "zero", "negzero", "zeropair"}
    assert {c[2] for c in L.KNN_CASES} == {5, 130, 513, 1030, 2304}
    assert {c[3] for c in L.KNN_CASES} == {16, 32, 51, 64, 96, 128, 200}
    assert {c[4] for c in L.KNN_CASES} == {1, 7, 16, 31, 32}
    assert {c[5] for c in L.KNN_CASES} == {True, False}
    assert {c[6] for c in L.KNN_CASES} == {0, 1, 2, 3, 4}
    assert {c[7] for c in L.KNN_CASES if c[6] == 1} == {0, 1}
    assert any(c[8] == 4 for c in L.KNN_CASES)
    for kind in ("asc", "negzero"):
        assert {c[6] for c in L.KNN_CASES if c[1] == kind} == {0, 1, 2, 3, 4}

"""Shared helpers of the parity tests (oracle = checker only)."""
from __future__ import annotations

import numpy as np
import torch

from oracle import sngnn_oracle as O

RTOL = 1e-5          # north_star: aggregated features within 1e-5 rtol
ATOL = 2e-6          # absolute floor for entries that cancel to ~0 (|h| ~ 1, fp32)
# A "near tie": two cosines (or a cosine and thr) whose ORDER depends on the summation order of
# whoever computes them (torch's vectorised CPU sum, a serial C loop and the kernel's lane order
# all differ in the last bits).  BASELINE.md's gate: every mismatch must be a <= 2-ulp near tie and
# the count is reported.  The unit is the fp32 ulp at the scale of the operands - a cosine is a sum
# of products of UNIT rows, so its rounding error is in ulps of 1.0 (2^-23) whatever the sum
# cancels to (a cosine of 1e-9 against thr = 0 is a near tie, although it is 1e7 of its own ulps).
# Every row that needed the rule is logged with the gap it needed (NEAR_TIE_GAPS, printed in the
# pytest summary: count, maximum in ulps), so the gate is a measured quantity, not a tolerance
# things hide in.  Round 3 allowed 6e-7 (5 ulps); the measured maximum is what justifies the 2.
ULP32 = 2.0 ** -23
TIE_ULPS = 2.0
TIE_TOL = TIE_ULPS * ULP32          # 2.38e-7
NEAR_TIE_GAPS = []                  # gap (absolute) each tolerated row needed, over all tests of the run


def random_graph(n, e, seed, hubs=()):
    """Random directed multigraph-free edge list sorted by (src, dst); ``hubs`` is a
    list of (node, in_degree) forced hubs."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=e)
    dst = rng.integers(0, n, size=e)
    for node, deg in hubs:
        s = rng.choice(n, size=min(deg, n), replace=False)
        src = np.concatenate([src, s])
        dst = np.concatenate([dst, np.full(s.size, node)])
    key = np.unique(src.astype(np.int64) * n + dst)
    return torch.from_numpy(np.stack([key // n, key % n]))


REGIMES = ("normal", "parallel", "sparse", "tiny", "near_eps")


def regime_rows(n, c, seed, kind):
    """Feature rows of the regimes a kernel meets: ``normal`` randn; ``parallel`` nearly parallel rows (every
    cosine within 1e-3 of 1: a deep layer's input); ``tiny`` a 1e-30 .. 1 channel range; ``near_eps`` unit rows
    scaled by 10 ** U(-15, -9) - norms on both sides of F.normalize's 1e-12 clamp while every square stays a
    normal fp32 number - with every third row plain randn; ``sparse`` post-ReLU rows with exact zeros and whole
    zero rows.  Always h[5] == h[6] (an exact tie) and h[9] == 0."""
    assert kind in REGIMES, kind
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        h = torch.randn(n, c, generator=g)
    elif kind == "parallel":           # nearly parallel rows: every cosine within 1e-3 of 1
        h = torch.randn(1, c, generator=g) + 1e-2 * torch.randn(n, c, generator=g)
    elif kind == "tiny":               # components far below fp16's range before the scaling
        h = torch.randn(n, c, generator=g) * torch.logspace(-30, 0, c).view(1, -1)
    elif kind == "near_eps":
        h = torch.nn.functional.normalize(torch.randn(n, c, generator=g), dim=1)
        h = h * 10.0 ** (torch.rand(n, 1, generator=g) * 6 - 15)
        h[::3] = torch.randn(n, c, generator=g)[::3]
    else:                              # sparse non-negative (bag-of-words after a ReLU)
        h = torch.relu(torch.randn(n, c, generator=g) - 1.0)
    h[5] = h[6]
    h[9] = 0.0
    return h


def regime_inputs(n, c, kind):
    """(h, gout) of one backward-regime case: regime_rows + a power-of-two multiple of the tied row."""
    h = regime_rows(n, c, 7 + c, kind)
    h[7] = 2 * h[6]
    gout = torch.randn(n, c, generator=torch.Generator().manual_seed(1000 + c))
    return h, gout


SIGNED_REGIMES = REGIMES + ("antiparallel", "lattice")
SIGNED_C2 = ((0.5, -0.3), (0.0, 0.7), (-1.25, -1.25))      # (c_pos, c_neg): mixed signs, a dead branch, equal and negative
LATTICE_MIN_SHARE = 0.03


def signed_coef(e, seed):
    """a_e of the signed-attention tests: signed, randn x 10 ** U(-3, 1), every 17th entry exactly 0 (the kernel takes
    any float; the model's own coef is positive)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(e, generator=g) * 10.0 ** (torch.rand(e, generator=g) * 4 - 3)
    a[::17] = 0.0
    return a


def signed_inputs(n, c, kind):
    """(h, gout, coef_of, c2 cases) of one signed-attention case; ``coef_of(E)`` gives a_e for a graph of E edges.
    The five REGIMES: regime_inputs unchanged.  ``antiparallel``: the ``parallel`` rows times a random +-1 per row -
    every cosine within 1e-3 of +1 or of -1, about half the edges on each side - with h[7] = -2 h[6], an exact
    anti-tie.  ``lattice``: rows of integers in {-1, 0, 1} (``LATTICE_VALUES``) times a power of two in
    2^-20 .. 2^20 per row: every partial sum of a raw dot product is exact in fp32 in any order, and many pairs
    have a cosine of exactly 0 on overlapping supports (S_e > 0): kappa's third branch."""
    assert kind in SIGNED_REGIMES, kind
    if kind in REGIMES:
        h, gout = regime_inputs(n, c, kind)
    else:
        g = torch.Generator().manual_seed(7 + c)
        if kind == "antiparallel":
            h = regime_rows(n, c, 7 + c, "parallel")
            h = h * (torch.randint(0, 2, (n, 1), generator=g) * 2 - 1).float()
            h[5] = h[6]
            h[7] = -2 * h[6]
        else:
            lo, hi = LATTICE_VALUES
            h = torch.randint(lo, hi + 1, (n, c), generator=g).float() * 2.0 ** torch.randint(-20, 21, (n, 1), generator=g).float()
            h[5] = h[6]
            h[7] = 2 * h[6]
        h[9] = 0.0
        gout = torch.randn(n, c, generator=torch.Generator().manual_seed(1000 + c))
    return h, gout, (lambda e: signed_coef(e, 2000 + c)), SIGNED_C2


LATTICE_VALUES = (-1, 1)


def lattice_zero_share(h, rowptr, col, row_offset=0):
    """Share of the CSR edges whose float64 cosine is exactly 0 although the two rows' supports overlap."""
    rowptr, col = torch.as_tensor(np.asarray(rowptr)).long(), torch.as_tensor(np.asarray(col)).long()
    dst = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr.diff()) + row_offset
    h64 = h.double()
    d, dabs = (h64[dst] * h64[col]).sum(1), (h64[dst].abs() * h64[col].abs()).sum(1)
    return float(((d == 0) & (dabs > 0)).double().mean())


def assert_lattice_share(h, rowptr, col, row_offset=0):
    share = lattice_zero_share(h, rowptr, col, row_offset)
    assert share >= LATTICE_MIN_SHARE, f"lattice C={h.size(1)}: only {share:.2%} of the edges have s == 0 with S > 0"
    return share


def adj_with_diagonal(ei, n):
    """Edge list (source, target) of ``ei`` without its loops plus every node's own: the pattern of a normalised
    adjacency with self-loops, which GGCNlayer_SP's plain branch propagates over (diagonal kept)."""
    ei = ei[:, ei[0] != ei[1]]
    return torch.unique(torch.cat([ei, torch.arange(n).repeat(2, 1)], 1), dim=1)


def oracle_signed_fixed(h, rowptr, col, coef, c2, sign, gout, row_offset=0, eps=1e-12):
    """The signed attention from the oracle's own blocks in h's dtype, the sign of every edge FIXED: F.normalize,
    O.edge_cosine, relu(s) / -relu(-s) (both 0 where ``sign`` is 0), index_add_ in edge order, autograd for the
    gradients of <out, gout>.  Keys as arbiter.signed: out, s, grad, u, grad_coef, grad_c2."""
    rowptr, col = torch.as_tensor(np.asarray(rowptr)).long(), torch.as_tensor(np.asarray(col)).long()
    n = rowptr.numel() - 1
    dst = torch.repeat_interleave(torch.arange(n), rowptr.diff())
    live = torch.as_tensor(np.asarray(sign)).long() != 0
    h = h.detach().clone().requires_grad_(True)
    coef = torch.as_tensor(coef).detach().to(h.dtype).clone().requires_grad_(True)
    c2 = torch.as_tensor(c2).detach().to(h.dtype).clone().requires_grad_(True)
    gout = gout.to(h.dtype)
    s = O.edge_cosine(torch.nn.functional.normalize(h, p=2., dim=-1, eps=eps), torch.stack([col, dst + row_offset]))
    zero = torch.zeros_like(s)
    e_pos = torch.where(live, torch.relu(s), zero)
    e_neg = torch.where(live, -torch.relu(-s), zero)
    hj = h.index_select(0, col)
    out = torch.zeros(n, h.size(1), dtype=h.dtype).index_add_(0, dst, (coef * (c2[0] * e_pos + c2[1] * e_neg)).view(-1, 1) * hj)
    (out * gout).sum().backward()
    with torch.no_grad():
        u = s * (gout.index_select(0, dst) * hj).sum(-1)
    return dict(out=out.detach(), s=s.detach(), grad=h.grad, u=u, grad_coef=coef.grad, grad_c2=c2.grad)


def oracle_weighted(x, rowptr, col, w, gout, n_total=None):
    """torch.sparse.mm autograd in x's dtype on a CSR's pattern: dict(out, grad_x, grad_w [E] in CSR order)."""
    rowptr, col = torch.as_tensor(np.asarray(rowptr)).long(), torch.as_tensor(np.asarray(col)).long()
    n = rowptr.numel() - 1
    dst = torch.repeat_interleave(torch.arange(n), rowptr.diff())
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().to(x.dtype).clone().requires_grad_(True)
    a = torch.sparse_coo_tensor(torch.stack([dst, col]), w, (n, x.size(0)))
    out = torch.sparse.mm(a, x)
    (out * gout.to(x.dtype)).sum().backward()
    return dict(out=out.detach(), grad_x=x.grad, grad_w=w.grad)


REGIME_HUB_SOURCE = 4
REGIME_ISOLATED = 50


def regime_edges(n=3000):
    """One edge list with every row class of the kernels: split targets (in-degree > 128: node 0 with an
    in-edge from EVERY other node, 900, 500, 300, 140, 129), wave targets (17 .. 128: 128, 60, 20, 17 and a
    block of 40 rows of random degree in that range), small targets (the rest, 16 among them), a hub SOURCE
    (node 4: n / 2 out-edges) and 50 nodes without any in-edge (the last 50) - the zero row 9 and the tied
    rows 5, 6, 7 are targets and sources like any other; targets 1000 .. 1004 and the block 800 .. 839 lie in
    the node range (n // 4, n // 4 + n // 3).  Sparse enough that most nodes are small on both sides."""
    hubs = ((3, 900), (9, 300), (11, 140), (12, 60), (13, 20), (1000, 500), (1001, 129), (1002, 128),
            (1003, 17), (1004, 16))
    ei = random_graph(n, 3 * n, seed=3, hubs=hubs)
    rng = np.random.default_rng(5)
    block = [(int(s), t) for t in range(800, 840)
             for s in rng.choice(n, size=int(rng.integers(17, 129)), replace=False)]
    every = torch.arange(1, n)
    ei = torch.cat([ei, torch.tensor(block).t(), torch.stack([every, torch.zeros_like(every)]),
                    torch.stack([torch.full((n // 2,), REGIME_HUB_SOURCE), torch.arange(n // 2) * 2 + 1])], 1)
    ei = torch.unique(ei, dim=1)
    return ei[:, ei[1] < n - REGIME_ISOLATED]


def csr_of_edge_list(ei, n):
    """CSR by target of an edge list (edge order kept inside a row): rowptr [n + 1], col [E], and the
    permutation ``order`` with col == ei[0][order]."""
    order = torch.argsort(ei[1], stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    return rowptr, ei[0][order], order


def oracle_fixed_mask(h, rowptr, col, kept, gout, row_offset=0):
    """The oracle's own blocks (F.normalize, O.edge_cosine, O.scatter_mean) on a CSR with the kept mask FIXED,
    in h's dtype, and autograd's gradient of <out, gout>: (out [N, C], grad_h [N_total, C]).  For a node-range
    partition the rows are the owned targets and ``col`` / ``h`` are global."""
    rowptr, col = torch.as_tensor(np.asarray(rowptr)).long(), torch.as_tensor(np.asarray(col)).long()
    n = rowptr.numel() - 1
    dst = torch.repeat_interleave(torch.arange(n), rowptr.diff())
    kept = torch.ones(col.numel(), dtype=torch.bool) if kept is None else torch.as_tensor(np.asarray(kept)).bool()
    h = h.detach().clone().requires_grad_(True)
    s = O.edge_cosine(torch.nn.functional.normalize(h, p=2., dim=-1), torch.stack([col, dst + row_offset]))
    w = torch.where(kept, s, torch.zeros_like(s))
    out = O.scatter_mean(w.view(-1, 1) * h.index_select(0, col), dst, n)
    (out * gout.to(h.dtype)).sum().backward()
    return out.detach(), h.grad


def ggcn_scalar_gradients64(ref, adj, dp, h, gout):
    """Float64 gradient AND magnitude of every scalar parameter (``coeff``, ``scale``, ``deg_coeff``) of the oracle
    layer ``ref`` (O.GGCNlayer_SP, any dtype) for the loss <out, gout>: (values, magnitudes), dicts by parameter name.
    The float64 arbiter's per-edge / per-coefficient results at F.cosine_similarity's eps = 1e-8 with G = scale x gout,
    chained as autograd writes it - the softmax c_k (g_k - sum_m c_m g_m) (magnitude c_k (M_k + sum_m c_m M_m)), the
    softplus' sigmoid, the degree scaling a_e = adj_e softplus(d_0 dv_e + d_1) - with absolute values throughout for
    the magnitude.  No dense or sparse-times-sparse intermediate: lean at any graph size."""
    from tests import arbiter
    idx, val = adj._indices(), adj._values().double()
    n = adj.size(0)
    p = {k: v.detach().double() for k, v in ref.named_parameters()}
    wh = h.double() @ p["fcn.weight"].t() + p["fcn.bias"]
    g = gout.double()
    coef, vals, mags = val, {}, {}
    if ref.use_degree:
        dv = dp._values().double()
        z = p["deg_coeff"][0] * dv + p["deg_coeff"][1]
        coef, sig = val * torch.nn.functional.softplus(z), torch.sigmoid(z)
    keep = idx[0] != idx[1] if ref.use_sign else torch.ones_like(idx[0], dtype=torch.bool)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(idx[0][keep], minlength=n), 0)              # coalesced: sorted by row
    if ref.use_sign:
        c, scale = torch.softmax(p["coeff"], -1), torch.nn.functional.softplus(p["scale"])[0]
        pos, neg = O.signed_attention_values(idx[:, keep], wh)
        arb = arbiter.signed(rowptr, idx[1][keep], wh, coef[keep], c[:2], torch.sign(pos + neg).long(), scale * g,
                             eps=1e-8, routes=False)
        gw, GW = (g * wh).sum(), (g.abs() * wh.abs()).sum()
        gc, mc = torch.cat([arb["grad_c2"], (scale * gw).view(1)]), torch.cat([arb["MAG_grad_c2"], (scale * GW).view(1)])
        vals["coeff"], mags["coeff"] = c * (gc - (c * gc).sum()), c * (mc + (c * mc).sum())
        dsp = torch.sigmoid(p["scale"])
        vals["scale"] = dsp * ((g * arb["out"]).sum() + c[2] * gw)
        mags["scale"] = dsp * ((g.abs() * arb["MAG_out"]).sum() + c[2] * GW)
        g_coef, m_coef = arb["grad_coef"], arb["MAG_grad_coef"]
    else:
        arb = arbiter.weighted(rowptr, idx[1], coef, wh, g)
        g_coef, m_coef = arb["grad_w"], arb["MAG_grad_w"]
    if ref.use_degree:
        va, sg, dk = val[keep], sig[keep], dv[keep]
        vals["deg_coeff"] = torch.stack([(g_coef * va * sg * dk).sum(), (g_coef * va * sg).sum()])
        mags["deg_coeff"] = torch.stack([(m_coef * va.abs() * sg * dk.abs()).sum(), (m_coef * va.abs() * sg).sum()])
    return vals, mags


def row_classes(rowptr, h, row_offset=0, loops_kept=False):
    """Names -> bool masks over the N_total feature rows, for reporting a gradient's worst element per class:
    zero rows, eps-clamped non-zero rows, the hub source, and the owned targets by the kernels' row class
    (in-degree > 128 split, 17 .. 128 wave, else small; isolated: no in-edge but - where loops are kept - its own)."""
    h = torch.as_tensor(h).double()
    nrm = h.norm(dim=1)
    deg = torch.as_tensor(np.asarray(rowptr)).long().diff()
    lo = int(row_offset)
    own = lambda m: torch.zeros(h.size(0), dtype=torch.bool).index_put_((torch.arange(lo, lo + deg.numel()),), m)
    iso = deg <= (1 if loops_kept else 0)
    hub = torch.zeros(h.size(0), dtype=torch.bool)
    hub[REGIME_HUB_SOURCE] = True
    return {"zero": nrm == 0, "clamped": (nrm > 0) & (nrm < 1e-12), "hub-src": hub,
            "split": own(deg > 128), "wave": own((deg > 16) & (deg <= 128)), "small": own((deg <= 16) & ~iso),
            "isolated": own(iso)}


def log_operator_rows(differ, rows, label=None):
    """One operator-level comparison for the pytest summary (tests/conftest.py)."""
    import os
    if label is None:
        label = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::", 1)[-1]
    OPERATOR_TIE_LOG.append((label, differ, rows))


def check_selection(res, sel_src_gpu, sel_w_gpu, top_k, thr, strict, h=None, tie_ulps=None, gaps=None,
                    exact_gate_ulps=None, exact_gaps=None, exact_unit=None):
    """Compare the GPU's per-row selection with the oracle's.

    Rows that agree exactly pass.  A row that differs is accepted only when the
    difference is explained by a near tie (oracle cosines within TIE_TOL of each
    other or of thr) - and never when ``strict``.  With ``h`` (the operator's input rows) a
    differing row must not involve a structural exact tie either.  Returns the number of rows
    that needed the near-tie rule.  ``tie_ulps``: the gate in ulps of 1.0 (default TIE_ULPS);
    ``gaps``: the list the needed gaps are appended to (default NEAR_TIE_GAPS).
    ``exact_gate_ulps`` (needs ``h``): a differing row is ALSO judged on the EXACT cosines of the operands -
    float64 dot products of the same fp32 unit rows both sides dot - where only the kernel's own rounding
    can put two edges out of order (the oracle's fp32 scores carry the oracle's summation error too): the
    gap the row needs there must be <= this many ulps; appended to ``exact_gaps``.  ``exact_unit``: the unit rows
    the KERNEL dots (``ops.normalize_rows`` of the same h: its sum of squares is added in another order than the
    CPU's, so a row's norm - and with it every element - can differ from F.normalize's by an ulp; the kernel's
    own rounding is judged on ITS operands)."""
    tol = (TIE_ULPS if tie_ulps is None else float(tie_ulps)) * ULP32
    gaps = NEAR_TIE_GAPS if gaps is None else gaps
    unit = None
    if h is not None:
        unit = torch.nn.functional.normalize(torch.as_tensor(h).detach().cpu().float(), p=2., dim=-1).numpy()
    sel_o = res["sel_src"].numpy()
    sel_g = sel_src_gpu.cpu().numpy().astype(np.int64)
    diff_rows = np.flatnonzero((sel_o != sel_g).any(axis=1))
    if tie_ulps is None:
        log_operator_rows(int(diff_rows.size), int(sel_o.shape[0]))
    if diff_rows.size == 0:
        return 0
    assert not strict, f"selection differs in rows {diff_rows[:10]} (strict case)"
    ei = res["ei"].numpy()
    s = res["s"].detach().numpy()
    thr32 = np.float32(thr)
    order = np.argsort(ei[1], kind="stable")
    dst_sorted = ei[1][order]
    for i in diff_rows:
        lo, hi = np.searchsorted(dst_sorted, [i, i + 1])
        pos = order[lo:hi]
        srcs, sc = ei[0][pos], s[pos]
        got = sel_g[i][sel_g[i] >= 0]
        # scores (oracle's) of what the GPU picked, by matching sources in edge order
        picked, picked_edges = [], []
        used = np.zeros(pos.size, bool)
        for j in got:
            cand = np.flatnonzero((srcs == j) & ~used)
            assert cand.size, f"row {i}: GPU selected source {j} that is not an in-neighbour"
            # among duplicates take the best-scoring unused one (the first of equals)
            c = cand[np.argmax(sc[cand])]
            used[c] = True
            picked.append(sc[c])
            picked_edges.append(c)
        picked = np.asarray(picked, np.float32)
        assert picked.size <= top_k
        # A STRUCTURAL exact tie - two in-edges whose sources' products with the target's unit
        # row are the same bits channel by channel (duplicate rows, power-of-two multiples, rows
        # with one non-zero channel, C == 1), so the cosines are equal in ANY summation order -
        # is decided by the edge position on both sides: the kernel scores normalise-then-dot
        # like the reference.  Inside such a group the GPU must therefore have taken a PREFIX in
        # edge-position order, and list it in that order - whatever near ties with unrelated
        # sources shift the ranks around it.  (Two unrelated cosines that merely round to the
        # same float in one summation order are an ordinary near tie.)
        if unit is not None:
            groups = {}
            for q in range(pos.size):                       # pos ascending = edge-position order
                groups.setdefault((unit[i] * unit[int(srcs[q])]).tobytes(), []).append(q)
            rank_of = {int(c): r for r, c in enumerate(picked_edges)}
            for members in groups.values():
                if len(members) < 2:
                    continue
                taken = [q for q in members if q in rank_of]
                assert taken == members[:len(taken)], \
                    f"row {i}: structural tie among sources {srcs[members].tolist()} not broken by edge position " \
                    f"(GPU took {srcs[taken].tolist()})"
                ranks = [rank_of[q] for q in taken]
                assert ranks == sorted(ranks), \
                    f"row {i}: structurally tied sources {srcs[taken].tolist()} listed out of edge-position order"
        # the smallest tolerance that explains this row: how far below thr a kept edge is in the
        # oracle's scores, how far out of rank order the kept list is, and how much better than the
        # worst kept edge (list full) or than thr (room left) an edge that was NOT kept is
        def needed(scores, thr_v):
            kept_s = scores[picked_edges]
            need = 0.0
            if kept_s.size:
                need = max(need, float(thr_v - kept_s.min()))
                if kept_s.size > 1:
                    need = max(need, float(np.diff(kept_s).max()))
            rest = scores[~used]
            if rest.size and top_k > 0:
                if kept_s.size == top_k:
                    need = max(need, float(rest.max() - kept_s.min()))
                else:
                    elig = rest[rest >= thr_v]
                    if elig.size:
                        need = max(need, float(elig.max() - thr_v))
            return need
        need = needed(sc, thr32)
        assert need <= tol, (f"row {i}: selection differs by more than a near tie: needs {need:.3e} "
                             f"= {need / ULP32:.2f} ulp (gate {tol / ULP32:.1f} ulp); kept {picked.tolist()}")
        gaps.append(need)
        if exact_gate_ulps is not None:
            assert unit is not None, "exact_gate_ulps needs h"
            eu = unit if exact_unit is None else exact_unit
            s64 = (eu[i].astype(np.float64)[None, :] * eu[srcs].astype(np.float64)).sum(axis=1)
            need64 = needed(s64, np.float64(thr32))
            assert need64 <= exact_gate_ulps * ULP32, (
                f"row {i}: in EXACT cosines of the same unit rows the selection needs {need64:.3e} = "
                f"{need64 / ULP32:.2f} ulp (gate {exact_gate_ulps} ulp): the kernel's own rounding is off")
            if exact_gaps is not None:
                exact_gaps.append(need64)
    return int(diff_rows.size)


def assert_close(got: torch.Tensor, want: torch.Tensor, what="out", rtol=RTOL, atol=ATOL):
    got, want = got.detach().cpu(), want.detach().cpu()
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} entries off; "
                           f"max abs err {err.max().item():.3e}, "
                           f"max rel {((err / want.abs().clamp_min(1e-30))[bad]).max().item():.3e}")


def oracle_aggregate(h, ei, add_loops, remove_loops, top_k, thr):
    return O.aggregate_reference(h, ei, add_loops=add_loops, remove_loops=remove_loops,
                                 top_k=top_k, thr=thr)


NEAR_TIE_LOG = []       # (test id, rows that needed the near-tie rule, rows compared): printed by conftest
REPORT_LINES = []       # free-form lines for the summary (measured errors of the full-size tests)
OPERATOR_TIE_LOG = []   # the same at operator level (same inputs on both sides)
# Model level: the two sides' ``lin`` results differ in the last ulp (rocBLAS / MFMA vs the CPU's
# GEMM), so the cosines differ by an INPUT perturbation on top of the summation order: one more
# ulp per operand.  Gate 3 ulps at a model's FIRST layer (2 + 1 for the perturbed operand; round 3
# allowed 5; the measured maximum over configs 1-3 at full size is 1.5, config 4's 1-layer model: no
# differing row of 169 343) and one more ulp per layer in front (that layer's ``lin`` and aggregation
# round differently on the two sides as well: the second layer of config 4's 2-layer model, whose input
# rows are nearly parallel - every cosine within 1.3e-5 of 1 - needs 3.5), gaps logged separately.
MODEL_TIE_ULPS = 3.0
MODEL_TIE_GAPS = []
# second and later layers at OPERATOR level: the oracle's own layer input fed to both sides (gate TIE_ULPS)
# A deep layer's rows are nearly parallel (arxiv 2-layer model: every cosine within 1.3e-5 of 1): all C
# products are positive and the partial sums run up to 1, so BOTH sides' fp32 summations carry ~1 ulp of
# their own, and a gap read off the ORACLE's scores measures the oracle's rounding as much as the kernel's
# (measured: 2.50 ulp at most, 151 of 189 097 rows).  The kernel is therefore held to the operator gate
# (TIE_ULPS = 2) on the EXACT cosines - float64 dot products of the same fp32 unit rows - where only its own
# rounding can reorder two edges (the KERNEL's unit rows: its sum of squares runs in another order than the CPU's,
# so a row's norm can differ from F.normalize's by an ulp); the gap in the oracle's fp32 scores, which also holds that
# normalisation difference, is gated one ulp wider (3) and printed.
DEEP_OPERATOR_LOG = []
DEEP_OPERATOR_GAPS = []
DEEP_EXACT_GAPS = []
# (SNGNN_DEEP_GATE_ULPS: a measurement aid - run with a wide gate to read the largest gap off the summary)
DEEP_GATE_ULPS = float(__import__("os").environ.get("SNGNN_DEEP_GATE_ULPS", TIE_ULPS + 1.0))


def model_selection_report(ours, ref, data_cpu, data_gpu, label):
    """Per selecting conv layer of a model pair (GPU module / oracle module, same parameters):
    compare the rows' selections on each side's OWN ``h = lin(x)`` - the two ``lin`` results
    differ in the last ulp (rocBLAS / MFMA vs the CPU's GEMM), which is where a model-level
    near-tie flip comes from.  A differing row must pass ``check_selection``'s near-tie rule
    (oracle cosines within MODEL_TIE_ULPS ulps, + 1 per layer in front; no structural tie involved).  Returns and logs
    (rows that differ, rows compared)."""
    from sngnn_amd import conv as CV
    from sngnn_amd import ops
    from sngnn_amd.graph import GLOBAL_CACHE
    cap_g, cap_r = {}, {}
    hooks = []
    for li, (cg, cr) in enumerate(zip(ours.lins, ref.lins)):
        hooks.append(cg.register_forward_pre_hook(lambda m, a, li=li: cap_g.__setitem__(li, a[0].detach())))
        hooks.append(cr.register_forward_pre_hook(lambda m, a, li=li: cap_r.__setitem__(li, a[0].detach())))
    was = ours.training, ref.training
    ours.eval(), ref.eval()
    with torch.no_grad():
        ours(data_gpu), ref(data_cpu)
    ours.train(was[0]), ref.train(was[1])
    for hk in hooks:
        hk.remove()
    differ = rows = 0
    for li, (cg, cr) in enumerate(zip(ours.lins, ref.lins)):
        k = getattr(cr, "top_k", None)
        if k is None:
            continue
        rem = bool(cr.is_remove_self_loops)
        with torch.no_grad():
            h_r = cr.lin(cap_r[li])
            h_g = CV._lin_aligned(cap_g[li], cg.lin)[0]
        res = O.aggregate_reference(h_r, data_cpu.edge_index, add_loops=True, remove_loops=rem,
                                    top_k=int(k), thr=float(cr.thr))
        g = GLOBAL_CACHE.get(data_gpu.edge_index, h_g.size(0), True, rem)
        _, _, _, sel_src, sel_w = ops.aggregate_forward(g, h_g.contiguous(), int(k), float(cr.thr),
                                                        want_selection=True)
        differ += check_selection(res, sel_src, sel_w, int(k), float(cr.thr), strict=False, h=h_r,
                                  tie_ulps=MODEL_TIE_ULPS + li, gaps=MODEL_TIE_GAPS)
        rows += h_r.size(0)
        if li >= 1:
            # OPERATOR level on a deep layer's actual input: the ORACLE's h on both sides (identical
            # operands), so only the kernel's own arithmetic can move a selection - held to the operator
            # gate (TIE_ULPS), where the end-to-end comparison above allows one more ulp per layer
            h_same = h_r.to(h_g.device).contiguous()
            _, _, _, s2, w2 = ops.aggregate_forward(g, h_same, int(k), float(cr.thr), want_selection=True)
            un_gpu, _ = ops.normalize_rows(h_same)               # the unit rows the kernel dots
            d2 = check_selection(res, s2, w2, int(k), float(cr.thr), strict=False, h=h_r,
                                 tie_ulps=DEEP_GATE_ULPS, gaps=DEEP_OPERATOR_GAPS,
                                 exact_gate_ulps=TIE_ULPS, exact_gaps=DEEP_EXACT_GAPS,
                                 exact_unit=un_gpu.cpu().numpy())
            DEEP_OPERATOR_LOG.append((f"{label}, layer {li + 1}", d2, h_r.size(0)))
    NEAR_TIE_LOG.append((label, differ, rows))
    return differ, rows

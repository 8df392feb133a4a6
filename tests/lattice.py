"""Lattice inputs: feature rows on which every selection of this project is decidable with ZERO tolerance.

A lattice row has exactly ``s`` non-zero channels, each ``+-2^e`` with one exponent ``e`` in [-3, 3] per row;
``s = support(c)`` is the largest of {1, 4, 16, 64} that is <= c.  Then every step of a cosine is exact in fp32 (and
with bf16 / fp16 operands): the sum of squares is s 4^e, its IEEE square root sqrt(s) 2^e, the unit entries
+-1/sqrt(s), the products +-1/s, and a sum of at most 64 of them is exact in ANY order.  So every cosine is d / s
with d an integer - equal integers are equal bits - and which edge or node survives a cut is fixed by the tie rule
alone: the earlier edge position in the aggregation, the lower node id in the kNN builder.  With 2 s + 1 levels
against in-degrees of hundreds (or N candidates) ties are everywhere, the cut included.

Two kinds of rows on top of that produce a cosine of -0.0, which must order like +0.0 ("the reference orders
floats, not bit patterns"):
  * the plain pair (``neg_zero_rows``): a dense all-positive row next to an all ``-0.0`` row - every product
    is -0.0.  A kernel that starts its accumulator at +0.0 turns that into +0.0 by itself (+0 + -0 = +0);
  * the UNDERFLOW rows (``underflow``): every channel ``+-TINY`` with ``TINY = fl32(1e-12) 2^-80``.  TINY^2
    underflows, the norm is 0, F.normalize's clamp divides by fl32(1e-12): unit entries of exactly +-2^-80.  The
    product of two of them is 2^-160, which rounds to +-0.0 with its SIGN kept - also as the first step of an fma
    chain that starts at +0.0, where the exact product, not a zero, is added.  An all-negative tiny row against
    an all-positive one therefore scores -0.0 in every lane of a kernel whose row layout the channel count fills
    (C = 64, 256, 512 here), and the lane tree adds -0.0 + -0.0 = -0.0.  Against a lattice row the cosine is
    d 2^-80 / sqrt(s), again exact in any order; the aggregated rows stay exact as well (``exact_out``'s note).
For the kNN builder, which scales a raw dot product by both inverse norms, the pair is ``underflow_pair_rows``:
<x_0, x_1> = -2^-80 (a normal number), inverse norms 2^-40 each, so the scaled cosine -2^-160 rounds to -0.0.

No GPU and no torch-geometric here: generators, exact references, and the case lists that the CPU premises
(tests/test_lattice_cpu.py) and the GPU comparison (tests/test_exact_selection_gpu.py) share.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests.helpers import random_graph

SUPPORTS = (1, 4, 16, 64)
TINY = float(np.float32(1e-12) * np.float32(2.0 ** -80))       # fl32(1e-12) is F.normalize's clamp: TINY / clamp == 2^-80
ZERO_ROWS = tuple(range(350, 357))                                    # all +0.0 (late ids: a zero source sits BEHIND others in a row)
NEG_ZERO_PAIR = (30, 31)                                         # (dense all-positive row, all -0.0 row)
TINY_NEG, TINY_POS = 41, (40, 42) + tuple(range(320, 346))       # underflow rows: one all -TINY, the others all +TINY


def support(c: int) -> int:
    return max(s for s in SUPPORTS if s <= c)


def lattice_rows(n, c, seed, scale=True, zero_rows=ZERO_ROWS, neg_zero_rows=False, underflow=False):
    """[n, c] fp32 lattice rows (module docstring).  ``scale=False``: every exponent 0.  ``zero_rows``: ids of all-+0.0
    rows.  ``neg_zero_rows`` (c in SUPPORTS only, where a row's support is every channel): NEG_ZERO_PAIR.
    ``underflow``: the TINY_NEG / TINY_POS rows."""
    rng = np.random.default_rng(seed)
    s = support(c)
    h = np.zeros((n, c), np.float32)
    cols = np.argsort(rng.random((n, c)), axis=1)[:, :s]          # s distinct channels per row
    sign = rng.integers(0, 2, size=(n, s)) * 2 - 1
    e = rng.integers(-3, 4, size=(n, 1)) if scale else np.zeros((n, 1), np.int64)
    np.put_along_axis(h, cols, (sign * 2.0 ** e).astype(np.float32), axis=1)
    for r in zero_rows:
        if r < n:
            h[r] = 0.0
    if neg_zero_rows:
        assert c == s and n > max(NEG_ZERO_PAIR), "the -0.0 pair needs a support of every channel"
        h[NEG_ZERO_PAIR[0]] = np.float32(2.0 ** int(e[NEG_ZERO_PAIR[0], 0]))
        h[NEG_ZERO_PAIR[1]] = np.float32(-0.0)
    if underflow:
        assert n > max(TINY_POS)
        h[list(TINY_POS)] = np.float32(TINY)
        h[TINY_NEG] = np.float32(-TINY)
    return torch.from_numpy(h)


STAIR_CHANNELS = 16


def staircase_rows(n, f, levels_ascending=True, seed=0):
    """[n, f] rows for the kNN builder: channels [0, 16) are +-1, the rest 0.  Node j of level a(j) in 0 .. 16 has the
    first 16 - a of them negated, so dot(j, j') = 16 - 2 |a - a'| and every level is one big tie group.  Levels
    ascending by id: every later column tile beats what a high-level row has seen before (repeated park overflow and
    merges - the scan's worst case); descending (``False``) admits nothing after a row's own tiles; ``"shuffled"``: a
    seeded permutation of the ascending levels."""
    assert f >= STAIR_CHANNELS
    a = (np.arange(n) * (STAIR_CHANNELS + 1)) // max(n, 1)
    if levels_ascending == "shuffled":
        a = a[np.random.default_rng(seed).permutation(n)]
    elif not levels_ascending:
        a = a[::-1]
    x = np.zeros((n, f), np.float32)
    x[:, :STAIR_CHANNELS] = np.where(np.arange(STAIR_CHANNELS)[None, :] < (STAIR_CHANNELS - a)[:, None], -1.0, 1.0)
    return torch.from_numpy(x)


def underflow_pair_rows(n, f, seed):
    """kNN rows whose cosine <0, 1> is -0.0 by underflow: x_0 = (2^-40, 2^40, 0, ..), x_1 = (-2^-40, 0, 2^40, 0, ..) - the
    dot product is -2^-80, the norms round to 2^40 - and lattice rows on the channels [3, f) behind them, so rows 0
    and 1 have a cosine of +0.0 with every other row.  Returns (x, surrogate): the surrogate has the two 2^-40
    entries zeroed and is a lattice; since -0.0 == +0.0 its exact kNN (``knn_exact``) is the answer for x as well -
    node 1 is node 0's FIRST neighbour of cosine 0, and node 0 is node 1's."""
    assert f >= 3 + 16 and n >= 2
    x = torch.zeros(n, f)
    x[2:, 3:] = lattice_rows(n - 2, f - 3, seed, zero_rows=())
    x[0, 1] = x[1, 2] = 2.0 ** 40
    sur = x.clone()
    x[0, 0], x[1, 0] = 2.0 ** -40, -(2.0 ** -40)
    return x, sur


def knn_exact(x, k, exclude_self=True):
    """The exact kNN of lattice rows (every row's non-zero entries share one magnitude): int64 dot products of the sign
    patterns, order (dot descending, node id ascending) by a stable sort, cosine dot / sqrt(s_i s_j) - asserted exact:
    s_i == s_j wherever the dot product is not 0.  A zero row has cosine +0.0 with everything (itself included).
    Returns (idx int64 [n, k], -1 padded; sim fp32 [n, k], 0 padded) - ``toolbox.knn_graph``'s convention."""
    xa = np.asarray(x, np.float64)
    mag = np.abs(xa)
    top = mag.max(axis=1, keepdims=True)
    assert ((mag == 0) | (mag == top)).all(), "not lattice rows"
    sg = np.sign(xa).astype(np.int64)
    n = sg.shape[0]
    live = sg[:, (sg != 0).any(axis=0)]                           # (channels that are zero in every row add nothing)
    dot = live @ live.T
    cnt = np.abs(sg).sum(axis=1)
    den = np.sqrt((cnt[:, None] * cnt[None, :]).astype(np.float64))
    assert ((dot == 0) | (cnt[:, None] == cnt[None, :])).all(), "a non-zero cosine between rows of different support"
    cos = np.where(dot == 0, 0.0, dot / np.maximum(den, 1.0))
    assert (cos.astype(np.float32).astype(np.float64) == cos).all()
    key = dot.astype(np.float64) / np.maximum(den, 1.0)           # (rows of one support: the order of dot)
    if exclude_self:
        key[np.arange(n), np.arange(n)] = -np.inf
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]         # stable: equal cosines stay in id order
    m = min(k, n - (1 if exclude_self else 0))
    idx = np.full((n, k), -1, np.int64)
    sim = np.zeros((n, k), np.float32)
    idx[:, :m] = order[:, :m]
    sim[:, :m] = np.take_along_axis(cos, order[:, :m], axis=1).astype(np.float32)
    return torch.from_numpy(idx), torch.from_numpy(sim)


# ---------------------------------------------------------------------------
# Forward cases: (name, n, C, top_k, thr numerator t (thr = t / support(C)), remove_loops, flags)
#   flags: "u" = underflow rows with planted edges, "z" = the plain -0.0 pair
# Small top_k (1, 2, 5) so that rows of a handful of in-edges have a cut at all; thr on the lattice for cos == thr.
# ---------------------------------------------------------------------------
HUBS_360 = ((0, 359), (3, 200), (5, 131), (9, 40), (11, 17))
HUBS_2000 = ((0, 1999), (1, 1500), (2, 700))


def _fc(c, k, t, rem, flags="", n=360):
    return (f"n{n}-C{c}-k{k}-t{t}-{'rem' if rem else 'keep'}{('-' + flags) if flags else ''}", n, c, k, t, rem, flags)


FORWARD_CASES = [
    _fc(1, 1, 0, True, "z"), _fc(1, 2, -1, False), _fc(1, 5, 1, True),
    _fc(3, 1, 0, False), _fc(3, 5, 1, True),
    _fc(4, 2, 0, True, "z"), _fc(4, 16, 2, False), _fc(4, 33, -2, True),
    _fc(7, 1, 2, True), _fc(7, 5, 0, False), _fc(7, 64, -2, True),
    _fc(16, 2, 2, False, "z"), _fc(16, 32, 0, True),
    _fc(20, 5, 0, True), _fc(20, 16, 4, False), _fc(20, 1, -2, True),
    _fc(33, 2, 0, False), _fc(33, 33, 2, True),
    _fc(40, 16, 0, True), _fc(40, 5, 4, False), _fc(40, 32, -2, True),
    _fc(47, 1, 0, True), _fc(47, 64, 2, False),
    _fc(64, 2, 0, True, "uz"), _fc(64, 16, 2, False), _fc(64, 32, 4, True), _fc(64, 5, 0, False, "u"),
    _fc(100, 5, 0, False), _fc(100, 33, 2, True),
    _fc(130, 1, 2, True), _fc(130, 16, 0, False), _fc(130, 64, -2, True),
    _fc(256, 2, 0, False, "u"), _fc(256, 64, 4, True),
    _fc(512, 5, 0, True, "u"), _fc(512, 16, 2, False),
    _fc(40, 16, 0, True, n=2000), _fc(40, 400, 0, False, n=2000),
]
FORWARD_IDS = [c[0] for c in FORWARD_CASES]
assert len(FORWARD_CASES) <= 40 and len(set(FORWARD_IDS)) == len(FORWARD_IDS)

# the half path runs the same lattice rows (|e| <= 3: fp16 holds them; no underflow rows - TINY is not a half number)
HALF_CASES = [_fc(7, 5, 0, False), _fc(16, 2, 2, False, "z"), _fc(40, 16, 0, True), _fc(64, 16, 2, False),
              _fc(130, 16, 0, False), _fc(256, 64, 4, True), _fc(40, 16, 0, True, n=2000)]
HALF_IDS = [c[0] for c in HALF_CASES]


def _planted_edges(ei, n):
    """The underflow rows' in-edges, chosen so that the -0.0 cosine sits at an EARLIER edge position than +0.0 ones
    and the cut falls between them: every random in-edge of TINY_POS[0] (small row) and TINY_POS[1] (wave row)
    is dropped; TINY_POS[0] <- TINY_NEG, then the zero rows; TINY_POS[1] <- TINY_NEG, then the other +TINY rows."""
    small, wave = TINY_POS[0], TINY_POS[1]
    keep = (ei[1] != small) & (ei[1] != wave)
    src_s = [TINY_NEG] + list(ZERO_ROWS)
    src_w = [TINY_NEG] + list(TINY_POS[2:])
    extra = torch.tensor([src_s + src_w, [small] * len(src_s) + [wave] * len(src_w)])
    ei = torch.cat([ei[:, keep], extra], 1)
    key = torch.unique(ei[0] * n + ei[1])                         # (src, dst) order, as random_graph leaves it
    return torch.stack([key // n, key % n])


@functools.lru_cache(maxsize=None)
def forward_inputs(case):
    """(h fp32 [n, C], edge_index [2, E], thr) of one forward case - built once, shared, never modified."""
    name, n, c, k, t, rem, flags = case
    seed = 1000 * c + 10 * k + (t + 8)
    if n == 360:
        ei = random_graph(n, 2400, seed=seed, hubs=HUBS_360)
    else:
        ei = random_graph(n, 30000, seed=seed, hubs=HUBS_2000)
    h = lattice_rows(n, c, seed + 1, neg_zero_rows="z" in flags, underflow="u" in flags)
    if "u" in flags:
        ei = _planted_edges(ei, n)
    return h, ei, t / support(c)


@functools.lru_cache(maxsize=None)
def forward_oracle(case):
    """``oracle.aggregate_reference`` of a case (the Python oracle, fp32 on the CPU) - computed once."""
    from oracle import sngnn_oracle as O
    h, ei, thr = forward_inputs(case)
    with torch.no_grad():
        return O.aggregate_reference(h, ei, add_loops=True, remove_loops=case[5], top_k=case[3], thr=thr)


def exact_out(h, res):
    """The aggregated rows in exact arithmetic, rounded once: float64 sum of weight x h[src] over the oracle's kept
    edges - exact, every term is a multiple of 2^-9 below 2^3 (or, on and from the underflow rows, a multiple of
    2^-86-3 below 2^-74, resp. a product below 2^-149 that BOTH sides round to 0) and there are at most 2000 -
    divided by the in-degree in float64 and rounded to fp32.  (53 >= 2 x 24 + 2 bits: rounding the float64
    quotient equals the correctly rounded fp32 division.)"""
    ei, w = res["ei"], res["weight"].double()
    n = h.size(0)
    msg = (w.view(-1, 1).float() * h.index_select(0, ei[0])).double()       # the fp32 product (exact; underflow -> 0)
    total = torch.zeros(n, h.size(1), dtype=torch.float64).index_add_(0, ei[1], msg)
    cnt = torch.bincount(ei[1], minlength=n).clamp_min(1).double()
    return (total / cnt.view(-1, 1)).float()


def row_classes_of(res, n):
    """In-degree per target of the oracle's edge list and the kernels' row classes: small <= 16 < wave <= 128 < split."""
    deg = torch.bincount(res["ei"][1], minlength=n)
    return deg, {"small": deg <= 16, "wave": (deg > 16) & (deg <= 128), "split": deg > 128}


def cut_facts(res, n, top_k, thr):
    """Per target row of an oracle result: ``cut_tie`` - an UNSELECTED in-edge with cos >= thr has the cosine of the worst
    selected one (the survivor is fixed by the edge position alone) - and ``at_thr`` - an in-edge with cos == thr."""
    s, dst = res["s"], res["ei"][1]
    kept = torch.zeros(s.numel(), dtype=torch.bool)
    pos = res["sel_pos"]
    kept[pos[pos >= 0]] = True
    thr32 = torch.tensor(thr, dtype=torch.float32)
    worst = torch.full((n,), float("inf")).scatter_reduce(0, dst[kept], s[kept], reduce="amin", include_self=True)
    tie = ~kept & (s >= thr32) & (s == worst[dst])
    cut_tie = torch.zeros(n, dtype=torch.bool).index_put_((dst[tie],), torch.tensor(True))
    at_thr = torch.zeros(n, dtype=torch.bool).index_put_((dst[s == thr32],), torch.tensor(True))
    return cut_tie, at_thr


# ---------------------------------------------------------------------------
# kNN cases: (name, kind, N, F, k, exclude_self, route (knob 6), fp32-only MFMA (knob 5), base offset in bytes)
# ---------------------------------------------------------------------------
def _kc(kind, n, f, k, excl, route=0, knob5=0, off=0):
    return (f"{kind}-N{n}-F{f}-k{k}-{'ex' if excl else 'self'}-r{route}-m{knob5}-o{off}", kind, n, f, k, excl, route, knob5, off)


KNN_CASES = (
    # the staircases on every route; 2304 rows: the most column splits, k_knn_merge over several rounds at k = 32
    [_kc("asc", 2304, 64, 32, True, r) for r in range(5)]
    + [_kc("desc", 2304, 128, 32, False, r) for r in (1, 2, 3)]
    + [_kc("shuffled", 1030, 96, 31, True, r) for r in (0, 1, 4)]
    + [_kc("asc", 1030, 51, 16, False, 1), _kc("asc", 513, 32, 7, True, 1), _kc("desc", 513, 200, 1, True, 1),
       _kc("shuffled", 2304, 32, 16, True, 3), _kc("asc", 130, 16, 32, True, 1), _kc("asc", 130, 16, 7, False, 2)]
    # fp32 MFMAs (knob 5) on the fused route, and the unaligned base (areg == false: the generic path)
    + [_kc("asc", 1030, 64, 32, True, 1, 1), _kc("shuffled", 513, 128, 16, False, 1, 1), _kc("lattice", 1030, 96, 7, True, 1, 1),
       _kc("asc", 1030, 64, 32, True, 1, 0, 4), _kc("lattice", 513, 128, 16, True, 1, 0, 4)]
    # lattice rows (zero rows among them), identical rows, zero rows, the -0.0 pairs
    + [_kc("lattice", 2304, 64, 32, True, r) for r in (0, 1, 2)]
    + [_kc("lattice", 1030, 200, 16, False, 1), _kc("lattice", 513, 51, 31, True, 1), _kc("lattice", 130, 16, 1, True, 1),
       _kc("lattice", 5, 32, 7, True, 1), _kc("lattice", 5, 16, 7, False, 2)]
    + [_kc("identical", 1030, 32, 32, True, r) for r in (1, 2, 4)] + [_kc("identical", 5, 64, 16, False, 1)]
    + [_kc("zero", 513, 96, 16, True, r) for r in (1, 2)] + [_kc("zero", 5, 16, 1, False, 1)]
    + [_kc("negzero", 130, 64, 7, True, r) for r in range(5)]
    + [_kc("negzero", 1030, 128, 32, True, 1), _kc("negzero", 513, 51, 16, False, 1), _kc("negzero", 130, 32, 1, True, 1, 1),
       _kc("zeropair", 130, 16, 7, True, 1), _kc("zeropair", 513, 64, 16, True, 2)]
)
KNN_IDS = [c[0] for c in KNN_CASES]
assert len(set(KNN_IDS)) == len(KNN_IDS)


@functools.lru_cache(maxsize=None)
def knn_rows(kind, n, f):
    """(x, the lattice whose exact kNN is x's) of one input kind - built once, shared, never modified."""
    if kind in ("asc", "desc", "shuffled"):
        x = staircase_rows(n, f, {"asc": True, "desc": False, "shuffled": "shuffled"}[kind], seed=n + f)
    elif kind == "lattice":
        x = lattice_rows(n, f, 7 * n + f, zero_rows=(1, n // 2))
    elif kind == "identical":
        x = lattice_rows(1, f, f, zero_rows=()).repeat(n, 1)
    elif kind == "zero":
        x = torch.zeros(n, f)
    elif kind == "negzero":
        return underflow_pair_rows(n, f, n + f)
    else:
        assert kind == "zeropair" and f in SUPPORTS
        x = lattice_rows(n, f, 3 * n + f, zero_rows=(1,), neg_zero_rows=True)
    return x, x


@functools.lru_cache(maxsize=None)
def knn_expected(kind, n, f, k, excl):
    return knn_exact(knn_rows(kind, n, f)[1], k, excl)

"""The lean main kernel of the forward (csrc/agg_fwd_roles.h: k_agg_fwd, LEAN - the instantiation a call that asks for
``out`` only runs; sngnn_tuning_set(12, v): 0 = that rule, 1 = the general kernel always) computes the bits of the
general kernel: in every row class, with the split rows finalized inside the main launch and in a launch of its own
(knob 9), in the buffer and the flat form of the gathers (knob 11), and on rows whose sums hold subnormals and values
near FLT_MAX.

One graph of 3 000 nodes holds rows of in-degree 0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 100 and 128, two split
rows of 129 and 700 in-edges (one task pair and six tasks: tasks, candidates and both finalize forms run), self-loops
for the build to remove, and every seventh feature row repeats its neighbour's, so exact ties exist in every class."""
import numpy as np
import pytest
import torch

from tests.helpers import random_graph

pytestmark = pytest.mark.gpu

N, E = 3000, 9000
# node -> forced in-degree (after the self-loops are removed)
DEGREES = {30: 0, 31: 1, 32: 2, 33: 3, 34: 4, 35: 5, 36: 7, 37: 8, 38: 15, 39: 16, 40: 17, 41: 31, 42: 32, 43: 100,
           44: 128, 45: 129, 46: 700}
# the division rows: targets of in-degree 1 and 2 whose sources' norms test_division_inputs scales by 2^120 / 2^-120
BIG_SRC, SMALL_SRC = (60, 61), (62, 63)
DIV_ROWS = {50: (60,), 51: (60, 61), 52: (62,), 53: (62, 63)}


def edges():
    ei = random_graph(N, E, seed=23).numpy()
    forced = list(DEGREES) + list(DIV_ROWS)
    ei = ei[:, ~np.isin(ei[1], forced)]
    rng = np.random.default_rng(9)
    extra = []
    for node, deg in DEGREES.items():
        src = rng.choice(np.setdiff1d(np.arange(N), [node]), size=deg, replace=False)
        extra.append(np.stack([src, np.full(src.size, node)]))
    for node, srcs in DIV_ROWS.items():
        extra.append(np.stack([np.array(srcs), np.full(len(srcs), node)]))
    loops = np.array([30, 31, 32, 39, 45, 50, 51, 700, 701, N - 1])           # removed by the build
    extra.append(np.stack([loops, loops]))
    ei = np.concatenate([ei] + extra, axis=1)
    key = np.unique(ei[0].astype(np.int64) * N + ei[1])
    return torch.from_numpy(np.stack([key // N, key % N]))


_GRAPH = {}


def graph(cuda):
    """The test graph on the device, built once per module (no loops added, the input's self-loops removed)."""
    from sngnn_amd.graph import Graph
    if str(cuda) not in _GRAPH:
        g = Graph(edges().to(cuda), N, False, True)
        deg = np.diff(g.array("rowptr").astype(np.int64))
        for node, d in DEGREES.items():
            assert deg[node] == d, (node, deg[node])
        for node, srcs in DIV_ROWS.items():
            assert deg[node] == len(srcs), (node, deg[node])
        _GRAPH[str(cuda)] = g
    return _GRAPH[str(cuda)]


_ROWS = {}


def rows(C):
    """Eight clusters of rows whose cosines inside a cluster lie on both sides of 0.9 (both thresholds keep and drop);
    every seventh row repeats the one before it: exact ties."""
    if C not in _ROWS:
        gen = torch.Generator().manual_seed(300 + C)
        centre = torch.randn(8, C, generator=gen)
        h = centre[torch.arange(N) % 8] + 0.35 * torch.randn(N, C, generator=gen)
        dup = torch.arange(7, N, 7)
        h[dup] = h[dup - 1]
        _ROWS[C] = h
    return _ROWS[C]


@pytest.fixture
def lib(cuda):
    from sngnn_amd import _lib
    handle = _lib.load()
    try:
        yield handle
    finally:
        handle.sngnn_tuning_set(12, 0)
        handle.sngnn_tuning_set(11, 0)
        handle.sngnn_tuning_set(9, 1)
        handle.sngnn_tuning_set(2, 0)


def lean_and_general(lib, run):
    """run() under knob 12 = 0 (the lean kernel where the call allows it) and 12 = 1 (the general kernel)."""
    res = []
    for general in (0, 1):
        lib.sngnn_tuning_set(12, general)
        out = run()
        torch.cuda.synchronize()
        res.append(out)
    lib.sngnn_tuning_set(12, 0)
    return res


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("thr", [0.0, 0.9])
@pytest.mark.parametrize("k", [None, 1, 4, 16])
@pytest.mark.parametrize("C", [8, 32, 40, 64, 100])
def test_lean_kernel_equals_general_kernel(cuda, lib, C, k, thr):
    from sngnn_amd import ops
    g, h = graph(cuda), rows(C).to(cuda)
    try:
        if k is None:
            lib.sngnn_tuning_set(2, 1)        # nothing selected: from the unit-row table as well (default: on the fly)
        for fin in (3, 0):                    # the finalize on three workgroups of the main launch / a launch of its own
            for addr in (0, 1):               # buffer / flat gathers
                lib.sngnn_tuning_set(9, fin)
                lib.sngnn_tuning_set(11, addr)
                lean, general = lean_and_general(lib, lambda: ops.aggregate_forward(g, h, k, thr)[0])
                if fin and k is not None:
                    assert lib.sngnn_last_forward_finalize_workgroups() == 3
                assert bool(torch.isfinite(general).all()) and float(general.abs().max()) > 0.0
                assert torch.equal(lean, general) and same_bits(lean, general), \
                    (C, k, thr, fin, addr, int((lean != general).any(1).sum()), "rows differ")
    finally:
        lib.sngnn_tuning_set(12, 0)
        lib.sngnn_tuning_set(11, 0)
        lib.sngnn_tuning_set(9, 1)
        lib.sngnn_tuning_set(2, 0)


@pytest.mark.parametrize("k,thr", [(16, 0.0), (4, 0.9), (1, 0.0)])
def test_calls_with_side_outputs_run_the_general_kernel(cuda, lib, k, thr):
    """wsel / inv_norm / the selection lists are asked for: the general kernel runs whatever knob 12 says - every
    result equals the knob-1 call's - and its `out` is the lean kernel's."""
    from sngnn_amd import ops
    g, h = graph(cuda), rows(40).to(cuda)
    try:
        lean_out = ops.aggregate_forward(g, h, k, thr)[0]
        for kwargs in (dict(save_for_backward=True), dict(save_for_backward=True, want_selection=True)):
            auto, general = lean_and_general(lib, lambda: ops.aggregate_forward(g, h, k, thr, **kwargs))
            for x, y in zip(auto, general):
                assert (x is None) == (y is None)
                if x is not None:
                    assert torch.equal(x, y)
            assert same_bits(auto[0], lean_out)
            assert float((auto[1] > -3.0).float().mean()) > 0.0          # wsel was written: some edges are kept
    finally:
        lib.sngnn_tuning_set(12, 0)


@pytest.mark.parametrize("k", [16, None])
def test_division_inputs(cuda, lib, k):
    """Rows of in-degree 1 and 2 whose sums hold subnormals, values near FLT_MAX and zeros of both signs among their
    terms: the mean row of the lean kernel against the general one's, by bit pattern (the inputs on which a division
    by a power of two and a multiplication by its reciprocal - profiles/fwd_lean.txt, part 4 - would have to agree).

    The source rows are "scaled by 2^120 / 2^-120" through their NORMS (the prepared call: unit rows and norms are the
    caller's): h itself scaled so far leaves the range of its own sum of squares, while the sums the division sees -
    score * norm * unit row - are those of such rows."""
    from sngnn_amd import ops
    g = graph(cuda)
    C = 40
    gen = torch.Generator().manual_seed(77)
    h = rows(C).clone()
    # channel magnitudes over fifteen binades (so that 2^-120 times them straddles the smallest normal number), a few -0.0
    v = torch.randn(C, generator=gen) * torch.exp2(torch.randint(-12, 4, (C,), generator=gen).float())
    v[3] = -0.0
    v[17] = 0.0
    v[5] = 32.0                                                # the dominant channel: 0.7 .. 1 of the row's norm
    for s in BIG_SRC + SMALL_SRC:
        h[s] = v
    h[61] = v * (1.0 + 0.01 * torch.rand(C, generator=gen))
    h[63] = v * (1.0 + 0.01 * torch.rand(C, generator=gen))
    for t in DIV_ROWS:
        h[t] = v                                               # cosine ~ 1 with their sources: every edge is kept
    n, nrm = ops.normalize_rows(h.to(cuda))
    nrm = nrm.clone()
    nrm[list(BIG_SRC)] *= 2.0 ** 120
    nrm[list(SMALL_SRC)] *= 2.0 ** -120
    nrm[60] = 2.4e38                  # the largest term of rows 50 and (halved, with row 61's ~5e37 added) 51: ~2e38
    try:
        lean, general = lean_and_general(lib, lambda: ops.aggregate_forward_normalized(g, n, nrm, k, 0.0)[0])
    finally:
        lib.sngnn_tuning_set(12, 0)
    assert same_bits(lean, general), [(t, int((lean[t].view(torch.int32) != general[t].view(torch.int32)).sum()))
                                      for t in DIV_ROWS]
    got = general[list(DIV_ROWS)].cpu()
    assert bool(torch.isfinite(got).all())
    assert float(got[0].abs().max()) > 1.5e38 and float(got[1].abs().max()) > 0.75e38     # near FLT_MAX, and halved
    for tiny in (got[2].abs(), got[3].abs()):                          # subnormal results in both small rows
        assert int(((tiny > 0) & (tiny < 1.1754944e-38)).sum()) >= 2

"""GPU: ``node_similarity_histogram`` (``sngnn_cosine_hist``) - the histogram of all off-diagonal cosines in one
scan, S never stored.

The parity rule ("band"): a cosine of the kernel may differ from the float64 cosine by DELTA = 2e-6 - the
tolerance tests/test_toolbox_gpu.py already uses for ``knn_graph`` and the per-edge cosines - so a value within
DELTA of a bin edge may fall on either side of it and per-bin equality with float64 does not hold.  What must hold
for EVERY edge e is the cumulative count:  #{s64 < e - DELTA} <= C_gpu(e) <= #{s64 <= e + DELTA},
C_gpu(e_b) = under + sum of the bins below b.  No bin is exempted; the largest number of float64 values inside
a band is printed to show how tight the check was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DELTA = 2e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------
def cos64(x):
    n = torch.nn.functional.normalize(x.double(), dim=1)
    return n @ n.t()


def sorted_groups(x, y):
    """sorted float64 off-diagonal cosines: (all, same label, different label); negative label = unlabelled."""
    s = cos64(x)
    n = x.size(0)
    off = ~torch.eye(n, dtype=torch.bool)
    if y is None:
        return np.sort(s[off].numpy()), None, None
    yl = y.long()
    same = (yl[:, None] == yl[None, :]) & (yl[:, None] >= 0) & off
    return np.sort(s[off].numpy()), np.sort(s[same].numpy()), np.sort(s[off & ~same].numpy())


class Weighted:
    """a sorted multiset: values with integer multiplicities"""

    def __init__(self, values, weights=None):
        order = np.argsort(values, kind="stable")
        self.v = np.asarray(values, dtype=np.float64)[order]
        w = np.ones(len(self.v), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)[order]
        self.cum = np.concatenate([[0], np.cumsum(w)])

    def below(self, t):             # #{v < t}
        return self.cum[np.searchsorted(self.v, t, side="left")]

    def upto(self, t):              # #{v <= t}
        return self.cum[np.searchsorted(self.v, t, side="right")]

    def total(self):
        return int(self.cum[-1])


def check_band(ref, counts, outside, edges, label):
    """the band rule at every edge (the outer ones included); returns the largest band occupancy"""
    ref = ref if isinstance(ref, Weighted) else Weighted(ref)
    counts = counts.cpu().numpy().astype(np.int64)
    under, over = (int(v) for v in outside.cpu().tolist())
    e = edges.cpu().double().numpy()
    bins = len(counts)
    assert len(e) == bins + 1
    assert counts.min() >= 0 and under >= 0 and over >= 0
    assert counts.sum() + under + over == ref.total(), (label, int(counts.sum()), under, over, ref.total())
    cum = under + np.concatenate([[0], np.cumsum(counts)])           # cum[b] = C_gpu(e_b): values below edge b
    worst = 0
    for b in range(bins):                                            # edge b as a LOWER edge: values < e_b
        lo, hi = ref.below(e[b] - DELTA), ref.upto(e[b] + DELTA)
        assert lo <= cum[b] <= hi, (label, "edge", b, float(e[b]), int(lo), int(cum[b]), int(hi))
        worst = max(worst, int(hi - lo))
    # the last edge closes its bin on the right: everything up to and including it is inside
    lo, hi = ref.upto(e[bins] - DELTA), ref.upto(e[bins] + DELTA)
    assert lo <= cum[bins] <= hi, (label, "last edge", float(e[bins]), int(lo), int(cum[bins]), int(hi))
    return max(worst, int(hi - lo))


def planted(x):
    x[5] = 0.0                      # a zero row: cosines exactly 0
    x[7] = x[6]                     # a duplicate pair: cosine 1 (may round to 1 + 1 ulp)
    x[9] = -x[8]                    # an antipodal pair: cosine -1
    return x


def shape_randn():
    g = torch.Generator().manual_seed(11)
    x = planted(torch.randn(3000, 64, generator=g))
    y = torch.randint(0, 7, (3000,), generator=g)
    y[torch.rand(3000, generator=g) < 0.05] = -1
    return x, y.int()


def shape_clusters():
    g = torch.Generator().manual_seed(12)
    c = torch.randint(0, 7, (2500,), generator=g)
    x = planted(torch.randn(7, 128, generator=g)[c] + 0.7 * torch.randn(2500, 128, generator=g))
    y = c.clone()
    y[torch.rand(2500, generator=g) < 0.05] = -1
    return x, y.int()


def shape_generic():                # F = 50: the any-F path (both panels through LDS)
    g = torch.Generator().manual_seed(13)
    x = planted(torch.randn(1100, 50, generator=g) + 0.3)
    return x, torch.randint(-1, 4, (1100,), generator=g).int()


SHAPES = {"randn_3000x64": shape_randn, "clusters_2500x128": shape_clusters, "generic_1100x50": shape_generic}
_cache = {}


def shape(name):
    if name not in _cache:
        x, y = SHAPES[name]()
        _cache[name] = (x, y) + sorted_groups(x, y)
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------
# 1. exact cases
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f", [(1, 7), (2, 1), (2, 33), (20, 7), (31, 1), (100, 33), (129, 7), (300, 128), (515, 200),
                                 (700, 128), (1000, 1)])
def test_exact_one_hot(cuda, n, f):
    """one-hot rows scaled by powers of two plus zero rows: every cosine is exactly 0 or exactly 1"""
    from sngnn_amd import toolbox as T
    g = torch.Generator().manual_seed(100 * n + f)
    cls = torch.randint(0, min(f, 5), (n,), generator=g)
    scale = 2.0 ** torch.randint(-3, 4, (n,), generator=g).float()
    x = torch.zeros(n, f)
    x[torch.arange(n), cls] = scale
    zero = torch.rand(n, generator=g) < 0.15
    x[zero] = 0.0
    y = cls.int()                                        # zero rows keep a label too
    nz = ~zero
    off = ~torch.eye(n, dtype=torch.bool)
    one = (cls[:, None] == cls[None, :]) & nz[:, None] & nz[None, :] & off
    same = (cls[:, None] == cls[None, :]) & off
    n_c = torch.bincount(cls[nz], minlength=5)
    ones = int((n_c * (n_c - 1)).sum())
    assert int(one.sum()) == ones
    pairs = n * (n - 1)

    h = T.node_similarity_histogram(x.to(cuda), bins=200, range=(-1.0, 1.0))
    assert h.counts.shape == (200,) and h.counts.dtype == torch.int64 and h.edges.shape == (201,)
    assert h.edges.dtype == torch.float32 and h.outside.shape == (2,)
    e = h.edges.cpu()
    # (float64 linspace puts edge 100 at -2.08e-17, not at 0.0: still at or below 0.0, which belongs above it)
    assert e[100] <= 0.0 < e[101] and e[0] == -1.0 and e[200] == 1.0
    want = torch.zeros(200, dtype=torch.int64)
    want[199] = ones                                     # 1.0: the last bin, closed on the right
    want[100] += pairs - ones                            # 0.0: an inner edge, the UPPER bin
    assert torch.equal(h.counts.cpu(), want), (h.counts.cpu().nonzero().flatten(), ones, pairs)
    assert int(h.outside.sum()) == 0
    if n <= 1:
        assert h.minimum.item() == float("inf") and h.maximum.item() == float("-inf")
    else:
        assert h.minimum.item() == (0.0 if pairs > ones else 1.0)
        assert h.maximum.item() == (1.0 if ones else 0.0)
        assert abs(h.mean.item() - ones / pairs) <= 1e-15    # (the sum is exact; the device's f64 division may be an ulp off)

    # four bins: the edges -1, -0.5, 0, 0.5, 1 are exact, 0.0 IS an inner edge and belongs to the bin above it
    h4 = T.node_similarity_histogram(x.to(cuda), bins=4, range=(-1.0, 1.0))
    assert h4.edges.cpu().tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0]
    assert h4.counts.cpu().tolist() == [0, 0, pairs - ones, ones]

    hy = T.node_similarity_histogram(x.to(cuda), bins=200, range=(-1.0, 1.0), y=y.to(cuda))
    assert hy.counts.shape == (2, 200) and hy.outside.shape == (2, 2)
    want2 = torch.zeros(2, 200, dtype=torch.int64)
    want2[0, 199] = ones                                 # the ones are all pairs of one class
    want2[0, 100] = int(same.sum()) - ones               # ... plus the zero-row pairs of equal label
    want2[1, 100] = pairs - int(same.sum())
    assert torch.equal(hy.counts.cpu(), want2)
    # unclamped, a range whose last edge is below 1: the ones are reported as `over`
    hu = T.node_similarity_histogram(x.to(cuda), bins=37, range=(0.0, 0.5), clamp=False)
    assert int(hu.counts.cpu()[0]) == pairs - ones and int(hu.counts.sum()) == pairs - ones
    assert hu.outside.cpu().tolist() == [0, ones]


# ---------------------------------------------------------------------------------------------------------
# 2. band check against float64
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob5", [0, 1])
@pytest.mark.parametrize("rng,clamp", [((-1.0, 1.0), True), ((0.25, 0.5), True), ((0.25, 0.5), False), (None, True)])
@pytest.mark.parametrize("bins", [1, 37, 200, 1024])
@pytest.mark.parametrize("name", list(SHAPES))
def test_band_against_float64(cuda, name, bins, rng, clamp, knob5):
    from sngnn_amd import _lib, toolbox as T
    x, y, s_all, s_same, s_diff = shape(name)
    n = x.size(0)
    lib = _lib.load()
    assert lib.sngnn_tuning_set(5, knob5) == 0
    try:
        h = T.node_similarity_histogram(x.to(cuda), bins=bins, range=rng, y=y.to(cuda), clamp=clamp)
        h1 = T.node_similarity_histogram(x.to(cuda), bins=bins, range=rng, clamp=clamp)
        torch.cuda.synchronize()
    finally:
        lib.sngnn_tuning_set(5, 0)
    label = (name, bins, rng, clamp, knob5)
    assert h.counts.shape == (2, bins) and h1.counts.shape == (bins,)
    assert int(h.counts.sum() + h.outside.sum()) == n * (n - 1)
    assert int(h1.counts.sum() + h1.outside.sum()) == n * (n - 1)
    if clamp:
        # the fold: judged as numpy would judge the values clipped into the range
        assert int(h.outside.sum()) == 0 and int(h1.outside.sum()) == 0
        lo, hi = float(h.edges[0]), float(h.edges[-1])
        refs = [np.clip(s, lo, hi) for s in (s_same, s_diff, s_all)]
    else:
        refs = [s_same, s_diff, s_all]
    if rng is None:
        assert abs(float(h.edges[0]) - s_all[0]) <= DELTA and abs(float(h.edges[-1]) - s_all[-1]) <= DELTA
        assert float(h1.edges[0]) == h1.minimum.item() and float(h1.edges[-1]) == h1.maximum.item()
    worst = max(check_band(refs[0], h.counts[0], h.outside[0], h.edges, label + ("same",)),
                check_band(refs[1], h.counts[1], h.outside[1], h.edges, label + ("different",)),
                check_band(refs[2], h1.counts, h1.outside, h1.edges, label + ("all",)))
    assert abs(h1.minimum.item() - s_all[0]) <= DELTA and abs(h1.maximum.item() - s_all[-1]) <= DELTA
    assert abs(h1.mean.item() - s_all.mean()) <= DELTA          # (every value is within DELTA, so is their mean)
    print(f"band {label}: largest band occupancy {worst} of {n * (n - 1)} values")


# ---------------------------------------------------------------------------------------------------------
# 3. scale: config 4's node count
# ---------------------------------------------------------------------------------------------------------
def scale_case():
    """R shuffled copies of a base table: the histogram is R^2 hist64(base, off-diagonal) + m R (R - 1) [1.0]."""
    from sngnn_amd import toolbox as T
    dev = torch.device("cuda:0")
    R, m, f = 85, 2000, 128
    g = torch.Generator().manual_seed(5)
    c = torch.randint(0, 6, (m,), generator=g)
    base = torch.randn(6, f, generator=g)[c] + 0.8 * torch.randn(m, f, generator=g)
    x = base.repeat(R, 1)[torch.randperm(R * m, generator=g)]
    n = R * m
    s = cos64(base)
    off = ~torch.eye(m, dtype=torch.bool)
    vals = np.concatenate([s[off].numpy(), [1.0]])
    weights = np.concatenate([np.full(m * (m - 1), R * R, dtype=np.int64), [m * R * (R - 1)]])
    ref = Weighted(vals, weights)
    assert ref.total() == n * (n - 1)
    h = T.node_similarity_histogram(x.to(dev), bins=200, range=(-1.0, 1.0), clamp=False)
    worst = check_band(ref, h.counts, h.outside, h.edges, ("scale",))
    mean = T.node_similarity_dense_large_parted(x.to(dev), corrected=True)[1]
    diff = abs(h.mean.item() - mean.item())
    print(f"scale N={n}: largest band occupancy {worst} of {n * (n - 1)}; mean {h.mean.item():.9f} "
          f"against the class-sum route {mean.item():.9f} (diff {diff:.2e})")
    assert diff <= 1e-6
    want_mean = float((ref.v * np.diff(ref.cum)).sum() / ref.total())
    assert abs(h.mean.item() - want_mean) <= 1e-6


def test_scale_170000(cuda):
    """run once, in a process of its own with its own time limit"""
    code = ("import sys; sys.path.insert(0, %r); "
            "from tests.test_similarity_hist_gpu import scale_case; scale_case()" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=420)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------
# 4. determinism and plumbing
# ---------------------------------------------------------------------------------------------------------
def bits(t):
    return t.cpu().numpy().tobytes()


def test_two_calls_agree_bit_for_bit(cuda):
    from sngnn_amd import toolbox as T
    x, y = shape("clusters_2500x128")[:2]
    xg, yg = x.to(cuda), y.to(cuda)
    for kw in (dict(), dict(y=yg), dict(range=None), dict(bins=1024, range=(0.25, 0.5), clamp=False, y=yg)):
        a, b = T.node_similarity_histogram(xg, **kw), T.node_similarity_histogram(xg, **kw)
        assert torch.equal(a.counts, b.counts) and torch.equal(a.outside, b.outside) and torch.equal(a.edges, b.edges)
        for k in ("minimum", "maximum", "mean"):
            assert bits(getattr(a, k)) == bits(getattr(b, k)), (kw.keys(), k)


def test_grouped_rows_add_up_to_the_ungrouped_counts(cuda):
    from sngnn_amd import toolbox as T
    for name in SHAPES:
        x, y = shape(name)[:2]
        for kw in (dict(), dict(bins=1024, range=(0.25, 0.5), clamp=False), dict(bins=37, range=None)):
            a = T.node_similarity_histogram(x.to(cuda), **kw)
            b = T.node_similarity_histogram(x.to(cuda), y=y.to(cuda), **kw)
            assert torch.equal(b.counts.sum(0), a.counts) and torch.equal(b.outside.sum(0), a.outside)
            assert bits(a.minimum) == bits(b.minimum) and bits(a.maximum) == bits(b.maximum)
            assert bits(a.mean) == bits(b.mean)


def test_counter_table_copies_do_not_change_a_count(cuda):
    """knob 10: one LDS copy of the counters (the plain form) against the spread forms"""
    from sngnn_amd import _lib, toolbox as T
    lib = _lib.load()
    x, y = shape("clusters_2500x128")[:2]
    want = T.node_similarity_histogram(x.to(cuda), y=y.to(cuda))
    try:
        for copies in (1, 2, 4, 8, 16):
            assert lib.sngnn_tuning_set(10, copies) == 0
            got = T.node_similarity_histogram(x.to(cuda), y=y.to(cuda))
            assert torch.equal(got.counts, want.counts) and bits(got.mean) == bits(want.mean), copies
    finally:
        lib.sngnn_tuning_set(10, 0)


def test_graph_capture_on_a_side_stream(cuda):
    from sngnn_amd import toolbox as T
    x, y = shape("randn_3000x64")[:2]
    xg, yg = x.to(cuda), y.to(cuda)
    want = T.node_similarity_histogram(xg, y=yg)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(side):
        T.node_similarity_histogram(xg, y=yg)          # warm-up on the side stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = T.node_similarity_histogram(xg, y=yg)
    for _ in range(2):
        got.counts.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got.counts, want.counts) and torch.equal(got.outside, want.outside)
        assert bits(got.mean) == bits(want.mean) and bits(got.minimum) == bits(want.minimum)
    with pytest.raises(RuntimeError, match="range=None"):
        graph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph2, stream=side):
            T.node_similarity_histogram(xg, range=None)


@pytest.mark.parametrize("n,f", [(3000, 64), (4099, 128), (1500, 50)])
def test_against_the_materialised_route(cuda, n, f):
    """the ungrouped histogram against the values ``node_similarity_dense_small`` returns (another kernel: the
    contraction is split differently, so the band rule, not bit equality)"""
    from sngnn_amd import toolbox as T
    g = torch.Generator().manual_seed(n)
    x = planted(torch.randn(n, f, generator=g) + 0.2).to(cuda)
    sim, mean = T.node_similarity_dense_small(x)
    ref = np.sort(sim.double().cpu().numpy())
    for kw in (dict(), dict(bins=1024, range=(-0.2, 0.4), clamp=False), dict(bins=37, range=None)):
        h = T.node_similarity_histogram(x, **kw)
        r = np.clip(ref, float(h.edges[0]), float(h.edges[-1])) if kw.get("clamp", True) else ref
        worst = check_band(r, h.counts, h.outside, h.edges, (n, f, tuple(kw)))
        print(f"materialised route ({n}, {f}) {kw}: largest band occupancy {worst}")
    assert abs(h.mean.item() - mean.item()) <= 1e-6

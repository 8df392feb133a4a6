// Node-similarity distribution at any N (gfx950): the histogram of all N (N - 1) off-diagonal cosines of
// a feature table, optionally split by whether the two nodes share a label - what the reference's toolbox draws
// (SimGFAToolbox/plot.py:61, `sns.distplot(sim, bins=200)`) from the `sim` of dense.py:144-149, and cannot draw
// where dense.py:9-30 returns `None, mean`.  One scan of the table; S is never stored.
//
// Tile walk.  The products come from the tile engine of the kNN scan (cosine_tiles.h: a workgroup's row block
// against one column tile after another on the matrix cores, fp32 rounding; knob 5 = 1: fp32 MFMAs).  S is
// symmetric and the count runs over ordered pairs i != j, so a row block only visits the column tiles that hold
// a j > i, counts the elements with j > i and gives each the weight 2: half the products of a kNN scan.  (The
// tiles that straddle the diagonal are computed whole and their j <= i part is dropped - at most KR / KC + 1
// tiles of a row block's N / KC.  The value counted for the pair {i, j} is the engine's S[i][j], i < j.)
// blockIdx.y cuts a row block's tiles into ranges so that the triangle's long first rows do not set the run time.
//
// Bin rule (numpy's): value s belongs to bin b with edges[b] <= s < edges[b + 1], the last bin closed on the
// right; s < edges[0] goes to the `under` slot, s > edges[bins] to `over`.  The candidate bin comes from one
// multiply-add, (s - edges[0]) * bins / (edges[bins] - edges[0]), and is then moved down / up against the edge
// table in LDS until the rule holds: the result agrees with the caller's table exactly, whatever the rounding of
// the candidate (and whatever the spacing of the table, as long as it ascends).
//
// Counting.  u32 counters in LDS, LDS integer atomics (`ds_add_u32`), flushed with vector u64 atomics to the
// global counters at the end of the workgroup's range (and every 2^16 tiles: a tile adds at most 2^15 to a
// counter).  Integer sums: the same bits in any order.  Cosine distributions are concentrated - the 64 lanes of
// one atomic instruction mostly hit the same few bins - so the table exists in up to 16 copies selected by the
// lane's low bits and the copies are added at the flush (knob 10: 1 = one copy, the plain form; DESIGN.md 4.5
// has the measurement).
//
// Groups.  With labels (y int32 [N]) the counters are [2][bins + 2]: row 0 for y_i == y_j, row 1 for
// y_i != y_j.  A NEGATIVE label means "unlabelled": every pair with an unlabelled node is counted in row 1.
//
// Statistics.  min, max (fp32) and sum (f64) of the counted values: per lane over its elements in scan order,
// then lanes, waves and workgroups in a fixed tree - the same bits on every run.  No float atomics.
//
// This header holds the kernels and the launch plan; cosine_hist.hip launches them on fp32 tables (sngnn_cosine_hist),
// cosine_hist_half.hip on fp16 / bf16 tables (sngnn_cosine_hist_half: the engine's PL < 3).
#pragma once
#include <algorithm>

#include "cosine_tiles.h"

namespace sngnn {

constexpr int CH_MAX_BINS = 1024;
constexpr int CH_CNT = 5632;                 // u32 counters in LDS: copies x groups x (bins + 2)
constexpr int CH_MAX_COPIES = 16;
constexpr int CH_FLUSH_TILES = 1 << 16;

template <int FH, bool BF3, int NWV, int CB, int PL = 3>
__global__ __launch_bounds__(64 * NWV) void k_cosine_hist(const typename CosineTiles<FH, BF3, NWV, CB, PL>::XT *__restrict__ x, int64_t N, int64_t F,
                                                         const float *__restrict__ inv, const int32_t *__restrict__ y,
                                                         const float *__restrict__ edges, int bins, int ncopy,
                                                         int tiles_per_split, unsigned long long *__restrict__ counts,
                                                         float *__restrict__ pmin, float *__restrict__ pmax,
                                                         double *__restrict__ psum)
{
    using Eng = CosineTiles<FH, BF3, NWV, CB, PL>;
    constexpr int KR = Eng::KR, KC = Eng::KC;
    __shared__ float sA[Eng::SA_FLOATS];
    __shared__ __align__(16) float sB[Eng::SB_FLOATS];
    __shared__ float s_edge[CH_MAX_BINS + 1];
    __shared__ unsigned s_cnt[CH_CNT];
    __shared__ float s_irow[KR];
    __shared__ int s_yrow[KR];
    __shared__ float s_mn[NWV], s_mx[NWV];
    __shared__ double s_sm[NWV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * KR;
    const int64_t ncol_tiles = (N + KC - 1) / KC;
    // the first tile with a column j > i for some row i of the block is the one that holds row0 + 1
    const int64_t ct_begin = std::max<int64_t>((row0 + 1) / KC, (int64_t)blockIdx.y * tiles_per_split);
    const int64_t ct_end = std::min<int64_t>(ncol_tiles, ((int64_t)blockIdx.y + 1) * tiles_per_split);
    const size_t slot_out = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (ct_begin >= ct_end) {                                   // (workgroup-uniform) nothing above the diagonal here
        if (tid == 0) { pmin[slot_out] = INFINITY; pmax[slot_out] = -INFINITY; psum[slot_out] = 0.0; }
        return;
    }
    const int groups = y != nullptr ? 2 : 1;
    const int width = groups * (bins + 2);                      // counters of one copy
    for (int q = tid; q <= bins; q += 64 * NWV) s_edge[q] = edges[q];
    for (int q = tid; q < ncopy * width; q += 64 * NWV) s_cnt[q] = 0u;
    for (int q = tid; q < KR; q += 64 * NWV) {
        const int64_t i = row0 + q;
        s_irow[q] = i < N ? inv[i] : 0.f;
        s_yrow[q] = (y != nullptr && i < N) ? y[i] : -1;
    }
    Eng eng;
    eng.load_rows(x, N, F, row0);
    __syncthreads();
    const float e_lo = s_edge[0], e_hi = s_edge[bins];
    const float scale = (float)bins / (e_hi - e_lo), off = -e_lo * scale;
    unsigned *my_cnt = s_cnt + (lane & (ncopy - 1)) * width + 1;       // (+ 1: slot 0 is `under`)
    float vmin = INFINITY, vmax = -INFINITY;
    double vsum = 0.0;

    auto flush = [&]() {
        __syncthreads();
        for (int q = tid; q < width; q += 64 * NWV) {
            unsigned long long v = 0ull;
            for (int c = 0; c < ncopy; ++c) {
                v += s_cnt[c * width + q];
                s_cnt[c * width + q] = 0u;
            }
            if (v != 0ull) atomicAdd(&counts[q], v);
        }
        __syncthreads();
    };

    for (int64_t ct = ct_begin; ct < ct_end; ++ct) {
        const int64_t col0 = ct * KC;
        f32x16 acc[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        // the tile's column ids, inverse norms and labels: requested here, they travel under the products
        float icol[CB];
        int64_t jcol[CB];
        int ycol[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            jcol[b] = col0 + b * 32 + l32;
            icol[b] = inv[min(jcol[b], N - 1)];
            ycol[b] = y != nullptr ? y[min(jcol[b], N - 1)] : 0;
        }
        eng.products(x, N, F, row0, ct, ct_begin, ct_end, sA, sB, acc);
        // ---- count: C/D layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        // Straight-line per accumulator register: candidate bins of its CB values by one multiply-add each, the two
        // edges around every candidate read together (no dependent LDS round trips), one step down / up where the
        // value is outside them.  Only a value that HAD to move is checked again, by the loops of the slow path
        // (for an evenly spaced table the candidate is off by at most one: a value within rounding of an edge;
        // the first version ran the two loops for every value - two dependent LDS reads each - and took 52 ms at
        // arxiv size where this takes less).
        const bool straddles = col0 < row0 + KR;                 // (workgroup-uniform) the tile holds some j <= i
        int jc[CB];
        bool jok[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b) { jc[b] = (int)jcol[b]; jok[b] = jcol[b] < N; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int i = (int)row0 + lr;
            const float irow = s_irow[lr];
            const int yrow = s_yrow[lr];
            float sv[CB], e0[CB], e1[CB];
            int cb[CB];
#pragma unroll
            for (int b = 0; b < CB; ++b) {
                sv[b] = acc[b][r] * (irow * icol[b]) + 0.0f;
                cb[b] = min(max((int)__fmaf_rn(sv[b], scale, off), 0), bins - 1);
                e0[b] = s_edge[cb[b]];
                e1[b] = s_edge[cb[b] + 1];
            }
            bool ok[CB], slow[CB], any_slow = false;
#pragma unroll
            for (int b = 0; b < CB; ++b) {
                ok[b] = jok[b] && (!straddles || jc[b] > i);              // (j > i and j < N: i < N too)
                const bool down = sv[b] < e0[b], up = sv[b] >= e1[b] && cb[b] < bins - 1;
                const bool outside = sv[b] < e_lo || sv[b] > e_hi;
                cb[b] += (up ? 1 : 0) - (down ? 1 : 0);
                slow[b] = ok[b] && (down || up) && !outside;
                any_slow |= slow[b];
            }
            if (any_slow) {                                               // rare: the moved values, against the table
#pragma unroll
                for (int b = 0; b < CB; ++b)
                    if (slow[b]) {
                        int bin = min(max(cb[b], 0), bins - 1);
                        while (bin > 0 && sv[b] < s_edge[bin]) --bin;
                        while (bin < bins - 1 && sv[b] >= s_edge[bin + 1]) ++bin;
                        cb[b] = bin;
                    }
            }
#pragma unroll
            for (int b = 0; b < CB; ++b) {
                int bin = cb[b];
                if (sv[b] < e_lo) bin = -1;
                if (sv[b] > e_hi) bin = bins;
                const int g = (groups == 2 && !(yrow >= 0 && yrow == ycol[b])) ? bins + 2 : 0;
                if (ok[b]) {
                    atomicAdd(my_cnt + g + bin, 2u);
                    vmin = fminf(vmin, sv[b]);
                    vmax = fmaxf(vmax, sv[b]);
                    vsum += (double)sv[b];
                }
            }
        }
        if (((ct - ct_begin) & (CH_FLUSH_TILES - 1)) == CH_FLUSH_TILES - 1) flush();
    }
    flush();
    // the workgroup's statistics: lanes (xor tree), then its waves in order
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        vmin = fminf(vmin, __shfl_xor(vmin, m, 64));
        vmax = fmaxf(vmax, __shfl_xor(vmax, m, 64));
        vsum += __shfl_xor(vsum, m, 64);
    }
    if (lane == 0) { s_mn[wave] = vmin; s_mx[wave] = vmax; s_sm[wave] = vsum; }
    __syncthreads();
    if (tid == 0) {
        float a = s_mn[0], c = s_mx[0];
        double d = s_sm[0];
        for (int w = 1; w < NWV; ++w) { a = fminf(a, s_mn[w]); c = fmaxf(c, s_mx[w]); d += s_sm[w]; }
        pmin[slot_out] = a;
        pmax[slot_out] = c;
        psum[slot_out] = 2.0 * d;                                // (every pair stands for (i, j) and (j, i))
    }
}

// (static, as k_hist_stats below: one copy per translation unit that launches it)
static __global__ void k_hist_zero(unsigned long long *__restrict__ counts, int n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) counts[t] = 0ull;
}

// stats = {min, max, sum} of the workgroups' partial results in a FIXED order (one workgroup: thread t takes
// parts t, t + 1024, ... in sequence, then a tree over the threads); no parts: +inf, -inf, 0
static __global__ __launch_bounds__(1024) void k_hist_stats(const float *__restrict__ pmin, const float *__restrict__ pmax,
                                                     const double *__restrict__ psum, int64_t n,
                                                     double *__restrict__ stats)
{
    __shared__ float s_a[1024], s_c[1024];
    __shared__ double s_d[1024];
    float a = INFINITY, c = -INFINITY;
    double d = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        a = fminf(a, pmin[i]);
        c = fmaxf(c, pmax[i]);
        d += psum[i];
    }
    s_a[threadIdx.x] = a; s_c[threadIdx.x] = c; s_d[threadIdx.x] = d;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_a[threadIdx.x] = fminf(s_a[threadIdx.x], s_a[threadIdx.x + w]);
            s_c[threadIdx.x] = fmaxf(s_c[threadIdx.x], s_c[threadIdx.x + w]);
            s_d[threadIdx.x] += s_d[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = (double)s_a[0];
        stats[1] = (double)s_c[0];
        stats[2] = s_d[0];
    }
}

// ---------------------------------------------------------------------------
// Launch plan (host), shared by the fp32 and the half entry - one workspace size for both.
// ---------------------------------------------------------------------------
struct HistPlan { int64_t nrb, nct; int tps, ns; };
// enough column ranges that the triangle's ~nrb ns / 2 non-empty workgroups keep the CUs busy to the end, at
// least 16 tiles each (the rows' operands and the counter flush are paid once per workgroup)
static HistPlan hist_plan(int64_t N, int rows_wg, int cols_tile)
{
    HistPlan p;
    p.nrb = (N + rows_wg - 1) / rows_wg;
    p.nct = (N + cols_tile - 1) / cols_tile;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>((4096 + p.nrb - 1) / p.nrb, p.nct / 16));
    p.tps = (int)((p.nct + want - 1) / want);
    p.ns = (int)((p.nct + p.tps - 1) / p.tps);
    return p;
}

static int64_t hist_parts(int64_t N)
{
    if (N <= 1) return 0;
    const HistPlan a = hist_plan(N, 256, 64), b = hist_plan(N, KN_M, KN_M);
    return std::max(a.nrb * a.ns, b.nrb * b.ns);
}

// copies of the LDS counter table for `width` counters a copy (copies_knob: knob 10, 0 = as many as fit)
static int hist_copies(int width, int copies_knob)
{
    int ncopy = 1;
    while (ncopy * 2 <= CH_MAX_COPIES && ncopy * 2 * width <= CH_CNT) ncopy *= 2;
    return copies_knob > 0 ? std::min(ncopy, copies_knob) : ncopy;
}

}  // namespace sngnn

// SNGNN++ adjacency-linear branch (gfx950): Linear(num_nodes, C) applied to the
// sparse adjacency, models/models.py:124-130, as a row gather-sum
//     forward   out0[i] = b + sum_{e : src_e - src_min == i} Wt[dst_e]      (CSC rows)
//     backward  dWt[d]  =     sum_{e : dst_e == d}           g0[src_e - src_min]   (CSR rows)
// Wt is the [N, C] transpose of the reference's w.weight so that every gathered
// operand is one contiguous row.  Same degree classes and fixed summation order
// as the aggregation kernels; no atomics.
#pragma once
#include "row_walk.h"

namespace sngnn {

struct AdjArgs : RowSide {      // segments (CSR or CSC), gathered ids, degree order: row_walk.h
    const float *table;         // rows to gather  [N, C]
    const float *w;             // per-entry weights in SEGMENT order (w[ptr[seg] + t]) or nullptr = 1 (weighted gather-sum:
                                // GGCNlayer_SP's plain propagation, models.py:1544-1549)
    const float *bias;          // [C] or nullptr
    float *out;                 // [N, C]
    float *partial;             // [n_tasks, C]
    int C, N;
    int seg_shift;              // output row r reads segment r + seg_shift
    int idx_shift;              // gathered row = idx[q] + idx_shift
};

template <int VEC, int G, int R>
__device__ __forceinline__ void adj_finish(const AdjArgs &a, int r, int lg, Row<VEC, G, R> &acc)
{
    if (a.bias) {
        Row<VEC, G, R> b;
        b.load(a.bias, a.C, lg);
        b.add(acc);              // bias first, then the gathered rows (sparse addmm order)
        acc = b;
    }
    acc.store(a.out + (size_t)r * a.C, a.C, lg);
}

// the gather-sum of table rows (value * row rounded, then added, where there are weights: a sparse mm's order), then
// adj_finish for the segments that have an output row
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_adj(const AdjArgs a)
{
    using RowT = Row<VEC, G, R>;
    RowT acc;
    walk_rows<G>(
        a, blockIdx.x, a.N, acc,
        [&](int, int qs, int e0, int e1, int stride, int first, int lg, RowT &s) {
            gather_rows<VEC, G, R, gather_unroll(R)>(a.table, a.C, a.C, a.idx, qs, e0, e1, stride, first, lg, s,
                                                     EntryWeight{a.w}, a.idx_shift);
        },
        [&](int tq, int lg, RowT &s) { s.store(a.partial + (size_t)tq * a.C, a.C, lg); },
        [&](int seg, int, int lg, RowT &s) {
            if (seg - a.seg_shift >= 0) adj_finish<VEC, G, R>(a, seg - a.seg_shift, lg, s);
        });
}

// split segments: the sum of the tasks' partial rows (+ bias)
static __global__ __launch_bounds__(256) void k_adj_fin(const AdjArgs a)
{
    __shared__ float s[4][64];
    const int p = blockIdx.x;
    const int seg = a.perm[p];
    const int r = seg - a.seg_shift;
    if (r < 0) return;                                  // block-uniform
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    for (int c0 = 0; c0 < a.C; c0 += 64) {
        const int c = c0 + cl;
        const float sum = combine_task_sums(s, sum_task_partials(a.partial, a.C, t0, t1, c, q), q, cl);
        if (q == 0 && c < a.C) a.out[(size_t)r * a.C + c] = sum + (a.bias ? a.bias[c] : 0.f);
        __syncthreads();
    }
}

// output rows whose segment lies beyond the node range (src_min > 0): bias only
static __global__ void k_adj_tail(const AdjArgs a, int first_row)
{
    const int64_t n = (int64_t)(a.N - first_row) * a.C;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x)
        a.out[(size_t)first_row * a.C + t] = a.bias ? a.bias[t % a.C] : 0.f;
}

// out[e] = <A[ia[e]], B[ib[e]]> for e in [0, E): one lane group per entry, two entries per group in flight
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_pair_dot(const float *__restrict__ A, const int32_t *__restrict__ ia,
                                                    const float *__restrict__ B, const int32_t *__restrict__ ib,
                                                    int64_t E, int C, float *__restrict__ out)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    const int lane = lane_id(), gid = lane / G, lg = lane % G;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6, nw = (int64_t)gridDim.x * WAVES;
    for (int64_t base = wave * 2 * NG; base < E; base += nw * 2 * NG) {
        const int64_t e0 = base + gid, e1 = base + NG + gid;
        const int64_t c0 = e0 < E ? e0 : E - 1, c1 = e1 < E ? e1 : E - 1;
        RowT a0, b0, a1, b1;
        a0.load(A + (size_t)ia[c0] * C, C, lg);
        b0.load(B + (size_t)ib[c0] * C, C, lg);
        a1.load(A + (size_t)ia[c1] * C, C, lg);
        b1.load(B + (size_t)ib[c1] * C, C, lg);
        const float d0 = group_sum<G>(a0.dot_partial(b0)), d1 = group_sum<G>(a1.dot_partial(b1));
        if (lg == 0) {
            if (e0 < E) out[e0] = d0;
            if (e1 < E) out[e1] = d1;
        }
    }
}
template <int VEC, int G, int R>
int launch_pair_dot(const float *A, const int32_t *ia, const float *B, const int32_t *ib, int64_t E, int C, float *out,
                    hipStream_t st)
{
    if (E == 0) return SNGNN_OK;
    const int grid = (int)std::min<int64_t>(ceil_div(E, (int64_t)2 * (64 / G) * WAVES), 256 * 8);
    k_pair_dot<VEC, G, R><<<grid, BLOCK, 0, st>>>(A, ia, B, ib, E, C, out);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <int VEC, int G, int R> int launch_adj(const AdjArgs &a0, hipStream_t st)
{
    AdjArgs a = a0;
    const int grid = plan_side(a, a.N, 64 / G);
    if (grid > 0) k_adj<VEC, G, R><<<grid, BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_adj_fin<<<a.n_split, 256, 0, st>>>(a);
    if (a.seg_shift > 0) k_adj_tail<<<std::min(1024, ceil_div((int64_t)a.seg_shift * a.C, 256)), 256, 0, st>>>(a, a.N - a.seg_shift);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

}  // namespace sngnn

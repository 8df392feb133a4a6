// GCNConv and MixHop's layer (models/models.py:539-580, 693-786; PyG 2.0.4's GCNConv), gfx950, fp32: one hop over
//     A^ = D^-1/2 (A + I) D^-1/2     (prop.hip's adjacency: deg_i = in-degree with the loop, dinv = deg^-1/2)
// on a COLUMN SLICE of a wider table, with a split store:
//     z_i = dinv_i S_i,  S_i = sum_{e -> i} dinv_src src[src, 0 .. W)
// The row-class walk of row_walk.h (small rows by lane group, medium rows by wave, hubs as 128-edge tasks + a finalize;
// the rows gathered UNSCALED and multiplied by dinv[src], which is loaded next to the column id; fixed summation order,
// no atomics; every product and sum rounded separately: -ffp-contract=off).  New here:
//   strided rows   source and destinations are W columns of tables with their own row strides
//   split store    the first W0 columns of z go to dst0 (with the epilogue: + bias, the running-statistics norm, relu),
//                  the other W - W0 to dst1.  MixHop's launch j gathers the hops - j + 1 slices that still need
//                  propagating as ONE wide row per edge (one read of the column id and of dinv[src] for all of them),
//                  stores the finished slice into its place in the concatenated output and the rest into a ping-pong
//                  buffer
//   pass-through   Wp columns of row i copied from pass_src to pass_dst by whoever completes row i (MixHop's slice 0)
// The lane layout (G lanes a group, 64 / G groups a wave) is row_cfg(W)'s, whatever the vector width: a narrower VEC
// than W's own (a misaligned slice, a W0 that W's vec does not divide) takes R * (vec_W / VEC) steps per lane on the
// SAME groups, so the edges a group sums and the order of the sums depend on W and the graph alone - a slice of a wide
// table gives the bits of the dense call.
#include <algorithm>

#include "entry.h"
#include "row_walk.h"

namespace sngnn {

constexpr int COLSUM_BLOCKS = 1024;          // partial column sums of sngnn_gcn_bias_grad

struct GcnArgs : RowSide {
    const float *src;            // column 0 of the gathered slice
    float *dst0, *dst1;
    const float *pass_src;
    float *pass_dst;
    int64_t ld_src, ld0, ld1, ld_ps, ld_pd;
    int W, W0, Wp, relu;
    const float *bias, *rm, *invstd, *gamma, *beta;
    const float *dinv;           // [N]
    float *partial;              // [n_tasks, W]
    int N;
};

// the epilogue of one dst0 element (column c < W0)
__device__ __forceinline__ float gcn_epilogue(const GcnArgs &a, int c, float z)
{
    if (a.bias) z = z + a.bias[c];
    if (a.rm) z = ((z - a.rm[c]) * a.invstd[c]) * a.gamma[c] + a.beta[c];
    if (a.relu) z = z > 0.f ? z : 0.f;
    return z;
}

// row r from its gathered sum s: the scale by dinv_r, the split store, the pass-through copy (G lanes)
template <int VEC, int G, int R>
__device__ __forceinline__ void gcn_finish(const GcnArgs &a, int r, int lg, Row<VEC, G, R> &s)
{
    s.scale(a.dinv[r]);
    float *d0 = a.dst0 + (size_t)r * a.ld0;
    float *d1 = a.dst1 + (size_t)r * a.ld1 - a.W0;          // (column c of z is d1[c]; touched only where dst1 is set)
    const bool epi = a.bias || a.rm || a.relu;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int c0 = (q * G + lg) * VEC;
        if (c0 < a.W0) {                                     // (VEC divides W0: a lane's channels are on one side)
            if (epi) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) s.x[q][v] = gcn_epilogue(a, c0 + v, s.x[q][v]);
            }
            store_vec<VEC>(d0 + c0, s.x[q]);
        } else if (c0 < a.W) {
            store_vec<VEC>(d1 + c0, s.x[q]);
        }
    }
    if (a.Wp > 0) {
        const float *ps = a.pass_src + (size_t)r * a.ld_ps;
        float *pd = a.pass_dst + (size_t)r * a.ld_pd;
        for (int c0 = lg * VEC; c0 < a.Wp; c0 += G * VEC) {
            float t[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) t[v] = ps[c0 + v];
            store_vec<VEC>(pd + c0, t);
        }
    }
}

// S_i = sum dinv[src] * src[src, 0 .. W) (gather_rows), then gcn_finish
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_gcn_hop(const GcnArgs a)
{
    using RowT = Row<VEC, G, R>;
    RowT acc;
    walk_rows<G>(
        a, blockIdx.x, a.N, acc,
        [&](int, int qs, int e0, int e1, int stride, int first, int lg, RowT &s) {
            gather_rows<VEC, G, R, gather_unroll(R)>(a.src, a.ld_src, a.W, a.idx, qs, e0, e1, stride, first, lg, s,
                                                     RowWeight{a.dinv});
        },
        [&](int tq, int lg, RowT &s) { s.store(a.partial + (size_t)tq * a.W, a.W, lg); },
        [&](int seg, int, int lg, RowT &s) { gcn_finish<VEC, G, R>(a, seg, lg, s); });
}

// split segments: the sum of the tasks' partial rows, then gcn_finish's arithmetic per element and the row's
// pass-through copy
static __global__ __launch_bounds__(256) void k_gcn_hop_fin(const GcnArgs a)
{
    __shared__ float s[4][64];
    const int p = blockIdx.x;
    const int r = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const float di = a.dinv[r];
    for (int c0 = 0; c0 < a.W; c0 += 64) {
        const int c = c0 + cl;
        const float sum = combine_task_sums(s, sum_task_partials(a.partial, a.W, t0, t1, c, q), q, cl);
        if (q == 0 && c < a.W) {
            const float z = sum * di;
            if (c < a.W0) a.dst0[(size_t)r * a.ld0 + c] = gcn_epilogue(a, c, z);
            else a.dst1[(size_t)r * a.ld1 + (c - a.W0)] = z;
        }
        __syncthreads();
    }
    for (int c = threadIdx.x; c < a.Wp; c += 256) a.pass_dst[(size_t)r * a.ld_pd + c] = a.pass_src[(size_t)r * a.ld_ps + c];
}

template <int VEC, int G, int R> int launch_gcn_hop(const GcnArgs &a0, hipStream_t st)
{
    GcnArgs a = a0;
    const int grid = plan_side(a, a.N, 64 / G);
    if (grid > 0) k_gcn_hop<VEC, G, R><<<grid, BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_gcn_hop_fin<<<a.n_split, 256, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

// the vector width of a call: the largest of 4, 2, 1 that divides every width, every stride and every table
// pointer's offset (in floats) from a 16-byte boundary
static int gcn_hop_vec(const sngnn_gcn_hop_t *h)
{
    uint64_t bits = (uint64_t)h->W | (uint64_t)h->W0 | (uint64_t)h->ld_src | (uint64_t)h->ld0;
    bits |= ((uintptr_t)h->src >> 2) | ((uintptr_t)h->dst0 >> 2);
    if (h->dst1) bits |= (uint64_t)h->ld1 | ((uintptr_t)h->dst1 >> 2);
    if (h->Wp > 0) {
        bits |= (uint64_t)h->Wp | (uint64_t)h->ld_ps | (uint64_t)h->ld_pd;
        bits |= ((uintptr_t)h->pass_src >> 2) | ((uintptr_t)h->pass_dst >> 2);
    }
    return bits % 4 == 0 ? 4 : bits % 2 == 0 ? 2 : 1;
}

// per-workgroup partial column sums in double: workgroup b takes the rows b * 4 + q, + 4 gridDim.x, ... (q = the
// thread's row lane of 4), 64 columns a pass; four rows in flight per thread (four chains, added pairwise)
static __global__ __launch_bounds__(256) void k_gcn_colsum_part(const float *__restrict__ g, int64_t N, int C,
                                                                double *__restrict__ part)
{
    __shared__ double s[4][64];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t step = (int64_t)gridDim.x * 4;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + cl;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
        if (c < C) {
            int64_t r = (int64_t)blockIdx.x * 4 + q;
            for (; r + 3 * step < N; r += 4 * step) {
                const float a0 = g[r * C + c], a1 = g[(r + step) * C + c], a2 = g[(r + 2 * step) * C + c],
                            a3 = g[(r + 3 * step) * C + c];
                v0 += (double)a0; v1 += (double)a1; v2 += (double)a2; v3 += (double)a3;
            }
            for (; r < N; r += step) v0 += (double)g[r * C + c];
        }
        s[q][cl] = (v0 + v1) + (v2 + v3);
        __syncthreads();
        if (q == 0 && c < C) part[(size_t)blockIdx.x * C + c] = (s[0][cl] + s[1][cl]) + (s[2][cl] + s[3][cl]);
        __syncthreads();
    }
}

// the sum of the nb partials of each column: 16 row lanes x 64 columns a workgroup, lane q takes the partials q, q + 16,
// ... on four chains, then the lanes' sums are added in order; rounded to fp32 once
static __global__ __launch_bounds__(1024) void k_gcn_colsum_fin(const double *__restrict__ part, int nb, int C,
                                                                float *__restrict__ out)
{
    __shared__ double s[16][64];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    if (c < C) {
        int b = q;
        for (; b + 48 < nb; b += 64) {
            v0 += part[(size_t)b * C + c]; v1 += part[(size_t)(b + 16) * C + c];
            v2 += part[(size_t)(b + 32) * C + c]; v3 += part[(size_t)(b + 48) * C + c];
        }
        for (; b < nb; b += 16) v0 += part[(size_t)b * C + c];
    }
    s[q][cl] = (v0 + v1) + (v2 + v3);
    __syncthreads();
    if (q == 0 && c < C) {
        double v = s[0][cl];
#pragma unroll
        for (int i = 1; i < 16; ++i) v += s[i][cl];
        out[c] = (float)v;
    }
}

}  // namespace sngnn

using namespace sngnn;

extern "C" int64_t sngnn_gcn_workspace_bytes(const sngnn_graph_t *g, int W)
{
    RowCfg cfg;
    if (g == nullptr || !row_cfg(W, cfg)) return 0;
    return std::max<int64_t>(task_partial_bytes(g, W) + 256, (int64_t)COLSUM_BLOCKS * W * 8);
}

extern "C" int sngnn_gcn_hop(const sngnn_graph_t *g, const sngnn_gcn_hop_t *h, const float *dinv, int transpose,
                             void *workspace, void *stream)
{
    SN_REQUIRE(g != nullptr && h != nullptr, SNGNN_EINVAL, "graph or hop description is NULL");
    SN_REQUIRE(whole_graph_with_loops(g), SNGNN_EINVAL,
               "the GCN hop needs an unpartitioned graph built with add_loops = 1, remove_loops = "
               "SNGNN_LOOPS_REPLACE (gcn_norm's edge list)");
    RowCfg cfg;
    SN_REQUIRE(row_cfg(h->W, cfg), SNGNN_ERANGE, "W must be in [1, " + std::to_string(SNGNN_MAX_CHANNELS) + "]");
    SN_REQUIRE(h->W0 >= 1 && h->W0 <= h->W, SNGNN_ERANGE, "W0 must be in [1, W]");
    SN_REQUIRE(h->Wp >= 0 && h->Wp <= SNGNN_MAX_CHANNELS, SNGNN_ERANGE,
               "Wp must be in [0, " + std::to_string(SNGNN_MAX_CHANNELS) + "]");
    SN_REQUIRE((h->dst1 == nullptr) == (h->W0 == h->W), SNGNN_EINVAL, "dst1 is NULL iff W0 == W");
    SN_REQUIRE((h->rm != nullptr) == (h->invstd != nullptr) && (h->rm != nullptr) == (h->gamma != nullptr) &&
                   (h->rm != nullptr) == (h->beta_bn != nullptr),
               SNGNN_EINVAL, "rm, invstd, gamma and beta_bn go together (all NULL: no norm epilogue)");
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(h->src && h->dst0 && dinv && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(h->Wp == 0 || (h->pass_src && h->pass_dst), SNGNN_EINVAL, "Wp > 0 needs pass_src and pass_dst");
    SN_REQUIRE(h->ld_src >= h->W && h->ld0 >= h->W0 && (!h->dst1 || h->ld1 >= h->W - h->W0) &&
                   (h->Wp == 0 || (h->ld_ps >= h->Wp && h->ld_pd >= h->Wp)),
               SNGNN_EINVAL, "a row stride is smaller than the slice's width");
    SN_REQUIRE((((uintptr_t)h->src | (uintptr_t)h->dst0 | (uintptr_t)h->dst1 | (uintptr_t)h->pass_src |
                 (uintptr_t)h->pass_dst) & 3) == 0,
               SNGNN_EINVAL, "tables must be aligned to 4 bytes");
    const int64_t N = g->N;
    const Slice rs{h->src, N, h->ld_src, h->W}, r0{h->dst0, N, h->ld0, h->W0}, r1{h->dst1, N, h->ld1, h->W - h->W0},
        rps{h->pass_src, N, h->ld_ps, h->Wp}, rpd{h->pass_dst, N, h->ld_pd, h->Wp};
    SN_REQUIRE(!overlap(r0, rs) && !overlap(r0, r1) && !overlap(r0, rps) && !overlap(r0, rpd) && !overlap(r1, rs) &&
                   !overlap(r1, rps) && !overlap(r1, rpd) && !overlap(rpd, rs) && !overlap(rpd, rps),
               SNGNN_EINVAL, "a destination overlaps the source or another destination (other rows still gather the "
                             "source); column slices of one table must be disjoint column ranges of the same stride");
    const int vec = gcn_hop_vec(h);
    const int r = cfg.r * (cfg.vec / vec);
    SN_REQUIRE(r <= 8, SNGNN_ERANGE,
               "W = " + std::to_string(h->W) + " at vector width " + std::to_string(vec) +
                   " needs more than 8 steps per lane (align the slices, or run the plain op sequence)");
    GcnArgs q;
    q.N = (int)g->N;
    bind_side(g, transpose != 0, q);
    q.nbA = q.nbB = 0;
    q.src = h->src; q.dst0 = h->dst0; q.dst1 = h->dst1; q.pass_src = h->pass_src; q.pass_dst = h->pass_dst;
    q.ld_src = h->ld_src; q.ld0 = h->ld0; q.ld1 = h->ld1; q.ld_ps = h->ld_ps; q.ld_pd = h->ld_pd;
    q.W = h->W; q.W0 = h->W0; q.Wp = h->Wp; q.relu = h->relu;
    q.bias = h->bias; q.rm = h->rm; q.invstd = h->invstd; q.gamma = h->gamma; q.beta = h->beta_bn;
    q.dinv = dinv;
    q.partial = (float *)workspace;
    return dispatch_slice_layout(vec, cfg.g, r, [&](auto v, auto g_, auto r_) {
        return launch_gcn_hop<decltype(v)::value, decltype(g_)::value, decltype(r_)::value>(q, (hipStream_t)stream);
    });
}

extern "C" int sngnn_gcn_bias_grad(const float *g, int64_t N, int C, float *grad_bias, void *workspace, void *stream)
{
    SN_REQUIRE(N >= 0, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(C >= 1 && C <= SNGNN_MAX_CHANNELS, SNGNN_ERANGE,
               "C must be in [1, " + std::to_string(SNGNN_MAX_CHANNELS) + "]");
    SN_REQUIRE(grad_bias && workspace && (g || N == 0), SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(COLSUM_BLOCKS, (N + 31) / 32));
    k_gcn_colsum_part<<<nb, 256, 0, st>>>(g, N, C, (double *)workspace);
    k_gcn_colsum_fin<<<ceil_div(C, 64), 1024, 0, st>>>((const double *)workspace, nb, C, grad_bias);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

// GCNII's layer, PyG 2.0.4's GCN2Conv with shared weights (models/models.py:1258-1260, 1296), gfx950, fp32:
//     s = (1 - alpha) (A^ x) + alpha x0,     out = (1 - beta) s + beta (s W)
// with A^ = D^-1/2 (A + I) D^-1/2 of gcn_norm (prop.hip's adjacency: deg_i = in-degree with the loop, dinv = deg^-1/2).
// Two launches:
//   hop   (A^ x)_i = dinv_i S_i,  S_i = sum_{e -> i} dinv_src x_src.  The rows of x are gathered UNSCALED and multiplied
//         by dinv[src], which is loaded next to the column id: 4 more bytes per edge (from a 4 N byte table that stays
//         in cache) instead of the read and the write of a scaled copy of x that prop.hip's iterate would cost per
//         layer.  The row-class walk of row_walk.h: small rows by lane group, medium rows by wave, hubs as
//         128-edge tasks + a finalize; fixed summation order, no atomics.  Store epilogue: s_i = a (dinv_i S_i) + b x0_i.
//         Every product and sum is rounded separately (-ffp-contract=off).  On the CSC side the same kernel is A^T.
//   map   out = c0 s + c1 (s W): s streamed once in 32-row tiles through LDS, W resident in LDS for the workgroup's
//         lifetime; a thread owns 4 rows x CT columns; each dot product is four interleaved fma chains (k mod 4) added
//         pairwise.  With the transposed weight it is the backward's g_s = (1 - beta) g + beta (g W^T).  Optional store
//         epilogue for evaluation: the running-statistics norm and the relu behind the layer.
// The map stays a launch of its own: training stores s for the weight gradient anyway, and a C x C product per row
// inside a lane group would run from LDS at about the cost of the read it saves (an estimate).
#include <algorithm>

#include "entry.h"
#include "row_walk.h"

namespace sngnn {

struct Gcn2Args : RowSide {
    const float *x;             // rows to gather  [N, C]
    const float *x0;            // [N, C] or nullptr: the b x0 term
    const float *dinv;          // [N]
    float a, b;
    float *out;                 // [N, C]
    float *partial;             // [n_tasks, C]
    int C, N;
};

// the epilogue of row r from its gathered sum s
template <int VEC, int G, int R>
__device__ __forceinline__ void gcn2_finish(const Gcn2Args &a, int r, int lg, Row<VEC, G, R> &s)
{
    const size_t off = (size_t)r * a.C;
    s.scale(a.dinv[r]);
    s.scale(a.a);
    if (a.x0) {
        Row<VEC, G, R> t;
        t.load(a.x0 + off, a.C, lg);
        t.scale(a.b);
        s.add(t);
    }
    s.store(a.out + off, a.C, lg);
}

// S_i = sum dinv[src] * x[src] (gather_rows), then gcn2_finish
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_gcn2_hop(const Gcn2Args a)
{
    using RowT = Row<VEC, G, R>;
    RowT acc;
    walk_rows<G>(
        a, blockIdx.x, a.N, acc,
        [&](int, int qs, int e0, int e1, int stride, int first, int lg, RowT &s) {
            gather_rows<VEC, G, R, gather_unroll(R)>(a.x, a.C, a.C, a.idx, qs, e0, e1, stride, first, lg, s,
                                                     RowWeight{a.dinv});
        },
        [&](int tq, int lg, RowT &s) { s.store(a.partial + (size_t)tq * a.C, a.C, lg); },
        [&](int seg, int, int lg, RowT &s) { gcn2_finish<VEC, G, R>(a, seg, lg, s); });
}

// split segments: the sum of the tasks' partial rows, then gcn2_finish's arithmetic per element
static __global__ __launch_bounds__(256) void k_gcn2_hop_fin(const Gcn2Args a)
{
    __shared__ float s[4][64];
    const int p = blockIdx.x;
    const int r = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const float di = a.dinv[r];
    for (int c0 = 0; c0 < a.C; c0 += 64) {
        const int c = c0 + cl;
        const float sum = combine_task_sums(s, sum_task_partials(a.partial, a.C, t0, t1, c, q), q, cl);
        if (q == 0 && c < a.C) {
            const size_t at = (size_t)r * a.C + c;
            float z = (sum * di) * a.a;
            if (a.x0) z = z + a.x0[at] * a.b;
            a.out[at] = z;
        }
        __syncthreads();
    }
}

template <int VEC, int G, int R> int launch_gcn2_hop(const Gcn2Args &a0, hipStream_t st)
{
    Gcn2Args a = a0;
    const int grid = plan_side(a, a.N, 64 / G);
    if (grid > 0) k_gcn2_hop<VEC, G, R><<<grid, BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_gcn2_hop_fin<<<a.n_split, 256, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

static int dispatch_gcn2_hop(const RowCfg &cfg, const Gcn2Args &a, hipStream_t st)
{
    return dispatch_vec(cfg, [&](auto vec) { SNGNN_DISPATCH_GR(launch_gcn2_hop, decltype(vec)::value, cfg, a, st) });
}

// ---- the identity map -------------------------------------------------------------------------------------------------
constexpr int MAP_ROWS = 32;          // rows of a tile: 8 row groups of 4 rows x 32 column lanes

struct Gcn2Norm { const float *rm, *invstd, *gamma, *beta; };

// CT: 32-column tiles of the output, C <= 32 CT.  LDS: W as [k][j] (rows k >= C and columns j >= C are zero) and one
// tile of s as [row][k] (row stride + 4 floats: 16-byte rows; columns k >= C are zero).  A workgroup loads W once and
// walks the tiles blockIdx.x, + gridDim.x, ...
template <int CT, bool NORM>
__global__ __launch_bounds__(256) void k_gcn2_map(const float *__restrict__ s, const float *__restrict__ w, float c0,
                                                  float c1, int64_t N, int C, int transpose_w, const Gcn2Norm nm,
                                                  float *__restrict__ out, int64_t ntiles)
{
    constexpr int CP = 32 * CT, LD = CP + 4;
    __shared__ __align__(16) float sw[CP * CP];
    __shared__ __align__(16) float ss[MAP_ROWS * LD];
    const int tid = threadIdx.x, cl = tid & 31, rg = tid >> 5;
    for (int e = tid; e < CP * CP; e += 256) {
        const int k = e / CP, j = e % CP;
        float v = 0.f;
        if (k < C && j < C) v = transpose_w ? w[(size_t)j * C + k] : w[(size_t)k * C + j];
        sw[e] = v;
    }
    for (int e = tid; e < MAP_ROWS * LD; e += 256) ss[e] = 0.f;
    float rm[CT], is[CT], ga[CT], be[CT];
#pragma unroll
    for (int q = 0; q < CT; ++q) {
        const int j = min(cl + 32 * q, C - 1);
        rm[q] = NORM ? nm.rm[j] : 0.f;
        is[q] = NORM ? nm.invstd[j] : 1.f;
        ga[q] = NORM ? nm.gamma[j] : 1.f;
        be[q] = NORM ? nm.beta[j] : 0.f;
    }
    const int kend = (C + 3) & ~3;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * MAP_ROWS;
        const int nrows = N - row0 < MAP_ROWS ? (int)(N - row0) : MAP_ROWS;
        const float *src = s + row0 * C;
        __syncthreads();                                   // the previous tile's reads (and the fills above) are done
        for (int e = tid; e < nrows * C; e += 256) ss[(e / C) * LD + e % C] = src[e];
        __syncthreads();
        float acc[4][CT][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < CT; ++q)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[i][q][kk] = 0.f;
        for (int k0 = 0; k0 < kend; k0 += 4) {
            float4 sv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[i] = *reinterpret_cast<const float4 *>(ss + (rg * 4 + i) * LD + k0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int q = 0; q < CT; ++q) {
                    const float wv = sw[(k0 + kk) * CP + cl + 32 * q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float xv = kk == 0 ? sv[i].x : kk == 1 ? sv[i].y : kk == 2 ? sv[i].z : sv[i].w;
                        acc[i][q][kk] = fmaf(xv, wv, acc[i][q][kk]);
                    }
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rg * 4 + i;
#pragma unroll
            for (int q = 0; q < CT; ++q) {
                const int j = cl + 32 * q;
                if (r < nrows && j < C) {
                    const float dot = (acc[i][q][0] + acc[i][q][1]) + (acc[i][q][2] + acc[i][q][3]);
                    float v = c0 * ss[r * LD + j] + c1 * dot;
                    if constexpr (NORM) {
                        v = ((v - rm[q]) * is[q]) * ga[q] + be[q];
                        v = v > 0.f ? v : 0.f;
                    }
                    out[(row0 + r) * C + j] = v;
                }
            }
        }
    }
}

template <int CT>
static int launch_gcn2_map(const float *s, const float *w, float c0, float c1, int64_t N, int C, int transpose_w,
                           const Gcn2Norm &nm, float *out, hipStream_t st)
{
    constexpr int64_t lds = (int64_t)(32 * CT * 32 * CT + MAP_ROWS * (32 * CT + 4)) * 4;
    const int64_t ntiles = (N + MAP_ROWS - 1) / MAP_ROWS;
    // workgroups that fit a CU's 160 KiB of LDS side by side (8 at most), on 256 CUs
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / lds));
    const int grid = (int)std::min<int64_t>(ntiles, 256 * per_cu);
    if (nm.rm) k_gcn2_map<CT, true><<<grid, 256, 0, st>>>(s, w, c0, c1, N, C, transpose_w, nm, out, ntiles);
    else k_gcn2_map<CT, false><<<grid, 256, 0, st>>>(s, w, c0, c1, N, C, transpose_w, nm, out, ntiles);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

}  // namespace sngnn

using namespace sngnn;

extern "C" int64_t sngnn_gcn2_workspace_bytes(const sngnn_graph_t *g, int C)
{
    RowCfg cfg;
    if (g == nullptr || !row_cfg(C, cfg)) return 0;
    return task_partial_bytes(g, C) + 256;
}

extern "C" int sngnn_gcn2_hop(const sngnn_graph_t *g, const float *x, const float *x0, const float *dinv, float a, float b,
                              int C, int transpose, float *out, void *workspace, void *stream)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    SN_REQUIRE(whole_graph_with_loops(g), SNGNN_EINVAL,
               "the GCN2 hop needs an unpartitioned graph built with add_loops = 1, remove_loops = "
               "SNGNN_LOOPS_REPLACE (gcn_norm's edge list)");
    RowCfg cfg;
    if (int rc = check_rows(C, 0, {x, x0, out}, cfg)) return rc;
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(x && dinv && out && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(x != out && x0 != out, SNGNN_EINVAL, "out must not alias x or x0 (other rows still gather them)");
    Gcn2Args q;
    q.N = (int)g->N;
    bind_side(g, transpose != 0, q);
    q.nbA = q.nbB = 0;
    q.x = x; q.x0 = x0; q.dinv = dinv; q.a = a; q.b = b; q.out = out; q.C = C;
    q.partial = (float *)workspace;
    return dispatch_gcn2_hop(cfg, q, (hipStream_t)stream);
}

extern "C" int sngnn_gcn2_map(const float *s, const float *w, float c0, float c1, int64_t N, int C, int transpose_w,
                              const float *rm, const float *invstd, const float *gamma, const float *beta_bn, float *out,
                              void *stream)
{
    SN_REQUIRE(N >= 0, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(C >= 1 && C <= SNGNN_GCN2_MAX_C, SNGNN_ERANGE,
               "C must be in [1, " + std::to_string(SNGNN_GCN2_MAX_C) + "] (a wider layer runs the plain op sequence)");
    SN_REQUIRE((rm != nullptr) == (invstd != nullptr) && (rm != nullptr) == (gamma != nullptr) &&
                   (rm != nullptr) == (beta_bn != nullptr),
               SNGNN_EINVAL, "rm, invstd, gamma and beta_bn go together (all NULL: no norm epilogue)");
    if (N == 0) return SNGNN_OK;
    SN_REQUIRE(s && w && out, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(s != out, SNGNN_EINVAL, "out must not alias s");
    const Gcn2Norm nm{rm, invstd, gamma, beta_bn};
    hipStream_t st = (hipStream_t)stream;
    switch ((C + 31) / 32) {
    case 1: return launch_gcn2_map<1>(s, w, c0, c1, N, C, transpose_w, nm, out, st);
    case 2: return launch_gcn2_map<2>(s, w, c0, c1, N, C, transpose_w, nm, out, st);
    case 3: return launch_gcn2_map<3>(s, w, c0, c1, N, C, transpose_w, nm, out, st);
    default: return launch_gcn2_map<4>(s, w, c0, c1, N, C, transpose_w, nm, out, st);
    }
}

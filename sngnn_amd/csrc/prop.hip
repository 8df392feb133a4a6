// Polynomial propagation with the GCN-normalised adjacency (gfx950, fp32): GPR_prop and APPNP,
// models/models.py:1191-1208 and PyG's APPNP as models.py:1033 uses it.
//     A^ = D^-1/2 (A + I) D^-1/2,  deg_i = in-degree with the loop,  dinv = deg^-1/2
//     (A^ x)_i = sum_{e -> i} dinv_src dinv_i x_src = dinv_i * sum_{e -> i} u_src     with u = dinv . x
// The kernels carry the SCALED iterate u, so a hop is an unweighted row gather-sum (the row-class walk of
// row_walk.h: small rows by lane group, medium rows by wave, hubs as 128-edge tasks + a finalize; fixed
// summation order, no atomics) with a store epilogue that does the rest of the recurrence:
//     z_i = a x0_i + b (dinv_i S_i),   [acc_i += c z_i,]   [dot += <z_i, xd_i>,]   store dinv_i z_i | z_i (last hop)
// a, b, c are read from device memory (they are functions of a parameter).  Every product and sum is rounded
// separately (-ffp-contract=off).  Hops are separate launches on the caller's stream.
//   GPR forward    Horner:  h_K = gamma_K x,  h_k = gamma_k x + A^ h_{k+1}                  (CSR side)
//   GPR backward   power form on the transpose: t_0 = g, t_{k+1} = A^T t_k, grad_x = sum gamma_k t_k (acc),
//                  grad_gamma_k = <t_k, x>: per-workgroup partial dots in double from the hops' own launches,
//                  one reducer launch adds them in a fixed order                             (CSC side)
//   APPNP          x_{k+1} = alpha h + (1 - alpha) A^ x_k; its backward is the same recurrence on A^T
#include "entry.h"
#include "row_walk.h"

namespace sngnn {

constexpr int PROP_INIT_BLOCKS = 1024;

struct PropArgs : RowSide {
    const float *u;             // scaled iterate to gather  [N, C]
    const float *x0;            // [N, C] or nullptr: the a x0 term
    const float *dinv;          // [N]
    const float *a, *b, *c;     // device scalars (a with x0, c with acc; b nullptr = 1)
    float *acc;                 // [N, C] or nullptr
    const float *xd;            // [N, C] or nullptr: rows the dot is taken with
    double *dotpart;            // this hop's per-workgroup partial dots
    float *out;                 // [N, C] or nullptr (the last backward hop has no next iterate)
    int scaled;                 // store dinv_i z_i (the next iterate) instead of z_i
    float *partial;             // [n_tasks, C]
    int C, N;
};

// the epilogue of row r from its gathered sum s; returns this lane's share of <z_r, xd_r>
template <int VEC, int G, int R>
__device__ __forceinline__ double prop_finish(const PropArgs &a, int r, int lg, Row<VEC, G, R> &s)
{
    using RowT = Row<VEC, G, R>;
    const float di = a.dinv[r];
    const size_t off = (size_t)r * a.C;
    s.scale(di);
    if (a.b) s.scale(*a.b);
    if (a.x0) {
        RowT x;
        x.load(a.x0 + off, a.C, lg);
        x.scale(*a.a);
        x.add(s);
        s = x;
    }
    if (a.acc) {
        RowT t;
        t.load(a.acc + off, a.C, lg);
        t.axpy(*a.c, s);
        t.store(a.acc + off, a.C, lg);
    }
    double d = 0.0;
    if (a.xd) {
        RowT t;
        t.load(a.xd + off, a.C, lg);
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) d += (double)s.x[q][v] * (double)t.x[q][v];
    }
    if (a.out) {
        if (a.scaled) s.scale(di);
        s.store(a.out + off, a.C, lg);
    }
    return d;
}

// S_i = sum u[src] (gather_rows), then prop_finish; the finishing lanes' shares of the dot are added per workgroup
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_prop(const PropArgs a)
{
    using RowT = Row<VEC, G, R>;
    __shared__ double sd[WAVES];
    const int b = blockIdx.x;
    RowT acc;
    double d = 0.0;
    walk_rows<G>(
        a, b, a.N, acc,
        [&](int, int qs, int e0, int e1, int stride, int first, int lg, RowT &s) {
            gather_rows<VEC, G, R, gather_unroll(R)>(a.u, a.C, a.C, a.idx, qs, e0, e1, stride, first, lg, s, NoWeight{});
        },
        [&](int tq, int lg, RowT &s) { s.store(a.partial + (size_t)tq * a.C, a.C, lg); },
        [&](int seg, int, int lg, RowT &s) { d = prop_finish<VEC, G, R>(a, seg, lg, s); });
    if (a.xd && b >= a.nbA) {                          // (block-uniform) the workgroup's partial dot, fixed order
        d = wave_sum_d(d);
        if (lane_id() == 0) sd[threadIdx.x >> 6] = d;
        __syncthreads();
        if (threadIdx.x == 0) a.dotpart[b - a.nbA] = (sd[0] + sd[1]) + (sd[2] + sd[3]);
    }
}

// split segments: the sum of the tasks' partial rows, then the epilogue per element (the arithmetic of prop_finish);
// the row's dot is partial number part0 + p
static __global__ __launch_bounds__(256) void k_prop_fin(const PropArgs a, int part0)
{
    __shared__ float s[4][64];
    const int p = blockIdx.x;
    const int r = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const float di = a.dinv[r];
    double d = 0.0;
    for (int c0 = 0; c0 < a.C; c0 += 64) {
        const int c = c0 + cl;
        const float sum = combine_task_sums(s, sum_task_partials(a.partial, a.C, t0, t1, c, q), q, cl);
        if (q == 0 && c < a.C) {
            const size_t at = (size_t)r * a.C + c;
            float z = sum * di;
            if (a.b) z = z * *a.b;
            if (a.x0) z = a.x0[at] * *a.a + z;
            if (a.acc) a.acc[at] = a.acc[at] + *a.c * z;
            if (a.xd) d += (double)z * (double)a.xd[at];
            if (a.out) a.out[at] = a.scaled ? z * di : z;
        }
        __syncthreads();
    }
    if (a.xd && q == 0) {                              // (wave 0 holds the row's elements)
        d = wave_sum_d(d);
        if (cl == 0) a.dotpart[part0 + p] = d;
    }
}

// the first scaled iterate u = dinv . (s x) (s nullptr: 1); with acc, acc = c x; with xd, the partial dots of <x, xd>
static __global__ __launch_bounds__(256) void k_prop_init(const float *__restrict__ x, const float *__restrict__ dinv,
                                                          const float *__restrict__ s, const float *__restrict__ c,
                                                          float *__restrict__ u, float *__restrict__ acc,
                                                          const float *__restrict__ xd, double *__restrict__ dotpart,
                                                          int64_t n, int C)
{
    __shared__ double sd[4];
    const float sv = s ? *s : 1.f, cv = c ? *c : 0.f;
    double d = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = x[i];
        const float di = dinv[i / C];
        u[i] = di * (s ? sv * v : v);
        if (acc) acc[i] = cv * v;
        if (xd) d += (double)v * (double)xd[i];
    }
    if (xd) {
        d = wave_sum_d(d);
        if ((threadIdx.x & 63) == 0) sd[threadIdx.x >> 6] = d;
        __syncthreads();
        if (threadIdx.x == 0) dotpart[blockIdx.x] = (sd[0] + sd[1]) + (sd[2] + sd[3]);
    }
}

// out[k] = the sum of row k of the partial dots (row 0: n0 of them, the init launch's; the others n), fixed order
static __global__ __launch_bounds__(256) void k_prop_dots(const double *__restrict__ dotpart, int64_t stride, int n0,
                                                          int n, double *__restrict__ out)
{
    __shared__ double s[256];
    const int k = blockIdx.x, cnt = k == 0 ? n0 : n;
    const double *p = dotpart + (size_t)k * stride;
    double v = 0.0;
    for (int i = threadIdx.x; i < cnt; i += 256) v += p[i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = s[0];
}

static __global__ void k_prop_dinv(const int32_t *__restrict__ rowptr, int64_t N, float *__restrict__ dinv)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) dinv[i] = 1.0f / ieee_sqrt((float)max(rowptr[i + 1] - rowptr[i], 1));
}

template <int VEC, int G, int R> int launch_prop(const PropArgs &a0, hipStream_t st)
{
    PropArgs a = a0;
    const int grid = plan_side(a, a.N, 64 / G);
    if (grid > 0) k_prop<VEC, G, R><<<grid, BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_prop_fin<<<a.n_split, 256, 0, st>>>(a, grid - a.nbA);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

static int dispatch_prop(const RowCfg &cfg, const PropArgs &a, hipStream_t st)
{
    return dispatch_vec(cfg, [&](auto vec) { SNGNN_DISPATCH_GR(launch_prop, decltype(vec)::value, cfg, a, st) });
}

// the structure a hop walks: the in-edges (CSR by target) or, for A^T, the out-edges (CSC by source)
static void prop_side(const sngnn_graph_t *g, bool transpose, PropArgs &a)
{
    a.N = (int)g->N;
    bind_side(g, transpose, a);
    a.nbA = a.nbB = 0;
}

// partial dots one hop of this side writes (the workgroups that finish rows + one per split row)
static int prop_parts(const sngnn_graph_t *g, bool transpose, const RowCfg &cfg)
{
    PropArgs a;
    prop_side(g, transpose, a);
    return plan_side(a, a.N, 64 / cfg.g) - a.nbA + a.n_split;
}

struct PropLayout { int64_t u1, partial, dots, total, stride; };

static PropLayout prop_layout(const sngnn_graph_t *g, int C, int K, const RowCfg &cfg)
{
    PropLayout L;
    const int64_t rows = up256(g->N * (int64_t)C * 4);
    L.u1 = rows;
    L.partial = 2 * rows;
    L.dots = L.partial + task_partial_bytes(g, C);
    L.stride = std::max<int64_t>(PROP_INIT_BLOCKS, std::max(prop_parts(g, false, cfg), prop_parts(g, true, cfg)));
    L.total = L.dots + up256((int64_t)(K + 1) * L.stride * 8);
    return L;
}

static int prop_init_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(PROP_INIT_BLOCKS, (n + 255) / 256)); }

}  // namespace sngnn

using namespace sngnn;

#define PROP_COMMON(g, C, K)                                                                                           \
    SN_REQUIRE((g) != nullptr, SNGNN_EINVAL, "graph is NULL");                                                         \
    SN_REQUIRE(whole_graph_with_loops(g), SNGNN_EINVAL,                                                                \
               "the propagation needs an unpartitioned graph built with add_loops = 1, remove_loops = "              \
               "SNGNN_LOOPS_REPLACE (gcn_norm's edge list)");                                                          \
    SN_REQUIRE((K) >= 1, SNGNN_EINVAL, "K must be at least 1");                                                        \
    RowCfg cfg;                                                                                                        \
    SN_REQUIRE(row_cfg((C), cfg), SNGNN_EINVAL, "C must be in [1, " + std::to_string(SNGNN_MAX_CHANNELS) + "]")

extern "C" int sngnn_prop_dinv(const sngnn_graph_t *g, float *dinv, void *stream)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    SN_REQUIRE(whole_graph_with_loops(g), SNGNN_EINVAL,
               "the propagation needs an unpartitioned graph built with add_loops = 1, remove_loops = "
               "SNGNN_LOOPS_REPLACE (gcn_norm's edge list)");
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(dinv, SNGNN_EINVAL, "NULL argument");
    k_prop_dinv<<<ceil_div(g->N, 256), 256, 0, (hipStream_t)stream>>>(g->rowptr, g->N, dinv);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int64_t sngnn_prop_workspace_bytes(const sngnn_graph_t *g, int C, int K)
{
    RowCfg cfg;
    if (g == nullptr || K < 0 || !row_cfg(C, cfg)) return 0;
    return prop_layout(g, C, K, cfg).total;
}

extern "C" int sngnn_prop_gpr_forward(const sngnn_graph_t *g, const float *x, const float *gamma, int K, int C,
                                      const float *dinv, float *out, void *workspace, void *stream)
{
    PROP_COMMON(g, C, K);
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(x && gamma && dinv && out && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {x, out}), SNGNN_EINVAL, "rows must be aligned to the row vector width");
    hipStream_t st = (hipStream_t)stream;
    const PropLayout L = prop_layout(g, C, K, cfg);
    float *u[2] = {(float *)workspace, (float *)((char *)workspace + L.u1)};
    const int64_t n = g->N * (int64_t)C;
    k_prop_init<<<prop_init_grid(n), 256, 0, st>>>(x, dinv, gamma + K, nullptr, u[0], nullptr, nullptr, nullptr, n, C);
    SN_HIP(hipGetLastError());
    PropArgs a;
    prop_side(g, false, a);
    a.C = C; a.dinv = dinv; a.partial = (float *)((char *)workspace + L.partial);
    a.x0 = x; a.b = nullptr; a.c = nullptr; a.acc = nullptr; a.xd = nullptr; a.dotpart = nullptr;
    int cur = 0;
    for (int j = K - 1; j >= 0; --j) {
        a.u = u[cur]; a.a = gamma + j;
        a.out = j == 0 ? out : u[cur ^ 1]; a.scaled = j > 0;
        const int rc = dispatch_prop(cfg, a, st);
        if (rc != SNGNN_OK) return rc;
        cur ^= 1;
    }
    return SNGNN_OK;
}

extern "C" int sngnn_prop_gpr_backward(const sngnn_graph_t *g, const float *grad_out, const float *x,
                                       const float *gamma, int K, int C, const float *dinv, float *grad_x,
                                       double *grad_gamma, void *workspace, void *stream)
{
    PROP_COMMON(g, C, K);
    hipStream_t st = (hipStream_t)stream;
    if (g->N == 0) {
        if (grad_gamma) k_prop_dots<<<K + 1, 256, 0, st>>>(nullptr, 0, 0, 0, grad_gamma);
        SN_HIP(hipGetLastError());
        return SNGNN_OK;
    }
    SN_REQUIRE(grad_out && gamma && dinv && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(!grad_gamma || x, SNGNN_EINVAL, "grad_gamma needs x");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {grad_out, x, grad_x}), SNGNN_EINVAL,
               "rows must be aligned to the row vector width");
    const PropLayout L = prop_layout(g, C, K, cfg);
    float *u[2] = {(float *)workspace, (float *)((char *)workspace + L.u1)};
    double *dots = (double *)((char *)workspace + L.dots);
    const float *xd = grad_gamma ? x : nullptr;
    const int64_t n = g->N * (int64_t)C;
    const int grid0 = prop_init_grid(n);
    k_prop_init<<<grid0, 256, 0, st>>>(grad_out, dinv, nullptr, gamma, u[0], grad_x, xd, dots, n, C);
    SN_HIP(hipGetLastError());
    PropArgs a;
    prop_side(g, true, a);
    a.C = C; a.dinv = dinv; a.partial = (float *)((char *)workspace + L.partial);
    a.x0 = nullptr; a.a = nullptr; a.b = nullptr; a.acc = grad_x; a.xd = xd; a.scaled = 1;
    int cur = 0;
    for (int k = 1; k <= K; ++k) {
        a.u = u[cur]; a.c = gamma + k; a.dotpart = dots + (size_t)k * L.stride;
        a.out = k < K ? u[cur ^ 1] : nullptr;
        const int rc = dispatch_prop(cfg, a, st);
        if (rc != SNGNN_OK) return rc;
        cur ^= 1;
    }
    if (grad_gamma) {
        k_prop_dots<<<K + 1, 256, 0, st>>>(dots, L.stride, grid0, prop_parts(g, true, cfg), grad_gamma);
        SN_HIP(hipGetLastError());
    }
    return SNGNN_OK;
}

extern "C" int sngnn_prop_appnp(const sngnn_graph_t *g, const float *h, const float *coef, int K, int C,
                                const float *dinv, int transpose, float *out, void *workspace, void *stream)
{
    PROP_COMMON(g, C, K);
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(h && coef && dinv && out && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {h, out}), SNGNN_EINVAL, "rows must be aligned to the row vector width");
    hipStream_t st = (hipStream_t)stream;
    const PropLayout L = prop_layout(g, C, K, cfg);
    float *u[2] = {(float *)workspace, (float *)((char *)workspace + L.u1)};
    const int64_t n = g->N * (int64_t)C;
    k_prop_init<<<prop_init_grid(n), 256, 0, st>>>(h, dinv, nullptr, nullptr, u[0], nullptr, nullptr, nullptr, n, C);
    SN_HIP(hipGetLastError());
    PropArgs a;
    prop_side(g, transpose != 0, a);
    a.C = C; a.dinv = dinv; a.partial = (float *)((char *)workspace + L.partial);
    a.x0 = h; a.a = coef; a.b = coef + 1; a.c = nullptr; a.acc = nullptr; a.xd = nullptr; a.dotpart = nullptr;
    int cur = 0;
    for (int k = 1; k <= K; ++k) {
        a.u = u[cur];
        a.out = k == K ? out : u[cur ^ 1]; a.scaled = k < K;
        const int rc = dispatch_prop(cfg, a, st);
        if (rc != SNGNN_OK) return rc;
        cur ^= 1;
    }
    return SNGNN_OK;
}

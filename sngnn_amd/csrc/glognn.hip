// MLPNORM's norm layer (GloGNN, models/models.py:1389-1437) on the sparse graph, gfx950, fp32 rows of 1 <= C <= 64
// channels (C = nclass).  With coe = 1/(alpha+beta), coe1 = 1-gamma, coe2 = 1/coe1, s = coe/coe1, D = diag(diag_weight)
// (I for norm_func1), G = x^T x, V = (coe2^2 I + coe G)^-1 (SPD, commutes with G):
//     M = s V D,   T = s D G V D,   S = P(A) x = sum_k w_k A^k x,
//     out = coe1 (x - gamma h0) T + beta S M + gamma h0
// (the reference's `I - coe V G` is coe2^2 V exactly, and a right factor commutes with the adjacency: the hops run on x
// itself).  A is to_dense_adj's matrix: (A v)_i = sum over the edges with edge_index[0] == i of v[edge_index[1]] - the
// CSC side of a graph built with add_loops = 0, remove_loops = 0 (sngnn_adj_linear_forward's orientation); A^T is its
// CSR side.  The pieces, each an entry of its own:
//   gram    a^T b for [N, C] rows into C x C float64: 32-row tiles through LDS, a thread owns up to 16 elements, per-
//           workgroup partials in double added by a reducer in workgroup order.  One read of b serves two products
//           (the backward's gT and gM).
//   solve   one workgroup, double: in-place Gauss-Jordan without pivoting (the matrix is SPD with smallest eigenvalue
//           >= coe2^2), then M, T and W = G V.  Its backward takes gM, gT to gG + gG^T and grad_diag.
//   hops    unweighted row gather-sums on the row-class walk of row_walk.h (lane group, wave, 128-entry
//           tasks + a finalize; fixed order, no atomics).  Forward: t_k = A t_{k-1}, S += w_k t_k in the stores, the mix
//           above in the last hop's store (M, T in LDS, the C x C products per row accumulated in double).  Backward:
//           a row-local pass forms q = beta g M^T, grad_h0 and coe1 g T^T; r_k = A^T r_{k-1}, grad_x += w_k r_k in the
//           stores, grad_w_k = <r_k, x> from per-workgroup partial dots in double, x (gG + gG^T) in the last store.
// Every fp32 product and sum is rounded separately (-ffp-contract=off).  Nothing synchronises with the host.
#include <algorithm>

#include "entry.h"
#include "row_walk.h"

namespace sngnn {

constexpr int GLO_MAX_C = SNGNN_GLOGNN_MAX_C;
constexpr int GLO_CC = GLO_MAX_C * GLO_MAX_C;
constexpr int GRAM_TILE = 32;
constexpr int GRAM_BLOCKS = 256;
constexpr int GRAM_EPT = GLO_CC / 256;             // elements of the product a thread owns at most
constexpr int GLO_PRE_BLOCKS = 2048;

// ---- gram ---------------------------------------------------------------------------------------------------------------
struct GramArgs {
    const float *a, *a_sub, *a2, *b;     // out = (a - sub a_sub)^T b, out2 = a2^T b (a_sub, a2 may be nullptr)
    double sub;
    int64_t N;
    int C;
    double *part;                        // [blocks][2][C * C]
};

static __global__ __launch_bounds__(256) void k_glo_gram(const GramArgs g)
{
    __shared__ double sa[GRAM_TILE * GLO_MAX_C];
    __shared__ float sa2[GRAM_TILE * GLO_MAX_C], sb[GRAM_TILE * GLO_MAX_C];
    const int C = g.C, CC = C * C, tid = threadIdx.x;
    double acc[GRAM_EPT], acc2[GRAM_EPT];
    int ei[GRAM_EPT], ej[GRAM_EPT];
#pragma unroll
    for (int k = 0; k < GRAM_EPT; ++k) {
        const int e = tid + 256 * k;
        acc[k] = acc2[k] = 0.0;
        ei[k] = e < CC ? e / C : 0;
        ej[k] = e < CC ? e % C : 0;
    }
    const int64_t tiles = (g.N + GRAM_TILE - 1) / GRAM_TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * GRAM_TILE;
        const int rows = (int)min((int64_t)GRAM_TILE, g.N - row0);
        __syncthreads();                           // (the previous tile has been read)
        for (int q = tid; q < rows * C; q += 256) {
            const size_t at = (size_t)row0 * C + q;
            double av = (double)g.a[at];
            if (g.a_sub) av = av - g.sub * (double)g.a_sub[at];
            sa[q] = av;
            if (g.a2) sa2[q] = g.a2[at];
            sb[q] = g.b[at];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < GRAM_EPT; ++k) {
            if (256 * k < CC) {                    // (block-uniform)
                double s = acc[k], s2 = acc2[k];
                for (int r = 0; r < rows; ++r) {
                    const double bv = (double)sb[r * C + ej[k]];
                    s += sa[r * C + ei[k]] * bv;
                    if (g.a2) s2 += (double)sa2[r * C + ei[k]] * bv;
                }
                acc[k] = s; acc2[k] = s2;
            }
        }
    }
    double *p = g.part + (size_t)blockIdx.x * 2 * CC;
#pragma unroll
    for (int k = 0; k < GRAM_EPT; ++k) {
        const int e = tid + 256 * k;
        if (e < CC) { p[e] = acc[k]; p[CC + e] = acc2[k]; }
    }
}

// out[e] = sum over the workgroups' partials, in workgroup order
static __global__ __launch_bounds__(256) void k_glo_gram_reduce(const double *__restrict__ part, int blocks, int CC,
                                                                double *__restrict__ out, double *__restrict__ out2)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * CC) return;
    double *dst = e < CC ? out : out2;
    if (!dst) return;
    double v = 0.0;
    for (int b = 0; b < blocks; ++b) v += part[(size_t)b * 2 * CC + e];
    dst[e < CC ? e : e - CC] = v;
}

static int gram_blocks(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>(GRAM_BLOCKS, (N + GRAM_TILE - 1) / GRAM_TILE)); }

// ---- solve --------------------------------------------------------------------------------------------------------------
struct SolveArgs {
    const double *G;
    const float *diag;                   // [C] or nullptr (D = I)
    double coe, coe1, coe2;
    int C;
    double *M, *T, *V, *W;               // [C, C] each
    float *MT32;                         // [2, C, C]: M then T, rounded to fp32
};

// A (LDS, row stride C) <- A^-1 in place: Gauss-Jordan without pivoting.  All 256 threads call it.
__device__ __forceinline__ void glo_invert(double *A, double *rowk, double *colk, int C)
{
    const int CC = C * C;
    for (int k = 0; k < C; ++k) {
        __syncthreads();
        if ((int)threadIdx.x < C) {
            rowk[threadIdx.x] = A[k * C + threadIdx.x];
            colk[threadIdx.x] = A[threadIdx.x * C + k];
        }
        __syncthreads();
        const double p = 1.0 / rowk[k];
        for (int e = threadIdx.x; e < CC; e += 256) {
            const int i = e / C, j = e % C;
            double v;
            if (i == k) v = j == k ? p : rowk[j] * p;
            else if (j == k) v = -(colk[i] * p);
            else v = A[e] - colk[i] * (rowk[j] * p);
            A[e] = v;
        }
    }
    __syncthreads();
}

static __global__ __launch_bounds__(256) void k_glo_solve(const SolveArgs a)
{
    __shared__ double A[GLO_CC];
    __shared__ double rowk[GLO_MAX_C], colk[GLO_MAX_C];
    const int C = a.C, CC = C * C;
    for (int e = threadIdx.x; e < CC; e += 256) {
        const int i = e / C, j = e % C;
        A[e] = a.coe * a.G[e] + (i == j ? a.coe2 * a.coe2 : 0.0);
    }
    glo_invert(A, rowk, colk, C);
    const double s = a.coe / a.coe1;
    for (int e = threadIdx.x; e < CC; e += 256) {
        const int i = e / C, j = e % C;
        const double di = a.diag ? (double)a.diag[i] : 1.0, dj = a.diag ? (double)a.diag[j] : 1.0;
        double w = 0.0;
        for (int k = 0; k < C; ++k) w += a.G[i * C + k] * A[k * C + j];
        const double m = s * A[e] * dj, t = s * di * w * dj;
        a.V[e] = A[e]; a.W[e] = w; a.M[e] = m; a.T[e] = t;
        a.MT32[e] = (float)m; a.MT32[CC + e] = (float)t;
    }
}

struct SolveBwdArgs {
    const double *gM, *gT;               // [C, C]; they enter as scale_m gM, scale_t gT
    double scale_m, scale_t;
    const double *G, *V, *W;
    const float *diag;
    double coe, coe1;
    int C;
    double *gG2;                         // [C, C]: gG + gG^T
    double *grad_diag;                   // [C] or nullptr
    double *tmp;                         // [2, C, C]
};

// dst[e] = sum_k L[i][k] R[k][j] for the elements of this thread (both operands in LDS)
__device__ __forceinline__ double glo_mm(const double *L, const double *R, int i, int j, int C)
{
    double v = 0.0;
    for (int k = 0; k < C; ++k) v += L[i * C + k] * R[k * C + j];
    return v;
}

static __global__ __launch_bounds__(256) void k_glo_solve_bwd(const SolveBwdArgs a)
{
    __shared__ double L0[GLO_CC], L1[GLO_CC];
    const int C = a.C, CC = C * C, tid = threadIdx.x;
    const double s = a.coe / a.coe1;
    double *t0 = a.tmp, *t1 = a.tmp + CC;
    double pv[GRAM_EPT];
    // L0 = G, L1 = P = D (scale_t gT) D
    for (int e = tid; e < CC; e += 256) {
        const int i = e / C, j = e % C;
        const double di = a.diag ? (double)a.diag[i] : 1.0, dj = a.diag ? (double)a.diag[j] : 1.0;
        L0[e] = a.G[e];
        L1[e] = di * (a.scale_t * a.gT[e]) * dj;
    }
    __syncthreads();
    // gV = s gM D + s G P
    for (int e = tid; e < CC; e += 256) {
        const int i = e / C, j = e % C;
        const double dj = a.diag ? (double)a.diag[j] : 1.0;
        t0[e] = s * (a.scale_m * a.gM[e]) * dj + s * glo_mm(L0, L1, i, j, C);
    }
    __syncthreads();
    for (int e = tid; e < CC; e += 256) L0[e] = a.V[e];
    __syncthreads();
    // P V, kept in registers
#pragma unroll
    for (int k = 0; k < GRAM_EPT; ++k) {
        const int e = tid + 256 * k;
        pv[k] = e < CC ? glo_mm(L1, L0, e / C, e % C, C) : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < CC; e += 256) L1[e] = t0[e];
    __syncthreads();
    // V gV
    for (int e = tid; e < CC; e += 256) t1[e] = glo_mm(L0, L1, e / C, e % C, C);
    __syncthreads();
    for (int e = tid; e < CC; e += 256) L1[e] = t1[e];
    __syncthreads();
    // gG = s P V - coe (V gV) V
#pragma unroll
    for (int k = 0; k < GRAM_EPT; ++k) {
        const int e = tid + 256 * k;
        if (e < CC) t0[e] = s * pv[k] - a.coe * glo_mm(L1, L0, e / C, e % C, C);
    }
    __syncthreads();
    for (int e = tid; e < CC; e += 256) {
        const int i = e / C, j = e % C;
        a.gG2[e] = t0[e] + t0[j * C + i];
    }
    // grad_diag_k = s sum_i V[i][k] gM[i][k] + s sum_j W[k][j] d_j gT[k][j] + s sum_i d_i W[i][k] gT[i][k]
    if (a.grad_diag && tid < C) {
        const int k = tid;
        double v = 0.0;
        for (int i = 0; i < C; ++i) {
            const double di = a.diag ? (double)a.diag[i] : 1.0;
            v += L0[i * C + k] * (a.scale_m * a.gM[i * C + k]);
            v += a.W[k * C + i] * di * (a.scale_t * a.gT[k * C + i]);
            v += di * a.W[i * C + k] * (a.scale_t * a.gT[i * C + k]);
        }
        a.grad_diag[k] = s * v;
    }
}

// ---- hops ---------------------------------------------------------------------------------------------------------------
struct GloArgs : RowSide {
    const float *t;             // iterate to gather [N, C]
    const float *x;             // forward: S's first term and the mix; backward: the dots and the last fold
    const float *h0;            // forward, last hop
    const float *w;             // this hop's weight in device memory; nullptr = 1
    float *acc;                 // forward: S; backward: grad_x
    float *tout;                // the next iterate, or nullptr
    float *out;                 // forward, last hop: the layer's output (else nullptr)
    const float *MT;            // forward, last hop: M then T, [2, C, C]
    const double *G2;           // backward, last hop: gG + gG^T [C, C] (else nullptr)
    double *dotpart;            // backward: this hop's per-workgroup partial dots, or nullptr
    int init;                   // forward: 0 S = w t, 1 S = x + t (the first hop), 2 S += w t
    double beta, gamma, coe1;
    float *partial;             // [n_tasks, C]
    int C, N;
};

// forward epilogue of row r from its gathered sum s (= t_k's row); su / ss: this lane group's staging rows in LDS
template <int VEC, int G>
__device__ __forceinline__ void glo_finish_fwd(const GloArgs &a, int r, int lg, Row<VEC, G, 1> &s, const float *sMT,
                                               double *su, float *ss)
{
    using RowT = Row<VEC, G, 1>;
    const size_t off = (size_t)r * a.C;
    const int C = a.C, c0 = lg * VEC;
    if (a.tout) s.store(a.tout + off, C, lg);
    RowT x;
    if (a.init == 1 || a.out) x.load(a.x + off, C, lg);
    RowT S;
    if (a.init == 2) {
        S.load(a.acc + off, C, lg);
        if (a.w) S.axpy(*a.w, s); else S.add(s);
    } else if (a.init == 1) {
        S = x;
        S.add(s);
    } else {
        S = s;
        if (a.w) S.scale(*a.w);
    }
    S.store(a.acc + off, C, lg);
    if (!a.out) return;
    RowT h;
    h.load(a.h0 + off, C, lg);
    if (c0 < C) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            su[c0 + v] = (double)x.x[0][v] - a.gamma * (double)h.x[0][v];
            ss[c0 + v] = S.x[0][v];
        }
    }
    wave_lds_sync();
    if (c0 < C) {
        const float *sM = sMT, *sT = sMT + C * C;
        double o[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = 0.0;
        for (int i = 0; i < C; ++i) {
            const double ui = a.coe1 * su[i], si = a.beta * (double)ss[i];
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                o[v] += ui * (double)sT[i * C + c0 + v] + si * (double)sM[i * C + c0 + v];
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) x.x[0][v] = (float)(o[v] + a.gamma * (double)h.x[0][v]);
    }
    x.store(a.out + off, C, lg);
}

// backward epilogue of row r from its gathered sum s (= r_k's row); returns this lane's share of <r_k, x>
template <int VEC, int G>
__device__ __forceinline__ double glo_finish_bwd(const GloArgs &a, int r, int lg, Row<VEC, G, 1> &s, const double *sG2,
                                                 float *ss)
{
    using RowT = Row<VEC, G, 1>;
    const size_t off = (size_t)r * a.C;
    const int C = a.C, c0 = lg * VEC;
    if (a.tout) s.store(a.tout + off, C, lg);
    RowT acc;
    acc.load(a.acc + off, C, lg);
    if (a.w) acc.axpy(*a.w, s); else acc.add(s);
    double d = 0.0;
    if (a.dotpart || a.G2) {
        RowT x;
        x.load(a.x + off, C, lg);
        if (a.dotpart) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) d += (double)s.x[0][v] * (double)x.x[0][v];
        }
        if (a.G2) {
            if (c0 < C) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) ss[c0 + v] = x.x[0][v];
            }
            wave_lds_sync();
            if (c0 < C) {
                double o[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) o[v] = 0.0;
                for (int i = 0; i < C; ++i) {
                    const double xi = (double)ss[i];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) o[v] += xi * sG2[i * C + c0 + v];
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc.x[0][v] = (float)((double)acc.x[0][v] + o[v]);
            }
        }
    }
    acc.store(a.acc + off, C, lg);
    return d;
}

// The body below is row_walk.h's walk_rows, spelled out: through the template, k_glo_hop<4, 64, false> takes 74 VGPRs
// instead of 72 and loses a wave per SIMD (7 -> 6).  The gather, the finalize sum and the launch plan are the shared ones.
template <int VEC, int G, bool BWD>
__global__ __launch_bounds__(BLOCK) void k_glo_hop(const GloArgs a)
{
    using RowT = Row<VEC, G, 1>;
    constexpr int NG = 64 / G;
    // the C x C matrices of the last hop's epilogue (forward: 2 C^2 floats; backward: C^2 doubles) and one staging row (two,
    // forward) per lane group: dynamic LDS, asked for by the LAST hop's launch only - the other hops are plain gathers
    // and keep their residency
    extern __shared__ double glo_lds[];
    double *smat = glo_lds;
    double *su = smat + a.C * a.C;
    float *ss = reinterpret_cast<float *>(su + (BWD ? 0 : WAVES * NG * GLO_MAX_C));
    __shared__ double sd[WAVES];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    const int b = blockIdx.x;
    const bool last = BWD ? a.G2 != nullptr : a.out != nullptr;
    if (last && b >= a.nbA) {                              // (block-uniform)
        if constexpr (BWD) {
            for (int e = threadIdx.x; e < a.C * a.C; e += BLOCK) smat[e] = a.G2[e];
        } else {
            float *m = reinterpret_cast<float *>(smat);
            for (int e = threadIdx.x; e < 2 * a.C * a.C; e += BLOCK) m[e] = a.MT[e];
        }
        __syncthreads();
    }
    const int slot_lds = (wave * NG + gid) * GLO_MAX_C;
    auto finish = [&](int r, RowT &s) -> double {
        if constexpr (BWD) {
            return glo_finish_bwd<VEC, G>(a, r, lg, s, smat, ss + slot_lds);
        } else {
            glo_finish_fwd<VEC, G>(a, r, lg, s, reinterpret_cast<const float *>(smat), su + slot_lds, ss + slot_lds);
            return 0.0;
        }
    };
    RowT acc;
    acc.zero();
    double d = 0.0;
    if (b < a.nbA + a.nbB) {
        // split task or one wave per segment
        const bool task = b < a.nbA;
        const int tq = b * WAVES + wave;
        const int slot = a.n_split + (b - a.nbA) * WAVES + wave;
        const bool live = task ? tq < a.n_tasks : slot < a.n_med_end;          // (wave-uniform)
        if (live) {
            const int seg = a.perm[task ? a.task_slot[tq] : slot];
            const int e0 = task ? a.task_chunk[tq] * CHUNK : 0;
            const int qs = a.ptr[seg];
            const int deg = a.ptr[seg + 1] - qs;
            const int e1 = task ? min(deg, e0 + CHUNK) : deg;
            gather_rows<VEC, G, 1, 4>(a.t, a.C, a.C, a.idx, qs, e0, e1, NG, gid, lg, acc, NoWeight{});
            acc.reduce_across_groups();
            if (gid == 0) {
                if (task) acc.store(a.partial + (size_t)tq * a.C, a.C, lg);
                else d = finish(seg, acc);
            }
        }
    } else {
        const int slot = a.n_med_end + ((b - a.nbA - a.nbB) * WAVES + wave) * NG + gid;
        if (slot < a.N) {
            const int seg = a.perm[slot];
            const int qs = a.ptr[seg];
            const int deg = a.ptr[seg + 1] - qs;
            gather_rows<VEC, G, 1, 4>(a.t, a.C, a.C, a.idx, qs, 0, deg, 1, 0, lg, acc, NoWeight{});
            d = finish(seg, acc);
        }
    }
    if (BWD && a.dotpart && b >= a.nbA) {              // (block-uniform) the workgroup's partial dot, fixed order
        d = wave_sum_d(d);
        if (lane == 0) sd[wave] = d;
        __syncthreads();
        if (threadIdx.x == 0) a.dotpart[b - a.nbA] = (sd[0] + sd[1]) + (sd[2] + sd[3]);
    }
}

// split segments: the sum of the tasks' partial rows, then the epilogue per element (the
// arithmetic of glo_finish_*; the matrices from global memory: there are few such rows); the row's dot is partial
// number part0 + p
static __global__ __launch_bounds__(256) void k_glo_fin(const GloArgs a, int bwd, int part0)
{
    __shared__ float s[4][64];
    __shared__ double su[64];
    __shared__ float ss[64];
    const int p = blockIdx.x;
    const int r = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int C = a.C;
    const bool mine = q == 0 && c < C;
    const size_t at = (size_t)r * C + (c < C ? c : 0);
    const float z = combine_task_sums(s, sum_task_partials(a.partial, C, t0, t1, c, q), q, c);
    float accv = 0.f, xv = 0.f, hv = 0.f;
    double d = 0.0;
    if (mine) {
        if (a.tout) a.tout[at] = z;
        if (!bwd) {
            if (a.init == 1 || a.out) xv = a.x[at];
            if (a.init == 2) accv = a.w ? a.acc[at] + *a.w * z : a.acc[at] + z;
            else if (a.init == 1) accv = xv + z;
            else accv = a.w ? z * *a.w : z;
            a.acc[at] = accv;
            if (a.out) {
                hv = a.h0[at];
                su[c] = (double)xv - a.gamma * (double)hv;
                ss[c] = accv;
            }
        } else {
            accv = a.w ? a.acc[at] + *a.w * z : a.acc[at] + z;
            if (a.dotpart || a.G2) xv = a.x[at];
            if (a.dotpart) d = (double)z * (double)xv;
            if (a.G2) ss[c] = xv;
        }
    }
    __syncthreads();
    if (mine) {
        if (!bwd && a.out) {
            const float *M = a.MT, *T = a.MT + C * C;
            double o = 0.0;
            for (int i = 0; i < C; ++i)
                o += (a.coe1 * su[i]) * (double)T[i * C + c] + (a.beta * (double)ss[i]) * (double)M[i * C + c];
            a.out[at] = (float)(o + a.gamma * (double)hv);
        }
        if (bwd) {
            if (a.G2) {
                double o = 0.0;
                for (int i = 0; i < C; ++i) o += (double)ss[i] * a.G2[i * C + c];
                accv = (float)((double)accv + o);
            }
            a.acc[at] = accv;
        }
    }
    if (bwd && a.dotpart && q == 0) {                  // (wave 0 holds the row's elements)
        d = wave_sum_d(d);
        if (c == 0) a.dotpart[part0 + p] = d;
    }
}

// the backward's row-local pass: r_0 = q = beta g M^T, grad_h0 = gamma g - gamma coe1 g T^T, grad_x = coe1 g T^T
// [+ q: order_func1's k = 0 term].  L lanes per row (a power of two >= C), 256 / L rows per step.
static __global__ __launch_bounds__(256) void k_glo_pre(const float *__restrict__ g, const float *__restrict__ MT,
                                                        int64_t N, int C, int L, double beta, double gamma, double coe1,
                                                        int add_q, float *__restrict__ r0, float *__restrict__ gh0,
                                                        float *__restrict__ gx)
{
    __shared__ float sMt[GLO_CC], sTt[GLO_CC];         // transposed: [j][i]
    __shared__ float sg[256];
    const int CC = C * C;
    for (int e = threadIdx.x; e < CC; e += 256) {
        const int i = e / C, j = e % C;
        sMt[j * C + i] = MT[e];
        sTt[j * C + i] = MT[CC + e];
    }
    const int rpb = 256 / L, lr = threadIdx.x / L, i = threadIdx.x % L;
    for (int64_t row0 = (int64_t)blockIdx.x * rpb; row0 < N; row0 += (int64_t)gridDim.x * rpb) {   // (block-uniform)
        const int64_t row = row0 + lr;
        const bool valid = row < N && i < C;
        const size_t at = valid ? (size_t)row * C + i : 0;
        __syncthreads();
        const float gv = valid ? g[at] : 0.f;
        sg[threadIdx.x] = gv;
        __syncthreads();
        if (valid) {
            double q = 0.0, e = 0.0;
            for (int j = 0; j < C; ++j) {
                const double gj = (double)sg[lr * L + j];
                q += gj * (double)sMt[j * C + i];
                e += gj * (double)sTt[j * C + i];
            }
            q = beta * q;
            e = coe1 * e;
            r0[at] = (float)q;
            gh0[at] = (float)(gamma * (double)gv - gamma * e);
            gx[at] = (float)(add_q ? e + q : e);
        }
    }
}

// out[k] = the sum of row k of the partial dots, fixed order
static __global__ __launch_bounds__(256) void k_glo_dots(const double *__restrict__ dotpart, int64_t stride, int n,
                                                         double *__restrict__ out)
{
    __shared__ double s[256];
    const int k = blockIdx.x;
    const double *p = dotpart + (size_t)k * stride;
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += p[i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = s[0];
}

template <int VEC, int G, bool BWD> int launch_glo(const GloArgs &a0, hipStream_t st)
{
    constexpr int NG = 64 / G;
    GloArgs a = a0;
    const int grid = plan_side(a, a.N, NG);
    const bool last = BWD ? a.G2 != nullptr : a.out != nullptr;
    const size_t lds = !last ? 0 : (size_t)a.C * a.C * 8 + (BWD ? 0 : WAVES * NG * GLO_MAX_C * 8) + WAVES * NG * GLO_MAX_C * 4;
    if (grid > 0) k_glo_hop<VEC, G, BWD><<<grid, BLOCK, lds, st>>>(a);
    if (a.n_split > 0) k_glo_fin<<<a.n_split, 256, 0, st>>>(a, BWD ? 1 : 0, grid - a.nbA);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <int VEC, bool BWD> int dispatch_glo_g(const RowCfg &cfg, const GloArgs &a, hipStream_t st)
{
    switch (cfg.g) {
    case 8: return launch_glo<VEC, 8, BWD>(a, st);
    case 16: return launch_glo<VEC, 16, BWD>(a, st);
    case 32: return launch_glo<VEC, 32, BWD>(a, st);
    default: return launch_glo<VEC, 64, BWD>(a, st);
    }
}

template <bool BWD> int dispatch_glo(const RowCfg &cfg, const GloArgs &a, hipStream_t st)
{
    return dispatch_vec(cfg, [&](auto vec) { return dispatch_glo_g<decltype(vec)::value, BWD>(cfg, a, st); });
}

// A walks the out-edges of edge_index[0] (the CSC side), A^T the CSR side
static void glo_side(const sngnn_graph_t *g, bool transpose, GloArgs &a)
{
    a.N = (int)g->N;
    bind_side(g, !transpose, a);
    a.nbA = a.nbB = 0;
}

static int glo_parts(const sngnn_graph_t *g, bool transpose, const RowCfg &cfg)
{
    GloArgs a;
    glo_side(g, transpose, a);
    return plan_side(a, a.N, 64 / cfg.g) - a.nbA + a.n_split;
}

static int64_t gram_bytes(int C) { return up256((int64_t)GRAM_BLOCKS * 2 * C * C * 8); }

struct GloLayout { int64_t u0, u1, partial, dots, total, stride; };

static GloLayout glo_layout(const sngnn_graph_t *g, int C, int K, const RowCfg &cfg)
{
    GloLayout L;
    const int64_t rows = up256(g->N * (int64_t)C * 4);
    L.u0 = gram_bytes(C);                              // (the gram partials come first: sngnn_glognn_gram's workspace)
    L.u1 = L.u0 + rows;
    L.partial = L.u1 + rows;
    L.dots = L.partial + task_partial_bytes(g, C);
    L.stride = std::max<int64_t>(1, glo_parts(g, true, cfg));
    L.total = L.dots + up256((int64_t)std::max(K, 1) * L.stride * 8);
    return L;
}

static bool glo_row_cfg(int C, RowCfg &cfg) { return C <= GLO_MAX_C && row_cfg(C, cfg) && cfg.r == 1; }

static bool glo_scalars_ok(double alpha, double beta, double gamma)
{
    return alpha + beta != 0.0 && gamma != 1.0 && alpha == alpha && beta == beta && gamma == gamma;
}

}  // namespace sngnn

using namespace sngnn;

#define GLO_COMMON(g, C, K)                                                                                            \
    SN_REQUIRE((g) != nullptr, SNGNN_EINVAL, "graph is NULL");                                                         \
    SN_REQUIRE((g)->add_loops == 0 && (g)->remove_loops == 0 && (g)->N == (g)->Ntot && (g)->row_off == 0, SNGNN_EINVAL, \
               "the GloGNN norm layer needs an unpartitioned graph built with add_loops = 0, remove_loops = 0 (the "    \
               "raw edge list)");                                                                                      \
    SN_REQUIRE((K) >= 1, SNGNN_EINVAL, "orders must be at least 1");                                                   \
    RowCfg cfg;                                                                                                        \
    SN_REQUIRE(glo_row_cfg((C), cfg), SNGNN_ERANGE, "C must be in [1, " + std::to_string(GLO_MAX_C) + "]")

extern "C" int64_t sngnn_glognn_gram_workspace_bytes(int C)
{
    RowCfg cfg;
    return glo_row_cfg(C, cfg) ? gram_bytes(C) : 0;
}

extern "C" int sngnn_glognn_gram(const float *a, const float *a_sub, double sub_scale, const float *a2, const float *b,
                                 int64_t N, int C, double *out, double *out2, void *workspace, void *stream)
{
    RowCfg cfg;
    SN_REQUIRE(glo_row_cfg(C, cfg), SNGNN_ERANGE, "C must be in [1, " + std::to_string(GLO_MAX_C) + "]");
    SN_REQUIRE(N >= 0, SNGNN_EINVAL, "negative row count");
    SN_REQUIRE(out && workspace && (N == 0 || (a && b)), SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((a2 != nullptr) == (out2 != nullptr), SNGNN_EINVAL, "a2 and out2 go together");
    hipStream_t st = (hipStream_t)stream;
    GramArgs g;
    g.a = a; g.a_sub = a_sub; g.a2 = a2; g.b = b; g.sub = sub_scale; g.N = N; g.C = C; g.part = (double *)workspace;
    const int blocks = gram_blocks(N);
    k_glo_gram<<<blocks, 256, 0, st>>>(g);
    k_glo_gram_reduce<<<ceil_div(2 * C * C, 256), 256, 0, st>>>(g.part, blocks, C * C, out, out2);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_glognn_solve(const double *G, const float *diag, double alpha, double beta, double gamma, int C,
                                  double *M, double *T, double *V, double *W, float *MT32, void *stream)
{
    RowCfg cfg;
    SN_REQUIRE(glo_row_cfg(C, cfg), SNGNN_ERANGE, "C must be in [1, " + std::to_string(GLO_MAX_C) + "]");
    SN_REQUIRE(G && M && T && V && W && MT32, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(glo_scalars_ok(alpha, beta, gamma), SNGNN_EINVAL, "alpha + beta must not be 0 and gamma must not be 1");
    SolveArgs a;
    a.G = G; a.diag = diag; a.coe = 1.0 / (alpha + beta); a.coe1 = 1.0 - gamma; a.coe2 = 1.0 / a.coe1; a.C = C;
    a.M = M; a.T = T; a.V = V; a.W = W; a.MT32 = MT32;
    k_glo_solve<<<1, 256, 0, (hipStream_t)stream>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_glognn_solve_backward(const double *gM, const double *gT, double scale_m, double scale_t,
                                           const double *G, const double *V, const double *W, const float *diag,
                                           double alpha, double beta, double gamma, int C, double *gG2,
                                           double *grad_diag, double *tmp, void *stream)
{
    RowCfg cfg;
    SN_REQUIRE(glo_row_cfg(C, cfg), SNGNN_ERANGE, "C must be in [1, " + std::to_string(GLO_MAX_C) + "]");
    SN_REQUIRE(gM && gT && G && V && W && gG2 && tmp, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(glo_scalars_ok(alpha, beta, gamma), SNGNN_EINVAL, "alpha + beta must not be 0 and gamma must not be 1");
    SolveBwdArgs a;
    a.gM = gM; a.gT = gT; a.scale_m = scale_m; a.scale_t = scale_t; a.G = G; a.V = V; a.W = W; a.diag = diag;
    a.coe = 1.0 / (alpha + beta); a.coe1 = 1.0 - gamma; a.C = C; a.gG2 = gG2; a.grad_diag = grad_diag; a.tmp = tmp;
    k_glo_solve_bwd<<<1, 256, 0, (hipStream_t)stream>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int64_t sngnn_glognn_workspace_bytes(const sngnn_graph_t *g, int C, int orders)
{
    RowCfg cfg;
    if (g == nullptr || orders < 0 || !glo_row_cfg(C, cfg)) return 0;
    return glo_layout(g, C, orders, cfg).total;
}

extern "C" int sngnn_glognn_forward(const sngnn_graph_t *g, const float *x, const float *h0, const float *MT32,
                                    const float *orders_weight, int orders, double beta, double gamma, int C, float *S,
                                    float *out, void *workspace, void *stream)
{
    GLO_COMMON(g, C, orders);
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(x && h0 && MT32 && S && out && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {x, h0, S, out}), SNGNN_EINVAL,
               "rows must be aligned to the row vector width");
    hipStream_t st = (hipStream_t)stream;
    const GloLayout L = glo_layout(g, C, orders, cfg);
    float *u[2] = {(float *)((char *)workspace + L.u0), (float *)((char *)workspace + L.u1)};
    GloArgs a;
    glo_side(g, false, a);
    a.C = C; a.x = x; a.h0 = h0; a.acc = S; a.MT = MT32; a.G2 = nullptr; a.dotpart = nullptr;
    a.beta = beta; a.gamma = gamma; a.coe1 = 1.0 - gamma;
    a.partial = (float *)((char *)workspace + L.partial);
    for (int k = 1; k <= orders; ++k) {
        a.t = k == 1 ? x : u[k & 1];
        a.tout = k < orders ? u[(k + 1) & 1] : nullptr;
        a.out = k == orders ? out : nullptr;
        a.w = orders_weight ? orders_weight + (k - 1) : nullptr;
        a.init = k > 1 ? 2 : orders_weight ? 0 : 1;
        const int rc = dispatch_glo<false>(cfg, a, st);
        if (rc != SNGNN_OK) return rc;
    }
    return SNGNN_OK;
}

extern "C" int sngnn_glognn_backward(const sngnn_graph_t *g, const float *grad_out, const float *x, const float *MT32,
                                     const double *gG2, const float *orders_weight, int orders, double beta,
                                     double gamma, int C, float *grad_x, float *grad_h0, double *grad_w, void *workspace,
                                     void *stream)
{
    GLO_COMMON(g, C, orders);
    hipStream_t st = (hipStream_t)stream;
    if (g->N == 0) {
        if (grad_w) k_glo_dots<<<orders, 256, 0, st>>>(nullptr, 0, 0, grad_w);
        SN_HIP(hipGetLastError());
        return SNGNN_OK;
    }
    SN_REQUIRE(grad_out && x && MT32 && gG2 && grad_x && grad_h0 && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(!grad_w || orders_weight, SNGNN_EINVAL, "grad_w needs orders_weight");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {grad_out, x, grad_x, grad_h0}), SNGNN_EINVAL,
               "rows must be aligned to the row vector width");
    const GloLayout L = glo_layout(g, C, orders, cfg);
    float *u[2] = {(float *)((char *)workspace + L.u0), (float *)((char *)workspace + L.u1)};
    double *dots = (double *)((char *)workspace + L.dots);
    int lanes = 1;
    while (lanes < C) lanes <<= 1;
    const int rpb = 256 / lanes;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(GLO_PRE_BLOCKS, (g->N + rpb - 1) / rpb));
    k_glo_pre<<<grid, 256, 0, st>>>(grad_out, MT32, g->N, C, lanes, beta, gamma, 1.0 - gamma, orders_weight ? 0 : 1,
                                    u[0], grad_h0, grad_x);
    SN_HIP(hipGetLastError());
    GloArgs a;
    glo_side(g, true, a);
    a.C = C; a.x = x; a.h0 = nullptr; a.acc = grad_x; a.MT = nullptr; a.out = nullptr; a.init = 2;
    a.beta = beta; a.gamma = gamma; a.coe1 = 1.0 - gamma;
    a.partial = (float *)((char *)workspace + L.partial);
    for (int k = 1; k <= orders; ++k) {
        a.t = u[(k - 1) & 1];
        a.tout = k < orders ? u[k & 1] : nullptr;
        a.w = orders_weight ? orders_weight + (k - 1) : nullptr;
        a.G2 = k == orders ? gG2 : nullptr;
        a.dotpart = grad_w ? dots + (size_t)(k - 1) * L.stride : nullptr;
        const int rc = dispatch_glo<true>(cfg, a, st);
        if (rc != SNGNN_OK) return rc;
    }
    if (grad_w) {
        k_glo_dots<<<orders, 256, 0, st>>>(dots, L.stride, glo_parts(g, true, cfg), grad_w);
        SN_HIP(hipGetLastError());
    }
    return SNGNN_OK;
}

// H2GCN (models/models.py:903-1024), gfx950: the strict two-hop adjacency built on the GPU, and one hop over the two
// loop-free normalised adjacencies with the results side by side.
//
// 1. The pattern.  A1 = the loop-free graph (CSR by target, duplicates kept as separate entries).  Row i of
//        A2 = [(A1 A1 != 0) - diag - A1 > 0]
//    is the set of k with k -> j -> i for some j, k != i, k not an in-neighbour of i.  One workgroup per row; the
//    candidates are the CSR rows of the row's in-neighbours, their number bounded by cb_i = sum_{j in N(i)} deg(j):
//        cb_i <= SNGNN_TWO_HOP_HASH_MAX   an open-addressing table in LDS of the power of two >= 2 cb_i slots (atomicCAS
//                                         inserts, the in-neighbours tombstoned), counted; the fill sorts it (bitonic)
//        larger                           a bitmap of N bits in the workspace (atomicOr; the in-neighbours' and the
//                                         row's own bit cleared), read in word order - the row comes out sorted
//    Count and fill are separate launches with the caller's scan in between; no workgroup waits for another.
// 2. The hop.  z = [A^1 x | A^2 x] with A^s = D_s^-1/2 A_s D_s^-1/2, D_s the ROW (in-)degree of A_s on both sides and
//    dinv = 0 for an empty row.  The row-class walk of row_walk.h (small rows by lane group, medium rows by wave, hubs as
//    128-edge tasks + a finalize; rows gathered unscaled and multiplied by dinv[src]; fixed order, no floating-point
//    atomics; -ffp-contract=off) over the work lists of BOTH graphs in one grid.  The transpose is two sequences on the CSC
//    sides, the second adding into what the first stored.
#include <algorithm>

#include "entry.h"
#include "row_walk.h"

namespace sngnn {

// ---- the two-hop pattern ----------------------------------------------------------------------------------------------
constexpr int TH_BLOCK = 256;
constexpr int TH_HASH_MAX = SNGNN_TWO_HOP_HASH_MAX;
constexpr int TH_TABLE_MAX = 2 * TH_HASH_MAX;
constexpr int TH_EMPTY = 0x7fffffff, TH_TOMB = 0x7ffffffe;          // (node ids are below both)
constexpr int TH_MAX_WGS = 2048;
constexpr int64_t TH_BITMAP_BUDGET = (int64_t)64 << 20;             // bytes of bitmaps: fewer workgroups at large N

// words of one workgroup's bitmap: whole 128-byte lines, so no two workgroups share one
static int64_t th_words(int64_t N) { return (N + 1023) / 1024 * 32; }

static int th_workgroups(int64_t N)
{
    if (N <= 0) return 0;
    const int64_t by_budget = std::max<int64_t>(64, TH_BITMAP_BUDGET / (th_words(N) * 4));
    return (int)std::min<int64_t>({N, (int64_t)TH_MAX_WGS, by_budget});
}

// exclusive prefix of c over the workgroup's threads and the total (sh: WAVES words of LDS; two barriers)
__device__ __forceinline__ int block_scan_i(int c, int *sh, int &total)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < TH_BLOCK / 64; ++k) {
        const int v = sh[k];
        if (k < wave) before += v;
        tot += v;
    }
    __syncthreads();
    total = tot;
    return before + incl - c;
}

__device__ __forceinline__ unsigned th_hash(int k, int mask) { return ((unsigned)k * 2654435761u >> 7) & (unsigned)mask; }

// FILL == false: count[i] = entries of row i of A2.  FILL == true: the rows' entries, sources ascending, at offs[i] of
// out [2, E2] (row 0 the sources, row 1 the targets).  bitmaps: gridDim.x x words words, all zero on entry and on exit.
template <bool FILL>
__global__ __launch_bounds__(TH_BLOCK) void k_two_hop(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                      int N, int words, unsigned *__restrict__ bitmaps,
                                                      int32_t *__restrict__ count, const int64_t *__restrict__ offs,
                                                      int64_t E2, int64_t *__restrict__ out)
{
    __shared__ int tab[TH_TABLE_MAX];
    __shared__ int sh[TH_BLOCK / 64];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    unsigned *bm = bitmaps + (size_t)blockIdx.x * words;
    for (int i = blockIdx.x; i < N; i += gridDim.x) {
        const int q0 = rowptr[i], d = rowptr[i + 1] - q0;
        // the candidate bound, saturated just above the threshold (every partial and their sum fit an int)
        int part = 0;
        for (int e = tid; e < d; e += TH_BLOCK) {
            const int j = col[q0 + e];
            part = min(part + (rowptr[j + 1] - rowptr[j]), TH_HASH_MAX + 1);
        }
        int cb;
        block_scan_i(part, sh, cb);
        int total = 0;
        const int64_t off = FILL ? offs[i] : 0;
        if (cb == 0) {
            // no candidate
        } else if (cb <= TH_HASH_MAX) {
            int T = 64;
            while (T < 2 * cb) T <<= 1;
            for (int s = tid; s < T; s += TH_BLOCK) tab[s] = TH_EMPTY;
            __syncthreads();
            for (int e = wave; e < d; e += TH_BLOCK / 64) {
                const int j = col[q0 + e];
                const int p1 = rowptr[j + 1];
                for (int p = rowptr[j] + lane; p < p1; p += 64) {
                    const int k = col[p];
                    if (k == i) continue;
                    unsigned h = th_hash(k, T - 1);
                    for (;;) {          // (at most cb <= T / 2 distinct keys: an empty slot is always found)
                        const int old = atomicCAS(&tab[h], TH_EMPTY, k);
                        if (old == TH_EMPTY || old == k) break;
                        h = (h + 1) & (unsigned)(T - 1);
                    }
                }
            }
            __syncthreads();
            // the in-neighbours leave (nothing is inserted any more: a tombstone keeps the probe chains whole)
            for (int e = tid; e < d; e += TH_BLOCK) {
                const int j = col[q0 + e];
                unsigned h = th_hash(j, T - 1);
                for (;;) {
                    const int v = tab[h];
                    if (v == TH_EMPTY) break;
                    if (v == j) { tab[h] = TH_TOMB; break; }
                    h = (h + 1) & (unsigned)(T - 1);
                }
            }
            __syncthreads();
            if constexpr (!FILL) {
                int c = 0;
                for (int s = tid; s < T; s += TH_BLOCK) c += tab[s] < TH_TOMB ? 1 : 0;
                block_scan_i(c, sh, total);
            } else {
                // bitonic sort, ascending: the entries in front, tombstones and empty slots behind
                for (int k = 2; k <= T; k <<= 1)
                    for (int j = k >> 1; j > 0; j >>= 1) {
                        for (int s = tid; s < T; s += TH_BLOCK) {
                            const int o = s ^ j;
                            if (o > s) {
                                const int a = tab[s], b = tab[o];
                                if ((a > b) == ((s & k) == 0)) { tab[s] = b; tab[o] = a; }
                            }
                        }
                        __syncthreads();
                    }
                for (int s = tid; s < T; s += TH_BLOCK) {
                    const int v = tab[s];
                    if (v < TH_TOMB) {
                        out[off + s] = v;
                        out[E2 + off + s] = i;
                    }
                }
                __syncthreads();
            }
        } else {
            for (int e = wave; e < d; e += TH_BLOCK / 64) {
                const int j = col[q0 + e];
                const int p1 = rowptr[j + 1];
                for (int p = rowptr[j] + lane; p < p1; p += 64) {
                    const int k = col[p];
                    atomicOr(&bm[k >> 5], 1u << (k & 31));
                }
            }
            __syncthreads();
            if (tid == 0) atomicAnd(&bm[i >> 5], ~(1u << (i & 31)));
            for (int e = tid; e < d; e += TH_BLOCK) {
                const int j = col[q0 + e];
                atomicAnd(&bm[j >> 5], ~(1u << (j & 31)));
            }
            __syncthreads();
            // read and clear in word order (an exchange: it reads where the atomics above wrote)
            for (int w0 = 0; w0 < words; w0 += TH_BLOCK) {
                const int w = w0 + tid;
                unsigned bits = w < words ? atomicExch(&bm[w], 0u) : 0u;
                int chunk;
                const int before = block_scan_i(__popc(bits), sh, chunk);
                if constexpr (FILL) {
                    int64_t p = off + total + before;
                    while (bits) {
                        const int b = __ffs(bits) - 1;
                        bits &= bits - 1;
                        out[p] = (int64_t)w * 32 + b;
                        out[E2 + p] = i;
                        ++p;
                    }
                }
                total += chunk;
            }
        }
        if constexpr (!FILL)
            if (tid == 0) count[i] = total;
    }
}

static __global__ void k_h2gcn_dinv(const int32_t *__restrict__ rowptr, int64_t N, float *__restrict__ dinv)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) {
        const int deg = rowptr[i + 1] - rowptr[i];
        dinv[i] = deg > 0 ? 1.0f / ieee_sqrt((float)deg) : 0.f;
    }
}

// ---- the hop ----------------------------------------------------------------------------------------------------------
// one adjacency's share of a launch
struct H2Side : RowSide {
    const float *src;            // column 0 of the gathered slice
    float *dst;                  // column 0 of the W columns this side stores
    int64_t ld_src, ld_dst;
    const float *dinv;           // [N]
    float *partial;              // [n_tasks, W]
    int nb;                      // workgroups of this side (split tasks, wave rows and small rows)
    int col0;                    // this side's first column in the epilogue vectors
    int add;                     // dst += z instead of dst = z (the transpose's second sequence)
};

struct H2Args {
    H2Side s[2];
    int sides, W, N;
    const float *rm, *invstd, *gamma, *beta;
};

// one stored element of column c (of this side's W) from z = dinv_r S: the norm, or the sum with what is there
__device__ __forceinline__ float h2_element(const H2Args &a, const H2Side &s, int c, float z, const float *d)
{
    if (a.rm) {
        const int cc = s.col0 + c;
        z = ((z - a.rm[cc]) * a.invstd[cc]) * a.gamma[cc] + a.beta[cc];
    }
    if (s.add) z = d[c] + z;
    return z;
}

template <int VEC, int G, int R>
__device__ __forceinline__ void h2_finish(const H2Args &a, const H2Side &s, int r, int lg, Row<VEC, G, R> &acc)
{
    acc.scale(s.dinv[r]);
    float *d = s.dst + (size_t)r * s.ld_dst;
    const bool epi = a.rm != nullptr || s.add != 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int c0 = (q * G + lg) * VEC;
        if (c0 < a.W) {
            if (epi) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc.x[q][v] = h2_element(a, s, c0 + v, acc.x[q][v], d);
            }
            store_vec<VEC>(d + c0, acc.x[q]);
        }
    }
}

// the workgroups of side 0, then those of side 1: S_i = sum dinv[src] * src[src, 0 .. W) (gather_rows), then h2_finish
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_h2gcn_hop(const H2Args a)
{
    using RowT = Row<VEC, G, R>;
    int b = blockIdx.x;
    const bool second = b >= a.s[0].nb;
    if (second) b -= a.s[0].nb;
    const H2Side s = second ? a.s[1] : a.s[0];
    RowT acc;
    walk_rows<G>(
        s, b, a.N, acc,
        [&](int, int qs, int e0, int e1, int stride, int first, int lg, RowT &x) {
            gather_rows<VEC, G, R, gather_unroll(R)>(s.src, s.ld_src, a.W, s.idx, qs, e0, e1, stride, first, lg, x,
                                                     RowWeight{s.dinv});
        },
        [&](int tq, int lg, RowT &x) { x.store(s.partial + (size_t)tq * a.W, a.W, lg); },
        [&](int seg, int, int lg, RowT &x) { h2_finish<VEC, G, R>(a, s, seg, lg, x); });
}

// split segments of either side: the sum of the tasks' partial rows, then h2_finish's arithmetic per element
static __global__ __launch_bounds__(256) void k_h2gcn_hop_fin(const H2Args a)
{
    __shared__ float sm[4][64];
    int p = blockIdx.x;
    const bool second = p >= a.s[0].n_split;
    if (second) p -= a.s[0].n_split;
    const H2Side &s = second ? a.s[1] : a.s[0];
    const int r = s.perm[p];
    const int t0 = s.split_task0[p], t1 = s.split_task0[p + 1];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const float di = s.dinv[r];
    float *d = s.dst + (size_t)r * s.ld_dst;
    for (int c0 = 0; c0 < a.W; c0 += 64) {
        const int c = c0 + cl;
        const float sum = combine_task_sums(sm, sum_task_partials(s.partial, a.W, t0, t1, c, q), q, cl);
        if (q == 0 && c < a.W) d[c] = h2_element(a, s, c, sum * di, d);
        __syncthreads();
    }
}

template <int VEC, int G, int R> int launch_h2gcn_hop(const H2Args &a0, hipStream_t st)
{
    H2Args a = a0;
    int blocks = 0, fin = 0;
    for (int i = 0; i < a.sides; ++i) {
        H2Side &s = a.s[i];
        s.nb = plan_side(s, a.N, 64 / G);
        blocks += s.nb;
        fin += s.n_split;
    }
    if (blocks > 0) k_h2gcn_hop<VEC, G, R><<<blocks, BLOCK, 0, st>>>(a);
    if (fin > 0) k_h2gcn_hop_fin<<<fin, 256, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

static int run_h2gcn_hop(int vec, int g, int r, const H2Args &a, hipStream_t st)
{
    return dispatch_slice_layout(vec, g, r, [&](auto v, auto g_, auto r_) {
        return launch_h2gcn_hop<decltype(v)::value, decltype(g_)::value, decltype(r_)::value>(a, st);
    });
}

// H2GCN's A1 and A2: unpartitioned, no loop added, every loop removed
static bool whole_graph_without_loops(const sngnn_graph_t *g)
{
    return g->add_loops == 0 && g->remove_loops == 1 && g->N == g->Ntot && g->row_off == 0;
}

static void bind_h2_side(const sngnn_graph_t *g, bool csc, const float *src, int64_t ld_src, float *dst, int64_t ld_dst,
                         const float *dinv, void *workspace, int col0, int add, H2Side &s)
{
    bind_side(g, csc, s);
    s.src = src; s.ld_src = ld_src; s.dst = dst; s.ld_dst = ld_dst;
    s.dinv = dinv; s.partial = (float *)workspace;
    s.nbA = s.nbB = s.nb = 0;
    s.col0 = col0; s.add = add;
}

}  // namespace sngnn

using namespace sngnn;

extern "C" int64_t sngnn_two_hop_workspace_bytes(const sngnn_graph_t *g)
{
    if (g == nullptr) return 0;
    return up256((int64_t)th_workgroups(g->N) * th_words(g->N) * 4) + 256;
}

static int two_hop_check(const sngnn_graph_t *g)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    SN_REQUIRE(whole_graph_without_loops(g), SNGNN_EINVAL,
               "the two-hop build needs the loop-free graph A1: unpartitioned, built with add_loops = 0, remove_loops = 1");
    SN_REQUIRE(g->N < (int64_t)TH_TOMB, SNGNN_ERANGE, "N does not fit the builder's 32-bit node ids");
    return SNGNN_OK;
}

extern "C" int sngnn_two_hop_count(const sngnn_graph_t *g, int32_t *count, void *workspace, void *stream)
{
    if (int rc = two_hop_check(g)) return rc;
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(count && workspace, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int wgs = th_workgroups(g->N);
    const int words = (int)th_words(g->N);
    SN_HIP(hipMemsetAsync(workspace, 0, (size_t)wgs * words * 4, st));
    k_two_hop<false><<<wgs, TH_BLOCK, 0, st>>>(g->rowptr, g->col, (int)g->N, words, (unsigned *)workspace, count, nullptr,
                                               0, nullptr);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_two_hop_fill(const sngnn_graph_t *g, const int64_t *offsets, int64_t E2, int64_t *edge_index,
                                  void *workspace, void *stream)
{
    if (int rc = two_hop_check(g)) return rc;
    SN_REQUIRE(E2 >= 0, SNGNN_EINVAL, "E2 is negative");
    SN_REQUIRE(E2 <= (int64_t)INT32_MAX, SNGNN_ERANGE, "the two-hop adjacency has more than 2^31 - 1 entries");
    if (g->N == 0 || E2 == 0) return SNGNN_OK;
    SN_REQUIRE(offsets && edge_index && workspace, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int wgs = th_workgroups(g->N);
    const int words = (int)th_words(g->N);
    SN_HIP(hipMemsetAsync(workspace, 0, (size_t)wgs * words * 4, st));
    k_two_hop<true><<<wgs, TH_BLOCK, 0, st>>>(g->rowptr, g->col, (int)g->N, words, (unsigned *)workspace, nullptr, offsets,
                                              E2, edge_index);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_h2gcn_dinv(const sngnn_graph_t *g, float *dinv, void *stream)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    SN_REQUIRE(whole_graph_without_loops(g), SNGNN_EINVAL,
               "H2GCN's dinv needs a loop-free graph: unpartitioned, built with add_loops = 0, remove_loops = 1");
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(dinv, SNGNN_EINVAL, "NULL argument");
    k_h2gcn_dinv<<<ceil_div(g->N, 256), 256, 0, (hipStream_t)stream>>>(g->rowptr, g->N, dinv);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int64_t sngnn_h2gcn_workspace_bytes(const sngnn_graph_t *g, int W)
{
    RowCfg cfg;
    if (g == nullptr || !row_cfg(W, cfg)) return 0;
    return task_partial_bytes(g, W) + 256;
}

extern "C" int sngnn_h2gcn_hop(const sngnn_graph_t *g1, const sngnn_graph_t *g2, const sngnn_h2gcn_hop_t *h,
                               const float *dinv1, const float *dinv2, int transpose, void *workspace1, void *workspace2,
                               void *stream)
{
    SN_REQUIRE(g1 != nullptr && g2 != nullptr && h != nullptr, SNGNN_EINVAL, "graph or hop description is NULL");
    SN_REQUIRE(whole_graph_without_loops(g1) && whole_graph_without_loops(g2), SNGNN_EINVAL,
               "the H2GCN hop needs two loop-free graphs: unpartitioned, built with add_loops = 0, remove_loops = 1");
    SN_REQUIRE(g1->N == g2->N, SNGNN_EINVAL, "the two graphs have different node counts");
    RowCfg cfg;
    SN_REQUIRE(row_cfg(h->W, cfg), SNGNN_ERANGE, "W must be in [1, " + std::to_string(SNGNN_MAX_CHANNELS) + "]");
    SN_REQUIRE((h->rm != nullptr) == (h->invstd != nullptr) && (h->rm != nullptr) == (h->gamma != nullptr) &&
                   (h->rm != nullptr) == (h->beta_bn != nullptr),
               SNGNN_EINVAL, "rm, invstd, gamma and beta_bn go together (all NULL: no norm epilogue)");
    SN_REQUIRE(h->rm == nullptr || transpose == 0, SNGNN_EINVAL, "the norm epilogue belongs to the forward hop");
    if (g1->N == 0) return SNGNN_OK;
    SN_REQUIRE(h->src && h->dst && dinv1 && dinv2 && workspace1 && workspace2, SNGNN_EINVAL, "NULL argument");
    const int W = h->W;
    const int w_src = transpose ? 2 * W : W, w_dst = transpose ? W : 2 * W;
    SN_REQUIRE(h->ld_src >= w_src && h->ld_dst >= w_dst, SNGNN_EINVAL, "a row stride is smaller than the slice's width");
    SN_REQUIRE((((uintptr_t)h->src | (uintptr_t)h->dst) & 3) == 0, SNGNN_EINVAL, "tables must be aligned to 4 bytes");
    const int64_t N = g1->N;
    SN_REQUIRE(!overlap(Slice{h->dst, N, h->ld_dst, w_dst}, Slice{h->src, N, h->ld_src, w_src}), SNGNN_EINVAL,
               "the destination overlaps the source (other rows still gather the source); column slices of one table "
               "must be disjoint column ranges of the same stride");
    const uint64_t bits = (uint64_t)W | (uint64_t)h->ld_src | (uint64_t)h->ld_dst | ((uintptr_t)h->src >> 2) |
                          ((uintptr_t)h->dst >> 2);
    const int vec = bits % 4 == 0 ? 4 : bits % 2 == 0 ? 2 : 1;
    const int r = cfg.r * (cfg.vec / vec);
    SN_REQUIRE(r <= 8, SNGNN_ERANGE,
               "W = " + std::to_string(W) + " at vector width " + std::to_string(vec) +
                   " needs more than 8 steps per lane (align the slices, or run the plain op sequence)");
    H2Args a;
    a.W = W; a.N = (int)N;
    a.rm = h->rm; a.invstd = h->invstd; a.gamma = h->gamma; a.beta = h->beta_bn;
    hipStream_t st = (hipStream_t)stream;
    if (!transpose) {
        a.sides = 2;
        bind_h2_side(g1, false, h->src, h->ld_src, h->dst, h->ld_dst, dinv1, workspace1, 0, 0, a.s[0]);
        bind_h2_side(g2, false, h->src, h->ld_src, h->dst + W, h->ld_dst, dinv2, workspace2, W, 0, a.s[1]);
        return run_h2gcn_hop(vec, cfg.g, r, a, st);
    }
    // A^1T g[:, 0:W] stored, then A^2T g[:, W:2W] added to it: stream order between the two sequences
    a.sides = 1;
    bind_h2_side(g1, true, h->src, h->ld_src, h->dst, h->ld_dst, dinv1, workspace1, 0, 0, a.s[0]);
    a.s[1] = a.s[0];
    if (int rc = run_h2gcn_hop(vec, cfg.g, r, a, st)) return rc;
    bind_h2_side(g2, true, h->src + W, h->ld_src, h->dst, h->ld_dst, dinv2, workspace2, 0, 1, a.s[0]);
    a.s[1] = a.s[0];
    return run_h2gcn_hop(vec, cfg.g, r, a, st);
}

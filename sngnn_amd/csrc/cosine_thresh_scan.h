// Threshold similarity graph at any N (gfx950): for every query row the base rows whose cosine reaches `thr`, as CSR,
// straight from the two feature tables - the M x N similarity is never stored.  The third consumer of the tile engine
// (cosine_tiles.h), beside the ranking of knn_scan.h and the counting into bins of cosine_hist_scan.h: it KEEPS a value
// with s >= thr.  The answer's size is not known beforehand, so the scan runs twice, like the sparse side's
// sngnn_sparse_cosine_count / _fill: a count pass, the caller's exclusive scan, a fill pass.
//
// Tile walk: sngnn_knn_query's.  A workgroup owns 32 NWV query rows and walks the column tiles of its range
// (blockIdx.y: knn_query_plan cuts the base into ranges when there are few row blocks); a wave owns 32 whole rows.
// C/D layout of a 32 x 32 block: acc[b][r] of lane l is column 32 b + (l & 31), row (r & 3) + 8 (r >> 2) + 4 (l >> 5)
// of the wave's 32 - for register r and block b one HALF-WAVE holds 32 consecutive columns of ONE row, and no other
// wave ever sees that row.
//
// Value and rule: s = acc * (inv_i * inv_j) + 0.0f, the kNN scan's expression on the same products (never -0.0);
// entry iff i < M, j < N, j != self_offset + i and s >= thr in fp32 (a NaN is no entry).
//
// Count pass: a lane adds its passing values into one register per accumulator register (16), the 32 lanes of a
// half-wave are added at the end of the range and one lane stores part[y][row] - one writer per slot.
// k_thresh_ranges then turns part[.][row] into the exclusive prefix over the ranges and stores the total to count[row].
//
// Fill pass: the same walk; a row's cursor lives in a register of its half-wave (the same value in its 32 lanes) and
// starts at rowptr[row] + part[y][row].  Per (r, b): one ballot; a passing lane writes (column, s) at cursor +
// popcount(its half of the mask below the lane); the cursor moves on by the half's popcount.  Blocks ascend inside a
// tile, tiles inside a range, ranges by y: a row's columns ascend without a sort.  A register none of whose values
// pass - almost every one at a useful threshold - costs one ballot for all its blocks.
//
// No atomics in either pass; the same bits on every run.  Both passes must take the same engine variant and plan:
// cosine_thresh.hip derives both from the same arguments and knob state.
//
// This header holds the kernels, the workspace layout and the shared refusals; cosine_thresh.hip launches them on fp32
// tables, cosine_thresh_half.hip on fp16 / bf16 tables (sngnn_cosine_threshold_count_half / _fill_half: the engine's
// PL < 3, see knn_half.hip).
#pragma once
#include <algorithm>
#include <cmath>

#include "knn_scan.h"          // knn_query_plan (and cosine_tiles.h)

namespace sngnn {

template <int FH, bool BF3, int NWV, int CB, bool FILL, int PL = 3>
__global__ __launch_bounds__(64 * NWV) void k_cosine_thresh(const typename CosineTiles<FH, BF3, NWV, CB, PL>::XT *__restrict__ xq, int64_t M,
                                                           const float *__restrict__ invq,
                                                           const typename CosineTiles<FH, BF3, NWV, CB, PL>::XT *__restrict__ xb, int64_t N, int64_t F,
                                                           const float *__restrict__ invb, float thr, int64_t self,
                                                           int tiles_per_split, int32_t *__restrict__ part,
                                                           const int64_t *__restrict__ rowptr, int64_t nnz,
                                                           int32_t *__restrict__ out_col, float *__restrict__ out_val)
{
    using Eng = CosineTiles<FH, BF3, NWV, CB, PL>;
    constexpr int KC = Eng::KC, KR = Eng::KR;
    __shared__ float sA[Eng::SA_FLOATS];
    __shared__ __align__(16) float sB[Eng::SB_FLOATS];
    __shared__ float s_irow[NWV][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * KR;
    if (lane < 32) s_irow[wave][lane] = (row0 + wave * 32 + lane < M) ? invq[row0 + wave * 32 + lane] : 0.f;
    const int64_t ncol_tiles = (N + KC - 1) / KC;
    const int64_t ct_begin = (int64_t)blockIdx.y * tiles_per_split;
    const int64_t ct_end = min(ncol_tiles, ct_begin + tiles_per_split);

    // per accumulator register: this lane's row, whether it exists, and its count (count pass) or cursor (fill pass)
    int run[16];
    unsigned rowmask = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t i = row0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (i < M) rowmask |= 1u << r;
        run[r] = 0;
        if constexpr (FILL) {
            if (i < M) run[r] = (int)rowptr[i] + part[(size_t)blockIdx.y * M + i];
        }
    }

    Eng eng;
    eng.load_rows(xq, M, F, row0);
    __syncthreads();

    for (int64_t ct = ct_begin; ct < ct_end; ++ct) {
        const int64_t col0 = ct * KC;
        f32x16 acc[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        // the tile's column ids and inverse norms: requested here, they travel under the products
        float icol[CB];
        int64_t jcol[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            jcol[b] = col0 + b * 32 + l32;
            icol[b] = invb[min(jcol[b], N - 1)];
        }
#pragma unroll
        for (int b = 0; b < CB; ++b) icol[b] = jcol[b] < N ? icol[b] : 0.f;
        eng.template products<true>(xb, N, F, row0, ct, ct_begin, ct_end, sA, sB, acc, xq, M);
        // ---- keep: C/D layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        int jc[CB];
        int64_t jown[CB];                                       // the row this column is the own node of (negative: none)
        bool jok[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            jc[b] = (int)jcol[b];
            jok[b] = jcol[b] < N;
            jown[b] = self >= 0 ? jcol[b] - self : -1;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int64_t i = row0 + wave * 32 + lr;
            const float irow = s_irow[wave][lr];
            const bool rowok = (rowmask >> r) & 1u;
            float sv[CB];
            bool pass[CB], any = false;
#pragma unroll
            for (int b = 0; b < CB; ++b) {
                sv[b] = acc[b][r] * (irow * icol[b]) + 0.0f;
                pass[b] = rowok && jok[b] && jown[b] != i && sv[b] >= thr;
                any |= pass[b];
            }
            if constexpr (!FILL) {
#pragma unroll
                for (int b = 0; b < CB; ++b) run[r] += pass[b] ? 1 : 0;
            } else {
                if (__ballot(any) == 0ull) continue;            // wave-uniform: nothing of this register is kept
#pragma unroll
                for (int b = 0; b < CB; ++b) {
                    const unsigned long long m = __ballot(pass[b]);
                    const unsigned mh = half ? (unsigned)(m >> 32) : (unsigned)m;
                    const int pos = run[r] + __popc(mh & ((1u << l32) - 1u));
                    // (pos < nnz whenever rowptr is the scan of the matching count; a caller's mistake must not
                    // become a store outside out_col / out_val)
                    if (pass[b] && (int64_t)pos < nnz && pos >= 0) {
                        out_col[pos] = jc[b];
                        out_val[pos] = sv[b];
                    }
                    run[r] += __popc(mh);
                }
            }
        }
    }
    if constexpr (!FILL) {
        // the 32 lanes of a half-wave hold one row's counts: add them, one lane stores
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int c = run[r];
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
            const int64_t i = row0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (l32 == 0 && i < M) part[(size_t)blockIdx.y * M + i] = c;
        }
    }
}

// part[y][row], y < ns: the range's count -> the count of the ranges before it; count[row] = the row's total.
// One thread per row, the ranges in order.
static __global__ __launch_bounds__(256) void k_thresh_ranges(int32_t *__restrict__ part, int64_t M, int ns,
                                                              int32_t *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    int total = 0;
    for (int y = 0; y < ns; ++y) {
        const int c = part[(size_t)y * M + i];
        part[(size_t)y * M + i] = total;
        total += c;
    }
    count[i] = total;
}

// (no base row: every count is 0)
static __global__ __launch_bounds__(256) void k_thresh_zero(int32_t *__restrict__ count, int64_t M)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < M) count[i] = 0;
}

// the column ranges either tile shape may use for M query rows against N base rows
static int thresh_ranges_max(int64_t M, int64_t N)
{
    return std::max(knn_query_plan(M, N, KN_M, KN_M).ns, knn_query_plan(M, N, 256, 64).ns);
}

// workspace: the inverse norms of the queries and of the base, then the column ranges' counts [ns][M]
struct ThreshWs { float *invq, *invb; int32_t *part; };
static inline ThreshWs thresh_ws(void *workspace, int64_t M, int64_t N)
{
    char *w = (char *)workspace;
    return {(float *)w, (float *)(w + (M + 63) / 64 * 256), (int32_t *)(w + (M + 63) / 64 * 256 + (N + 63) / 64 * 256)};
}

// the refusals every count and fill entry shares
static inline int thresh_check(int64_t M, int64_t N, int64_t F, float thr, int64_t self_offset)
{
    SN_REQUIRE(M >= 0 && N >= 0 && F >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(M < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), SNGNN_EINVAL, "too many rows");
    SN_REQUIRE(!std::isnan(thr), SNGNN_EINVAL, "thr is NaN");
    SN_REQUIRE(self_offset >= -1 && (self_offset < 0 || self_offset + M <= N), SNGNN_EINVAL,
               "self_offset: the queries are not rows [self_offset, self_offset + M) of the base");
    return SNGNN_OK;
}

}  // namespace sngnn

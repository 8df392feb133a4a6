// The classification head of the last layer inside the forward (FwdArgs::head_*): a finished mean row through
// head_row.h's log-softmax, the per-wave and per-workgroup entries of head_part, and the role that reads back every
// row that is not a split row (k_agg_head_rows, or workgroups of the mixed finalize: agg_fwd_fin.h).
// Needs agg_fwd_args.h and head_row.h.
#pragma once
#include "agg_fwd_args.h"
#include "head_row.h"

namespace sngnn {

// what a wave has added up over its rows (lanes lg == 0 of every lane group hold terms)
struct HeadAcc { float loss = 0.f, corr = 0.f, lossb = 0.f, corrb = 0.f; };

// the finished mean row `acc` of target i, held by a G-lane group, goes through the head; yy / sv = the
// row's label and split byte (loaded early by the caller: not a round trip at the end of the row)
// (in_memory: `out` already holds the row as it is in acc - stored again only if the bias changes it)
template <int VEC, int G, int R>
__device__ __forceinline__ void head_store_row(const FwdArgs &a, const Row<VEC, G, R> &acc, int i, int lg, int yy,
                                               unsigned sv, HeadAcc &ha, bool in_memory = false)
{
    if constexpr (VEC == 4 && R == 1 && (G == 8 || G == 16)) {
        const bool in = 4 * lg < a.C;
        const int c0 = in ? 4 * lg : 0;
        float4 t = make_float4(acc.x[0][0], acc.x[0][1], acc.x[0][2], acc.x[0][3]);
        if (a.epi_flags & 2) {
            const float4 b = *reinterpret_cast<const float4 *>(a.epi_bias + c0);
            t.x += b.x; t.y += b.y; t.z += b.z; t.w += b.w;
        }
        float4 *o = reinterpret_cast<float4 *>(a.out + (size_t)i * a.C + c0);
        const bool grad = (a.head_flags & 2) != 0;
        if (sv == 0) {                                        // (group-uniform) the row is in no split
            if (in && grad) *o = make_float4(0.f, 0.f, 0.f, 0.f);
            else if (in && (!in_memory || (a.epi_flags & 2))) *o = t;
            return;
        }
        if (in && !grad && (!in_memory || (a.epi_flags & 2))) *o = t;
        const HeadRow hr = head_row<G>(t, in, c0, yy);
        if (lg == 0) {
            if (a.head_flags & 1) {
                if (sv & 1) { ha.loss += hr.loss; ha.corr += hr.corr; }
                if (sv & 2) { ha.lossb += hr.loss; ha.corrb += hr.corr; }
            } else {
                ha.loss += hr.loss;
                ha.corr += hr.corr;
            }
        }
        if (in && grad) *o = head_row_grad(hr, a.head_scale);
    }
}

// one entry of head_part from a wave's accumulators (fixed order: a shuffle tree over the lanes)
__device__ __forceinline__ void head_write_entry(const FwdArgs &a, int entry, const HeadAcc &ha)
{
    float v0 = ha.loss, v1 = ha.corr, v2 = ha.lossb, v3 = ha.corrb;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        v0 += __shfl_xor(v0, m, 64); v1 += __shfl_xor(v1, m, 64);
        v2 += __shfl_xor(v2, m, 64); v3 += __shfl_xor(v3, m, 64);
    }
    if (lane_id() == 0) *reinterpret_cast<float4 *>(a.head_part + 4 * (size_t)entry) = make_float4(v0, v1, v2, v3);
}

// Every row that is NOT a split row (in-degree <= WAVE_T), in natural order, read back from `out`: wave w of
// nw walks 2 x 64 / G rows per step and returns what it has added up.
template <int VEC, int G, int R>
__device__ __forceinline__ HeadAcc head_rows_role(const FwdArgs &a, int w, int nw)
{
    HeadAcc ha;
    if constexpr (VEC == 4 && R == 1 && (G == 8 || G == 16)) {
        constexpr int RPW = 64 / G, U = 2;
        const int lane = lane_id();
        const int gid = lane / G, lg = lane % G;
        const int c0 = 4 * lg < a.C ? 4 * lg : 0;
        for (int64_t base = (int64_t)w * (RPW * U); base < a.N; base += (int64_t)nw * (RPW * U)) {
            Row<VEC, G, R> row[U];
            int yy[U], deg[U];
            unsigned sv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {                       // all loads first
                const int64_t i = base + u * RPW + gid;
                const int64_t ic = i < a.N ? i : a.N - 1;
                deg[u] = a.rowptr[ic + 1] - a.rowptr[ic];
                sv[u] = a.head_sel[ic];
                yy[u] = (int)a.head_y[ic];
                const float4 t = *reinterpret_cast<const float4 *>(a.out + ic * a.C + c0);
                row[u].x[0][0] = t.x; row[u].x[0][1] = t.y; row[u].x[0][2] = t.z; row[u].x[0][3] = t.w;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + u * RPW + gid;
                if (i >= a.N || deg[u] > WAVE_T) continue;      // (group-uniform; split rows: their finalize)
                head_store_row<VEC, G, R>(a, row[u], (int)i, lg, yy[u], sv[u], ha, true);
            }
        }
    }
    return ha;
}

// one entry of head_part per WORKGROUP of the head role: the waves' sums through LDS, added in wave order
// (s_mem: 4 floats per wave).  Called by every thread of the workgroup.
__device__ __forceinline__ void head_block_entry(const FwdArgs &a, int entry, const HeadAcc &ha, float *s_mem)
{
    float v0 = ha.loss, v1 = ha.corr, v2 = ha.lossb, v3 = ha.corrb;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        v0 += __shfl_xor(v0, m, 64); v1 += __shfl_xor(v1, m, 64);
        v2 += __shfl_xor(v2, m, 64); v3 += __shfl_xor(v3, m, 64);
    }
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    if (lane_id() == 0) *reinterpret_cast<float4 *>(s_mem + 4 * wave) = make_float4(v0, v1, v2, v3);
    __syncthreads();
    if (threadIdx.x == 0) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int w = 0; w < nwaves; ++w) {
            const float4 q = *reinterpret_cast<const float4 *>(s_mem + 4 * w);
            t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w;
        }
        *reinterpret_cast<float4 *>(a.head_part + 4 * (size_t)entry) = t;
    }
}

template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_agg_head_rows(const FwdArgs a)
{
    __shared__ __align__(16) float s_mem[4 * WAVES];
    const int nw = gridDim.x * WAVES;
    const HeadAcc ha = head_rows_role<VEC, G, R>(a, blockIdx.x * WAVES + (threadIdx.x >> 6), nw);
    head_block_entry(a, blockIdx.x, ha, s_mem);
}

}  // namespace sngnn

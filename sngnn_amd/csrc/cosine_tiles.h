// The tile engine of the fused cosine scans (gfx950): raw products X_rows X_cols^T of one workgroup's
// row block against one column tile after another, on the matrix cores at fp32 rounding, never stored.
// Three consumers: knn_scan.h ranks the values of a tile (k_knn_mfma), cosine_hist_scan.h counts them
// (k_cosine_hist), cosine_thresh_scan.h keeps the ones that reach a threshold (k_cosine_thresh); knn.hip /
// cosine_hist.hip / cosine_thresh.hip launch them on fp32 tables, knn_half.hip / cosine_hist_half.hip /
// cosine_thresh_half.hip on fp16 / bf16 tables.  The consumer owns the tile loop, the accumulators and the
// epilogue; the engine owns the rows' register operands, the panels in flight and the staging + MFMA loops of
// one tile.
// The rows may come from a table of their own (sngnn_knn_query: load_rows takes it, products<true> is told of it).
//
// FH > 0 (F == 2 FH, FH a multiple of 16, F <= 128): the wave's 32 rows never change, so their
// MFMA operands stay in REGISTERS for the whole scan - the k order of a contraction is free,
// lane (row, half h) keeps the contiguous half k in [h FH, (h + 1) FH) of its row - and only
// the column panel streams through LDS (half the staging, 4 LDS reads per 4 MFMAs).
// FH == 0: any F, both panels through LDS.
// BF3 (with FH > 0; default): the products on the bf16 matrix cores (device_utils.h: exact
// three-way split of both operands, eight partial products, fp32 accumulation) - the rows'
// operands are split once, into registers; the column panel is split when it is staged (three
// bf16 planes, rows of 64 + 16 bytes); a step of 16 k-slots per half is 2 x 8
// `v_mfma_f32_32x32x16_bf16` per column block instead of 16 fp32 MFMAs.
// NWV waves per workgroup (32 rows each), CB column blocks of 32 per tile.  <4, 4>: 128 x 128 tiles, one wave per
// SIMD (64 accumulator registers).  <8, 2> (round 5, F = 128): 256 rows x 64-column tiles - 32 accumulator registers,
// the kernel fits the 256-register budget of TWO waves per SIMD, so one wave's epilogue, staging and barrier waits
// run under the other's products (at one wave per SIMD nothing overlapped them: products ~24-35 ms, everything else
// ~45 of the 76 ms at arxiv size).
//
// Result layout (C/D of a 32 x 32 block): acc[b][r] of lane l is column 32 b + (l & 31), row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the wave's 32 rows.
#pragma once
#include <type_traits>

#include "device_utils.h"

namespace sngnn {

using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int KN_M = 128, KN_K = 32, KN_LD = KN_K + 4, KN_LOADS = KN_M * KN_K / 256;   // (stride 36: 16-byte rows, conflict-free b128 reads)
typedef float knn_f4 __attribute__((ext_vector_type(4)));
constexpr int KN_PS = 80;                      // bytes per row of a bf16 plane of the column panel

// PL = the bf16 planes a stored value has, i.e. the table's storage type: 3 = fp32 (the forms above), 2 = fp16
// (11 significant bits: plane 3 of the widened value is +0.0), 1 = bf16 (the stored 16 bits ARE plane 1).  PL < 3
// exists for the <8, 2> register-operand shape only.  The table is `const XT *`, 2 F bytes a row; the planes that
// are kept are the bits the fp32 form computes from the widened table, the products that are issued are the fp32
// form's products of those planes in its order, and the planes and products that are left out are the ones whose
// operands are all +0.0 there (the contract this rests on).
template <int FH, bool BF3, int NWV = 4, int CB = 4, int PL = 3>
struct CosineTiles {
    static_assert(!BF3 || FH > 0, "the bf16 form is the register-operand path's");
    static_assert((NWV == 4 && CB == 4) || (BF3 && FH > 0), "other tile shapes: the bf16 register-operand path only");
    static_assert((4 * CB) % NWV == 0 && 4 * CB / NWV >= 1 && 4 * CB / NWV <= 4, "staging: 1..4 vectors per thread and step");
    static_assert(PL == 3 || ((PL == 1 || PL == 2) && BF3 && FH > 0 && NWV == 8 && CB == 2), "half tables: the <8, 2> register-operand shape only");
    static constexpr int KR = 32 * NWV, KC = 32 * CB;                  // rows per workgroup, columns per tile
    using XT = std::conditional_t<PL == 3, float, unsigned short>;     // one stored value
    // floats of the two LDS panels the consumer declares (__shared__, sB aligned to 16 bytes)
    static constexpr int SA_FLOATS = FH > 0 ? 1 : KN_M * KN_LD;
    static constexpr int SB_FLOATS = (FH > 0 ? 2 : 1) * (BF3 ? PL * KC * KN_PS / 4 : KC * KN_LD);   // FH > 0: two buffers

    float areg[(FH > 0 && !BF3) ? FH : 1];
    sn_u32x4 ap1[BF3 ? FH / 8 : 1], ap2[BF3 && PL >= 2 ? FH / 8 : 1], ap3[BF3 && PL == 3 ? FH / 8 : 1];     // the rows' bf16 planes
    knn_f4 rb0, rb1, rb2, rb3;                                                       // the column panel in flight (FH > 0)
    sn_u32x4 rh;                                                                     // ... of a half table: 8 k-slots as stored

    // 8 stored fp16 values -> planes 1 and 2 of their (exact) fp32 values
    static __device__ __forceinline__ void split_f16x8(const sn_u32x4 &h, sn_u32x4 &p1, sn_u32x4 &p2)
    {
        float av[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            av[2 * i] = Half16<__half>::widen((unsigned short)(h[i] & 0xFFFFu));
            av[2 * i + 1] = Half16<__half>::widen((unsigned short)(h[i] >> 16));
        }
        sn_u32x4 p3;                                                      // +0.0 in every slot: not kept
        split_bf16x8(av, p1, p2, p3);
    }

    // once per workgroup, before the first tile: the wave's rows into registers (FH > 0)
    __device__ __forceinline__ void load_rows(const XT *__restrict__ x, int64_t N, int64_t F, int64_t row0)
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int half = lane >> 5, l32 = lane & 31;
        if constexpr (FH > 0) {
            const int64_t ar = min(row0 + wave * 32 + l32, N - 1);          // (rows >= N are never used)
            if constexpr (PL < 3) {
#pragma unroll
                for (int q = 0; q < FH / 8; ++q) {
                    const sn_u32x4 h = *reinterpret_cast<const sn_u32x4 *>(x + ar * F + half * FH + 8 * q);
                    if constexpr (PL == 1) ap1[q] = h;
                    else split_f16x8(h, ap1[q], ap2[q]);
                }
            } else if constexpr (!BF3) {
#pragma unroll
                for (int q = 0; q < FH / 4; ++q) {
                    const float4 v = *reinterpret_cast<const float4 *>(x + ar * F + half * FH + 4 * q);
                    areg[4 * q] = v.x; areg[4 * q + 1] = v.y; areg[4 * q + 2] = v.z; areg[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < FH / 8; ++q) {
                    const float4 v0 = *reinterpret_cast<const float4 *>(x + ar * F + half * FH + 8 * q);
                    const float4 v1 = *reinterpret_cast<const float4 *>(x + ar * F + half * FH + 8 * q + 4);
                    const float av[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                    split_bf16x8(av, ap1[q], ap2[q], ap3[q]);
                }
            }
        }
        const knn_f4 z = {0.f, 0.f, 0.f, 0.f};
        rb0 = z; rb1 = z; rb2 = z; rb3 = z;
        const sn_u32x4 zh = {0u, 0u, 0u, 0u};
        rh = zh;
    }

    // acc += the products of rows [row0, row0 + KR) with columns [ct KC, (ct + 1) KC).  The consumer calls
    // it for ct = ct_begin, ct_begin + 1, ... ct_end - 1 in this order (FH > 0: the panels of the next
    // steps are fetched and staged ahead, across tile boundaries), every thread of the workgroup.
    // TWO (sngnn_knn_query): the rows are rows of a table of their own, xr [M, F] - the one load_rows was given -
    // and x [N, F] is the column table only (FH > 0 reads the rows in load_rows alone).  !TWO: one table, the
    // trailing arguments are not read.
    template <bool TWO = false>
    __device__ __forceinline__ void products(const XT *__restrict__ x, int64_t N, int64_t F, int64_t row0, int64_t ct,
                                             int64_t ct_begin, int64_t ct_end, float *sA, float *sB, f32x16 (&acc)[CB],
                                             const XT *__restrict__ xr = nullptr, int64_t M = 0)
    {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int half = lane >> 5, l32 = lane & 31;
        const int sc = tid & 31, sr = tid >> 5;
        const int64_t col0 = ct * KC;
        if constexpr (FH > 0) {
            // k-step = 16 steps of each half: columns [s0, s0 + 16) and [FH + s0, FH + s0 + 16) of
            // the column block's rows, as 16-byte vectors: thread t owns vector (t & 7) - four
            // of each half - of rows (t >> 3) + 32 u.  The panel of the NEXT step travels while
            // this one is multiplied, and the first panel of the NEXT TILE while this tile's
            // cosines go through the consumer's epilogue.  (Named registers: see toolbox.hip,
            // k_cosine_mfma - a private array that lives across the tile loop's back edge goes
            // to scratch memory and its loads are waited for at once.)
            // Round 5: the column panel is DOUBLE-BUFFERED - step L's products read buffer L & 1 while the
            // panel of step L + 1 (requested a step earlier, split here) is written into the other one and the
            // panel of step L + 2 is requested: ONE workgroup barrier per step instead of two, and the staging's
            // vector work (the bf16 split: ~100 instructions per step and thread) sits in the same block as the
            // step's 64 matrix instructions, where the wave issues it beside them (one wave per SIMD: nobody
            // else would).  The steps run on across tile boundaries (the next tile's first panel is staged
            // under this tile's last products and waits in LDS during the epilogue).
            // Staging map: 16 consecutive lanes write rows r and r + 4 (not r and r + 1): with the 80-byte
            // plane rows their 8-byte stores cover all 32 banks once - adjacent rows overlapped in four
            // (SQ_LDS_BANK_CONFLICT 777 M cycles at arxiv size, 1.24 per LDS instruction, all from these stores).
            // A half table (PL < 3): a step's panel is KC rows of 4 vectors of 8 k-slots (two of each half) - 256
            // vectors, one for each thread of the first four waves; the others stage nothing.  Thread t owns vector
            // (t & 3) of row slot (t >> 2), the same row permutation: 8 consecutive lanes write rows r and r + 4, 16
            // bytes each, and cover the 32 banks once.
            const int seg = PL < 3 ? tid & 3 : tid & 7, slot = PL < 3 ? tid >> 2 : tid >> 3;
            const int pr = (slot & ~7) | ((slot & 7) >> 1) | ((slot & 1) << 2);
            const int kseg = PL < 3 ? (seg < 2 ? 8 * seg : FH + 8 * (seg - 2)) : (seg < 4 ? 4 * seg : FH + 4 * (seg - 4));
            const bool stager = PL == 3 || slot < KC;                     // (wave-uniform)
            constexpr int NS = FH / 16;                                   // steps per tile
            constexpr int PANEL = BF3 ? PL * KC * KN_PS : KC * KN_LD * 4;    // bytes of one buffer
            constexpr int SROWS = 8 * NWV, UV = KC / SROWS;               // rows staged per vector slot, vectors per thread
#define SN_KNN_FETCH(COL0, S0)                                                                            \
            if constexpr (PL < 3) {                                                                       \
                if (stager) rh = *(const sn_u32x4 *)(x + (S0) + kseg + min((COL0) + pr, N - 1) * F);      \
            } else {                                                                                      \
                const XT *g_ = x + (S0) + kseg;                                                           \
                rb0 = *(const knn_f4 *)(g_ + min((COL0) + pr, N - 1) * F);                                \
                if constexpr (UV > 1) rb1 = *(const knn_f4 *)(g_ + min((COL0) + pr + SROWS, N - 1) * F);  \
                if constexpr (UV > 2) rb2 = *(const knn_f4 *)(g_ + min((COL0) + pr + 2 * SROWS, N - 1) * F); \
                if constexpr (UV > 3) rb3 = *(const knn_f4 *)(g_ + min((COL0) + pr + 3 * SROWS, N - 1) * F); \
            }
            unsigned char *sBb = reinterpret_cast<unsigned char *>(sB);
            // BF3: plane p of column row r at byte (p * KN_M + r) * KN_PS; its 32 k-slots are the
            // step's 16 of half 0 followed by the 16 of half 1 (seg 0..3 | 4..7, 8 bytes each)
            auto stage = [&](int boff) {
                if constexpr (PL < 3) {
                    // the vector's 8 k-slots are 16 bytes of the plane row as they stand (bf16), or widened and split
                    if (stager) {
                        unsigned char *wbh = sBb + boff + pr * KN_PS + 16 * seg;
                        if constexpr (PL == 1) *(sn_u32x4 *)(wbh) = rh;
                        else {
                            sn_u32x4 p1, p2;
                            split_f16x8(rh, p1, p2);
                            *(sn_u32x4 *)(wbh) = p1;
                            *(sn_u32x4 *)(wbh + KC * KN_PS) = p2;
                        }
                    }
                } else if constexpr (!BF3) {
                    float *wb = reinterpret_cast<float *>(sBb + boff) + pr * KN_LD + 4 * seg;
                    *(knn_f4 *)(wb) = rb0;
                    if constexpr (UV > 1) *(knn_f4 *)(wb + SROWS * KN_LD) = rb1;
                    if constexpr (UV > 2) *(knn_f4 *)(wb + 2 * SROWS * KN_LD) = rb2;
                    if constexpr (UV > 3) *(knn_f4 *)(wb + 3 * SROWS * KN_LD) = rb3;
                } else {
                    unsigned char *wb3 = sBb + boff + pr * KN_PS + 8 * seg;
                    auto put = [&](int u, const knn_f4 &v) {
                        const float vv[4] = {v[0], v[1], v[2], v[3]};
                        sn_u32x2 p1, p2, p3;
                        split_bf16x4(vv, p1, p2, p3);
                        unsigned char *d_ = wb3 + SROWS * u * KN_PS;
                        *(sn_u32x2 *)(d_) = p1;
                        *(sn_u32x2 *)(d_ + KC * KN_PS) = p2;
                        *(sn_u32x2 *)(d_ + 2 * KC * KN_PS) = p3;
                    };
                    put(0, rb0);
                    if constexpr (UV > 1) put(1, rb1);
                    if constexpr (UV > 2) put(2, rb2);
                    if constexpr (UV > 3) put(3, rb3);
                }
            };
            // linear step L = (ct - ct_begin) NS + s0 / 16 lives in buffer L & 1
            auto fetch_step = [&](int64_t L) {
                const int64_t t_ = ct_begin + L / NS;
                const int st_ = (int)(L % NS) * 16;
                if (t_ < ct_end) { SN_KNN_FETCH(t_ * KC, st_) }
            };
            if (ct == ct_begin) {
                fetch_step(0);
                stage(0);
                fetch_step(1);
                __syncthreads();
            }
            const int64_t L0 = (ct - ct_begin) * NS;
#pragma unroll
            for (int s0 = 0; s0 < FH; s0 += 16) {
                const int64_t L = L0 + s0 / 16;
                const int cur = (int)(L & 1) * PANEL;
                if (s0 + 16 < FH || ct + 1 < ct_end) stage(cur ^ PANEL);      // step L + 1's panel (in the registers)
                fetch_step(L + 2);
                const float *pb = reinterpret_cast<const float *>(sBb + cur) + l32 * KN_LD + half * 16;
                const unsigned char *pb3 = sBb + cur + l32 * KN_PS + 32 * half;
                if constexpr (BF3) {
#pragma unroll
                    for (int g = 0; g < 2; ++g) {          // 8 k-slots of each half per MFMA
                        const int aq = s0 / 8 + g;
#pragma unroll
                        for (int b = 0; b < CB; ++b) {
                            const unsigned char *r_ = pb3 + 32 * b * KN_PS + 16 * g;
                            const sn_u32x4 b1 = *(const sn_u32x4 *)(r_);
                            const sn_u32x4 b2 = *(const sn_u32x4 *)(r_ + (PL >= 2 ? KC * KN_PS : 0));          // (PL planes exist)
                            const sn_u32x4 b3 = *(const sn_u32x4 *)(r_ + (PL == 3 ? 2 * KC * KN_PS : 0));
#if defined(SNGNN_KNN_EXP) && SNGNN_KNN_EXP == 2        // timing experiment: one product of eight
#define SN_KNN_M3(PA, PB) asm volatile("" ::"v"(PA), "v"(PB));
                            acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(sn_bf16x8, ap1[aq]),
                                                                             __builtin_bit_cast(sn_bf16x8, b1), acc[b], 0, 0, 0);
#else
#define SN_KNN_M3(PA, PB)                                                                                   \
                            acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(sn_bf16x8, PA), \
                                                                             __builtin_bit_cast(sn_bf16x8, PB), acc[b], 0, 0, 0);
#endif
                            // (row plane, column plane): (3,2)(2,3)(3,1)(2,2)(1,3)(2,1)(1,2)(1,1) - of these, the ones
                            // whose planes the table has, in this order
                            if constexpr (PL == 3) {
                            SN_KNN_M3(ap3[aq], b2) SN_KNN_M3(ap2[aq], b3) SN_KNN_M3(ap3[aq], b1) SN_KNN_M3(ap2[aq], b2)
                            SN_KNN_M3(ap1[aq], b3) SN_KNN_M3(ap2[aq], b1) SN_KNN_M3(ap1[aq], b2) SN_KNN_M3(ap1[aq], b1)
                            } else if constexpr (PL == 2) {
                            SN_KNN_M3(ap2[aq], b2) SN_KNN_M3(ap2[aq], b1) SN_KNN_M3(ap1[aq], b2) SN_KNN_M3(ap1[aq], b1)
                            } else {
                            SN_KNN_M3(ap1[aq], b1)
                            }
#undef SN_KNN_M3
                        }
                    }
                } else
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const knn_f4 b0 = *(const knn_f4 *)(pb + 4 * q), b1 = *(const knn_f4 *)(pb + 32 * KN_LD + 4 * q);
                    const knn_f4 b2 = *(const knn_f4 *)(pb + 64 * KN_LD + 4 * q), b3 = *(const knn_f4 *)(pb + 96 * KN_LD + 4 * q);
#define SN_KNN_MFMA(E, SS)                                                                                \
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[s0 + 4 * q + SS], b0.E, acc[0], 0, 0, 0);  \
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[s0 + 4 * q + SS], b1.E, acc[1], 0, 0, 0);  \
                    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[s0 + 4 * q + SS], b2.E, acc[2], 0, 0, 0);  \
                    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[s0 + 4 * q + SS], b3.E, acc[3], 0, 0, 0);
                    SN_KNN_MFMA(x, 0) SN_KNN_MFMA(y, 1) SN_KNN_MFMA(z, 2) SN_KNN_MFMA(w, 3)
#undef SN_KNN_MFMA
                }
                __syncthreads();       // step L's reads are done, step L + 1's panel is complete
            }
#undef SN_KNN_FETCH
        } else {
        float ra[KN_LOADS], rb[KN_LOADS];
        auto fetch = [&](int64_t k0) {
            const int64_t kk = k0 + sc;
#pragma unroll
            for (int u = 0; u < KN_LOADS; ++u) {
                const int64_t r_a = row0 + sr + 8 * u, r_b = col0 + sr + 8 * u;
                if constexpr (TWO) ra[u] = (r_a < M && kk < F) ? xr[r_a * F + kk] : 0.f;
                else ra[u] = (r_a < N && kk < F) ? x[r_a * F + kk] : 0.f;
                rb[u] = (r_b < N && kk < F) ? x[r_b * F + kk] : 0.f;
            }
        };
        fetch(0);
        for (int64_t k0 = 0; k0 < F; k0 += KN_K) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < KN_LOADS; ++u) {
                sA[(sr + 8 * u) * KN_LD + sc] = ra[u];
                sB[(sr + 8 * u) * KN_LD + sc] = rb[u];
            }
            __syncthreads();
            if (k0 + KN_K < F) fetch(k0 + KN_K);
#pragma unroll
            for (int kk = 0; kk < KN_K; kk += 2) {
                // 32x32x2: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
                const float a = sA[(wave * 32 + l32) * KN_LD + kk + half];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float bv = sB[(b * 32 + l32) * KN_LD + kk + half];
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[b], 0, 0, 0);
                }
            }
        }
        }   // FH == 0
    }
};

// inv[i] = 1 / max(||x_i||, eps): one wave per row (F.normalize's clamp - a zero row's cosines are exactly 0)
// (static: one copy per translation unit that launches it)
static __global__ __launch_bounds__(256) void k_knn_inv_norm(const float *__restrict__ x, int64_t N, int64_t F,
                                                             float *__restrict__ inv)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float *p = x + row * F;
    float ss = 0.f;
    for (int64_t c = lane; c < F; c += 64) ss = fmaf(p[c], p[c], ss);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    if (lane == 0) inv[row] = 1.0f / fmaxf(sqrtf(ss), EPS_NORM);
}

// the same of a half table (S = __half or __hip_bfloat16): every value widened, then the lane striding, the fmaf
// chain and the shuffle tree above - the bits of k_knn_inv_norm on the widened table
template <typename S>
static __global__ __launch_bounds__(256) void k_knn_inv_norm_half(const unsigned short *__restrict__ x, int64_t N, int64_t F,
                                                                  float *__restrict__ inv)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const unsigned short *p = x + row * F;
    float ss = 0.f;
    for (int64_t c = lane; c < F; c += 64) {
        const float v = Half16<S>::widen(p[c]);
        ss = fmaf(v, v, ss);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    if (lane == 0) inv[row] = 1.0f / fmaxf(sqrtf(ss), EPS_NORM);
}

}  // namespace sngnn

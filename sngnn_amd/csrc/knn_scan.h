// kNN similarity-graph builder (gfx950): for every node the k most cosine-similar
// nodes, straight from the feature table - the N x N similarity is never stored.
// the producer of edges for the aggregation kernel (the
// "Node-Similarity build" of the north star; the reference only ever materialises S,
// SimGFAToolbox/dense.py:138-141, and has no graph builder).
//
// Workgroup = 4 waves = 128 rows; it walks ALL column tiles of 128 nodes.  A tile
// S[128 x 128] = diag(inv) X_rows X_cols^T diag(inv) comes from the matrix cores at fp32 rounding
// (exact bf16 split or v_mfma_f32_32x32x2_f32) like sngnn_cosine_dense; each WAVE owns 32 whole rows of it
// (1 x 4 blocks of 32 x 32), so a row's 128 new similarities sit in one half-wave and
// its running top-k list (LDS, k 64-bit keys) is private to the wave: no atomics, no
// workgroup barrier in the selection.  A similarity only enters the selection when it
// beats the row's current k-th key (one ballot per accumulator register); after the
// first few tiles that is rare (~k ln(N/k) times per row in total), so the epilogue
// costs a fraction of the MFMA time.
//
// Order: (cosine descending, node id ascending) - the aggregation's tie rule; a node is
// never its own neighbour when exclude_self is set.
//
// This header holds the kernels; knn.hip launches them on fp32 tables (sngnn_knn_graph, sngnn_knn_query) and
// knn_half.hip on fp16 / bf16 tables (sngnn_knn_graph_half, sngnn_knn_query_half: the engine's PL < 3).
#pragma once
#include <algorithm>

#include "cosine_tiles.h"

namespace sngnn {

constexpr int KNN_MAX_K = 32;
#if defined(SNGNN_KNN_EXP) && SNGNN_KNN_EXP == 4            // measurement build: event counters of the selection
static __device__ unsigned long long g_knn_dbg[8];          // (one per translation unit: knn.hip reads its own)
#define SN_KNN_COUNT(i, v) do { if (lane_id() == 0) atomicAdd(&g_knn_dbg[i], (unsigned long long)(v)); } while (0)
#else
#define SN_KNN_COUNT(i, v) do { } while (0)
#endif

// k-th largest of the (unique, non-zero) keys held two per lane; at least k keys are set
__device__ __forceinline__ unsigned long long kth_largest(unsigned long long key0, unsigned long long key1, int k)
{
    unsigned long long T = 0;
    for (int b = 63; b >= 0; --b) {
        const unsigned long long cand = T | (1ull << b);
        const int c = __popcll(__ballot(key0 >= cand)) + __popcll(__ballot(key1 >= cand));
        if (c >= k) T = cand;
    }
    return T;
}

// smallest of the wave's 64-bit values (all lanes get it)
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, m, 64), hi = __shfl_xor((unsigned)(v >> 32), m, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// Merge the row's list (k slots, 0 = empty) with cnt candidates (cnt + k <= 128); returns
// the row's new threshold key (k-th largest, or 0 while the list is not full).
// Round 5: the k largest by the aggregation's early-exit search (wave_topk_keys_n: it walks the cosine word
// and stops at the first prefix that separates exactly k keys - ~15 ballot steps for unrelated cosines) instead
// of a 64-step search for the k-th key; the threshold is then the smallest kept key.  A scan at arxiv size
// makes 1.65 M merges (9.7 per row), and a merge in one wave holds the workgroup's other three at the step's
// barrier.
__device__ __forceinline__ unsigned long long merge_row(unsigned long long *list, const unsigned long long *cand,
                                                        int cnt, int k)
{
    const int lane = lane_id();
    const int q0 = lane, q1 = lane + 64;
    auto pick = [&](int q) -> unsigned long long {
        return q < k ? list[q] : (q - k < cnt ? cand[q - k] : 0ull);
    };
    const unsigned long long key[2] = {pick(q0), pick(q1)};
    const int total = __popcll(__ballot(key[0] != 0ull)) + __popcll(__ballot(key[1] != 0ull));
    bool kept[2];
    wave_topk_keys_n<2>(key, k, 31, kept);               // (low word = ~node id: 31 bits can differ)
    const unsigned long long m0 = __ballot(kept[0]), m1 = __ballot(kept[1]);
    const int n0 = __popcll(m0), ns = n0 + __popcll(m1);
    unsigned long long T = 0ull;
    if (total >= k) T = wave_min_u64(min(kept[0] ? key[0] : ~0ull, kept[1] ? key[1] : ~0ull));
    wave_lds_sync();                       // every lane has read the old list
    if (kept[0]) list[prefix_popc(m0)] = key[0];
    if (kept[1]) list[n0 + prefix_popc(m1)] = key[1];
    if (lane >= ns && lane < k) list[lane] = 0ull;
    wave_lds_sync();
    return T;
}

// blockIdx.y = column split: this workgroup covers column tiles [y * tiles_per_split, ...) and
// writes its lists as KEYS to part[y][rows][k] (nsplit > 1) or the final idx / sim (nsplit == 1).
//
// The products of a tile come from the engine in cosine_tiles.h (FH, BF3, NWV, CB: see there); this kernel owns
// the tile loop and the selection.
//
// Two tables (RECT, sngnn_knn_query): the workgroup's rows are rows of rows.xq [M, F] with inverse norms rows.invq,
// the column tiles walk x [N, F] with inv, column rows.self_offset + i is no neighbour of row i (-1: every column is
// eligible; exclude_self is not read) and the lists are M rows.  One table (!RECT, sngnn_knn_graph): `rows` is
// empty, the rows are x's, and the instantiation is the kernel it was before the second table existed.
template <bool RECT>
struct KnnRows { const void *xq; int64_t M; const float *invq; int64_t self_offset; };       // (xq: a table of the scan's storage type)
template <>
struct KnnRows<false> {};

template <int FH, bool BF3, int NWV = 4, int CB = 4, bool RECT = false, int PL = 3>
__global__ __launch_bounds__(64 * NWV) void k_knn_mfma(const typename CosineTiles<FH, BF3, NWV, CB, PL>::XT *__restrict__ x, int64_t N, int64_t F,
                                                  const float *__restrict__ inv, int k, int exclude_self,
                                                  int tiles_per_split, unsigned long long *__restrict__ part,
                                                  int32_t *__restrict__ out_idx, float *__restrict__ out_sim,
                                                  KnnRows<RECT> rows = {})
{
    using Eng = CosineTiles<FH, BF3, NWV, CB, PL>;
    const typename Eng::XT *xq = x;
    const float *invq = inv;
    int64_t M = N, self = -1;
    if constexpr (RECT) { xq = static_cast<const typename Eng::XT *>(rows.xq); M = rows.M; invq = rows.invq; self = rows.self_offset; }
    constexpr int KC = Eng::KC, KR = Eng::KR;                  // columns per tile, rows per workgroup
    __shared__ float sA[Eng::SA_FLOATS];
    __shared__ __align__(16) float sB[Eng::SB_FLOATS];
    __shared__ unsigned long long s_list[NWV][32][KNN_MAX_K];   // running top-k keys per row
    __shared__ unsigned long long s_thr[NWV][32];               // k-th key per row (0: list not full)
    __shared__ float s_thrf[NWV][32];                           // its cosine (-inf: list not full)
    __shared__ float s_ts[NWV][32];                             // the fast reject's threshold on acc * icol (see the selection)
    __shared__ float s_irow[NWV][32];                           // the rows' inverse norms (a hot register reads LDS, not memory)
    __shared__ int s_pend[NWV][32];                             // candidates parked in list[k .. KNN_MAX_K)
    __shared__ unsigned long long s_cand[NWV][2][128];          // candidates of the two rows of a register
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * KR;
    for (int q = lane; q < 32 * KNN_MAX_K; q += 64) s_list[wave][q / KNN_MAX_K][q % KNN_MAX_K] = 0ull;
    if (lane < 32) {
        s_thr[wave][lane] = 0ull; s_thrf[wave][lane] = -INFINITY; s_pend[wave][lane] = 0;
        s_ts[wave][lane] = (row0 + wave * 32 + lane < M) ? -INFINITY : INFINITY;      // (rows beyond M: never a candidate)
        s_irow[wave][lane] = (row0 + wave * 32 + lane < M) ? invq[row0 + wave * 32 + lane] : 0.f;
    }
    const int cap = KNN_MAX_K - k;                               // spare slots behind a row's list
    const int64_t ncol_tiles = (N + KC - 1) / KC;
    const int64_t ct_begin = (int64_t)blockIdx.y * tiles_per_split;
    const int64_t ct_end = min(ncol_tiles, ct_begin + tiles_per_split);

    Eng eng;
    eng.load_rows(xq, M, F, row0);

    for (int64_t ct = ct_begin; ct < ct_end; ++ct) {
        const int64_t col0 = ct * KC;
        f32x16 acc[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        // the tile's column ids and inverse norms (for the selection): requested here, they travel under the products
        float icol[CB];
        int64_t jcol[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b) {
            jcol[b] = col0 + b * 32 + l32;
            icol[b] = inv[min(jcol[b], N - 1)];
        }
#pragma unroll
        for (int b = 0; b < CB; ++b) icol[b] = jcol[b] < N ? icol[b] : 0.f;
        eng.template products<RECT>(x, N, F, row0, ct, ct_begin, ct_end, sA, sB, acc, xq, M);
#if defined(SNGNN_KNN_EXP) && SNGNN_KNN_EXP == 1        // timing experiment: no selection at all
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" ::"v"(acc[b][r]));
        continue;
#endif
        // ---- selection: C/D layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        // Round 5: the fast reject of ALL sixteen registers first, from thresholds fetched together.  Register r
        // holds two rows of the wave's 32 (one per half-wave), each row sits in exactly one register, so the
        // sixteen thresholds of a tile can be read up front: one LDS round trip instead of sixteen serial ones,
        // and no read of the rows' inverse norms at all - s_ts[row] is the row's k-th cosine DIVIDED by its
        // inverse norm, lowered by a relative 1e-6 (a superset test: `acc * icol >= ts` holds whenever the exact
        // `acc * (irow * icol) >= thrf` below does; the exact rule still decides).  Before, every register cost a
        // dependent LDS read and a global read of inv[i]: the selection was 34 of the kernel's 88 ms at arxiv
        // size (a build without any selection: 54 ms), 26 of 80 now.  What is left are the ~3.6 registers per tile
        // and wave that do hold a candidate (k ln(N / k) insertions per row over the scan) and their LDS round
        // trips, which nothing hides at one wave per SIMD.  Measured and dropped: the candidates appended by their
        // lanes to a wave-private LDS queue (LDS atomic) and worked off one by one - 85.6 ms against 80.0 (64
        // divergent tests per tile cost more than 16 ballots; an entry still costs three dependent LDS reads).
        float tsr[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) tsr[r] = s_ts[wave][(r & 3) + 8 * (r >> 2) + 4 * half];
        unsigned hot16 = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            bool m_ = false;
#pragma unroll
            for (int b = 0; b < CB; ++b) m_ |= acc[b][r] * icol[b] >= tsr[r];
            if (__ballot(m_) != 0ull) hot16 |= 1u << r;
        }
        SN_KNN_COUNT(0, 1);                                             // tiles x waves
        SN_KNN_COUNT(1, __popc(hot16));                                 // registers that pass the superset test
        // ONE copy of the hot path's code, looped over the set bits: unrolled per register it was sixteen copies of
        // ~700 instructions each (the merges inlined) - far more than the instruction cache holds, and the ~2 hot
        // registers of a tile jump to different copies every time.  Only the four accumulator values are fetched
        // per register (a switch of sixteen four-move cases: accumulator indices must be literals).
        unsigned hm_ = hot16;
#if defined(SNGNN_KNN_EXP) && SNGNN_KNN_EXP == 5        // timing experiment: the fast test of every register, no hot path
        asm volatile("" ::"s"(hm_));
        hm_ = 0u;
#endif
        while (hm_ != 0u) {
            const int r = __builtin_ctz(hm_);                            // (wave-uniform)
            hm_ &= hm_ - 1u;
            float ar[CB];
            switch (r) {
#define SN_KNN_PICK(R) case R: _Pragma("unroll") for (int b_ = 0; b_ < CB; ++b_) ar[b_] = acc[b_][R]; break;
            SN_KNN_PICK(0) SN_KNN_PICK(1) SN_KNN_PICK(2) SN_KNN_PICK(3) SN_KNN_PICK(4) SN_KNN_PICK(5) SN_KNN_PICK(6) SN_KNN_PICK(7)
            SN_KNN_PICK(8) SN_KNN_PICK(9) SN_KNN_PICK(10) SN_KNN_PICK(11) SN_KNN_PICK(12) SN_KNN_PICK(13) SN_KNN_PICK(14)
            default: _Pragma("unroll") for (int b_ = 0; b_ < CB; ++b_) ar[b_] = acc[b_][15]; break;
#undef SN_KNN_PICK
            }
            const int lr = (r & 3) + 8 * (r >> 2) + 4 * half;          // this lane's row within the wave's 32
            const int64_t i = row0 + wave * 32 + lr;
            const float irow = s_irow[wave][lr];
            // fast reject on the cosine alone: nothing of this register reaches its row's
            // k-th value - the common case once the lists have warmed up
            const float thrf = s_thrf[wave][lr];
            float sv[CB];
            bool maybe = false;
#pragma unroll
            for (int b = 0; b < CB; ++b) {
                sv[b] = ar[b] * (irow * icol[b]) + 0.0f;
                maybe |= sv[b] >= thrf;
            }
            if (__ballot(maybe) == 0ull) continue;
            const unsigned long long thr = s_thr[wave][lr];
            unsigned long long key[CB];
            bool any = false;
#pragma unroll
            for (int b = 0; b < CB; ++b) {
                const bool ok = i < M && jcol[b] < N &&
                                !(RECT ? (self >= 0 && jcol[b] == i + self) : (exclude_self && jcol[b] == i));
                key[b] = ok ? sel_key(sv[b], (unsigned)jcol[b]) : 0ull;
                if (key[b] <= thr) key[b] = 0ull;                        // cannot enter the list
                any |= key[b] != 0ull;
            }
            const unsigned long long hot = __ballot(any);
            if (hot == 0ull) continue;
            SN_KNN_COUNT(2, 1);                                         // registers with a real candidate
            // The common hot register after warm-up holds ONE candidate in the whole wave: its lane parks it behind
            // its row's list by itself - no ballots, no compaction through LDS, no per-half hand-off (a full
            // spare area falls through to the general path below, which merges).
            if (__popcll(hot) == 1) {
                int nk_ = 0;
                unsigned long long kor_ = 0ull;
#pragma unroll
                for (int b = 0; b < CB; ++b) { nk_ += key[b] != 0ull; kor_ |= key[b]; }
                if (__builtin_amdgcn_readlane(nk_, __ffsll((long long)hot) - 1) == 1) {
                    bool parked = false;
                    if (any) {
                        const int pc_ = s_pend[wave][lr];
                        if (pc_ < cap) {
                            s_list[wave][lr][k + pc_] = kor_;
                            s_pend[wave][lr] = pc_ + 1;
                            parked = true;
                        }
                    }
                    if (__ballot(parked) != 0ull) {
                        SN_KNN_COUNT(3, 1);                             // ... parked by their one lane
                        wave_lds_sync();
                        continue;
                    }
                }
            }
            // compact the candidates of the two rows (one per half-wave) into LDS
            int cnt = 0;                                                 // per half
#pragma unroll
            for (int b = 0; b < CB; ++b) {
                const unsigned long long m = __ballot(key[b] != 0ull);
                const unsigned mh = half ? (unsigned)(m >> 32) : (unsigned)m;
                if (key[b] != 0ull) s_cand[wave][half][cnt + __popc(mh & ((1u << l32) - 1u))] = key[b];
                cnt += __popc(mh);
            }
            wave_lds_sync();
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int c = __builtin_amdgcn_readlane(cnt, h * 32);
                if (c == 0) continue;
                const int rowh = (r & 3) + 8 * (r >> 2) + 4 * h;
                unsigned long long *cand = s_cand[wave][h];
                unsigned long long *list = s_list[wave][rowh];
                const int pc = s_pend[wave][rowh];
                if (pc + c <= cap) {
                    // park them behind the list: the merge waits until the spare slots are full
                    // (the row's threshold goes stale meanwhile - it only lets more through)
                    if (lane < c) list[k + pc + lane] = cand[lane];
                    if (lane == 0) s_pend[wave][rowh] = pc + c;
                    continue;
                }
                if (c + pc + k > 128) {
                    // too many for one merge (first tiles only): keep the best k candidates
                    const unsigned long long c0 = lane < c ? cand[lane] : 0ull, c1 = lane + 64 < c ? cand[lane + 64] : 0ull;
                    const unsigned long long T = kth_largest(c0, c1, k);
                    const bool k0 = c0 != 0ull && c0 >= T, k1 = c1 != 0ull && c1 >= T;
                    const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1);
                    wave_lds_sync();
                    if (k0) cand[prefix_popc(m0)] = c0;
                    if (k1) cand[__popcll(m0) + prefix_popc(m1)] = c1;
                    wave_lds_sync();
                    c = k;
                }
                if (lane < pc) cand[c + lane] = list[k + lane];        // the parked ones join
                wave_lds_sync();
                const unsigned long long T = merge_row(list, cand, c + pc, k);
                SN_KNN_COUNT(4, 1);                                     // merges
                if (lane == 0) {
                    s_pend[wave][rowh] = 0;
                    s_thr[wave][rowh] = T;
                    const unsigned u = (unsigned)(T >> 32);
                    const float tf = T ? __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u) : -INFINITY;
                    s_thrf[wave][rowh] = tf;
                    // (rows beyond M never get here: their lists take no key)
                    const float tq = tf / s_irow[wave][rowh];
                    s_ts[wave][rowh] = tq - (fabsf(tq) * 1e-6f + 1e-30f);
                }
            }
            wave_lds_sync();
        }
    }
    // parked candidates of every row
    wave_lds_sync();
    for (int lr = 0; lr < 32; ++lr) {
        const int pc = s_pend[wave][lr];
        if (pc == 0) continue;                                           // wave-uniform (LDS value)
        unsigned long long *cand = s_cand[wave][0];
        if (lane < pc) cand[lane] = s_list[wave][lr][k + lane];
        wave_lds_sync();
        merge_row(s_list[wave][lr], cand, pc, k);
    }
    // ---- output: the lists in rank order, or as keys for the merge of the column splits
    wave_lds_sync();
    for (int lr = 0; lr < 32; ++lr) {
        const int64_t i = row0 + wave * 32 + lr;
        if (i >= M) break;
        const unsigned long long *list = s_list[wave][lr];
        if (part != nullptr) {
            if (lane < k) part[((size_t)blockIdx.y * M + i) * k + lane] = list[lane];
            continue;
        }
        if (lane < k) {
            const unsigned long long kq = list[lane];
            int rk = 0, n = 0;
            for (int q = 0; q < k; ++q) {
                const unsigned long long o = list[q];
                rk += o > kq;
                n += o != 0ull;
            }
            if (kq != 0ull) {
                const unsigned u = (unsigned)(kq >> 32);
                out_idx[i * k + rk] = (int32_t)(0xFFFFFFFFu - (unsigned)kq);
                out_sim[i * k + rk] = __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
            }
            if (lane >= n) {               // fewer than k eligible nodes: pad
                out_idx[i * k + lane] = -1;
                out_sim[i * k + lane] = 0.f;
            }
        }
    }
}

// top-k of the column splits' lists of one row (nsplit * k keys, 128 at a time); N = the rows of the lists
// (static, as k_row_topk below: one copy per translation unit that launches it)
static __global__ __launch_bounds__(256) void k_knn_merge(const unsigned long long *__restrict__ part, int64_t N,
                                                   int k, int nsplit, int32_t *__restrict__ out_idx,
                                                   float *__restrict__ out_sim)
{
    __shared__ unsigned long long s_list[4][KNN_MAX_K];
    __shared__ unsigned long long s_cand[4][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= N) return;                                   // wave-uniform
    if (lane < KNN_MAX_K) s_list[wave][lane] = 0ull;
    wave_lds_sync();
    const int per = (128 - k) / k;                        // splits merged per round
    for (int s0 = 0; s0 < nsplit; s0 += per) {
        const int ns = min(per, nsplit - s0), cnt = ns * k;
        for (int q = lane; q < cnt; q += 64)
            s_cand[wave][q] = part[((size_t)(s0 + q / k) * N + i) * k + q % k];
        wave_lds_sync();
        merge_row(s_list[wave], s_cand[wave], cnt, k);    // (zero keys of short lists are ignored)
    }
    const unsigned long long *list = s_list[wave];
    if (lane < k) {
        const unsigned long long kq = list[lane];
        int rk = 0, n = 0;
        for (int q = 0; q < k; ++q) {
            const unsigned long long o = list[q];
            rk += o > kq;
            n += o != 0ull;
        }
        if (kq != 0ull) {
            const unsigned u = (unsigned)(kq >> 32);
            out_idx[i * k + rk] = (int32_t)(0xFFFFFFFFu - (unsigned)kq);
            out_sim[i * k + rk] = __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
        }
        if (lane >= n) {
            out_idx[i * k + lane] = -1;
            out_sim[i * k + lane] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// Small graphs: materialise + select.  When S fits comfortably (N <= KNN_DENSE_MAX_N) the dense cosine
// kernel (toolbox.hip: upper triangle on the matrix cores, mirrored) followed by this row selection
// beats the fused scan - whose both-panels-through-LDS path (wide features) pays eight barriers per
// tile and whose column splits (few row blocks) each warm their lists up from empty: Chameleon
// (2 277 x 2 325) and Actor (7 600 x 932) - BASELINE configs 2 and 3 - are this case.
// One wave per row of S: 256 entries per step (16 bytes per lane), an entry enters the selection
// only when its key beats the row's current k-th key; survivors are parked behind the list in
// LDS and merged when the buffer is full (the aggregation's early-exit k-th-key search).
// Same keys, same order and padding as the fused kernel.
// ---------------------------------------------------------------------------
constexpr int64_t KNN_DENSE_MAX_N = 32768;       // S = 4.3 GB at most (a stream-ordered allocation)

static __global__ __launch_bounds__(256) void k_row_topk(const float *__restrict__ S, int64_t N, int k, int exclude_self,
                                                  int lowbits, int32_t *__restrict__ out_idx,
                                                  float *__restrict__ out_sim)
{
    __shared__ unsigned long long s_key[4][128];          // [0, k): the list (0 = empty); [k, k + pend): parked
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= N) return;                                   // wave-uniform
    unsigned long long *keys = s_key[wave];
    keys[lane] = 0ull;
    keys[lane + 64] = 0ull;
    const int cap = 128 - k;
    int pend = 0;
    unsigned long long T = 0ull;                          // the list's k-th key (0: not full yet)
    auto merge = [&]() {
        wave_lds_sync();
        const unsigned long long key[2] = {keys[lane], keys[lane + 64]};
        bool kept[2];
        wave_topk_keys_n<2>(key, k, lowbits, kept);
        const unsigned long long m0 = __ballot(kept[0]), m1 = __ballot(kept[1]);
        const int n0 = __popcll(m0), ns = n0 + __popcll(m1);
        // the new threshold: the smallest kept key once the list is full
        unsigned long long mn = ~0ull;
        if (kept[0]) mn = key[0];
        if (kept[1] && key[1] < mn) mn = key[1];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = __shfl_xor(mn, m, 64);
            mn = o < mn ? o : mn;
        }
        wave_lds_sync();                                  // every lane has read the old contents
        keys[lane] = 0ull;
        keys[lane + 64] = 0ull;
        wave_lds_sync();
        if (kept[0]) keys[prefix_popc(m0)] = key[0];
        if (kept[1]) keys[n0 + prefix_popc(m1)] = key[1];
        wave_lds_sync();
        T = ns >= k ? mn : 0ull;
        pend = 0;
    };
    const float *row = S + i * N;
    const bool vec = (N % 4 == 0) && ((uintptr_t)S % 16 == 0);
    for (int64_t base = 0; base < N; base += 256) {
        const int64_t c0 = base + lane * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && c0 + 3 < N) {
            const float4 t = *reinterpret_cast<const float4 *>(row + c0);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (c0 + u < N) v[u] = row[c0 + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t c = c0 + u;
            const bool valid = c < N && !(exclude_self && c == i);
            const unsigned long long key = valid ? sel_key(v[u] + 0.0f, (unsigned)c) : 0ull;
            const bool pass = key > T;                    // (an invalid slot's key 0 never passes)
            unsigned long long m = __ballot(pass);
            if (m == 0ull) continue;                      // wave-uniform: the common case after the first steps
            if (pend + __popcll(m) > cap) merge();        // (at most 64 new ones, cap >= 96)
            const bool still = pass && key > T;           // the merge may have raised the threshold
            m = __ballot(still);
            if (still) keys[k + pend + prefix_popc(m)] = key;
            pend += __popcll(m);
        }
    }
    if (pend > 0) merge();
    wave_lds_sync();
    if (lane < k) {
        const unsigned long long kq = keys[lane];
        int rk = 0, n = 0;
        for (int q = 0; q < k; ++q) {
            const unsigned long long o = keys[q];
            rk += o > kq;
            n += o != 0ull;
        }
        if (kq != 0ull) {
            const unsigned u = (unsigned)(kq >> 32);
            out_idx[i * k + rk] = (int32_t)(0xFFFFFFFFu - (unsigned)kq);
            out_sim[i * k + rk] = __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
        }
        if (lane >= n) {               // fewer than k eligible nodes: pad
            out_idx[i * k + lane] = -1;
            out_sim[i * k + lane] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// Launch plans of the fused scan (host), shared by the fp32 and the half entries - one workspace size for both.
// ---------------------------------------------------------------------------
// column splits: enough workgroups to fill the chip when there are few row blocks
static int knn_splits(int64_t N, int rows_per_wg = KN_M)
{
    const int64_t nrb = (N + rows_per_wg - 1) / rows_per_wg;
    // (every split warms its lists up from empty: only as many as it takes to occupy the CUs)
    return (int)std::max<int64_t>(1, std::min<int64_t>(nrb, (320 + nrb - 1) / nrb));
}

// Two tables: the column splits are sized for occupancy from the base's tile count - few row blocks against many
// column tiles is the common case here, and a cap at the number of row blocks (knn_splits: the square scan never has
// more column tiles than 2 x row blocks) would leave one 128-row query block on one CU.
struct KnnQueryPlan { int64_t nrb, nct; int tps, ns; };
static KnnQueryPlan knn_query_plan(int64_t M, int64_t N, int rows_wg, int cols_tile)
{
    KnnQueryPlan p;
    p.nrb = (M + rows_wg - 1) / rows_wg;
    p.nct = (N + cols_tile - 1) / cols_tile;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(p.nct, (320 + p.nrb - 1) / std::max<int64_t>(p.nrb, 1)));
    p.tps = (int)((p.nct + want - 1) / std::max<int64_t>(want, 1));          // column tiles per split
    p.ns = p.tps > 0 ? (int)((p.nct + p.tps - 1) / p.tps) : 0;              // splits in use (<= want <= 320)
    return p;
}

}  // namespace sngnn

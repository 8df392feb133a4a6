// Structural cosine similarity of a sparse input at any N (gfx950): S = M_n^T M_n kept SPARSE, M_n the column-normalised
// [rows, cols] input of SimGFAToolbox/sparse.py:8-14 (coalesced, explicit zeros dropped) - the numeric half of the
// two-hop builder's scheme (h2gcn.hip), and a second consumer of the same rows that counts instead of storing.
//
// Row i of S.  S[i, j] = sum_k M_n[k, i] M_n[k, j] over the rows k of column i, ASCENDING, each product rounded and
// then added (-ffp-contract=off): the order of additions is fixed by the matrix alone.  The pattern is structural -
// every j that shares a row with column i, the diagonal included, a sum that cancels to 0.0 included; a zero column
// gives an empty row.  One workgroup per output row (rows dealt round robin to a fixed grid); the candidates are the
// CSR rows of column i's entries, their number bounded by cb_i = sum_{k in col i} deg_row(k):
//     cb_i <= SNGNN_SPARSE_COSINE_HASH_MAX   keys in an open-addressing table in LDS of the power of two >= 2 cb_i slots
//                                            (atomicCAS inserts), the sums in a table of floats beside it; both sorted by
//                                            key (bitonic) - the row in canonical order
//     larger                                 an accumulator of `cols` floats and a bitmap of `cols` bits per workgroup in
//                                            the workspace (zero on entry, zeroed again while read), read in word order
// No floating-point atomics.  The lanes of a wave spread over ONE row k at a time: inside a row the j are distinct, so
// a plain read-add-write per lane meets no other lane; rows follow each other in program order.  The four waves of a
// workgroup own disjoint classes of j (j mod 4): every wave walks all k, no two waves touch one slot.  (The count only
// inserts keys - integer atomics - and splits the k among the waves instead.)
//
// Three epilogues of one row engine (template MODE): the count of the row's entries; the store of its column ids and
// values at the caller's offsets; the histogram - numpy's bin rule against the caller's `edges` table, as
// cosine_hist.hip - of exactly the fp32 values the store would write, with min / max / sum.  Counters are u64 in LDS
// (integer atomics), written per workgroup to a table in the workspace and added by a last launch, which also adds the
// cols^2 - nnz structural zeros arithmetically.  Sums: per thread over the sorted row in slot order, threads, waves and
// workgroups in fixed trees, f64 - the same bits on every run.
//
// A fourth epilogue, SC_TOPK, selects: the k best entries of the row in the order (value descending, column id
// ascending) - knn.hip's rule and the aggregation's - as 64-bit keys (sel_key: the order-preserving word of the value in
// the high half, the complemented id in the low half; keys of one row are unique, so "the k largest" is one set whatever
// the order they are met in).  The accumulators start at +0.0f (the tables' `tv[s] = 0.f`, the workspace's memset and the
// `acc[j] = 0.f` of the read-and-clear) and x + p is -0.0 only where both are: a stored value is never -0.0, the order
// of the keys is the order of the floats.  The selection is a search for the k-th largest key over (id, sum) slots in
// LDS, one ballot count of the whole workgroup per bit, the value word first and left as soon as a prefix separates
// exactly k keys (sc_select).  Table path: over the table's slots as the inserts left them - the keys carry the ids, so
// the by-key sort of the store is not needed.  Accumulator path: `tab` / `tv` are free there and hold a candidate
// buffer of SC_TABLE_MAX slots; the read-and-clear goes over 64 words a step (four threads a word: at most
// SC_HASH_MAX entries), appends what beats the running threshold - the k-th key so far - and, when fewer than
// SC_HASH_MAX slots are free, the buffer is reduced to its k largest and the threshold raised.
#include <algorithm>
#include <string>

#include "common.h"
#include "device_utils.h"
#include "ws_layout.h"

namespace sngnn {

constexpr int SC_BLOCK = 256;
constexpr int SC_WAVES = SC_BLOCK / 64;
constexpr int SC_HASH_MAX = SNGNN_SPARSE_COSINE_HASH_MAX;
constexpr int SC_TABLE_MAX = 2 * SC_HASH_MAX;                     // 4 096 keys + 4 096 sums: 32 KiB of the CU's 160
constexpr int SC_EMPTY = 0x7fffffff;                              // (column ids are below it)
constexpr int SC_MAX_WGS = 2048;
constexpr int64_t SC_ACC_BUDGET = (int64_t)512 << 20;             // bytes of accumulators: fewer workgroups at large N
constexpr int SC_MAX_BINS = 1024;
constexpr int SC_MAX_K = 32;                                      // knn.hip's KNN_MAX_K
constexpr int SC_WAVE_KEYS = 4;                                   // keys a lane holds where one wave selects
enum { SC_COUNT = 0, SC_FILL = 1, SC_HIST = 2, SC_TOPK = 3 };
static_assert((SC_WAVES & (SC_WAVES - 1)) == 0, "the waves' classes of j are j & (SC_WAVES - 1)");

// words of one workgroup's bitmap: whole 128-byte lines, so no two workgroups share one; its accumulator has a float
// per bit
static int64_t sc_words(int64_t cols) { return (cols + 1023) / 1024 * 32; }

static int sc_workgroups(int64_t cols)
{
    if (cols <= 0) return 0;
    const int64_t per = sc_words(cols) * 4 * 33;
    const int64_t by_budget = std::max<int64_t>(64, SC_ACC_BUDGET / per);
    return (int)std::min<int64_t>({cols, (int64_t)SC_MAX_WGS, by_budget});
}

// the workspace: [bitmaps | accumulators (fill, hist) | per-workgroup counters, sums, minima, maxima (hist)]
struct ScLayout { int wgs; int64_t words, acc, cnt, psum, pmin, pmax, total; };
static ScLayout sc_layout(int64_t cols, int mode, int bins)
{
    ScLayout L;
    L.wgs = sc_workgroups(cols);
    L.words = sc_words(cols);
    L.acc = up256(L.wgs * L.words * 4);
    L.cnt = L.acc + (mode == SC_COUNT ? 0 : up256(L.wgs * L.words * 32 * 4));      // (the selection's workspace: the fill's)
    L.psum = L.cnt + (mode == SC_HIST ? up256((int64_t)L.wgs * (bins + 2) * 8) : 0);
    L.pmin = L.psum + (mode == SC_HIST ? up256((int64_t)L.wgs * 8) : 0);
    L.pmax = L.pmin + (mode == SC_HIST ? up256((int64_t)L.wgs * 4) : 0);
    L.total = L.pmax + (mode == SC_HIST ? up256((int64_t)L.wgs * 4) : 0) + 256;
    return L;
}

struct ScArgs {
    const int64_t *colptr; const int32_t *rowidx; const float *vals;      // M_n by column
    const int64_t *rowptr; const int32_t *colidx; const float *rvals;     // M_n by row
    int cols, words;
    unsigned *bitmaps; float *acc;
    int32_t *count;                                                       // SC_COUNT
    const int64_t *offs; int32_t *out_col; float *out_val;                // SC_FILL
    const float *edges; int bins, diagonal;                               // SC_HIST
    unsigned long long *wg_cnt; double *psum; float *pmin, *pmax;
    int k, exclude_self; int32_t *nbr_idx; float *nbr_sim;                // SC_TOPK
};

// exclusive prefix of c over the workgroup's threads and the total (sh: SC_WAVES words of LDS; two barriers)
__device__ __forceinline__ int sc_block_scan(int c, int *sh, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
    for (int k = 0; k < SC_WAVES; ++k) {
        const int v = sh[k];
        if (k < wave) before += v;
        tot += v;
    }
    __syncthreads();
    total = tot;
    return before + incl - c;
}

__device__ __forceinline__ unsigned sc_hash(int k, int mask) { return ((unsigned)k * 2654435761u >> 7) & (unsigned)mask; }

// numpy's bin of v against the table: -1 below edges[0], bins above edges[bins], else b with edges[b] <= v <
// edges[b + 1], the last bin closed on the right.  The candidate comes from one multiply-add and is moved against the
// table until the rule holds.
__device__ __forceinline__ int sc_bin(float v, const float *s_edge, int bins, float scale, float off)
{
    if (v < s_edge[0]) return -1;
    if (v > s_edge[bins]) return bins;
    int b = min(max((int)__fmaf_rn(v, scale, off), 0), bins - 1);
    while (b > 0 && v < s_edge[b]) --b;
    while (b < bins - 1 && v >= s_edge[b + 1]) ++b;
    return b;
}

// The k largest keys of the slots [0, n) of (tab, tv) - a slot that is empty or holds column `skip` has no key - into
// top[] in no particular order; returns their number m <= k.  thr: a key that exactly the kept ones reach when the
// workgroup searched and there were more than k (then m == k), else 0 - the weakest threshold.  The whole workgroup calls it behind a barrier that follows the slots'
// writes, and leaves it behind one.  A count is one ballot per 256 slots and wave and one barrier (cnt[2][SC_WAVES],
// used in turn: a wave that writes a pair again has passed the barrier behind every wave's read of it).  The search is
// wave_topk_keys_n's: the bits of the value word from the top, left at the first prefix that exactly k keys reach; the
// `lowbits` bits of the id only when equal values lie on both sides of the cut.  Up to 64 SC_WAVE_KEYS slots are wave
// 0's alone - that function itself, no barrier per step.
__device__ __forceinline__ int sc_select(const int *tab, const float *tv, int n, int skip, int k, int lowbits,
                                         unsigned long long *top, int *ntop, int (*cnt)[SC_WAVES],
                                         unsigned long long &thr)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto key_at = [&](int s) -> unsigned long long {
        if (s >= n) return 0ull;
        const int j = tab[s];
        return j == SC_EMPTY || j == skip ? 0ull : sel_key(tv[s], (unsigned)j);
    };
    thr = 0ull;
    if (n <= 64 * SC_WAVE_KEYS) {
        // few slots - most rows of a sparse graph: wave 0 holds them all and searches with ballots alone
        if (wave == 0) {
            unsigned long long key[SC_WAVE_KEYS];
            bool kept[SC_WAVE_KEYS];
#pragma unroll
            for (int q = 0; q < SC_WAVE_KEYS; ++q) key[q] = key_at(64 * q + lane);
            wave_topk_keys_n<SC_WAVE_KEYS>(key, k, lowbits, kept);
            int m = 0;
#pragma unroll
            for (int q = 0; q < SC_WAVE_KEYS; ++q) {
                const unsigned long long mask = __ballot(kept[q]);
                if (kept[q]) top[m + prefix_popc(mask)] = key[q];
                m += __popcll(mask);
            }
            if (lane == 0) *ntop = m;
        }
        __syncthreads();
        const int m = *ntop;
        __syncthreads();
        return m;
    }
    int turn = 0;
    auto count = [&](auto pred) -> int {
        int c = 0;
        for (int s0 = 0; s0 < n; s0 += SC_BLOCK) c += __popcll(__ballot(pred(key_at(s0 + tid))));
        int *mine = cnt[turn];
        turn ^= 1;
        if (lane == 0) mine[wave] = c;
        __syncthreads();
        int t = 0;
#pragma unroll
        for (int w = 0; w < SC_WAVES; ++w) t += mine[w];
        return t;
    };
    if (tid == 0) *ntop = 0;
    unsigned long long T = 1ull;                                  // (every key reaches it)
    if (count([](unsigned long long q) { return q != 0ull; }) > k) {
        unsigned Th = 0u;
        bool cut = false;
        for (int b = 31; b >= 0 && !cut; --b) {
            const unsigned cand = Th | (1u << b);
            const int c = count([cand](unsigned long long q) { return (unsigned)(q >> 32) >= cand; });
            if (c >= k) { Th = cand; cut = c == k; }
        }
        T = (unsigned long long)Th << 32;
        if (!cut) {                                               // equal values on both sides of the cut: the id decides
            T |= 0xFFFFFFFFull & ~((1ull << lowbits) - 1ull);
            for (int b = lowbits - 1; b >= 0; --b) {
                const unsigned long long cand = T | (1ull << b);
                const int c = count([cand](unsigned long long q) { return q >= cand; });
                if (c >= k) { T = cand; if (c == k) break; }
            }
        }
        thr = T;
    }
    for (int s0 = 0; s0 < n; s0 += SC_BLOCK) {
        const unsigned long long q = key_at(s0 + tid);
        if (q != 0ull && q >= T) {
            const int p = atomicAdd(ntop, 1);                     // (their order is not the result's: the ranks are)
            if (p < SC_MAX_K) top[p] = q;
        }
    }
    __syncthreads();
    const int m = min(*ntop, k);
    __syncthreads();
    return m;
}

template <int MODE>
__global__ __launch_bounds__(SC_BLOCK) void k_sparse_cosine(ScArgs a)
{
    constexpr bool NUM = MODE != SC_COUNT, HIST = MODE == SC_HIST, TOPK = MODE == SC_TOPK;
    __shared__ int tab[SC_TABLE_MAX];
    __shared__ float tv[NUM ? SC_TABLE_MAX : 1];
    __shared__ int sh[SC_WAVES];
    __shared__ float s_edge[HIST ? SC_MAX_BINS + 1 : 1];
    __shared__ unsigned long long s_cnt[HIST ? SC_MAX_BINS + 2 : 1];
    __shared__ float s_mn[SC_WAVES], s_mx[SC_WAVES];
    __shared__ double s_sm[SC_WAVES];
    __shared__ unsigned long long s_top[TOPK ? SC_MAX_K : 1];
    __shared__ int s_ntop, s_c[2][SC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned *bm = a.bitmaps + (size_t)blockIdx.x * a.words;
    float *acc = NUM ? a.acc + (size_t)blockIdx.x * a.words * 32 : nullptr;
    float vmin = INFINITY, vmax = -INFINITY, scale = 0.f, off_bin = 0.f;
    double vsum = 0.0;
    if constexpr (HIST) {
        for (int q = tid; q <= a.bins; q += SC_BLOCK) s_edge[q] = a.edges[q];
        for (int q = tid; q < a.bins + 2; q += SC_BLOCK) s_cnt[q] = 0ull;
        __syncthreads();
        scale = (float)a.bins / (s_edge[a.bins] - s_edge[0]);
        off_bin = -s_edge[0] * scale;
    }
    // the histogram's epilogue for one entry (j, v) of row i
    auto tally = [&](int i, int j, float v) {
        if (a.diagonal == 0 && j == i) return;
        atomicAdd(&s_cnt[sc_bin(v, s_edge, a.bins, scale, off_bin) + 1], 1ull);
        vmin = fminf(vmin, v);
        vmax = fmaxf(vmax, v);
        vsum += (double)v;
    };

    // the selection's epilogue for row i: the m keys of s_top at their ranks, pads behind them
    int lowbits = 1;
    if constexpr (TOPK)
        while (lowbits < 31 && (1 << lowbits) < a.cols) ++lowbits;
    auto emit = [&](int i, int m) {
        if (tid < a.k) {
            const int64_t o = (int64_t)i * a.k;
            if (tid < m) {
                const unsigned long long q = s_top[tid];
                int rk = 0;
                for (int u = 0; u < m; ++u) rk += s_top[u] > q ? 1 : 0;
                a.nbr_idx[o + rk] = (int32_t)sel_key_index(q);
                a.nbr_sim[o + rk] = sel_key_score(q);
            } else {
                a.nbr_idx[o + tid] = -1;
                a.nbr_sim[o + tid] = 0.f;
            }
        }
        __syncthreads();                                          // (s_top is the next row's too)
    };

    for (int i = blockIdx.x; i < a.cols; i += gridDim.x) {
        const int64_t p0 = a.colptr[i], d = a.colptr[i + 1] - p0;
        // the candidate bound, saturated just above the threshold (every partial and their sum fit an int)
        int part = 0;
        for (int64_t e = tid; e < d; e += SC_BLOCK) {
            const int k = a.rowidx[p0 + e];
            part = (int)std::min<int64_t>(part + (a.rowptr[k + 1] - a.rowptr[k]), SC_HASH_MAX + 1);
        }
        int cb;
        sc_block_scan(part, sh, cb);
        // visit(j, product) for the entries of the rows k of column i, k ascending: 64 of the column's entries are
        // read by the lanes at once and handed round; the lanes then spread over one row k at a time.  NUM: every wave
        // walks all k and keeps its own class of j; the count splits the chunks of k among the waves.
        auto walk = [&](auto visit) {
            for (int64_t e0 = NUM ? 0 : wave * 64; e0 < d; e0 += NUM ? 64 : SC_BLOCK) {
                const int64_t e = e0 + lane;
                float av = 0.f;
                long long q0 = 0;
                int n = 0;
                if (e < d) {
                    const int k = a.rowidx[p0 + e];
                    if constexpr (NUM) av = a.vals[p0 + e];
                    q0 = a.rowptr[k];
                    n = (int)(a.rowptr[k + 1] - q0);
                }
                const int m = (int)std::min<int64_t>(64, d - e0);
                for (int t = 0; t < m; ++t) {
                    const float at = __shfl(av, t, 64);
                    const long long qt = __shfl(q0, t, 64);
                    const int nt = __shfl(n, t, 64);
                    for (int u = lane; u < nt; u += 64) {
                        const int j = a.colidx[qt + u];
                        if (!NUM || (j & (SC_WAVES - 1)) == wave) {
                            float p = 0.f;
                            if constexpr (NUM) p = at * a.rvals[qt + u];
                            visit(j, p);
                        }
                    }
                    visit.next_row();
                }
            }
        };
        int total = 0;
        const int64_t off = MODE == SC_FILL ? a.offs[i] : 0;
        const int skip = TOPK && a.exclude_self != 0 ? i : -1;
        if (cb == 0) {
            // a zero column: an empty row
            if constexpr (TOPK) emit(i, 0);
        } else if (cb <= SC_HASH_MAX) {
            int T = 64;
            while (T < 2 * cb) T <<= 1;
            for (int s = tid; s < T; s += SC_BLOCK) {
                tab[s] = SC_EMPTY;
                if constexpr (NUM) tv[s] = 0.f;
            }
            __syncthreads();
            struct {
                int *tab; float *tv; int mask;
                __device__ void operator()(int j, float p) const
                {
                    unsigned h = sc_hash(j, mask);
                    for (;;) {          // (at most cb <= T / 2 distinct keys: an empty slot is always found)
                        const int old = atomicCAS(&tab[h], SC_EMPTY, j);
                        if (old == SC_EMPTY || old == j) break;
                        h = (h + 1) & (unsigned)mask;
                    }
                    if constexpr (NUM) tv[h] = tv[h] + p;
                }
                // rows of M follow each other in program order; the LDS serves one wave's accesses in order
                __device__ void next_row() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
            } insert{tab, tv, T - 1};
            walk(insert);
            __syncthreads();
            if constexpr (!NUM) {
                int c = 0;
                for (int s = tid; s < T; s += SC_BLOCK) c += tab[s] != SC_EMPTY ? 1 : 0;
                sc_block_scan(c, sh, total);
            } else if constexpr (TOPK) {
                unsigned long long thr;
                emit(i, sc_select(tab, tv, T, skip, a.k, lowbits, s_top, &s_ntop, s_c, thr));
            } else {
                // bitonic sort by key, ascending, the sums carried along: the entries in front, empty slots behind
                for (int k = 2; k <= T; k <<= 1)
                    for (int j = k >> 1; j > 0; j >>= 1) {
                        for (int s = tid; s < T; s += SC_BLOCK) {
                            const int o = s ^ j;
                            if (o > s) {
                                const int x = tab[s], y = tab[o];
                                if ((x > y) == ((s & k) == 0)) {
                                    const float fx = tv[s], fy = tv[o];
                                    tab[s] = y; tab[o] = x;
                                    tv[s] = fy; tv[o] = fx;
                                }
                            }
                        }
                        __syncthreads();
                    }
                for (int s = tid; s < T; s += SC_BLOCK) {
                    const int j = tab[s];
                    if (j != SC_EMPTY) {
                        if constexpr (MODE == SC_FILL) {
                            a.out_col[off + s] = j;
                            a.out_val[off + s] = tv[s];
                        } else {
                            tally(i, j, tv[s]);
                        }
                    }
                }
                __syncthreads();
            }
        } else {
            struct {
                unsigned *bm; float *acc;
                __device__ void operator()(int j, float p) const
                {
                    if constexpr (NUM) acc[j] = acc[j] + p;
                    atomicOr(&bm[j >> 5], 1u << (j & 31));
                }
                // a row's stores are performed before the next row's loads (one CU: one vector L1)
                __device__ void next_row() const
                {
                    if constexpr (NUM) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                }
            } mark{bm, acc};
            walk(mark);
            __syncthreads();
            if constexpr (TOPK) {
                // read and clear in word order, 64 words a step: thread t has byte t & 3 of word w0 + (t >> 2), so the
                // ids ascend with t and a step appends at most 64 * 32 = SC_HASH_MAX entries, which are free
                int fill = 0;
                unsigned long long thr = 0ull;
                for (int w0 = 0; w0 < a.words; w0 += SC_BLOCK / 4) {
                    const int w = w0 + (tid >> 2);
                    unsigned bits = (tid & 3) == 0 && w < a.words ? atomicExch(&bm[w], 0u) : 0u;
                    bits = (__shfl(bits, lane & ~3, 64) >> (8 * (tid & 3))) & 0xFFu;
                    unsigned long long ck[8];
                    int np = 0;
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        ck[b] = 0ull;
                        if (bits >> b & 1u) {
                            const int j = w * 32 + 8 * (tid & 3) + b;
                            const unsigned long long q = sel_key(acc[j], (unsigned)j);
                            acc[j] = 0.f;
                            if (j != skip && q > thr) { ck[b] = q; ++np; }
                        }
                    }
                    int chunk;
                    int p = fill + sc_block_scan(np, sh, chunk);
#pragma unroll
                    for (int b = 0; b < 8; ++b)
                        if (ck[b] != 0ull) {
                            tab[p] = (int)sel_key_index(ck[b]);
                            tv[p] = sel_key_score(ck[b]);
                            ++p;
                        }
                    fill += chunk;
                    __syncthreads();
                    if (SC_TABLE_MAX - fill < SC_HASH_MAX) {
                        const int m = sc_select(tab, tv, fill, skip, a.k, lowbits, s_top, &s_ntop, s_c, thr);
                        if (tid < m) {
                            tab[tid] = (int)sel_key_index(s_top[tid]);
                            tv[tid] = sel_key_score(s_top[tid]);
                        }
                        fill = m;
                        __syncthreads();
                    }
                }
                emit(i, sc_select(tab, tv, fill, skip, a.k, lowbits, s_top, &s_ntop, s_c, thr));
                continue;
            }
            // read and clear in word order (an exchange: it reads where the atomics above wrote)
            for (int w0 = 0; w0 < a.words; w0 += SC_BLOCK) {
                const int w = w0 + tid;
                unsigned bits = w < a.words ? atomicExch(&bm[w], 0u) : 0u;
                int chunk;
                const int before = sc_block_scan(__popc(bits), sh, chunk);
                if constexpr (NUM) {
                    int64_t p = off + total + before;
                    while (bits) {
                        const int j = w * 32 + __ffs(bits) - 1;
                        bits &= bits - 1;
                        const float v = acc[j];
                        acc[j] = 0.f;
                        if constexpr (MODE == SC_FILL) {
                            a.out_col[p] = j;
                            a.out_val[p] = v;
                            ++p;
                        } else {
                            tally(i, j, v);
                        }
                    }
                }
                total += chunk;
            }
            __syncthreads();
        }
        if constexpr (MODE == SC_COUNT)
            if (tid == 0) a.count[i] = total;
    }
    if constexpr (HIST) {
        __syncthreads();
        for (int q = tid; q < a.bins + 2; q += SC_BLOCK) a.wg_cnt[(size_t)blockIdx.x * (a.bins + 2) + q] = s_cnt[q];
        // the workgroup's statistics: lanes (xor tree), then its waves in order
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            vmin = fminf(vmin, __shfl_xor(vmin, m, 64));
            vmax = fmaxf(vmax, __shfl_xor(vmax, m, 64));
            vsum += __shfl_xor(vsum, m, 64);
        }
        if (lane == 0) { s_mn[wave] = vmin; s_mx[wave] = vmax; s_sm[wave] = vsum; }
        __syncthreads();
        if (tid == 0) {
            float x = s_mn[0], y = s_mx[0];
            double z = s_sm[0];
            for (int w = 1; w < SC_WAVES; ++w) { x = fminf(x, s_mn[w]); y = fmaxf(y, s_mx[w]); z += s_sm[w]; }
            a.pmin[blockIdx.x] = x;
            a.pmax[blockIdx.x] = y;
            a.psum[blockIdx.x] = z;
        }
    }
}

// counts = the workgroups' counters added up + the structural zeros (entries - counted) in the slot that holds 0.0;
// stats = {min, max, sum} of the workgroups' partial results in a FIXED order (thread t takes parts t, t + 1024, ...
// in sequence, then a tree over the threads), the zeros taking part in min and max.  No parts and no zeros: +inf, -inf, 0
__global__ __launch_bounds__(1024) void k_sc_hist_final(const unsigned long long *__restrict__ wg_cnt, int wgs,
                                                        const float *__restrict__ pmin, const float *__restrict__ pmax,
                                                        const double *__restrict__ psum, const float *__restrict__ edges,
                                                        int bins, unsigned long long entries,
                                                        unsigned long long *__restrict__ counts, double *__restrict__ stats)
{
    __shared__ float s_a[1024], s_c[1024];
    __shared__ double s_d[1024];
    __shared__ unsigned long long s_n[1024];
    const int t = threadIdx.x;
    unsigned long long mine = 0ull;
    for (int q = t; q < bins + 2; q += 1024) {
        unsigned long long v = 0ull;
        for (int w = 0; w < wgs; ++w) v += wg_cnt[(size_t)w * (bins + 2) + q];
        counts[q] = v;
        mine += v;
    }
    float x = INFINITY, y = -INFINITY;
    double z = 0.0;
    for (int w = t; w < wgs; w += 1024) {
        x = fminf(x, pmin[w]);
        y = fmaxf(y, pmax[w]);
        z += psum[w];
    }
    s_a[t] = x; s_c[t] = y; s_d[t] = z; s_n[t] = mine;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (t < w) {
            s_a[t] = fminf(s_a[t], s_a[t + w]);
            s_c[t] = fmaxf(s_c[t], s_c[t + w]);
            s_d[t] += s_d[t + w];
            s_n[t] += s_n[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        const unsigned long long zeros = entries - s_n[0];
        x = s_a[0]; y = s_c[0];
        if (zeros != 0ull) {
            int b = 0;                                            // the bin of 0.0 against the table itself
            if (0.f < edges[0]) b = -1;
            else if (0.f > edges[bins]) b = bins;
            else
                while (b < bins - 1 && 0.f >= edges[b + 1]) ++b;
            counts[b + 1] += zeros;
            x = fminf(x, 0.f);
            y = fmaxf(y, 0.f);
        }
        stats[0] = (double)x;
        stats[1] = (double)y;
        stats[2] = s_d[0];
    }
}

static int sc_check(const int64_t *colptr, const int32_t *rowidx, const int64_t *rowptr, const int32_t *colidx,
                    int64_t rows, int64_t cols)
{
    SN_REQUIRE(rows >= 0 && cols >= 0, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(rows < (int64_t)SC_EMPTY && cols < (int64_t)SC_EMPTY, SNGNN_ERANGE,
               "the matrix does not fit the kernel's 32-bit row and column ids");
    SN_REQUIRE(colptr && rowptr, SNGNN_EINVAL, "NULL argument");
    (void)rowidx; (void)colidx;          // (may be NULL: a matrix without entries)
    return SNGNN_OK;
}

static int sc_bind(ScArgs &a, const ScLayout &L, int64_t cols, void *workspace, int64_t workspace_bytes, hipStream_t st)
{
    SN_REQUIRE(workspace != nullptr, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(workspace_bytes >= L.total, SNGNN_EINVAL,
               "the workspace is smaller than the size function's " + std::to_string(L.total) + " bytes");
    a.cols = (int)cols;
    a.words = (int)L.words;
    a.bitmaps = (unsigned *)workspace;
    a.acc = (float *)((char *)workspace + L.acc);
    if (L.cnt > 0) SN_HIP(hipMemsetAsync(workspace, 0, (size_t)L.cnt, st));
    return SNGNN_OK;
}

}  // namespace sngnn

using namespace sngnn;

extern "C" int64_t sngnn_sparse_cosine_count_workspace_bytes(int64_t rows, int64_t cols)
{
    (void)rows;
    return cols < 0 ? 0 : sc_layout(cols, SC_COUNT, 0).total;
}

extern "C" int64_t sngnn_sparse_cosine_fill_workspace_bytes(int64_t rows, int64_t cols)
{
    (void)rows;
    return cols < 0 ? 0 : sc_layout(cols, SC_FILL, 0).total;
}

extern "C" int64_t sngnn_sparse_cosine_hist_workspace_bytes(int64_t rows, int64_t cols, int bins)
{
    (void)rows;
    return cols < 0 || bins < 1 || bins > SC_MAX_BINS ? 0 : sc_layout(cols, SC_HIST, bins).total;
}

extern "C" int64_t sngnn_sparse_cosine_topk_workspace_bytes(int64_t rows, int64_t cols, int k)
{
    (void)rows;
    return cols < 0 || k < 1 || k > SC_MAX_K ? 0 : sc_layout(cols, SC_TOPK, 0).total;
}

extern "C" int sngnn_sparse_cosine_count(const int64_t *colptr, const int32_t *rowidx, const int64_t *rowptr,
                                         const int32_t *colidx, int64_t rows, int64_t cols, int32_t *count,
                                         void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = sc_check(colptr, rowidx, rowptr, colidx, rows, cols)) return rc;
    if (cols == 0) return SNGNN_OK;
    SN_REQUIRE(count, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const ScLayout L = sc_layout(cols, SC_COUNT, 0);
    ScArgs a{};
    a.colptr = colptr; a.rowidx = rowidx; a.rowptr = rowptr; a.colidx = colidx;
    a.count = count;
    a.diagonal = 1;
    if (int rc = sc_bind(a, L, cols, workspace, workspace_bytes, st)) return rc;
    k_sparse_cosine<SC_COUNT><<<L.wgs, SC_BLOCK, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_sparse_cosine_fill(const int64_t *colptr, const int32_t *rowidx, const float *vals,
                                        const int64_t *rowptr, const int32_t *colidx, const float *rvals, int64_t rows,
                                        int64_t cols, const int64_t *offsets, int64_t nnz, int32_t *out_col,
                                        float *out_val, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = sc_check(colptr, rowidx, rowptr, colidx, rows, cols)) return rc;
    SN_REQUIRE(nnz >= 0, SNGNN_EINVAL, "nnz is negative");
    SN_REQUIRE(nnz <= (int64_t)INT32_MAX, SNGNN_ERANGE, "the similarity has more than 2^31 - 1 entries");
    if (cols == 0 || nnz == 0) return SNGNN_OK;
    SN_REQUIRE(vals && rvals && rowidx && colidx && offsets && out_col && out_val, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const ScLayout L = sc_layout(cols, SC_FILL, 0);
    ScArgs a{};
    a.colptr = colptr; a.rowidx = rowidx; a.vals = vals; a.rowptr = rowptr; a.colidx = colidx; a.rvals = rvals;
    a.offs = offsets; a.out_col = out_col; a.out_val = out_val;
    a.diagonal = 1;
    if (int rc = sc_bind(a, L, cols, workspace, workspace_bytes, st)) return rc;
    k_sparse_cosine<SC_FILL><<<L.wgs, SC_BLOCK, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_sparse_cosine_hist(const int64_t *colptr, const int32_t *rowidx, const float *vals,
                                        const int64_t *rowptr, const int32_t *colidx, const float *rvals, int64_t rows,
                                        int64_t cols, const float *edges, int bins, int diagonal,
                                        unsigned long long *counts, double *stats, void *workspace,
                                        int64_t workspace_bytes, void *stream)
{
    if (int rc = sc_check(colptr, rowidx, rowptr, colidx, rows, cols)) return rc;
    SN_REQUIRE(bins >= 1 && bins <= SC_MAX_BINS, SNGNN_EINVAL, "bins must be in [1, " + std::to_string(SC_MAX_BINS) + "]");
    SN_REQUIRE(edges && counts && stats, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const ScLayout L = sc_layout(cols, SC_HIST, bins);
    ScArgs a{};
    a.colptr = colptr; a.rowidx = rowidx; a.vals = vals; a.rowptr = rowptr; a.colidx = colidx; a.rvals = rvals;
    a.edges = edges; a.bins = bins; a.diagonal = diagonal != 0 ? 1 : 0;
    if (int rc = sc_bind(a, L, cols, workspace, workspace_bytes, st)) return rc;
    a.wg_cnt = (unsigned long long *)((char *)workspace + L.cnt);
    a.psum = (double *)((char *)workspace + L.psum);
    a.pmin = (float *)((char *)workspace + L.pmin);
    a.pmax = (float *)((char *)workspace + L.pmax);
    if (L.wgs > 0) k_sparse_cosine<SC_HIST><<<L.wgs, SC_BLOCK, 0, st>>>(a);
    const unsigned long long entries = (unsigned long long)cols * (unsigned long long)(diagonal != 0 ? cols : cols - 1);
    k_sc_hist_final<<<1, 1024, 0, st>>>(a.wg_cnt, L.wgs, a.pmin, a.pmax, a.psum, edges, bins, cols > 0 ? entries : 0ull,
                                        counts, stats);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_sparse_cosine_topk(const int64_t *colptr, const int32_t *rowidx, const float *vals,
                                        const int64_t *rowptr, const int32_t *colidx, const float *rvals, int64_t rows,
                                        int64_t cols, int k, int exclude_self, int32_t *nbr_idx, float *nbr_sim,
                                        void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = sc_check(colptr, rowidx, rowptr, colidx, rows, cols)) return rc;
    SN_REQUIRE(k >= 1 && k <= SC_MAX_K, SNGNN_EINVAL, "k must be in [1, " + std::to_string(SC_MAX_K) + "]");
    if (cols == 0) return SNGNN_OK;
    SN_REQUIRE(nbr_idx && nbr_sim, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const ScLayout L = sc_layout(cols, SC_TOPK, 0);
    ScArgs a{};
    a.colptr = colptr; a.rowidx = rowidx; a.vals = vals; a.rowptr = rowptr; a.colidx = colidx; a.rvals = rvals;
    a.k = k; a.exclude_self = exclude_self != 0 ? 1 : 0; a.nbr_idx = nbr_idx; a.nbr_sim = nbr_sim;
    a.diagonal = 1;
    if (int rc = sc_bind(a, L, cols, workspace, workspace_bytes, st)) return rc;
    k_sparse_cosine<SC_TOPK><<<L.wgs, SC_BLOCK, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

// Scoring and selection primitives of the forward's roles and finalize forms: the per-edge cosine in its table and
// on-the-fly forms, the top-k key routines on a wave and on a lane group, and the per-wave LDS layout of the main
// kernel.  Needs device_utils.h only (Row, group_sum, wave_topk_keys_n, sel_key).
#pragma once
#include "device_utils.h"

namespace sngnn {

// source rows in flight per lane group (x 64/G groups per wave): ~16 registers of row data
template <int R> struct Unroll { static constexpr int U = (R == 1) ? 4 : (R == 2 ? 2 : 1); };

// words of LDS per wave of the main kernel: 4 regions of SETW words
//   small rows: column ids (two buffers) | scores | kept weights      [64/G rows][SMALL_T] each
//   wave rows / tasks: scores [128] | kept list [128] | column ids [128]
template <int G> struct WaveLds {
    static constexpr int RPW = 64 / G;
    static constexpr int SETW = (RPW * SMALL_T > 128) ? RPW * SMALL_T : 128;
    //   finalize role (fin_group_batch): 96 words per row, one row per lane group
    static constexpr int WORDS = 4 * SETW > RPW * 96 ? 4 * SETW : RPW * 96;
};
static_assert(WAVE_T == 128 && SMALL_T == 16 && CHUNK == 128, "LDS layouts of the main kernel assume these");

// per-edge cosine of two unit rows (fma chain over the lane's channels, fixed-order
// group sum); -0.0 -> +0.0: the reference orders floats, not bit patterns
template <int VEC, int G, int R>
__device__ __forceinline__ float unit_dot(const Row<VEC, G, R> &a, const Row<VEC, G, R> &x)
{
    return group_sum<G>(a.dot_partial(x)) + 0.0f;
}

// F.normalize of a row held in registers - the instruction sequence of k_normalize_rows (same
// fma chain, DPP tree, IEEE square root and division: the same bits); returns the clamped norm
template <int VEC, int G, int R>
__device__ __forceinline__ float normalize_in_place(Row<VEC, G, R> &x)
{
    const float q = group_sum<G>(x.dot_partial(x));
    const float d = fmaxf(ieee_sqrt(q), EPS_NORM);
    x.div_rn(d);
    return d;
}

// the reference-order cosine of a UNIT target row and a RAW source row (OTF mode's exact score:
// what the table path computes from its two table rows)
template <int VEC, int G, int R>
__device__ __forceinline__ float exact_score_raw(const Row<VEC, G, R> &nu, Row<VEC, G, R> x)
{
    normalize_in_place<VEC, G, R>(x);
    return unit_dot<VEC, G, R>(nu, x);
}

// the G bits of a wave ballot that belong to lane group gid
template <int G> __device__ __forceinline__ unsigned long long fwd_group_bits(unsigned long long m, int gid)
{
    if constexpr (G == 64) return m;
    else return (m >> (gid * G)) & ((1ull << G) - 1ull);
}

// ---------------------------------------------------------------------------
// Wave-level top-k of up to 128 selection keys, two per lane (0 = no key).
// Keys are unique, so "the k largest" is well defined: bitwise search for the
// k-th largest key T, then keep key >= T.  lowbits = bits of the largest
// row-local edge index (the low word of a key is 0xFFFFFFFF - index, so its
// upper 32 - lowbits bits are all ones and need no search).
// ---------------------------------------------------------------------------
// (CAND_MAX_K - split rows: chunk-local candidates are kept for k <= this: ws_layout.h, which sizes their records)

// (wave_topk_keys_n: device_utils.h)
__device__ __forceinline__ void wave_topk_keys(unsigned long long key0, unsigned long long key1,
                                               int k, int lowbits, bool &kept0, bool &kept1)
{
    const unsigned long long key[2] = {key0, key1};
    bool kept[2];
    wave_topk_keys_n<2>(key, k, lowbits, kept);
    kept0 = kept[0];
    kept1 = kept[1];
}

// the same among CANDIDATES (keys that already won a selection: wave_topk_keys_n's PREFIX note) - the finalize's calls
__device__ __forceinline__ void wave_topk_cands(unsigned long long key0, unsigned long long key1,
                                                int k, int lowbits, bool &kept0, bool &kept1)
{
    const unsigned long long key[2] = {key0, key1};
    bool kept[2];
    wave_topk_keys_n<2, true>(key, k, lowbits, kept);
    kept0 = kept[0];
    kept1 = kept[1];
}

__device__ __forceinline__ float key_score(unsigned long long key)
{
    const unsigned u = (unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ int key_index(unsigned long long key)
{
    return (int)(0xFFFFFFFFu - (unsigned)key);
}

// Top-k (and >= thr) of the scores sc[0, n) of one wave's edges; edge t of the
// wave has row-local index base + t.  An edge below thr gets no key at all:
// "top-k, then drop < thr" == "drop < thr, then top-k" because the order is by score.
struct WaveSel {
    bool kept0, kept1;
    unsigned long long key0, key1;
};

__device__ __forceinline__ WaveSel wave_select(const float *sc, int n, int base, int k, float thr,
                                               int lowbits)
{
    const int lane = lane_id();
    const int i0 = lane, i1 = lane + 64;
    const float s0 = i0 < n ? sc[i0] : 0.f, s1 = i1 < n ? sc[i1] : 0.f;
    WaveSel r;
    r.key0 = (i0 < n && s0 >= thr) ? sel_key(s0, base + i0) : 0ull;
    r.key1 = (i1 < n && s1 >= thr) ? sel_key(s1, base + i1) : 0ull;
    wave_topk_keys(r.key0, r.key1, k, lowbits, r.kept0, r.kept1);
    return r;
}

// Top-k of the keys of ONE LANE GROUP (NK per lane, 0 = no key): wave_topk_keys_n's search with every count taken
// over the group (the groups of a wave search different rows: no uniform early return - a group that is done
// idles until the last one is).  The kept set is the k largest keys: the same set whichever routine picks it.
template <int G, int NK>
__device__ __forceinline__ void group_topk_keys_n(const unsigned long long (&key)[NK], int k, int lowbits,
                                                  bool (&kept)[NK])
{
    const float fk = (float)k;                                // (counts <= 64 NK / (64 / G): exact in fp32)
    float c0 = 0.f;
#pragma unroll
    for (int u = 0; u < NK; ++u) c0 += key[u] != 0ull ? 1.f : 0.f;
    const bool fits = group_sum<G>(c0) <= fk;                 // everything that passed thr fits
    unsigned hi[NK];
#pragma unroll
    for (int u = 0; u < NK; ++u) hi[u] = (unsigned)(key[u] >> 32);
    bool done = fits, exact = false;
    // the score bits all of the group's keys share need no search (wave_topk_keys_n's PREFIX note); the wave starts at
    // the highest bit in which any of its groups' keys differ
    unsigned o = 0u, an = 0xFFFFFFFFu;
#pragma unroll
    for (int u = 0; u < NK; ++u)
        if (key[u] != 0ull) { o |= hi[u]; an &= hi[u]; }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) { o |= __shfl_xor(o, m, 64); an &= __shfl_xor(an, m, 64); }
    const unsigned diff = o ^ an;                             // (a group without keys: all ones - and `fits`)
    const int top = diff ? 31 - __clz(diff) : -1;
    unsigned Th = top >= 0 ? (an & ~((2u << top) - 1u)) : an;
    for (int b = wave_max_i(done ? -1 : top); b >= 0; --b) {
        if (__all(done)) break;
        const unsigned cand = Th | (1u << b);
        float c = 0.f;
#pragma unroll
        for (int u = 0; u < NK; ++u) c += hi[u] >= cand ? 1.f : 0.f;
        c = group_sum<G>(c);
        if (!done && c >= fk) {
            Th = cand;
            if (c == fk) { exact = true; done = true; }       // no further bit changes the set
        }
    }
    unsigned long long T = ((unsigned long long)Th << 32) | (0xFFFFFFFFull & ~((1ull << lowbits) - 1ull));
    for (int b = lowbits - 1; b >= 0; --b) {
        if (__all(done)) break;
        const unsigned long long cand = T | (1ull << b);
        float c = 0.f;
#pragma unroll
        for (int u = 0; u < NK; ++u) c += key[u] >= cand ? 1.f : 0.f;
        c = group_sum<G>(c);
        if (!done && c >= fk) {
            T = cand;
            if (c == fk) done = true;
        }
    }
#pragma unroll
    for (int u = 0; u < NK; ++u) kept[u] = fits ? key[u] != 0ull : (exact ? hi[u] >= Th : key[u] >= T);
}

}  // namespace sngnn

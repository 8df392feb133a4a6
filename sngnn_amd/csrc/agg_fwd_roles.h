// The passes in front of the main kernel (unit rows, fp16 filter rows), the three work-item roles of the main kernel
// - small-row sets, wave rows, split-row tasks - with the scoring passes they share, and the kernel itself
// (k_agg_fwd), whose last workgroups may run the in-launch finalize.  Needs agg_fwd_args.h, agg_fwd_select.h,
// agg_fwd_src.h (FwdSrc: every role reads its gathered inputs through one, `src`), agg_fwd_filter.h (filter_scores,
// approx_candidates), agg_fwd_fin.h and fwd_plan.h (FWD_WAVES_PER_SIMD).
#pragma once
#include "agg_fwd_args.h"
#include "agg_fwd_filter.h"
#include "agg_fwd_fin.h"
#include "agg_fwd_select.h"
#include "agg_fwd_src.h"
#include "fwd_plan.h"

namespace sngnn {

// ---------------------------------------------------------------------------
// F.normalize (models.py:122,238,325): n = h / max(|h|_2, eps), one lane group per row.
// IEEE sqrt and division: a row with a single non-zero channel becomes exactly +-1 there.
// ---------------------------------------------------------------------------
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_normalize_rows(const float *__restrict__ h, int64_t rows, int C,
                                                          float *__restrict__ n, float *__restrict__ nrm,
                                                          uint2 *__restrict__ filt)
{
    using RowT = Row<VEC, G, R>;
    constexpr int RPW = 64 / G;
    constexpr int U = Unroll<R>::U >= 2 ? 2 : 1;      // rows per lane group per step
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    const int64_t w0 = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    for (int64_t base = w0 * RPW * U; base < rows; base += nw * RPW * U) {
        RowT x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = base + u * RPW + gid;
            x[u].load(h + (r < rows ? r : rows - 1) * C, C, lg);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = base + u * RPW + gid;
            const float q = group_sum<G>(x[u].dot_partial(x[u]));
            const float d = fmaxf(ieee_sqrt(q), EPS_NORM);
            x[u].div_rn(d);
            if (r < rows) {
                x[u].store(n + r * C, C, lg);
                if (lg == 0) nrm[r] = d;
                if constexpr (VEC == 4) {
                    // fp16 filter row (agg_fwd_filter.h): the lanes' 4-channel vectors cover exactly
                    // filter_row_halfs(C) = 4 G R channels, the ones beyond C hold zeros
                    if (filt) {
#pragma unroll
                        for (int q = 0; q < R; ++q)
                            filt[(size_t)r * (G * R) + q * G + lg] =
                                make_uint2(pack_half2(x[u].x[q][0] * FILT_SCALE, x[u].x[q][1] * FILT_SCALE),
                                           pack_half2(x[u].x[q][2] * FILT_SCALE, x[u].x[q][3] * FILT_SCALE));
                    }
                }
            }
        }
    }
}

// fp16 filter rows from unit rows the caller already holds (sngnn_agg_forward_normalized)
template <int G, int R>
__global__ __launch_bounds__(BLOCK) void k_filter_rows(const float *__restrict__ n, int64_t rows, int C,
                                                       uint2 *__restrict__ filt)
{
    using RowT = Row<4, G, R>;
    constexpr int RPW = 64 / G;
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    for (int64_t r = ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * RPW + gid; r < rows; r += nw * RPW) {
        RowT x;
        x.load(n + r * C, C, lg);
#pragma unroll
        for (int q = 0; q < R; ++q)
            filt[(size_t)r * (G * R) + q * G + lg] =
                make_uint2(pack_half2(x.x[q][0] * FILT_SCALE, x.x[q][1] * FILT_SCALE),
                           pack_half2(x.x[q][2] * FILT_SCALE, x.x[q][3] * FILT_SCALE));
    }
}

// ---------------------------------------------------------------------------
// Class C: deg <= SMALL_T, one group per row.
// ---------------------------------------------------------------------------
// One set of 64/G small rows (one per lane group) whose column ids are already in
// LDS (s_col[gid][t]).  d = this group's row descriptor (deg 0 for a padding slot).
// src: how the gathered inputs are read (agg_fwd_src.h).  The buffer form gives a slot beyond the row's edges an
// out-of-range offset instead of `self`, and skips a slot beyond EVERY row of the set altogether (t0 + u >= dmax is
// wave-uniform: a scalar branch around the load and the dot) - the sets are dealt by four-degree buckets, so on an
// arxiv-like graph, where most rows have one or two in-edges, that is half the slots.
// LEAN (k_agg_fwd's note): the call wants `out` only - no kept bits, no wsel / inv_norm stores, no selection lists.
template <int VEC, int G, int R, bool OTF, int EPI, typename S, bool LEAN, typename SRC>
__device__ __forceinline__ void small_rows_set(const FwdArgs &a, const SRC &src, const int4 d, bool valid,
                                               int *lds_wave, const int *s_col_set)
{
    static_assert(!LEAN || (!OTF && EPI == 0), "the lean form: table mode, plain stores");
    using RowT = Row<VEC, G, R>;
    constexpr int U = Unroll<R>::U;
    constexpr int SETW = WaveLds<G>::SETW;
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const int i = d.x, rs = d.y, deg = d.z;
    const bool emit = !LEAN && a.sel_src != nullptr && a.k >= 0;
    const bool rank = a.k >= 0 && deg > a.k;
    const bool need_sc = rank || emit;
    const int self = i + a.row_off;

    const int *s_col = s_col_set + gid * SMALL_T;
    float *s_sc = reinterpret_cast<float *>(lds_wave + 2 * SETW) + gid * SMALL_T;
    float *s_w = reinterpret_cast<float *>(lds_wave + 3 * SETW) + gid * SMALL_T;

    RowT ni;
    src.row(ni, self);
    // (the form that skips slots takes the maximum into a scalar register: the skip is a scalar branch)
    const int dmax = SRC::skips_dead ? __builtin_amdgcn_readfirstlane(wave_max_i(deg)) : wave_max_i(deg);
    float inv_i = 0.f, q_i = 0.f;
    if constexpr (OTF) {
        q_i = group_sum<G>(ni.dot_partial(ni));
        inv_i = inv_norm_of(q_i);
    }

    RowT acc;
    acc.zero();
    [[maybe_unused]] unsigned kb = 0u;                 // the row's kept bits (a.kbits)
    // one step: NU slots, t0 .. t0 + NU - 1, of every row of the set - their loads first, all in flight together
    auto step = [&](int t0, auto nu_c) __attribute__((always_inline)) {
        constexpr int NU = decltype(nu_c)::value;
        RowT x[NU];
        float nj[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const bool live = (t0 + u) < deg;
            const int j = src.pick(live, s_col[t0 + u], self);
            src.row_if(x[u], j, live);
            if constexpr (OTF) nj[u] = 1.f;
            else nj[u] = src.nrm_unless(j, live, rank);   // a streaming row weighs the row it has just scored
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            float s;
            if constexpr (OTF) {
                s = edge_score<VEC, G, R>(ni, inv_i, x[u]);
                if (a.k >= 0 && !rank) {
                    // the threshold decides this edge: exact where the fast value cannot tell
                    const bool amb = (t0 + u < deg) && fabsf(s - a.thr) <= a.delta;
                    if (__ballot(amb) != 0ull) {                 // (wave-uniform; rare)
                        RowT nu = ni;
                        normalize_in_place<VEC, G, R>(nu);
                        const float se = exact_score_raw<VEC, G, R>(nu, x[u]);
                        if (amb) s = se;
                    }
                }
            } else {
                s = unit_dot<VEC, G, R>(ni, x[u]);
            }
            if (t0 + u < deg) {
                if (need_sc && lg == 0) s_sc[t0 + u] = s;
                if (!rank) {
                    const bool sel = (a.k < 0) || (s >= a.thr);
                    if (sel) acc.axpy(s * nj[u], x[u]);
                    if (!LEAN && a.wsel && lg == 0) a.wsel[rs + t0 + u] = sel ? s : SNGNN_UNSELECTED;
                    if constexpr (!OTF && !LEAN) kb |= sel ? (1u << (t0 + u)) : 0u;     // (group-uniform; table mode only)
                }
            }
        }
    };
    for (int t0 = 0; t0 < dmax; t0 += U) {
        // (the form that skips slots: a step of as many slots as the set's longest row still has - wave-uniform, a
        // scalar branch to a step without the others' loads and dots; every step is branch-free inside)
        // (Not a branch around each slot's load and dot inside one step: the compiler then keeps every slot's
        // column-id read, its wait and its load behind the slot's own branch - four LDS round trips in a row in front
        // of four loads that are meant to be in flight together.  Copies of the step cost code, not time.)
        const int nu = SRC::skips_dead ? min(dmax - t0, U) : U;
        if (nu == U) step(t0, std::integral_constant<int, U>{});
        else if constexpr (SRC::skips_dead && U > 1) {
            if (nu == 1) step(t0, std::integral_constant<int, 1>{});
            else if constexpr (U > 2) {                           // U == 4
                if (nu == 2) step(t0, std::integral_constant<int, 2>{});
                else step(t0, std::integral_constant<int, 3>{});
            }
        }
    }
    if (!LEAN && a.inv_norm && valid && lg == 0) {
        if constexpr (OTF) a.inv_norm[i] = ieee_div(1.0f, fmaxf(ieee_sqrt(q_i), EPS_NORM));
        else a.inv_norm[i] = ieee_div(1.0f, src.nrm(self));
    }

    if constexpr (OTF) {
        if (need_sc) {
            // ranks are asked for: wherever two fast scores of a row (or one and thr) are too close
            // to order, the whole row (<= 16 edges, cache-hot) is scored again exactly
            wave_lds_sync();
            bool amb = false;
            for (int e = lg; e < deg; e += G) {
                const float se = s_sc[e];
                // edges surely above / possibly above this one: its side of the top_k cut is in
                // doubt iff the cut falls between the two counts (ranks emitted: any near pair)
                int above = 0, maybe = 0;
                for (int b = 0; b < deg; ++b) {
                    const float sb = s_sc[b];
                    above += sb > se + 2.0f * a.delta;
                    maybe += (b != e) && sb >= se - 2.0f * a.delta;
                }
                amb |= emit ? (maybe > above) : (above < a.k && maybe >= a.k);
                amb |= above < a.k && fabsf(se - a.thr) <= a.delta;
            }
            const bool row_amb = fwd_group_bits<G>(__ballot(amb), gid) != 0ull;
            if (__ballot(row_amb) != 0ull) {                         // (wave-uniform)
                RowT nu = ni;
                normalize_in_place<VEC, G, R>(nu);
                const int dm = wave_max_i(row_amb ? deg : 0);
                for (int t = 0; t < dm; ++t) {
                    const bool live = row_amb && t < deg;
                    RowT xr;
                    src.row_if(xr, src.pick(live, s_col[t], self), live);
                    const float se = exact_score_raw<VEC, G, R>(nu, xr);
                    if (live && lg == 0) s_sc[t] = se;
                }
            }
        }
    }

    if (need_sc) {
        wave_lds_sync();
        // rank of every edge of the row under (score desc, position asc)
        for (int e = lg; e < deg; e += G) {
            const float se = s_sc[e];
            int rk = 0;
            for (int b = 0; b < deg; ++b) {
                const float sb = s_sc[b];
                rk += (sb > se) || (sb == se && b < e);
            }
            const bool sel = rk < a.k && se >= a.thr;
            s_w[e] = sel ? se : SNGNN_UNSELECTED;
            if (!LEAN && rank && a.wsel) a.wsel[rs + e] = sel ? se : SNGNN_UNSELECTED;
            // (lane lg == 0 runs every iteration any lane of its group runs: it ends with all the bits)
            if constexpr (!OTF && !LEAN)
                if (rank && a.kbits) kb |= (unsigned)fwd_group_bits<G>(__ballot(sel), gid) << (e - lg);
            if (emit && sel) {
                a.sel_src[(size_t)i * a.k + rk] = s_col[e];
                a.sel_w[(size_t)i * a.k + rk] = se;
            }
        }
        if (rank) {
            wave_lds_sync();
            // second pass: gather only the kept source rows, in edge order
            // (group-divergent trip count: no cross-lane operation inside)
            for (int t = 0; t < deg; ++t) {
                const float w = s_w[t];
                if (w != SNGNN_UNSELECTED) {
                    const int j = s_col[t];
                    RowT xr;
                    src.row(xr, j);
                    if constexpr (OTF) acc.axpy(w, xr);
                    else acc.axpy(w * src.nrm(j), xr);
                }
            }
        }
        wave_lds_sync();       // s_sc / s_w are reused by the next set
    }
    if constexpr (!OTF && !LEAN)
        if (a.kbits && valid && lg == 0) reinterpret_cast<unsigned short *>(a.kbits)[i] = (unsigned short)kb;
    if (valid) {
        acc.div((float)max(deg, 1));
        if constexpr (EPI == 1) row_epilogue<VEC, G, R>(a, acc, i, lg);
        acc.store(a.outs<S>() + (size_t)i * a.C, a.C, lg);
    }
}

// The same set with the fp16 FILTER in front (agg_fwd_filter.h; the FILT kernel, table mode, G >= 16 >=
// SMALL_T: lane lg of a group owns edge lg of its row).  The unfiltered set gathers the fp32 unit row of
// EVERY in-edge to score it - two lines at C = 40 or 64 - although a ranking row keeps top_k of them and
// a threshold may drop most: 95 % of an arxiv-like graph's rows are small rows.  Here every edge is scored
// from its one-line filter row first (|s~ - s| <= FILT_EPS), and only the CANDIDATES
//        s~ >= thr - eps   and   fewer than top_k edges with s~' > s~ + 2 eps
// are fetched and scored in fp32: every edge of the exact selection is a candidate (the filter header's
// argument), the exact rule then runs on the candidates' exact scores, so indices, weights, ranks and kept
// bits are those of the unfiltered set, bit for bit.
template <int VEC, int G, int R, int EPI, typename SRC>
__device__ __forceinline__ void small_rows_set_filt(const FwdArgs &a, const SRC &src, const int4 d, bool valid,
                                                    int *lds_wave, const int *s_col_set)
{
    static_assert(G >= SMALL_T, "one lane per edge of a small row");
    using RowT = Row<VEC, G, R>;
    constexpr int U = Unroll<R>::U;
    constexpr int UF = (R == 1) ? 4 : 2;                 // filter rows in flight per lane group
    constexpr int SETW = WaveLds<G>::SETW;
    constexpr int FR = G * R;                            // 8-byte lane entries per filter row
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const int i = d.x, rs = d.y, deg = d.z;
    const bool emit = a.sel_src != nullptr;
    const bool rank = deg > a.k;                         // (a.k >= 0: the filter belongs to selecting calls)
    const bool need_sc = rank || emit;
    const int self = i + a.row_off;

    const int *s_col = s_col_set + gid * SMALL_T;
    float *s_sc = reinterpret_cast<float *>(lds_wave + 2 * SETW) + gid * SMALL_T;   // approximate, then exact scores
    float *s_w = reinterpret_cast<float *>(lds_wave + 3 * SETW) + gid * SMALL_T;    // kept weights
    int *s_c = reinterpret_cast<int *>(s_w);                                        // (before that: candidate edges)

    uint2 fi[R];
#pragma unroll
    for (int q = 0; q < R; ++q) fi[q] = src.template filt<uint2>(self, FR, q * G + lg);
    const int dmax = wave_max_i(deg);

    // phase 1: approximate scores of all edges from the filter rows
    for (int t0 = 0; t0 < dmax; t0 += UF) {
        uint2 x[UF][R];
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const bool live = (t0 + u) < deg;
            const int j = src.pick(live, s_col[t0 + u], self);
#pragma unroll
            for (int q = 0; q < R; ++q) x[u][q] = src.template filt_if<uint2>(j, live, FR, q * G + lg);
        }
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            float pr = 0.f;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                pr = __builtin_amdgcn_fdot2(__builtin_bit_cast(half2_t, fi[q].x), __builtin_bit_cast(half2_t, x[u][q].x), pr, false);
                pr = __builtin_amdgcn_fdot2(__builtin_bit_cast(half2_t, fi[q].y), __builtin_bit_cast(half2_t, x[u][q].y), pr, false);
            }
            const float sa = group_sum<G>(pr) * FILT_UNSCALE;
            if (t0 + u < deg && lg == 0) s_sc[t0 + u] = sa;
        }
    }
    wave_lds_sync();

    // phase 2: lane lg decides edge lg
    const bool has = lg < deg;
    const float sa = has ? s_sc[lg] + 0.0f : -INFINITY;
    const float lo = a.thr - FILT_EPS;
    bool cand = has && sa >= lo;
    if (cand && rank) {
        int above = 0;
        for (int b = 0; b < deg; ++b) {
            const float sb = s_sc[b];
            above += (sb >= lo) && (sb > sa + 2.0f * FILT_EPS);
        }
        cand = above < a.k;
    }
    const unsigned long long gm = fwd_group_bits<G>(__ballot(cand), gid);
    const int nc = __popcll(gm);
    wave_lds_sync();                                          // (every s_sc read above is done)
    if (cand) s_c[__popcll(gm & ((1ull << lg) - 1ull))] = lg;
    if (has && !cand) {
        s_sc[lg] = -INFINITY;                                 // never selected, ranks below every candidate
        if (!need_sc && a.wsel) a.wsel[rs + lg] = SNGNN_UNSELECTED;
    }
    wave_lds_sync();

    // phase 3: the candidates' fp32 rows and exact scores
    RowT acc;
    acc.zero();
    unsigned kb = 0u;
    const int ncmax = wave_max_i(nc);
    // (the row's own fp32 unit row only now, with the first candidates' rows: a set without candidates - most
    // sets behind a threshold that prunes - touches one-line filter rows only)
    RowT ni;
    if (ncmax > 0) src.row(ni, self);
    else ni.zero();
    for (int q0 = 0; q0 < ncmax; q0 += U) {
        RowT x[U];
        float nj[U];
        int e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            e[u] = (q0 + u) < nc ? s_c[q0 + u] : -1;
            const bool live = e[u] >= 0;
            const int j = src.pick(live, s_col[live ? e[u] : 0], self);
            src.row_if(x[u], j, live);
            nj[u] = src.nrm_unless(j, live, need_sc);         // a streaming row weighs the row it has just scored
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float sx = unit_dot<VEC, G, R>(ni, x[u]);
            if (e[u] >= 0) {
                if (need_sc) {
                    if (lg == 0) s_sc[e[u]] = sx;
                } else {
                    const bool sel = sx >= a.thr;
                    if (sel) acc.axpy(sx * nj[u], x[u]);
                    if (a.wsel && lg == 0) a.wsel[rs + e[u]] = sel ? sx : SNGNN_UNSELECTED;
                    kb |= sel ? (1u << e[u]) : 0u;
                }
            }
        }
    }
    if (a.inv_norm && valid && lg == 0) a.inv_norm[i] = ieee_div(1.0f, src.nrm(self));

    if (need_sc) {
        wave_lds_sync();
        // phase 4: the exact rule on the exact scores (non-candidates hold -inf) - the unfiltered set's code
        for (int e = lg; e < deg; e += G) {
            const float se = s_sc[e];
            int rk = 0;
            for (int b = 0; b < deg; ++b) {
                const float sb = s_sc[b];
                rk += (sb > se) || (sb == se && b < e);
            }
            const bool sel = rk < a.k && se >= a.thr;
            s_w[e] = sel ? se : SNGNN_UNSELECTED;
            if (a.wsel) a.wsel[rs + e] = sel ? se : SNGNN_UNSELECTED;
            if (a.kbits) kb |= (unsigned)fwd_group_bits<G>(__ballot(sel), gid) << (e - lg);
            if (emit && sel) {
                a.sel_src[(size_t)i * a.k + rk] = s_col[e];
                a.sel_w[(size_t)i * a.k + rk] = se;
            }
        }
        wave_lds_sync();
        // the kept rows again (they were candidates a moment ago: cache-hot), in edge order
        for (int t = 0; t < deg; ++t) {
            const float w = s_w[t];
            if (w != SNGNN_UNSELECTED) {
                const int j = s_col[t];
                RowT xr;
                src.row(xr, j);
                acc.axpy(w * src.nrm(j), xr);
            }
        }
        wave_lds_sync();       // s_sc / s_w are reused by the next set
    }
    if (a.kbits && valid && lg == 0) reinterpret_cast<unsigned short *>(a.kbits)[i] = (unsigned short)kb;
    if (valid) {
        acc.div((float)max(deg, 1));
        if constexpr (EPI == 1) row_epilogue<VEC, G, R>(a, acc, i, lg);
        acc.store(a.out + (size_t)i * a.C, a.C, lg);
    }
}

// ---------------------------------------------------------------------------
// Class C driver: waves are persistent, each walks sets wave_id, wave_id + n_waves, ...
// and keeps the NEXT set's descriptors and column ids in flight while it works on the
// current one, so a set costs one memory round trip (its feature rows) instead of a
// chain of three (descriptor -> columns -> rows).
// ---------------------------------------------------------------------------
template <int VEC, int G, int R, bool OTF, int EPI, bool FS, typename S, bool LEAN, typename SRC>
__device__ __forceinline__ void role_small(const FwdArgs &a, const SRC &src, int set0, int stride, int nsets, int *lds_wave)
{
    constexpr int RPW = 64 / G;
    constexpr int CPL = (RPW * SMALL_T + 63) / 64;      // column ids per lane per set
    constexpr int SETW = WaveLds<G>::SETW;
    const int lane = lane_id();
    const int gid = lane / G;

    auto load_desc = [&](int st) -> int4 {
        const int slot = a.n_med_end + st * RPW + gid;
        int4 d = src.desc_if(slot, st < nsets && slot < a.N);
        if (!LEAN && a.row_flag != nullptr && d.w >= 0 && a.skip_row(d.x)) d = make_int4(0, 0, 0, -1);   // not this pass's row
        return d;
    };
    // lane l fetches column ids q = l + 64 m of the set: row q / SMALL_T, edge q % SMALL_T
    auto load_cols = [&](const int4 d, int (&c)[CPL]) {
#pragma unroll
        for (int m = 0; m < CPL; ++m) {
            const int q = lane + 64 * m;
            const int r = q / SMALL_T, t = q % SMALL_T;
            // descriptor of row r of the set lives in the lanes of group r
            const int rss = __shfl(d.w, r * G, 64), dg = __shfl(d.z, r * G, 64);
            c[m] = src.col_s_if(rss + t, r < RPW && t < dg);        // consecutive slots: one stream
        }
    };
    auto store_cols = [&](const int (&c)[CPL], int *dst) {
#pragma unroll
        for (int m = 0; m < CPL; ++m) {
            const int q = lane + 64 * m;
            if (q < RPW * SMALL_T) dst[q] = c[m];
        }
    };

    int s_cur = set0;
    if (s_cur >= nsets) return;
    int s_nxt = s_cur + stride;
    // two [RPW][SMALL_T] column-id buffers at lds_wave + SETW * buf.  (Plain pointer arithmetic:
    // an array of the two pointers loses the LDS address space and every read of a column
    // id becomes a FLAT load, which must drain the whole memory pipeline - s_waitcnt
    // vmcnt(0) - in the middle of a batch of row gathers.)
    int4 d_cur = load_desc(s_cur);
    int4 d_nxt = load_desc(s_nxt);
    int cols[CPL];
    load_cols(d_cur, cols);
    store_cols(cols, lds_wave);
    int buf = 0;
    while (s_cur < nsets) {
        const int s_n2 = s_nxt + stride;
        const int4 d_n2 = load_desc(s_n2);
        load_cols(d_nxt, cols);                 // in flight during this set's work
        wave_lds_sync();
        if (LEAN || a.row_flag == nullptr || __ballot(d_cur.w >= 0) != 0ull) {
            bool done = false;
            if constexpr (FS && G >= SMALL_T && !OTF) {
                if (a.filt_small) {                               // (uniform)
                    small_rows_set_filt<VEC, G, R, EPI>(a, src, d_cur, d_cur.w >= 0, lds_wave, lds_wave + SETW * buf);
                    done = true;
                }
            }
            if (!done) small_rows_set<VEC, G, R, OTF, EPI, S, LEAN>(a, src, d_cur, d_cur.w >= 0, lds_wave, lds_wave + SETW * buf);
        }
        store_cols(cols, lds_wave + SETW * (buf ^ 1));
        d_cur = d_nxt;
        d_nxt = d_n2;
        s_cur = s_nxt;
        s_nxt = s_n2;
        buf ^= 1;
    }
}

// ---------------------------------------------------------------------------
// Scoring pass shared by classes A and B: the wave's 64/G groups stride over
// the edges [e0, e1) of row i (row-local indices).
//   STREAM: accumulate kept rows into acc (threshold only) and write wsel
//   sc: where to put the scores (LDS or HBM scratch - every CALL SITE passes one kind only: a
//           pointer that is LDS on one path and HBM on another becomes FLAT, and FLAT accesses
//           wait for vmcnt(0), i.e. drain the gathers in flight), or nullptr; edge t goes to
//           sc[t - sc_off]  (never form an out-of-range LDS pointer: LDS pointer
//           arithmetic is 32-bit and does not survive the cast to a flat address)
// ---------------------------------------------------------------------------
//   OTF: ni is the RAW target row, inv_i its fast inverse norm.  Scores are the fast cosine,
//           except: a streaming edge within delta of thr is scored exactly; with exact_all EVERY
//           edge is (the paths that rank from scores in HBM scratch: top_k > CAND_MAX_K, hubs
//           beyond the candidate finalize, ranks of a streaming split row).
//   MODE: SCORE_ANY = all of the above decided at run time (wave-uniform tests, per slot); the lean kernel's call sites
//           say what they know at compile time - SCORE_STREAM: stream, no scores kept (sc, ids_lds unused; no wsel);
//           SCORE_KEEP: scores to sc (and ids to ids_lds when WITH_IDS), nothing accumulated, no norm loaded - so the
//           norm load of a slot joins its row load without a branch region between them.
enum { SCORE_ANY = 0, SCORE_STREAM = 1, SCORE_KEEP = 2 };
template <int VEC, int G, int R, bool OTF, typename S, int MODE = SCORE_ANY, bool WITH_IDS = false, typename SRC>
__device__ __forceinline__ void score_edges(const FwdArgs &a, const SRC &src, int self, int rs, int e0, int e1,
                                            const Row<VEC, G, R> &ni, float inv_i, bool stream,
                                            float *sc, int sc_off, Row<VEC, G, R> &acc,
                                            int *ids_lds = nullptr, bool exact_all = false)
{
    static_assert(MODE == SCORE_ANY || !OTF, "the compile-time modes: table mode");
    if constexpr (MODE == SCORE_STREAM) stream = true;
    if constexpr (MODE == SCORE_KEEP) stream = false;
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    constexpr int U = Unroll<R>::U;
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    RowT nu;                                   // OTF + exact_all: the unit target row
    if constexpr (OTF) {
        if (exact_all) { nu = ni; normalize_in_place<VEC, G, R>(nu); }
    }
    // column ids one iteration ahead: the col -> row dependency of iteration n+1
    // overlaps the row loads of iteration n
    int jn[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t = e0 + u * NG + gid;
        jn[u] = src.col_if(rs + t, t < e1, self);
    }
    for (int base = e0; base < e1; base += NG * U) {
        int t[U], j[U];
        bool act[U];
        RowT x[U];
        float nj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            t[u] = base + u * NG + gid;
            act[u] = t[u] < e1;
            j[u] = jn[u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            src.row_if(x[u], j[u], act[u]);
            if constexpr (OTF) nj[u] = 1.f;
            else nj[u] = stream ? src.nrm_if(j[u], act[u]) : 0.f;       // (stream: wave-uniform)
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int tn = t[u] + NG * U;
            jn[u] = src.col_if(rs + tn, tn < e1, self);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s;
            if constexpr (OTF) {
                if (exact_all) {
                    s = exact_score_raw<VEC, G, R>(nu, x[u]);
                } else {
                    s = edge_score<VEC, G, R>(ni, inv_i, x[u]);
                    if (stream && a.k >= 0) {
                        const bool amb = act[u] && fabsf(s - a.thr) <= a.delta;
                        if (__ballot(amb) != 0ull) {             // (wave-uniform; rare)
                            RowT nt = ni;
                            normalize_in_place<VEC, G, R>(nt);
                            const float se = exact_score_raw<VEC, G, R>(nt, x[u]);
                            if (amb) s = se;
                        }
                    }
                }
            } else {
                s = unit_dot<VEC, G, R>(ni, x[u]);
            }
            if constexpr (MODE == SCORE_STREAM) {
                if (act[u] && ((a.k < 0) || (s >= a.thr))) acc.axpy(s * nj[u], x[u]);
                continue;
            }
            if constexpr (MODE == SCORE_KEEP) {
                if (act[u] & (lg == 0)) {
                    sc[t[u] - sc_off] = s;
                    if constexpr (WITH_IDS) ids_lds[t[u] - sc_off] = j[u];
                }
                continue;
            }
            if (act[u]) {
                if (sc && lg == 0) sc[t[u] - sc_off] = s;
                if (ids_lds && lg == 0) ids_lds[t[u] - sc_off] = j[u];      // for the re-gather of the kept rows
                if (stream) {
                    const bool sel = (a.k < 0) || (s >= a.thr);
                    if (sel) acc.axpy(s * nj[u], x[u]);
                    if (a.wsel && lg == 0) a.wsel[rs + t[u]] = sel ? s : SNGNN_UNSELECTED;
                }
            }
        }
    }
}

// Exact scores of the listed edges (list[q] = chunk-local edge index, ids[idx] = its source):
// sc[idx] = <n_i, n_j>.  U rows per lane group in flight; a slot past the end repeats the
// last listed edge and stores nothing.
// (OTF: ni is the UNIT target row, the listed rows are raw and are normalised in registers)
template <int VEC, int G, int R, bool OTF, typename S, typename SRC>
__device__ __forceinline__ void score_list(const SRC &src, const Row<VEC, G, R> &ni, const int *list, int ncand,
                                           const int *ids, float *sc)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
#ifndef SNGNN_LIST_U
#define SNGNN_LIST_U 1
#endif
    constexpr int U = Unroll<R>::U * (R == 1 ? SNGNN_LIST_U : 1);     // the usual k + a few candidates: one trip
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    for (int q0 = 0; q0 < ncand; q0 += NG * U) {
        RowT x[U];
        int idx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * NG + gid;
            idx[u] = list[min(q, ncand - 1)];
            src.row(x[u], ids[idx[u]]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s;
            if constexpr (OTF) s = exact_score_raw<VEC, G, R>(ni, x[u]);
            else s = unit_dot<VEC, G, R>(ni, x[u]);
            if (q0 + u * NG + gid < ncand && lg == 0) sc[idx[u]] = s;
        }
    }
}

// "Score the edges [e0, e1) of a ranking row and select" in two precisions: approximate scores
// of all n = e1 - e0 <= 128 edges, exact scores of the CANDIDATES only - the edges within
// 2 eps of the top_k-th approximate score and not below thr - eps, where eps bounds
// |approximate - exact| (agg_fwd_filter.h has the argument) - and the exact selection among them.
//   FILT: approximate = fp16 filter rows (eps = FILT_EPS), exact = table rows;
//   OTF:  approximate = the fast cosine of the raw rows (eps = a.delta), exact = rows normalised
//         in registers; ni = raw target row, inv_i its fast inverse norm.
// On return sc[t] holds the exact score of every candidate (in particular of every kept edge),
// ids[t] the source of every edge, and the returned keys / flags are what wave_select would have
// given on exact scores of all edges.  list[] is scratch.
//   OTF, optimistic = true: the selection is first made on the fast scores alone and kept when it
//         is beyond doubt - no edge within delta of thr, and the weakest kept edge more than
//         2 delta above the strongest valid edge left out (then the exact scores would select
//         the same set; the kept edges' weights are the fast values, within delta of the exact
//         ones).  Only a row that fails this test - ties and near ties at the cut - takes the
//         candidate path.  (Not for split-row tasks: their keys are merged with other tasks'
//         keys by the finalize, which needs them exact; not when ranks are emitted.)
template <int VEC, int G, int R, bool OTF, typename S, typename SRC>
__device__ __forceinline__ WaveSel banded_select(const FwdArgs &a, const SRC &src, const Row<VEC, G, R> &ni, float inv_i, int self,
                                                 int rs, int e0, int e1, float *sc, int *list, int *ids, int lowbits,
                                                 bool optimistic = false)
{
    using RowT = Row<VEC, G, R>;
    const int lane = lane_id();
    const int n = e1 - e0;
    float eps;
    if constexpr (OTF) {
        RowT unused;
        unused.zero();
        score_edges<VEC, G, R, true, S>(a, src, self, rs, e0, e1, ni, inv_i, false, sc, e0, unused, ids);
        eps = a.delta;
    } else {
        constexpr int GF = G * R / 2;                // 16-byte lanes per filter row (VEC == 4)
        filter_scores<GF>(src, self, rs, e0, e1, sc, ids);
        eps = FILT_EPS;
    }
    wave_lds_sync();
    if constexpr (OTF) {
        if (optimistic) {
            const int i0 = lane, i1 = lane + 64;
            const float f0 = i0 < n ? sc[i0] + 0.0f : 0.f, f1 = i1 < n ? sc[i1] + 0.0f : 0.f;
            WaveSel r;
            r.key0 = (i0 < n && f0 >= a.thr) ? sel_key(f0, e0 + i0) : 0ull;
            r.key1 = (i1 < n && f1 >= a.thr) ? sel_key(f1, e0 + i1) : 0ull;
            wave_topk_keys(r.key0, r.key1, a.k, lowbits, r.kept0, r.kept1);
            bool doubt = (i0 < n && fabsf(f0 - a.thr) <= eps) || (i1 < n && fabsf(f1 - a.thr) <= eps);
            // weakest kept against strongest valid edge left out
            float kmin = fminf(r.kept0 ? f0 : INFINITY, r.kept1 ? f1 : INFINITY);
            float umax = fmaxf((r.key0 != 0ull && !r.kept0) ? f0 : -INFINITY, (r.key1 != 0ull && !r.kept1) ? f1 : -INFINITY);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                kmin = fminf(kmin, __shfl_xor(kmin, m, 64));
                umax = fmaxf(umax, __shfl_xor(umax, m, 64));
            }
            doubt = doubt || (kmin - umax <= 2.0f * eps);      // (umax = -inf: nothing was left out)
            if (__ballot(doubt) == 0ull) return r;
        }
    }
    bool c0, c1;
    approx_candidates(sc, n, a.k, a.thr, eps, c0, c1);
    const unsigned long long m0 = __ballot(c0), m1 = __ballot(c1);
    const int n0 = __popcll(m0), ncand = n0 + __popcll(m1);
    if (c0) list[prefix_popc(m0)] = lane;
    if (c1) list[n0 + prefix_popc(m1)] = lane + 64;
    wave_lds_sync();
    if (ncand > 0) {
        if constexpr (OTF) {
            RowT nu = ni;
            normalize_in_place<VEC, G, R>(nu);
            score_list<VEC, G, R, true, S>(src, nu, list, ncand, ids, sc);
        } else {
            score_list<VEC, G, R, false, S>(src, ni, list, ncand, ids, sc);
        }
    }
    wave_lds_sync();
    WaveSel r;
    const float s0 = c0 ? sc[lane] : 0.f, s1 = c1 ? sc[lane + 64] : 0.f;
    r.key0 = (c0 && s0 >= a.thr) ? sel_key(s0, e0 + lane) : 0ull;
    r.key1 = (c1 && s1 >= a.thr) ? sel_key(s1, e0 + lane + 64) : 0ull;
    wave_topk_keys(r.key0, r.key1, a.k, lowbits, r.kept0, r.kept1);
    return r;
}

// ---------------------------------------------------------------------------
// Class B: SMALL_T < deg <= WAVE_T, one wave per row.
// ---------------------------------------------------------------------------
template <int VEC, int G, int R, bool FILT, bool OTF, int EPI, typename S, bool LEAN, typename SRC>
__device__ __forceinline__ void role_wave(const FwdArgs &a, const SRC &src, int item, int *lds_wave)
{
    static_assert(!LEAN || (!FILT && !OTF && EPI == 0), "the lean form: table mode, no filter, plain stores");
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const int slot = a.n_split + item;
    const int4 d = a.rdesc[slot];
    const int i = d.x, rs = d.y, deg = d.z;
    if (!LEAN && a.skip_row(i)) return;                     // (wave-uniform)
    const int self = i + a.row_off;
    const bool emit = !LEAN && a.sel_src != nullptr && a.k >= 0;
    const bool rank = a.k >= 0 && deg > a.k;
    const bool need_sc = rank || emit;

    float *s_sc = reinterpret_cast<float *>(lds_wave);     // [WAVE_T]
    int *s_list = lds_wave + WAVE_T;                         // [WAVE_T]
    int *s_ids = lds_wave + 2 * WAVE_T;                      // [WAVE_T]

    RowT ni;
    src.row(ni, self);
    float inv_i = 0.f, q_i = 0.f;
    if constexpr (OTF) {
        q_i = group_sum<G>(ni.dot_partial(ni));
        inv_i = inv_norm_of(q_i);
    }

    RowT acc;
    acc.zero();
    // two-precision selection: the filter for ranking rows; OTF whenever scores are kept (ranks
    // asked for on a streaming row included: their order needs exact scores too)
    const bool banded = OTF ? need_sc : (FILT && rank && deg >= a.filt_min_deg);
    if constexpr (LEAN) {
        // (need_sc == rank, never banded: which of the two passes this row takes is known here)
        if (rank) score_edges<VEC, G, R, false, S, SCORE_KEEP, true>(a, src, self, rs, 0, deg, ni, inv_i, false, s_sc, 0, acc, s_ids);
        else score_edges<VEC, G, R, false, S, SCORE_STREAM>(a, src, self, rs, 0, deg, ni, inv_i, true, nullptr, 0, acc);
    } else if (!banded)
        score_edges<VEC, G, R, OTF, S>(a, src, self, rs, 0, deg, ni, inv_i, !rank, need_sc ? s_sc : nullptr, 0, acc,
                                    rank ? s_ids : nullptr);

    if (need_sc) {
        WaveSel ws;
        if constexpr (FILT || OTF) {
            if (banded) {
                ws = banded_select<VEC, G, R, OTF, S>(a, src, ni, inv_i, self, rs, 0, deg, s_sc, s_list, s_ids, 7,
                                                   /*optimistic=*/OTF && !emit);
            } else {
                wave_lds_sync();
                ws = wave_select(s_sc, deg, 0, a.k, a.thr, 7);
            }
        } else {
            wave_lds_sync();
            ws = wave_select(s_sc, deg, 0, a.k, a.thr, 7);
        }
        const int i0 = lane, i1 = lane + 64;
        // kept list in ascending position order
        const unsigned long long m0 = __ballot(ws.kept0), m1 = __ballot(ws.kept1);
        const int n0 = __popcll(m0);
        if (ws.kept0) s_list[prefix_popc(m0)] = i0;
        if (ws.kept1) s_list[n0 + prefix_popc(m1)] = i1;
        const int nsel = n0 + __popcll(m1);
        if (!LEAN && (rank || banded) && a.wsel) {
            if (i0 < deg) a.wsel[rs + i0] = ws.kept0 ? s_sc[i0] : SNGNN_UNSELECTED;
            if (i1 < deg) a.wsel[rs + i1] = ws.kept1 ? s_sc[i1] : SNGNN_UNSELECTED;
        }
        if constexpr (!OTF && !LEAN)
            if (a.kbits && lane < 4)          // the row's 128 kept bits at its slot
                a.kbits[a.kb_wbase + 4 * item + lane] = (unsigned)((lane < 2 ? m0 : m1) >> (32 * (lane & 1)));
        wave_lds_sync();
        if (emit) {
            // rank of a kept edge = number of keys above it
            for (int q = 0; q < nsel; ++q) {
                const int idx = s_list[q];
                const unsigned long long kq = sel_key(s_sc[idx], idx);
                const int rk = __popcll(__ballot(ws.key0 > kq)) + __popcll(__ballot(ws.key1 > kq));
                if (lane == 0) {
                    a.sel_src[(size_t)i * a.k + rk] = a.col[rs + idx];
                    a.sel_w[(size_t)i * a.k + rk] = s_sc[idx];
                }
            }
        }
        if ((rank || banded) && nsel > 0) {
            // the kept rows again, U per lane group in flight, unconditionally (a slot past the
            // end repeats the last kept edge with weight 0): their column ids wait in LDS, so
            // this is ONE memory round trip instead of a col -> row chain per kept edge
            constexpr int U = Unroll<R>::U;
            for (int q0 = 0; q0 < nsel; q0 += U * NG) {
                RowT x[U];
                float w[U], nj[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int q = q0 + u * NG + gid;
                    const int idx = s_list[min(q, nsel - 1)];
                    const int j = s_ids[idx];
                    w[u] = q < nsel ? s_sc[idx] : 0.f;
                    src.row(x[u], j);
                    if constexpr (OTF) nj[u] = 1.f;
                    else nj[u] = src.nrm(j);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) acc.axpy(w[u] * nj[u], x[u]);
            }
        }
    }
    acc.reduce_across_groups();
    if (gid == 0) {
        acc.div((float)deg);
        if constexpr (EPI == 1) row_epilogue<VEC, G, R>(a, acc, i, lg);
        acc.store(a.outs<S>() + (size_t)i * a.C, a.C, lg);
    }
    // (stored at the END of the row: a store up front would pin the scoring pass's first
    // column-id loads behind it - the pointers are not restrict)
    if (!LEAN && lane == 0 && a.inv_norm) {
        if constexpr (OTF) a.inv_norm[i] = ieee_div(1.0f, fmaxf(ieee_sqrt(q_i), EPS_NORM));
        else a.inv_norm[i] = ieee_div(1.0f, src.nrm(self));
    }
    wave_lds_sync();            // the wave's LDS scratch is reused by its next item
}

// ---------------------------------------------------------------------------
// Class A: one CHUNK-edge task of a split row.
// ---------------------------------------------------------------------------
// FIN: the row's finalize runs in THIS launch (fin_block_pair / fin_group_batch / fin_stream_row) - what it reads
// or overwrites is stored at agent scope, then the task says "done".  The launches whose finalize is the next
// launch run the FIN = false instantiation: plain stores, the code of round 4.
template <int VEC, int G, int R, bool FILT, bool OTF, bool FIN, typename S, bool LEAN, typename SRC>
__device__ __forceinline__ void role_task(const FwdArgs &a, const SRC &src, int tq, int *lds_wave)
{
    using RowT = Row<VEC, G, R>;
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const int p = a.task_slot[tq], c = a.task_chunk[tq];
    const int4 d = a.rdesc[p];
    const int i = d.x, rs = d.y, deg = d.z;
    static_assert(!LEAN || (!FILT && !OTF), "the lean form: table mode, no filter");
    if (!LEAN && a.skip_row(i)) return;                     // (wave-uniform)
    const int self = i + a.row_off;
    const int e0 = c * CHUNK, e1 = min(deg, e0 + CHUNK);
    const bool emit = !LEAN && a.sel_src != nullptr && a.k >= 0;
    const bool rank = a.k >= 0 && deg > a.k;
    const bool cand = rank && a.use_cand;        // chunk-local top-k -> candidates

    RowT ni;
    src.row(ni, self);
    float inv_i = 0.f;
    if constexpr (OTF) {
        const float q_i = group_sum<G>(ni.dot_partial(ni));
        inv_i = inv_norm_of(q_i);
        if (c == 0 && lane == 0 && a.inv_norm) a.inv_norm[i] = ieee_div(1.0f, fmaxf(ieee_sqrt(q_i), EPS_NORM));
    } else {
        if (!LEAN && c == 0 && lane == 0 && a.inv_norm) a.inv_norm[i] = ieee_div(1.0f, src.nrm(self));
    }

    RowT acc;
    acc.zero();
    float *s_sc = reinterpret_cast<float *>(lds_wave);          // [CHUNK], chunk-local
    float *sc_glb = (!cand && (rank || emit)) ? a.scores + a.split_soff[p] : nullptr;   // HBM scratch
    if constexpr (LEAN) {
        // (which pass a task takes is known here: candidates' scores to LDS, a ranking row's to the HBM scratch, or
        // a streaming row's sum)
        if (cand) score_edges<VEC, G, R, false, S, SCORE_KEEP>(a, src, self, rs, e0, e1, ni, inv_i, false, s_sc, e0, acc);
        else if (rank) score_edges<VEC, G, R, false, S, SCORE_KEEP>(a, src, self, rs, e0, e1, ni, inv_i, false, sc_glb, 0, acc);
        else score_edges<VEC, G, R, false, S, SCORE_STREAM>(a, src, self, rs, e0, e1, ni, inv_i, true, nullptr, 0, acc);
    }
    else if ((FILT || OTF) && cand) { /* scored below, in two precisions */ }
    else if (cand) score_edges<VEC, G, R, OTF, S>(a, src, self, rs, e0, e1, ni, inv_i, !rank, s_sc, e0, acc);   // LDS
    // HBM scratch (ranked later from those scores: OTF writes exact ones) / none (pure streaming)
    else score_edges<VEC, G, R, OTF, S>(a, src, self, rs, e0, e1, ni, inv_i, !rank, sc_glb, 0, acc, nullptr,
                                     /*exact_all=*/sc_glb != nullptr);
    if (cand) {
        WaveSel ws;
        if constexpr (FILT || OTF) {
            ws = banded_select<VEC, G, R, OTF, S>(a, src, ni, inv_i, self, rs, e0, e1, s_sc, lds_wave + CHUNK,
                                               lds_wave + 2 * CHUNK, a.lowbits);
        } else {
            wave_lds_sync();
            ws = wave_select(s_sc, e1 - e0, e0, a.k, a.thr, a.lowbits);
        }
        // (FIN: agent-scope stores - the row's finalize runs in another workgroup of THIS launch, on another XCD;
        // what it reads, and what it overwrites, must be in memory before the task says "done")
        auto put = [](auto *q, auto v) {
            if constexpr (FIN) st_agent(q, v);
            else *q = v;
        };
        unsigned long long *ck = a.cand_key + (size_t)tq * CAND_MAX_K;
        const unsigned long long m0 = __ballot(ws.kept0), m1 = __ballot(ws.kept1);
        const int n0 = __popcll(m0), nsel = n0 + __popcll(m1);
        if (ws.kept0) put(ck + prefix_popc(m0), ws.key0);
        if (ws.kept1) put(ck + n0 + prefix_popc(m1), ws.key1);
        if (lane >= nsel && lane < a.k) put(ck + lane, 0ull);          // empty slots (k <= 32 < 64)
        int32_t *cs = a.cand_src + (size_t)tq * CAND_MAX_K;       // saves the finalize a dependent load
        if (ws.kept0) put(cs + prefix_popc(m0), a.col[rs + e0 + lane]);
        if (ws.kept1) put(cs + n0 + prefix_popc(m1), a.col[rs + e0 + 64 + lane]);
        if (!LEAN && a.wsel) {     // the finalize overwrites the kept edges of the row
            float *w = a.wsel + rs + e0;
            if (lane < e1 - e0) put(w + lane, SNGNN_UNSELECTED);
            if (lane + 64 < e1 - e0) put(w + lane + 64, SNGNN_UNSELECTED);
        }
        if constexpr (!OTF && !LEAN)
            if (a.kbits && lane < 4) put(a.kbits + a.kb_tbase + 4 * tq + lane, 0u);      // the finalize sets the winners' bits
    } else if (!rank) {
        acc.reduce_across_groups();
        if constexpr (FIN) {
            if (gid == 0) {
                float *pr = a.partial + (size_t)tq * a.C;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if ((r * G + lg) * VEC < a.C) st_agent_vec<VEC>(pr + (r * G + lg) * VEC, acc.x[r]);
            }
        } else {
            if (gid == 0) acc.store(a.partial + (size_t)tq * a.C, a.C, lg);
        }
    }
    if constexpr (FIN) {
        if (cand || !rank) {                                      // (uniform) publish
            wave_vmem_drain();
            if (lane == 0) st_agent(a.fin_done + tq, a.fin_nonce);
        }
    }
    wave_lds_sync();            // the wave's LDS scratch is reused by its next item
}

// Persistent waves: wave w of the grid takes work items w, w + n_waves, ... of the
// list [split-row tasks | wave rows | small-row sets], each class in order of
// descending degree, so every wave gets a similar mix and the grid drains evenly.
// EPI: the hidden-layer store epilogue (FwdArgs::epilogue) compiled into the row stores - its own
// instantiation, so the plain forward keeps its register allocation (a runtime flag cost the
// filter variant two spilled registers and 2 us)
// FS: the filter also in front of the small rows (small_rows_set_filt) - its own instantiation: compiled into
// the plain FILT kernel it cost that kernel's other calls 2.5 us (41.8 against 39.3 us at top_k 1 / thr 0.99
// without the small-row form: six spilled registers)
// FIN: the launch's last workgroups finalize the split rows (role_task's note); its own instantiation, so the
// launches without the role run the kernel they ran before it existed
// BUF: the work-item roles read through buffer resources (agg_fwd_src.h; fp32 tables below 2 GiB - the launcher's rule,
// fwd_plan.h: fwd_buffer_form); false = the flat form.  The finalize role reads flat in both.
// LEAN: the call wants `out` and nothing else - wsel, inv_norm, sel_src, sel_w and kbits are NULL, no epilogue, no
// head, no row filter (the benchmark's call; every eval-mode forward of a model) - in table mode on fp32 rows without
// the fp16 filter (launch_agg_fwd_impl's rule).  What exists only for those outputs - kept-bit words, the stores and
// their address arithmetic, the selection lists, the wave-uniform tests of the pointers behind them, evaluated per
// slot - is compiled out of every role, the finalize role included, and the scoring loop knows at compile time which
// of its passes it is (score_edges: MODE).  The same arithmetic in the same order: the same bits as the general kernel
// (tests/test_fwd_lean_gpu.py); its own instantiation, so every other call runs the kernel it ran before.
// (Three further steps were built and measured on top of this and taken out again - select-based straight-line
// slots, the set's longest row by v_readlane, no division for power-of-two in-degrees: each made the launch with
// the finalize role slower or moved nothing; profiles/fwd_lean.txt has the series.)
template <int VEC, int G, int R, bool FILT, bool OTF, int EPI = 0, bool FS = false, bool FIN = false, typename S = float,
          bool BUF = false, bool LEAN = false>
__global__ __launch_bounds__(BLOCK, FWD_WAVES_PER_SIMD) void k_agg_fwd(const FwdArgs a)
{
    static_assert(!LEAN || (!FILT && !OTF && EPI == 0 && std::is_same<S, float>::value), "the lean form's domain");
    static_assert(!BUF || std::is_same<S, float>::value, "buffer-addressed reads: fp32 tables");
    static_assert(!(FILT && OTF), "the filter belongs to the table mode");
    static_assert(FILT || !FS, "the small-row filter belongs to the FILT kernel");
    static_assert(std::is_same<S, float>::value || (OTF && EPI == 0), "half rows: on the fly, no store epilogue");
    __shared__ __align__(16) int lds[WAVES][WaveLds<G>::WORDS];
    const int wave = threadIdx.x >> 6;
    int *lw = lds[wave];
    constexpr int RPW = 64 / G;
    const int nsets = (a.N - a.n_med_end + RPW - 1) / RPW;
    if constexpr (FIN) if ((int)blockIdx.x >= a.main_blocks) {                   // (workgroup-uniform) the finalize role
        // Its arguments through the kernel-argument segment itself, behind an opaque pointer: read through `a`,
        // the role's two dozen fields were loaded at the kernel's entry and held in scalar registers across the
        // OTHER roles (55-72 spilled scalars, 6-8 spilled vector registers, 60 bytes of scratch per lane in
        // every instantiation); this way they are loaded here, and the work-item roles compile as before.
        auto kp = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const FwdArgs &fa = *(const FwdArgs *)kp;             // (the kernel's only explicit argument: offset 0)
        const int nfb = (int)gridDim.x - fa.main_blocks, fb = (int)blockIdx.x - fa.main_blocks;
        bool dead = false, seen = false;
        if (fa.k < 0) {                                       // (uniform) nothing selected: sums of partial rows
            for (int p = fb * WAVES + wave; p < fa.n_split; p += nfb * WAVES)
                fin_stream_row<VEC, G, R, S>(fa, p, p + nfb * WAVES, dead, seen);
            return;
        }
        const int n_big = min(fa.n_split, fa.n_split_gt_wave);
        for (int p0 = 2 * fb; p0 < n_big; p0 += 2 * nfb) fin_block_pair<VEC, G, R, S, LEAN>(fa, p0, n_big, lds, dead);
        for (int pb = n_big + (fb * WAVES + wave) * RPW; pb < fa.n_split; pb += nfb * WAVES * RPW)
            fin_group_batch<VEC, G, R, S, LEAN>(fa, pb, pb + nfb * WAVES * RPW, lw, dead, seen);
        // (Small-row sets kept back for these waves to take behind their rows - 400 .. 1 600 of 40 383 - moved
        // nothing: 50.9-51.6 us against 51.0; the launch is 6 % slower than without the role's 96 workgroups, the
        // share of the chip's wave slots they hold.)
        return;
    }
    const FwdSrc<BUF, VEC, G, R, S> src(a, lane_id() % G);
    const int nw = a.main_blocks * WAVES;
    const int n_wave_rows = a.n_med_end - a.n_split;
    int it = blockIdx.x * WAVES + wave;
    for (; it < a.n_tasks; it += nw)
        if (a.role_mask & 1) role_task<VEC, G, R, FILT, OTF, FIN, S, LEAN>(a, src, a.task_order[it], lw);
    it -= a.n_tasks;
    for (; it < n_wave_rows; it += nw)
        if (a.role_mask & 2) role_wave<VEC, G, R, FILT, OTF, EPI, S, LEAN>(a, src, it, lw);
    it -= n_wave_rows;
    if (a.role_mask & 4) role_small<VEC, G, R, OTF, EPI, FS, S, LEAN>(a, src, it, nw, nsets, lw);
}

}  // namespace sngnn

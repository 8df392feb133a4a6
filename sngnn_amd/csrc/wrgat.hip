// Weighted relational graph attention (models.py:1903-2014, WeightedRGATConv after its linear maps) on the row classes
// of row_walk.h (gfx950, fp32, one GPU).  Edges carry a relation r in [0, R) and a weight w:
//     P [N, R, C],  P[n,r,:] = x[n] W_r,   s_dst[n,r] = <P[n,r], atten[r,:C]>,   s_src[n,r] = <P[n,r], atten[r,C:]>
//     per in-edge e = (j -> i, r, w):   raw_e = s_dst[i,r] + s_src[j,r],   a_e = leaky_relu(raw_e)
//     per segment (i, r) of n_ir edges: m = max a_e,  l = sum exp(a_e - m),  alpha_e = exp(a_e - m) / l
//     out[i] = sum_r (1 / n_ir) sum_{e in (i,r)} w_e alpha_e P[j,r,:]  +  self[i]  +  bias        (relu in the store)
// A non-empty segment holds the edge that attains its maximum: l >= 1 and the reference's + 1e-16 vanishes in fp32.
//
// The graph is built from the edge list sorted stably by relation (add_loops = 0, remove_loops = 0: every edge kept), so
// every CSR row is grouped by relation in ascending order and rel_ptr [N, R + 1] - offsets inside the row - names an
// entry's relation; n_ir is a difference of two of its elements.
//
// Forward:  the score pass of gat.hip (H = R), then
//   statistics  m, l [N, R] from a 4-byte gather per edge: a loop over the row's R segments, an xor butterfly over each;
//               split rows: 128-entry tasks write (m_t, l_t) [tasks, R], a finalize merges them in task order,
//               m = max m_t, l = sum l_t exp(m_t - m) - scalars only
//   gather      a plain weighted gather-sum: c_e = w_e exp(a_e - m_ir) / l_ir / n_ir formed per edge, ONLY the slice
//               P[j,r,:] the edge's relation names is fetched (4C bytes an edge), everything added into one C-wide
//               accumulator; root slice, bias and relu in the store.  Split rows: the tasks' partial rows are plain
//               sums (m and l are the row's final ones), added in task order by the finalize.
// Backward from G = grad_out (zeroed where a fused relu gave out <= 0), saved: P, the scores, m, l (and out for the relu):
//   pass T (in-edges)   t_e = <G_i, P[j,r]>  written per CSR entry (the one pass that fetches P's slices again)
//   pass D (scalars)    per segment A = sum alpha w t (= D_ir), B = sum alpha leaky' w t, K = sum alpha leaky':
//                       grad_s_dst[i,r] = (B - A K) / n_ir; split rows by tasks and a finalize, in task order
//   pass R (scalars)    {c_e = w alpha / n, da_e = alpha (w t - D) leaky' / n} written at the entry's CSC position
//   pass S (out-edges)  relations on gridDim.y: a workgroup serves one relation of its sources, reads every record and
//                       gathers G_i for the entries of its relation only: grad_P[j,r,:] = sum c_e G_i, grad_s_src[j,r] =
//                       sum da_e, and in the store += grad_s_src[j,r] atten[r,C:] + grad_s_dst[j,r] atten[r,:C]
//   grad_atten          gat.hip's per-workgroup partials in double and its reducer (workgroup order); grad_bias alike
// All six row-class kernels (k_wr_stats, k_wr_fwd, k_wr_bwd_t, k_wr_bwd_d, k_wr_bwd_rec, k_wr_bwd_s) decode their unit with
// row_walk.h's row_unit - the scalar passes at WR_SG lanes a small row -, the cohort reductions and leaky are
// device_utils.h's.  Every sum has a fixed order; no floating-point atomic, no host synchronisation.
#include "entry.h"
#include "row_walk.h"

namespace sngnn {

constexpr int WR_MAX_REL = 16;
constexpr int WR_SG = 16;                // lanes of a small row in the scalar passes (one per entry)

struct WrArgs : RowSide {          // the in-edges or, in pass S, the out-edges: row_walk.h
    const float *P;                // [N, R, C], rows ldp floats apart
    int64_t ldp;
    const float *self;             // forward: the root slice [N, C] (rows lds apart) or nullptr
    int64_t lds;
    const float *bias;             // [C] or nullptr
    const float *g;                // backward: the (masked) grad_out [N, C], rows ldg apart
    int64_t ldg;
    float *out;                    // forward: out [N, C] (ldo = C); pass S: grad_P [N, R, C] or nullptr
    int64_t ldo;
    const float *ssrc, *sdst;      // [N, R]
    float *m, *l;                  // [N, R]
    const int32_t *rel_ptr;        // [N, R + 1]
    const int32_t *rel_csc;        // [E] the relation of every CSC entry (pass S)
    const float *w;                // [E] in CSR order or nullptr (= 1)
    float *partial;                // forward [tasks, C]; pass S [stasks, R, C]
    float *ts;                     // [tasks, R, 3] task scalars: forward (m_t, l_t); pass D (A, B, K); pass S: sum da
    float *te;                     // [E] t_e in CSR order
    float *rec;                    // [E, 2] {c_e, da_e} in CSC order
    float *D, *gsrc, *gdst;        // [N, R]
    const float *atten;            // [R, 2C]
    float slope;
    int relu;
    int R, C, N;
    const int32_t *csc_pos;
};

// the relation of entry t of a row: the last r with rp[r] <= t (empty segments in between are skipped)
__device__ __forceinline__ int wr_rel(const int32_t *__restrict__ rp, int R, int t)
{
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rp[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// alpha_e of entry t of segment (seg, r)
__device__ __forceinline__ float wr_alpha(const WrArgs &a, size_t sr, int j, int r, float sd, float &raw)
{
    raw = a.ssrc[(size_t)j * a.R + r] + sd;
    return expf(leaky(raw, a.slope) - a.m[sr]) / a.l[sr];
}

// ---- forward: statistics ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(BLOCK) void k_wr_stats(const WrArgs a)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    bool wide;
    const RowUnit u = row_unit<WR_SG>(a, a.N, blockIdx.x, wave, lane / WR_SG, wide);
    const int32_t *rp = a.rel_ptr + (size_t)u.seg * (a.R + 1);
    const int P = wide ? 64 : WR_SG, p = wide ? lane : lane % WR_SG;
    for (int r = 0; r < a.R; ++r) {                                            // (R is uniform: the butterflies converge)
        const int s0 = max(u.e0, rp[r]), s1 = min(u.e1, rp[r + 1]);
        const float sd = a.sdst[(size_t)u.seg * a.R + r];
        float mx = -INFINITY;
        for (int t = s0 + p; t < s1; t += P)
            mx = fmaxf(mx, leaky(a.ssrc[(size_t)a.idx[u.qs + t] * a.R + r] + sd, a.slope));
        mx = wide ? cohort_max<64>(mx) : cohort_max<WR_SG>(mx);
        float s = 0.f;
        for (int t = s0 + p; t < s1; t += P)
            s += expf(leaky(a.ssrc[(size_t)a.idx[u.qs + t] * a.R + r] + sd, a.slope) - mx);
        s = wide ? cohort_sum<64>(s) : cohort_sum<WR_SG>(s);
        if (u.live && p == 0) {
            if (u.task) {
                a.ts[((size_t)u.tq * a.R + r) * 3] = mx;
                a.ts[((size_t)u.tq * a.R + r) * 3 + 1] = s;
            } else {
                a.m[(size_t)u.seg * a.R + r] = mx;                             // (an empty segment: -inf and 0, never read)
                a.l[(size_t)u.seg * a.R + r] = s;
            }
        }
    }
}

// split rows: the max-carrying merge of the tasks' (m_t, l_t) in task order
static __global__ void k_wr_stats_fin(const WrArgs a)
{
    const int p = blockIdx.x, r = threadIdx.x;
    if (r >= a.R) return;
    const int row = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    float m = -INFINITY;
    for (int t = t0; t < t1; ++t) m = fmaxf(m, a.ts[((size_t)t * a.R + r) * 3]);
    float l = 0.f;
    for (int t = t0; t < t1; ++t) {
        const float mt = a.ts[((size_t)t * a.R + r) * 3];
        if (mt != -INFINITY) l += a.ts[((size_t)t * a.R + r) * 3 + 1] * expf(mt - m);
    }
    a.m[(size_t)row * a.R + r] = m;
    a.l[(size_t)row * a.R + r] = l;
}

// ---- forward: the gather ---------------------------------------------------------------------------------------------
template <int VEC, int G, int RR> __global__ __launch_bounds__(BLOCK) void k_wr_fwd(const WrArgs a)
{
    using RowT = Row<VEC, G, RR>;
    constexpr int NG = 64 / G;
    constexpr int U = gather_unroll(RR);
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    bool wide;
    const RowUnit u = row_unit<G>(a, a.N, blockIdx.x, wave, gid, wide);
    const int32_t *rp = a.rel_ptr + (size_t)u.seg * (a.R + 1);
    const int stride = wide ? NG : 1, first = wide ? gid : 0;
    RowT acc;
    acc.zero();
    for (int b = u.e0 + first; b < u.e1; b += stride * U) {
        RowT x[U];
        float c[U];
        bool act[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int t = b + q * stride;
            act[q] = t < u.e1;
            const int j = act[q] ? a.idx[u.qs + t] : 0;
            const int r = act[q] ? wr_rel(rp, a.R, t) : 0;
            x[q].load(a.P + (size_t)j * a.ldp + (size_t)r * a.C, a.C, lg);
            const size_t sr = (size_t)u.seg * a.R + r;
            float raw;
            const float alpha = wr_alpha(a, sr, j, r, a.sdst[sr], raw);
            const float we = a.w && act[q] ? a.w[u.qs + t] : 1.f;
            c[q] = (we * alpha) / (float)(rp[r + 1] - rp[r]);
        }
#pragma unroll
        for (int q = 0; q < U; ++q)
            if (act[q]) acc.axpy(c[q], x[q]);
    }
    if (wide) acc.reduce_across_groups();
    if (!u.live || (wide && gid != 0)) return;
    if (u.task) {
        acc.store(a.partial + (size_t)u.tq * a.C, a.C, lg);
        return;
    }
    RowT e;
    if (a.self) {
        e.load(a.self + (size_t)u.seg * a.lds, a.C, lg);
        acc.add(e);
    }
    if (a.bias) {
        e.load(a.bias, a.C, lg);
        acc.add(e);
    }
    if (a.relu) {
#pragma unroll
        for (int s = 0; s < RR; ++s)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc.x[s][v] = fmaxf(acc.x[s][v], 0.f);
    }
    acc.store(a.out + (size_t)u.seg * a.ldo, a.C, lg);
}

// split rows: the tasks' partial rows in task order, then the store epilogue
static __global__ __launch_bounds__(256) void k_wr_fwd_fin(const WrArgs a)
{
    const int p = blockIdx.x;
    const int row = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    for (int c = threadIdx.x; c < a.C; c += 256) {
        float s = 0.f;
        for (int t = t0; t < t1; ++t) s += a.partial[(size_t)t * a.C + c];
        if (a.self) s += a.self[(size_t)row * a.lds + c];
        if (a.bias) s += a.bias[c];
        if (a.relu) s = fmaxf(s, 0.f);
        a.out[(size_t)row * a.ldo + c] = s;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------
// G with the fused relu's mask, rows ldd floats apart (the root slice's gradient is exactly this)
static __global__ __launch_bounds__(256) void k_wr_gmask(const float *__restrict__ g, const float *__restrict__ out,
                                                         int relu, int64_t NC, int C, float *__restrict__ dst, int64_t ldd)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    float v = g[i];
    if (relu && !(out[i] > 0.f)) v = 0.f;
    dst[(i / C) * ldd + i % C] = v;
}

// pass T.  The loops' bounds are wave-uniform (an inactive slot loads row 0 and is discarded): the group sums are
// never taken under divergence.
template <int VEC, int G, int RR> __global__ __launch_bounds__(BLOCK) void k_wr_bwd_t(const WrArgs a)
{
    using RowT = Row<VEC, G, RR>;
    constexpr int NG = 64 / G;
    constexpr int U = RR >= 2 ? 1 : 2;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    bool wide;
    const RowUnit u = row_unit<G>(a, a.N, blockIdx.x, wave, gid, wide);
    const int32_t *rp = a.rel_ptr + (size_t)u.seg * (a.R + 1);
    RowT gi;
    gi.load(a.g + (size_t)u.seg * a.ldg, a.C, lg);
    const int stride = wide ? NG : 1, first = wide ? gid : 0;
    const int e_end = wide ? u.e1 : wave_max_i(u.e1);          // (small rows: the longest row of the wave bounds the loop)
    for (int b = u.e0; b < e_end; b += stride * U) {
        RowT x[U];
        bool act[U];
        int t[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            t[q] = b + first + q * stride;
            act[q] = t[q] < u.e1;
            const int j = act[q] ? a.idx[u.qs + t[q]] : 0;
            const int r = act[q] ? wr_rel(rp, a.R, t[q]) : 0;
            x[q].load(a.P + (size_t)j * a.ldp + (size_t)r * a.C, a.C, lg);
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const float te = group_sum<G>(gi.dot_partial(x[q]));
            if (act[q] && lg == 0) a.te[u.qs + t[q]] = te;
        }
    }
}

// pass D: the three sums of a segment
static __global__ __launch_bounds__(BLOCK) void k_wr_bwd_d(const WrArgs a)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    bool wide;
    const RowUnit u = row_unit<WR_SG>(a, a.N, blockIdx.x, wave, lane / WR_SG, wide);
    const int32_t *rp = a.rel_ptr + (size_t)u.seg * (a.R + 1);
    const int P = wide ? 64 : WR_SG, p = wide ? lane : lane % WR_SG;
    for (int r = 0; r < a.R; ++r) {
        const int s0 = max(u.e0, rp[r]), s1 = min(u.e1, rp[r + 1]);
        const size_t sr = (size_t)u.seg * a.R + r;
        const float sd = a.sdst[sr];
        float A = 0.f, B = 0.f, K = 0.f;
        for (int t = s0 + p; t < s1; t += P) {
            float raw;
            const float alpha = wr_alpha(a, sr, a.idx[u.qs + t], r, sd, raw);
            const float wt = (a.w ? a.w[u.qs + t] : 1.f) * a.te[u.qs + t];
            const float al = raw > 0.f ? alpha : alpha * a.slope;
            A += alpha * wt;
            B += al * wt;
            K += al;
        }
        if (wide) { A = cohort_sum<64>(A); B = cohort_sum<64>(B); K = cohort_sum<64>(K); }
        else { A = cohort_sum<WR_SG>(A); B = cohort_sum<WR_SG>(B); K = cohort_sum<WR_SG>(K); }
        if (u.live && p == 0) {
            if (u.task) {
                float *ts = a.ts + ((size_t)u.tq * a.R + r) * 3;
                ts[0] = A; ts[1] = B; ts[2] = K;
            } else {
                const int n = rp[r + 1] - rp[r];
                a.D[sr] = A;
                a.gdst[sr] = n > 0 ? (B - A * K) / (float)n : 0.f;
            }
        }
    }
}

static __global__ void k_wr_bwd_d_fin(const WrArgs a)
{
    const int p = blockIdx.x, r = threadIdx.x;
    if (r >= a.R) return;
    const int row = a.perm[p];
    float A = 0.f, B = 0.f, K = 0.f;
    for (int t = a.split_task0[p]; t < a.split_task0[p + 1]; ++t) {
        const float *ts = a.ts + ((size_t)t * a.R + r) * 3;
        A += ts[0]; B += ts[1]; K += ts[2];
    }
    const int32_t *rp = a.rel_ptr + (size_t)row * (a.R + 1);
    const int n = rp[r + 1] - rp[r];
    a.D[(size_t)row * a.R + r] = A;
    a.gdst[(size_t)row * a.R + r] = n > 0 ? (B - A * K) / (float)n : 0.f;
}

// pass R: the records of pass S at the entries' CSC positions
static __global__ __launch_bounds__(BLOCK) void k_wr_bwd_rec(const WrArgs a)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    bool wide;
    const RowUnit u = row_unit<WR_SG>(a, a.N, blockIdx.x, wave, lane / WR_SG, wide);
    if (!u.live) return;
    const int32_t *rp = a.rel_ptr + (size_t)u.seg * (a.R + 1);
    const int P = wide ? 64 : WR_SG, p = wide ? lane : lane % WR_SG;
    for (int r = 0; r < a.R; ++r) {
        const int s0 = max(u.e0, rp[r]), s1 = min(u.e1, rp[r + 1]);
        const size_t sr = (size_t)u.seg * a.R + r;
        const float sd = a.sdst[sr], D = a.D[sr], n = (float)(rp[r + 1] - rp[r]);
        for (int t = s0 + p; t < s1; t += P) {
            float raw;
            const float alpha = wr_alpha(a, sr, a.idx[u.qs + t], r, sd, raw);
            const float we = a.w ? a.w[u.qs + t] : 1.f;
            const float ds = alpha * (we * a.te[u.qs + t] - D) / n;
            const float da = raw > 0.f ? ds : ds * a.slope;
            *reinterpret_cast<float2 *>(a.rec + (size_t)a.csc_pos[u.qs + t] * 2) = make_float2((we * alpha) / n, da);
        }
    }
}

// pass S over the out-edges (ptr / idx / perm are the CSC side's; the records are in its order), one relation
template <int VEC, int G, int RR> __global__ __launch_bounds__(BLOCK) void k_wr_bwd_s(const WrArgs a)
{
    using RowT = Row<VEC, G, RR>;
    constexpr int NG = 64 / G;
    constexpr int U = gather_unroll(RR);
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    const int r = blockIdx.y;
    bool wide;
    const RowUnit u = row_unit<G>(a, a.N, blockIdx.x, wave, gid, wide);
    const int stride = wide ? NG : 1, first = wide ? gid : 0;
    RowT acc;
    acc.zero();
    float sda = 0.f;
    for (int b = u.e0 + first; b < u.e1; b += stride * U) {
        RowT x[U];
        float2 rc[U];
        bool act[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int t = b + q * stride;
            const int e = t < u.e1 ? u.qs + t : -1;
            act[q] = e >= 0 && a.rel_csc[e] == r;
            const int ee = act[q] ? e : 0;
            x[q].load(a.g + (size_t)(act[q] ? a.idx[ee] : 0) * a.ldg, a.C, lg);
            rc[q] = *reinterpret_cast<const float2 *>(a.rec + (size_t)ee * 2);
        }
#pragma unroll
        for (int q = 0; q < U; ++q)
            if (act[q]) {
                acc.axpy(rc[q].x, x[q]);
                sda += rc[q].y;
            }
    }
    if (wide) {
        acc.reduce_across_groups();
        sda = cross_group_sum<G>(sda);
    }
    if (!u.live || (wide && gid != 0)) return;
    if (u.task) {
        acc.store(a.partial + ((size_t)u.tq * a.R + r) * a.C, a.C, lg);
        if (lg == 0) a.ts[(size_t)u.tq * a.R + r] = sda;
        return;
    }
    const size_t sr = (size_t)u.seg * a.R + r;
    if (lg == 0) a.gsrc[sr] = sda;
    if (a.out) {
        RowT w;
        w.load(a.atten + (size_t)r * 2 * a.C + a.C, a.C, lg);
        acc.axpy(sda, w);
        w.load(a.atten + (size_t)r * 2 * a.C, a.C, lg);
        acc.axpy(a.gdst[sr], w);
        acc.store(a.out + (size_t)u.seg * a.ldo + (size_t)r * a.C, a.C, lg);
    }
}

// split sources of pass S: the tasks' partial rows and sums in task order, then the store epilogue
static __global__ __launch_bounds__(256) void k_wr_bwd_s_fin(const WrArgs a)
{
    const int p = blockIdx.x, r = blockIdx.y;
    const int row = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const size_t sr = (size_t)row * a.R + r;
    float sda = 0.f;
    for (int t = t0; t < t1; ++t) sda += a.ts[(size_t)t * a.R + r];
    if (threadIdx.x == 0) a.gsrc[sr] = sda;
    if (!a.out) return;
    const float gd = a.gdst[sr];
    for (int c = threadIdx.x; c < a.C; c += 256) {
        float s = 0.f;
        for (int t = t0; t < t1; ++t) s += a.partial[((size_t)t * a.R + r) * a.C + c];
        s += sda * a.atten[(size_t)r * 2 * a.C + a.C + c];
        s += gd * a.atten[(size_t)r * 2 * a.C + c];
        a.out[(size_t)row * a.ldo + (size_t)r * a.C + c] = s;
    }
}

// grad_bias: workgroup b's column sums over its npb rows, in double; then the partials in workgroup order
static __global__ __launch_bounds__(256) void k_wr_bias_part(const float *__restrict__ g, int64_t ldg, int N, int C,
                                                             int npb, double *__restrict__ part)
{
    const int n0 = blockIdx.x * npb, n1 = min(N, n0 + npb);
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int n = n0; n < n1; ++n) s += (double)g[(size_t)n * ldg + c];
        part[(size_t)blockIdx.x * C + c] = s;
    }
}

static __global__ __launch_bounds__(256) void k_wr_bias_red(const double *__restrict__ part, int B, int C,
                                                            float *__restrict__ gbias)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += part[(size_t)b * C + c];
    gbias[c] = (float)s;
}

// ---- host ------------------------------------------------------------------------------------------------------------
template <int VEC, int G, int RR> int launch_wr_fwd(WrArgs a, hipStream_t st)
{
    const int nb = plan_side(a, a.N, 64 / G);
    if (nb > 0) k_wr_fwd<VEC, G, RR><<<nb, BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_wr_fwd_fin<<<a.n_split, 256, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <int VEC, int G, int RR> int launch_wr_bwd_t(WrArgs a, hipStream_t st)
{
    const int nb = plan_side(a, a.N, 64 / G);
    if (nb > 0) k_wr_bwd_t<VEC, G, RR><<<nb, BLOCK, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <int VEC, int G, int RR> int launch_wr_bwd_s(WrArgs a, hipStream_t st)
{
    const int nb = plan_side(a, a.N, 64 / G);
    if (nb > 0) k_wr_bwd_s<VEC, G, RR><<<dim3(nb, a.R), BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_wr_bwd_s_fin<<<dim3(a.n_split, a.R), 256, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

SNGNN_DEFINE_DISPATCH(dispatch_wr_fwd, launch_wr_fwd, WrArgs)
SNGNN_DEFINE_DISPATCH(dispatch_wr_bwd_t, launch_wr_bwd_t, WrArgs)
SNGNN_DEFINE_DISPATCH(dispatch_wr_bwd_s, launch_wr_bwd_s, WrArgs)

// workspace regions (256-byte aligned): the tasks' partial rows of either side | three scalars per task and relation |
// t_e | the records | D, grad_s_src, grad_s_dst | the masked G of a layer without a root slice | the f64 partials of
// grad_atten and of grad_bias
struct WrLayout { int64_t ts, te, rec, D, gsrc, gdst, gm, att, bpart, total; };

static WrLayout wr_layout(const sngnn_graph_t *g, int R, int C)
{
    WrLayout L;
    const int64_t tasks = std::max(g->n_tasks, g->n_stasks), B = gat_att_blocks(g->N);
    L.ts = up256(std::max<int64_t>((int64_t)g->n_tasks * C, (int64_t)g->n_stasks * R * C) * 4);
    L.te = L.ts + up256(tasks * R * 3 * 4);
    L.rec = L.te + up256(g->Ep * 4);
    L.D = L.rec + up256(g->Ep * 2 * 4);
    L.gsrc = L.D + up256(g->N * R * 4);
    L.gdst = L.gsrc + up256(g->N * R * 4);
    L.gm = L.gdst + up256(g->N * R * 4);
    L.att = L.gm + up256(g->N * C * 4);
    L.bpart = L.att + up256(B * 2 * R * C * 8);
    L.total = L.bpart + up256(B * C * 8);
    return L;
}

static bool wr_shape_ok(int R, int C, RowCfg &cfg)
{
    return R >= 1 && R <= WR_MAX_REL && C >= 1 && (int64_t)R * C <= SNGNN_MAX_CHANNELS && row_cfg(C, cfg);
}

}  // namespace sngnn

using namespace sngnn;

#define WR_CHECKS(g, R, C)                                                                                             \
    SN_REQUIRE((g) != nullptr, SNGNN_EINVAL, "graph is NULL");                                                         \
    SN_REQUIRE((g)->add_loops == 0 && (g)->remove_loops == 0 && (g)->N == (g)->Ntot && (g)->row_off == 0, SNGNN_EINVAL, \
               "the relational attention needs an unpartitioned graph built with add_loops = 0, remove_loops = 0 "    \
               "(every edge kept)");                                                                                   \
    RowCfg cfg;                                                                                                        \
    SN_REQUIRE(wr_shape_ok((R), (C), cfg), SNGNN_ERANGE,                                                               \
               "relations must be in [1, " + std::to_string(WR_MAX_REL) + "], C at least 1 and relations * C at most " \
                   + std::to_string(SNGNN_MAX_CHANNELS));                                                              \
    SN_REQUIRE((g)->N * (int64_t)(R) < (int64_t)1 << 31, SNGNN_ERANGE, "N * relations must fit 31 bits")

extern "C" int64_t sngnn_wrgat_workspace_bytes(const sngnn_graph_t *g, int R, int C)
{
    RowCfg cfg;
    if (g == nullptr || !wr_shape_ok(R, C, cfg)) return 0;
    return wr_layout(g, R, C).total;
}

extern "C" int sngnn_wrgat_forward(const sngnn_graph_t *g, const float *P, int64_t P_stride, const float *self_rows,
                                   int64_t self_stride, const float *bias, const int32_t *rel_ptr, const float *w_csr,
                                   const float *atten, int R, int C, float negative_slope, int relu, float *out,
                                   float *scores, float *ml, void *workspace, void *stream)
{
    WR_CHECKS(g, R, C);
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(P && rel_ptr && atten && out && scores && ml && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(P_stride >= (int64_t)R * C && (!self_rows || self_stride >= C), SNGNN_EINVAL, "a row stride is too short");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {P, self_rows, bias, atten, out, workspace}) &&
                   P_stride % cfg.vec == 0 && (!self_rows || self_stride % cfg.vec == 0),
               SNGNN_EINVAL, "rows must be aligned to the row vector width");
    hipStream_t st = (hipStream_t)stream;
    const WrLayout L = wr_layout(g, R, C);
    const int64_t NR = g->N * (int64_t)R;
    WrArgs a = {};
    bind_softmax_side(g, false, a);
    a.P = P; a.ldp = P_stride; a.self = self_rows; a.lds = self_stride; a.bias = bias;
    a.out = out; a.ldo = C;
    a.ssrc = scores; a.sdst = scores + NR; a.m = ml; a.l = ml + NR;
    a.rel_ptr = rel_ptr; a.w = w_csr; a.atten = atten;
    a.partial = (float *)workspace; a.ts = (float *)((char *)workspace + L.ts);
    a.slope = negative_slope; a.relu = relu; a.R = R; a.C = C;
    int rc = launch_gat_scores(P, P_stride, atten + C, atten, 2 * (int64_t)C, g->N, R, C, scores, scores + NR, st);
    if (rc != SNGNN_OK) return rc;
    const int nb = plan_side(a, a.N, 64 / WR_SG);
    if (nb > 0) k_wr_stats<<<nb, BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_wr_stats_fin<<<a.n_split, 64, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return dispatch_wr_fwd(cfg, a, st);
}

extern "C" int sngnn_wrgat_backward(const sngnn_graph_t *g, const float *grad_out, const float *out, const float *P,
                                    int64_t P_stride, const int32_t *rel_ptr, const int32_t *rel_csc, const float *w_csr,
                                    const float *atten, const float *scores, const float *ml, int R, int C,
                                    float negative_slope, int relu, float *grad_P, int64_t grad_P_stride,
                                    float *grad_self, int64_t grad_self_stride, float *grad_atten, float *grad_bias,
                                    void *workspace, void *stream)
{
    WR_CHECKS(g, R, C);
    if (g->N == 0) return SNGNN_OK;
    // (rel_csc has one element per edge: a graph without edges has none to point at, and pass S reads none)
    SN_REQUIRE(grad_out && P && rel_ptr && (rel_csc || g->Ep == 0) && atten && scores && ml && workspace && (out || !relu),
               SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(P_stride >= (int64_t)R * C && (!grad_P || grad_P_stride >= (int64_t)R * C) &&
                   (!grad_self || grad_self_stride >= C), SNGNN_EINVAL, "a row stride is too short");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {grad_out, P, atten, grad_P, grad_self, workspace}) &&
                   P_stride % cfg.vec == 0 && (!grad_P || grad_P_stride % cfg.vec == 0) &&
                   (!grad_self || grad_self_stride % cfg.vec == 0),
               SNGNN_EINVAL, "rows must be aligned to the row vector width");
    hipStream_t st = (hipStream_t)stream;
    const WrLayout L = wr_layout(g, R, C);
    const int64_t NR = g->N * (int64_t)R, NC = g->N * (int64_t)C;
    const int B = gat_att_blocks(g->N), npb = ceil_div(g->N, B);
    WrArgs a = {};
    a.P = P; a.ldp = P_stride;
    a.ssrc = scores; a.sdst = scores + NR; a.m = const_cast<float *>(ml); a.l = a.m + NR;
    a.rel_ptr = rel_ptr; a.rel_csc = rel_csc; a.w = w_csr; a.atten = atten;
    a.partial = (float *)workspace; a.ts = (float *)((char *)workspace + L.ts);
    a.te = (float *)((char *)workspace + L.te); a.rec = (float *)((char *)workspace + L.rec);
    a.D = (float *)((char *)workspace + L.D); a.gsrc = (float *)((char *)workspace + L.gsrc);
    a.gdst = (float *)((char *)workspace + L.gdst);
    a.slope = negative_slope; a.relu = relu; a.R = R; a.C = C;
    // the masked G: the root slice's gradient where that is wanted, scratch otherwise, grad_out itself without either
    if (grad_self || relu) {
        float *gm = grad_self ? grad_self : (float *)((char *)workspace + L.gm);
        a.g = gm; a.ldg = grad_self ? grad_self_stride : C;
        k_wr_gmask<<<ceil_div(NC, 256), 256, 0, st>>>(grad_out, out, relu, NC, C, gm, a.ldg);
    } else {
        a.g = grad_out; a.ldg = C;
    }
    if (grad_bias) {
        double *bp = (double *)((char *)workspace + L.bpart);
        k_wr_bias_part<<<B, 256, 0, st>>>(a.g, a.ldg, (int)g->N, C, npb, bp);
        k_wr_bias_red<<<ceil_div(C, 256), 256, 0, st>>>(bp, B, C, grad_bias);
    }
    SN_HIP(hipGetLastError());
    if (!grad_P && !grad_atten) return SNGNN_OK;
    bind_softmax_side(g, false, a);
    int rc = dispatch_wr_bwd_t(cfg, a, st);
    if (rc != SNGNN_OK) return rc;
    const int nb = plan_side(a, a.N, 64 / WR_SG);
    if (nb > 0) k_wr_bwd_d<<<nb, BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_wr_bwd_d_fin<<<a.n_split, 64, 0, st>>>(a);
    if (nb > 0) k_wr_bwd_rec<<<nb, BLOCK, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    bind_softmax_side(g, true, a);
    a.out = grad_P; a.ldo = grad_P_stride;
    rc = dispatch_wr_bwd_s(cfg, a, st);
    if (rc != SNGNN_OK) return rc;
    if (grad_atten) {
        double *part = (double *)((char *)workspace + L.att);
        rc = launch_gat_att_part(P, P_stride, a.gsrc, a.gdst, g->N, R, C, part, st);
        if (rc != SNGNN_OK) return rc;
        return launch_gat_att_red(part, g->N, R, C, true, grad_atten, st);      // (the source half is atten[:, C:])
    }
    return SNGNN_OK;
}

// ACM-GCN's adaptive channel mixing layer after its linear map (gfx950, fp32): GraphConvolution2.forward for
// model_type 'acmgcn' / 'acmsgc', variant = False, models/models.py:1787-1830.
//     L = adj_low Pl,  H = adj_high Ph,  M = Pm            P = X [W_low | W_high | W_mlp] = [Pl | Ph | Pm]   [N, 3C]
//     o* = relu(L | H | M)   (acmsgc: no relu)
//     d  = (<ol, a_low>, <oh, a_high>, <om, a_mlp>),  s = sigmoid(d),  att = softmax(s att_vec / 3)
//     out = 3 (att_0 ol + att_1 oh + att_2 om)
// for the row-normalised adjacency whose row i holds n_i entries (diagonal included) of weight 1 / n_i each and
// adj_high = I - adj_low:  L_i = S^l_i / n_i,  H_i = (1 - 1 / n_i) Ph_i - S^h_i / n_i  with  S^l_i the sum of Pl[col] over
// row i and S^h_i the sum of Ph[col] over its OFF-diagonal entries (the reference's own terms: with the diagonal
// inside the sum, Ph_i - Ph_i / n_i cancels - completely for an isolated node - what the reference never adds) -
// an unweighted gather-sum of one contiguous 2C-wide slice per entry on the row-class walk of row_walk.h (small rows by lane
// group, medium rows by wave, hubs as 128-entry tasks + a finalize; fixed summation order, no atomics), n_i from the
// graph's own rowptr.  Whoever completes a row runs the whole epilogue and stores out, the pre-activations [L | H]
// and six scalars (d, att) a row: all the backward needs next to P.
//   backward, pass A  row-local: grad_out -> the mix, softmax, 3x3, sigmoid, dots, relu' -> gL, gH, gM;
//                     GP = [gL / n_i | gH / n_i] for pass B, (1 - 1 / n_i) gH_i and gM into grad_P, and the 3C + 9 parameter gradients
//                     as per-workgroup partials in double that one reducer launch adds in a fixed order
//   backward, pass B  the transpose gather-sum of GP over the other side of the graph:
//                     grad_Pl_j = sum_{i : j in row i} gL_i / n_i,
//                     grad_Ph_j = (1 - 1 / n_j) gH_j - sum_{i != j : j in row i} gH_i / n_i
// A lane holds the SAME channels of the l and the h half (two rows of the C-wide layout), so the epilogue is
// lane-local up to three group sums.  Every product and sum is rounded separately (-ffp-contract=off).
#include "entry.h"
#include "row_walk.h"

namespace sngnn {

constexpr int ACM_PARAM_BLOCKS = 512;       // most workgroups (= partials per parameter gradient) of pass A

struct AcmArgs : RowSide {
    const float *src;           // rows gathered: [N, ld], the [l | h] slice in front
    int ld;
    int mode;                   // 0 forward, 1 backward pass B
    int relu;
    const float *P;             // forward: [N, 3C], the row's own Ph_i and Pm_i
    const float *a_low, *a_high, *a_mlp, *att_vec;
    float *out, *LH, *datt;     // forward: [N, C], [N, 2C], [N, 6] = (d, att)
    float *gP;                  // pass B: grad_P [N, 3C]; its h third holds (1 - 1 / n_j) gH_j on entry
    float *partial;             // [n_tasks, 2C]
    int C, N;
};

// a row's two gathered sums: the l half and the h half without the diagonal
template <int VEC, int G, int R> struct AcmSums {
    Row<VEC, G, R> l, h;
    __device__ __forceinline__ void zero() { l.zero(); h.zero(); }
    __device__ __forceinline__ void reduce_across_groups() { l.reduce_across_groups(); h.reduce_across_groups(); }
};

// relu that keeps a NaN (torch's)
__device__ __forceinline__ float acm_relu(float v) { return v < 0.f ? 0.f : v; }

// s = sigmoid(d), att = softmax(s att_vec / 3) with the maximum subtracted
__device__ __forceinline__ void acm_attention(const float (&d)[3], const float *__restrict__ A, float (&att)[3])
{
    float s[3], z[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = 1.0f / (1.0f + expf(-d[j]));
#pragma unroll
    for (int k = 0; k < 3; ++k) z[k] = ((s[0] * A[k] + s[1] * A[3 + k]) + s[2] * A[6 + k]) / 3.0f;
    const float m = fmaxf(fmaxf(z[0], z[1]), z[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) z[k] = expf(z[k] - m);
    const float sum = (z[0] + z[1]) + z[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) att[k] = z[k] / sum;
}

template <int VEC, int G, int R>
__device__ __forceinline__ void acm_gather(const AcmArgs &a, int self, int qs, int e0, int e1, int stride, int first,
                                           int lg, Row<VEC, G, R> &sl, Row<VEC, G, R> &sh)
{
    using RowT = Row<VEC, G, R>;
    constexpr int U = (R * VEC >= 4) ? 2 : 4;
    for (int base = e0 + first; base < e1; base += stride * U) {
        RowT xl[U], xh[U];
        bool act[U], off[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = base + u * stride;
            act[u] = t < e1;
            const int row = act[u] ? a.idx[qs + t] : 0;
            off[u] = act[u] && row != self;           // the h half leaves the diagonal to the epilogue
            const float *p = a.src + (size_t)row * a.ld;
            xl[u].load(p, a.C, lg);
            xh[u].load(p + a.C, a.C, lg);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (act[u]) sl.add(xl[u]);
            if (off[u]) sh.add(xh[u]);
        }
    }
}

// the epilogue of row r (deg entries) from its gathered sums; the G lanes of the group are all active
template <int VEC, int G, int R>
__device__ __forceinline__ void acm_finish(const AcmArgs &a, int r, int deg, int lg, Row<VEC, G, R> &sl,
                                           Row<VEC, G, R> &sh)
{
    using RowT = Row<VEC, G, R>;
    const int C = a.C;
    if (a.mode == 1) {
        float *g = a.gP + (size_t)r * 3 * C;
        RowT h;
        h.load(g + C, C, lg);
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) h.x[q][v] = h.x[q][v] - sh.x[q][v];
        sl.store(g, C, lg);
        h.store(g + C, C, lg);
        return;
    }
    const float n = (float)max(deg, 1);
    const float *p = a.P + (size_t)r * 3 * C;
    RowT oh, om;
    oh.load(p + C, C, lg);
    om.load(p + 2 * C, C, lg);
    const float wd = 1.0f - 1.0f / n;            // adj_high's diagonal
    sl.div(n);
    sh.div(n);
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
        for (int v = 0; v < VEC; ++v) oh.x[q][v] = wd * oh.x[q][v] - sh.x[q][v];
    sl.store(a.LH + (size_t)r * 2 * C, C, lg);
    oh.store(a.LH + (size_t)r * 2 * C + C, C, lg);
    if (a.relu) {
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                sl.x[q][v] = acm_relu(sl.x[q][v]);
                oh.x[q][v] = acm_relu(oh.x[q][v]);
                om.x[q][v] = acm_relu(om.x[q][v]);
            }
    }
    RowT w;
    float d[3], att[3];
    w.load(a.a_low, C, lg);
    d[0] = group_sum<G>(sl.dot_partial(w));
    w.load(a.a_high, C, lg);
    d[1] = group_sum<G>(oh.dot_partial(w));
    w.load(a.a_mlp, C, lg);
    d[2] = group_sum<G>(om.dot_partial(w));
    acm_attention(d, a.att_vec, att);
#pragma unroll
    for (int q = 0; q < R; ++q)
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            w.x[q][v] = 3.0f * ((att[0] * sl.x[q][v] + att[1] * oh.x[q][v]) + att[2] * om.x[q][v]);
    w.store(a.out + (size_t)r * C, C, lg);
    if (lg == 0) {
        float *o = a.datt + (size_t)r * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[k] = d[k]; o[3 + k] = att[k]; }
    }
}

template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_acm(const AcmArgs a)
{
    using Sums = AcmSums<VEC, G, R>;
    Sums acc;
    walk_rows<G>(
        a, blockIdx.x, a.N, acc,
        [&](int seg, int qs, int e0, int e1, int stride, int first, int lg, Sums &s) {
            acm_gather<VEC, G, R>(a, seg, qs, e0, e1, stride, first, lg, s.l, s.h);
        },
        [&](int tq, int lg, Sums &s) {
            float *pt = a.partial + (size_t)tq * 2 * a.C;
            s.l.store(pt, a.C, lg);
            s.h.store(pt + a.C, a.C, lg);
        },
        [&](int seg, int deg, int lg, Sums &s) { acm_finish<VEC, G, R>(a, seg, deg, lg, s.l, s.h); });
}

// split rows: the sum of the tasks' partial rows in a fixed order, then the epilogue of acm_finish with one channel
// per thread (2C <= SNGNN_MAX_CHANNELS: C <= 256 = the workgroup)
static __global__ __launch_bounds__(256) void k_acm_fin(const AcmArgs a)
{
    __shared__ float s[SNGNN_MAX_CHANNELS];
    __shared__ float red[3][4];
    const int p = blockIdx.x;
    const int r = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const int C = a.C, W = 2 * a.C;
    for (int j = threadIdx.x; j < W; j += 256) {
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        int t = t0;
        for (; t + 3 < t1; t += 4) {
            v0 += a.partial[(size_t)t * W + j];
            v1 += a.partial[(size_t)(t + 1) * W + j];
            v2 += a.partial[(size_t)(t + 2) * W + j];
            v3 += a.partial[(size_t)(t + 3) * W + j];
        }
        for (; t < t1; ++t) v0 += a.partial[(size_t)t * W + j];
        s[j] = (v0 + v1) + (v2 + v3);
    }
    __syncthreads();
    const int c = threadIdx.x;
    const bool in = c < C;
    if (a.mode == 1) {
        if (in) {
            float *g = a.gP + (size_t)r * 3 * C;
            g[c] = s[c];
            g[C + c] = g[C + c] - s[C + c];
        }
        return;
    }
    const float n = (float)max(a.ptr[r + 1] - a.ptr[r], 1);
    float ol = 0.f, oh = 0.f, om = 0.f, pd[3] = {0.f, 0.f, 0.f};
    if (in) {
        const float *pr = a.P + (size_t)r * 3 * C;
        ol = s[c] / n;
        oh = (1.0f - 1.0f / n) * pr[C + c] - s[C + c] / n;
        om = pr[2 * C + c];
        a.LH[(size_t)r * 2 * C + c] = ol;
        a.LH[(size_t)r * 2 * C + C + c] = oh;
        if (a.relu) { ol = acm_relu(ol); oh = acm_relu(oh); om = acm_relu(om); }
        pd[0] = ol * a.a_low[c];
        pd[1] = oh * a.a_high[c];
        pd[2] = om * a.a_mlp[c];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = wave_sum_f(pd[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    float d[3], att[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
    acm_attention(d, a.att_vec, att);
    if (in) a.out[(size_t)r * C + c] = 3.0f * ((att[0] * ol + att[1] * oh) + att[2] * om);
    if (threadIdx.x == 0) {
        float *o = a.datt + (size_t)r * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[k] = d[k]; o[3 + k] = att[k]; }
    }
}

struct AcmBwdArgs {
    const float *g, *P, *LH, *datt;          // grad_out [N, C], P [N, 3C], [L | H] [N, 2C], (d, att) [N, 6]
    const float *a_low, *a_high, *a_mlp, *att_vec;
    const int32_t *rowptr;
    float *GP;                                // [N, 2C] = [gL / n | gH / n]
    float *gP;                                // grad_P [N, 3C]: (1 - 1 / n_i) gH_i and gM are written here
    double *part;                             // [3C + 9, nb] per-workgroup partials of the parameter gradients
    int C, N, relu, nb;
};

__device__ __forceinline__ double acm_shfl_d(double v, int m) { return __shfl_xor(v, m, 64); }

// pass A: one lane group per row, rows dealt round robin (the same trip count in every wave of the launch's
// grid-stride loop: a group past the end works on row 0 and drops the result)
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_acm_bwd_a(const AcmBwdArgs a)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G, CH = R * G * VEC;
    __shared__ double sd[WAVES][3][CH];
    __shared__ double sv[WAVES][9];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    const int C = a.C;
    RowT al, ah, am;
    al.load(a.a_low, C, lg);
    ah.load(a.a_high, C, lg);
    am.load(a.a_mlp, C, lg);
    float A[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k] = a.att_vec[k];
    double acc[3][R][VEC], accv[9];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[k][q][v] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) accv[k] = 0.0;
    const int per = gridDim.x * WAVES * NG;
    for (int base = (blockIdx.x * WAVES + wave) * NG; base < a.N; base += per) {
        const bool live = base + gid < a.N;
        const int r = live ? base + gid : 0;
        RowT g, ol, oh, om;
        g.load(a.g + (size_t)r * C, C, lg);
        ol.load(a.LH + (size_t)r * 2 * C, C, lg);
        oh.load(a.LH + (size_t)r * 2 * C + C, C, lg);
        om.load(a.P + (size_t)r * 3 * C + 2 * C, C, lg);
        const float n = (float)max(a.rowptr[r + 1] - a.rowptr[r], 1);
        float d[3], att[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { d[k] = a.datt[(size_t)r * 6 + k]; att[k] = a.datt[(size_t)r * 6 + 3 + k]; }
        bool ml[R][VEC], mh[R][VEC], mm[R][VEC];
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                ml[q][v] = !a.relu || ol.x[q][v] > 0.f;
                mh[q][v] = !a.relu || oh.x[q][v] > 0.f;
                mm[q][v] = !a.relu || om.x[q][v] > 0.f;
                if (a.relu) {
                    ol.x[q][v] = acm_relu(ol.x[q][v]);
                    oh.x[q][v] = acm_relu(oh.x[q][v]);
                    om.x[q][v] = acm_relu(om.x[q][v]);
                }
            }
        // the mix: g_att_k = 3 <g, o_k>
        float ga[3];
        ga[0] = 3.0f * group_sum<G>(g.dot_partial(ol));
        ga[1] = 3.0f * group_sum<G>(g.dot_partial(oh));
        ga[2] = 3.0f * group_sum<G>(g.dot_partial(om));
        // softmax, the 3x3 product with its / 3, sigmoid (s (1 - s) as s(d) s(-d): no cancellation near s = 1)
        const float mean = (att[0] * ga[0] + att[1] * ga[1]) + att[2] * ga[2];
        float gz[3], gd[3], s[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) gz[k] = att[k] * (ga[k] - mean);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            s[j] = 1.0f / (1.0f + expf(-d[j]));
            const float gs = ((A[3 * j] * gz[0] + A[3 * j + 1] * gz[1]) + A[3 * j + 2] * gz[2]) / 3.0f;
            gd[j] = gs * (s[j] * (1.0f / (1.0f + expf(d[j]))));
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) accv[3 * j + k] += (double)s[j] * (double)gz[k] / 3.0;
        }
        RowT gl, gh, gm;
        const float c0 = 3.0f * att[0], c1 = 3.0f * att[1], c2 = 3.0f * att[2];
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float gv = g.x[q][v];
                if (live) {
                    acc[0][q][v] += (double)gd[0] * (double)ol.x[q][v];
                    acc[1][q][v] += (double)gd[1] * (double)oh.x[q][v];
                    acc[2][q][v] += (double)gd[2] * (double)om.x[q][v];
                }
                const float tl = c0 * gv + gd[0] * al.x[q][v];
                const float th = c1 * gv + gd[1] * ah.x[q][v];
                const float tm = c2 * gv + gd[2] * am.x[q][v];
                gl.x[q][v] = ml[q][v] ? tl : 0.f;
                gh.x[q][v] = mh[q][v] ? th : 0.f;
                gm.x[q][v] = mm[q][v] ? tm : 0.f;
            }
        if (live) {
            RowT gd_ = gh;                          // the diagonal's own term, (1 - 1 / n_i) gH_i
            gd_.scale(1.0f - 1.0f / n);
            gd_.store(a.gP + (size_t)r * 3 * C + C, C, lg);
            gm.store(a.gP + (size_t)r * 3 * C + 2 * C, C, lg);
            gl.div(n);
            gh.div(n);
            gl.store(a.GP + (size_t)r * 2 * C, C, lg);
            gh.store(a.GP + (size_t)r * 2 * C + C, C, lg);
        }
    }
    // the workgroup's partials: groups of a wave, then the four waves, in a fixed order
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                double t = acc[k][q][v];
#pragma unroll
                for (int m = G; m < 64; m <<= 1) t += acm_shfl_d(t, m);
                if (gid == 0) sd[wave][k][(q * G + lg) * VEC + v] = t;
            }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        double t = lg == 0 ? accv[k] : 0.0;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) t += acm_shfl_d(t, m);
        if (lane == 0) sv[wave][k] = t;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * C; i += BLOCK) {
        const int k = i / C, c = i % C;
        a.part[(size_t)i * a.nb + blockIdx.x] = (sd[0][k][c] + sd[1][k][c]) + (sd[2][k][c] + sd[3][k][c]);
    }
    if (threadIdx.x < 9)
        a.part[(size_t)(3 * C + threadIdx.x) * a.nb + blockIdx.x] =
            (sv[0][threadIdx.x] + sv[1][threadIdx.x]) + (sv[2][threadIdx.x] + sv[3][threadIdx.x]);
}

// out[k] = the sum of row k of the partials, fixed order
static __global__ __launch_bounds__(256) void k_acm_params(const double *__restrict__ part, int nb,
                                                           double *__restrict__ out)
{
    __shared__ double s[256];
    const int k = blockIdx.x;
    const double *p = part + (size_t)k * nb;
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) v += p[i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = s[0];
}

// the lane layouts of C <= 256 channels hold at most 256 of them (row_cfg): the others are not instantiated
#define ACM_DISPATCH_GR(FN, VEC, cfg, ...)                                                                             \
    return sngnn::dispatch_gr(cfg, [&](auto g, auto r) {                                                               \
        if constexpr (VEC * decltype(g)::value * decltype(r)::value <= SNGNN_MAX_CHANNELS / 2)                         \
            return FN<VEC, decltype(g)::value, decltype(r)::value>(__VA_ARGS__);                                       \
        else {                                                                                                         \
            set_error("unsupported channel layout");                                                                   \
            return (int)SNGNN_ERANGE;                                                                                  \
        }                                                                                                              \
    });

template <int VEC, int G, int R> int launch_acm(const AcmArgs &a0, hipStream_t st)
{
    AcmArgs a = a0;
    const int grid = plan_side(a, a.N, 64 / G);
    if (grid > 0) k_acm<VEC, G, R><<<grid, BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_acm_fin<<<a.n_split, 256, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

static int dispatch_acm(const RowCfg &cfg, const AcmArgs &a, hipStream_t st)
{
    return dispatch_vec(cfg, [&](auto vec) { ACM_DISPATCH_GR(launch_acm, decltype(vec)::value, cfg, a, st) });
}

static int acm_bwd_blocks(int64_t N, const RowCfg &cfg)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(ACM_PARAM_BLOCKS, ceil_div(N, (int64_t)WAVES * (64 / cfg.g))));
}

template <int VEC, int G, int R> int launch_acm_bwd_a(const AcmBwdArgs &a, hipStream_t st)
{
    k_acm_bwd_a<VEC, G, R><<<a.nb, BLOCK, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

static int dispatch_acm_bwd_a(const RowCfg &cfg, const AcmBwdArgs &a, hipStream_t st)
{
    return dispatch_vec(cfg, [&](auto vec) { ACM_DISPATCH_GR(launch_acm_bwd_a, decltype(vec)::value, cfg, a, st) });
}

struct AcmLayout { int64_t gp, parts, total; };       // the task partials are in front

static AcmLayout acm_layout(const sngnn_graph_t *g, int C)
{
    AcmLayout L;
    L.gp = task_partial_bytes(g, 2 * C);
    L.parts = L.gp + up256(g->N * (int64_t)2 * C * 4);
    L.total = L.parts + up256((int64_t)(3 * C + 9) * ACM_PARAM_BLOCKS * 8);
    return L;
}

static bool acm_width_ok(int C) { return C >= 1 && 2 * (int64_t)C <= SNGNN_MAX_CHANNELS; }

}  // namespace sngnn

using namespace sngnn;

#define ACM_COMMON(g, C)                                                                                               \
    SN_REQUIRE((g) != nullptr, SNGNN_EINVAL, "graph is NULL");                                                         \
    SN_REQUIRE((g)->N == (g)->Ntot && (g)->row_off == 0, SNGNN_EINVAL,                                                 \
               "the ACM filterbank needs an unpartitioned graph");                                                     \
    SN_REQUIRE(acm_width_ok(C), SNGNN_ERANGE,                                                                          \
               "C must be in [1, " + std::to_string(SNGNN_MAX_CHANNELS / 2) + "] (2C <= SNGNN_MAX_CHANNELS)");         \
    RowCfg cfg;                                                                                                        \
    SN_REQUIRE(row_cfg((C), cfg), SNGNN_ERANGE, "unsupported channel count")

extern "C" int64_t sngnn_acm_workspace_bytes(const sngnn_graph_t *g, int C)
{
    if (g == nullptr || !acm_width_ok(C)) return 0;
    return acm_layout(g, C).total;
}

extern "C" int sngnn_acm_forward(const sngnn_graph_t *g, const float *P, const float *a_low, const float *a_high,
                                 const float *a_mlp, const float *att_vec, int C, int relu, float *out, float *LH,
                                 float *datt, void *workspace, void *stream)
{
    ACM_COMMON(g, C);
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(P && a_low && a_high && a_mlp && att_vec && out && LH && datt && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {P, a_low, a_high, a_mlp, out, LH, workspace}), SNGNN_EINVAL,
               "rows must be aligned to the row vector width");
    AcmArgs a;
    a.N = (int)g->N;
    bind_side(g, false, a);
    a.nbA = a.nbB = 0;
    a.src = P; a.ld = 3 * C; a.mode = 0; a.relu = relu != 0; a.P = P;
    a.a_low = a_low; a.a_high = a_high; a.a_mlp = a_mlp; a.att_vec = att_vec;
    a.out = out; a.LH = LH; a.datt = datt; a.gP = nullptr;
    a.partial = (float *)workspace; a.C = C;
    return dispatch_acm(cfg, a, (hipStream_t)stream);
}

extern "C" int sngnn_acm_backward(const sngnn_graph_t *g, const float *grad_out, const float *P, const float *LH,
                                  const float *datt, const float *a_low, const float *a_high, const float *a_mlp,
                                  const float *att_vec, int C, int relu, float *grad_P, double *grad_params,
                                  void *workspace, void *stream)
{
    ACM_COMMON(g, C);
    hipStream_t st = (hipStream_t)stream;
    SN_REQUIRE(grad_params, SNGNN_EINVAL, "NULL argument");
    if (g->N == 0) {
        k_acm_params<<<3 * C + 9, 256, 0, st>>>(nullptr, 0, grad_params);
        SN_HIP(hipGetLastError());
        return SNGNN_OK;
    }
    SN_REQUIRE(grad_out && P && LH && datt && a_low && a_high && a_mlp && att_vec && grad_P && workspace, SNGNN_EINVAL,
               "NULL argument");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * 4, {grad_out, P, LH, a_low, a_high, a_mlp, grad_P, workspace}),
               SNGNN_EINVAL, "rows must be aligned to the row vector width");
    const AcmLayout L = acm_layout(g, C);
    AcmBwdArgs b;
    b.g = grad_out; b.P = P; b.LH = LH; b.datt = datt;
    b.a_low = a_low; b.a_high = a_high; b.a_mlp = a_mlp; b.att_vec = att_vec;
    b.rowptr = g->rowptr;
    b.GP = (float *)((char *)workspace + L.gp); b.gP = grad_P;
    b.part = (double *)((char *)workspace + L.parts);
    b.C = C; b.N = (int)g->N; b.relu = relu != 0; b.nb = acm_bwd_blocks(g->N, cfg);
    int rc = dispatch_acm_bwd_a(cfg, b, st);
    if (rc != SNGNN_OK) return rc;
    k_acm_params<<<3 * C + 9, 256, 0, st>>>(b.part, b.nb, grad_params);
    SN_HIP(hipGetLastError());
    AcmArgs a;
    a.N = (int)g->N;
    bind_side(g, true, a);
    a.nbA = a.nbB = 0;
    a.src = b.GP; a.ld = 2 * C; a.mode = 1; a.relu = 0; a.P = nullptr;
    a.a_low = a.a_high = a.a_mlp = a.att_vec = nullptr;
    a.out = a.LH = a.datt = nullptr; a.gP = grad_P;
    a.partial = (float *)workspace; a.C = C;
    return dispatch_acm(cfg, a, st);
}

// Graph attention (PyG 2.0.4 GATConv's propagate) on the row classes of row_walk.h (gfx950, fp32, one GPU).
//     xp [N, H, C] = lin_src(x),   a_src[n,h] = <xp[n,h,:], att_src[h,:]>,   a_dst alike
//     per in-edge e = (j -> i) and head h:   a_e = leaky_relu(a_src[j,h] + a_dst[i,h])
//     alpha_e = exp(a_e - m_i) / (l_i + 1e-16),   m_i = max_e a_e,   l_i = sum_e exp(a_e - m_i)
//     out[i,h,:] = sum_e alpha_e xp[j,h,:]
// The edge list is the loop-replaced one (add_loops = 1, SNGNN_LOOPS_REPLACE): every row has its loop, the edge that
// attains the maximum adds exp(0) = 1, so l_i >= 1 and l_i + 1e-16 == l_i in fp32 - the kernels divide by l_i.
//
// The score is unbounded (unlike attn_impl.h's cosine), so the softmax carries its maximum; and it is known from two
// scalars per node before any row is fetched, so a row's m and l are settled from a 4-byte gather per edge and head
// (pass one) and the 4C-byte head slices are then gathered exactly once, weighted by exp(a_e - m) (pass two), the
// division by l in the store.  Heads ride on gridDim.y: a workgroup serves one head of its rows, the row layout
// (Row<VEC, G, R>) is that of C channels, and the H slices of a source row are fetched by H workgroups, once each.
//   rows of <= 16 in-edges   one G-lane group: its lanes share the edges in pass one
//   rows of <= 128           one wave: a lane per edge in pass one, a group per edge in pass two
//   split rows               128-edge wave tasks that write the partial row sum_e exp(a_e - m_t) xp_j, m_t and l_t;
//                            the finalize merges them in task order: m = max m_t, l = sum l_t exp(m_t - m),
//                            out = (sum_t exp(m_t - m) partial_t) / l
// Which row or task a wave or lane group serves is row_walk.h's row_unit (k_gat_fwd, k_gat_bwd_t, k_gat_bwd_s; wrgat.hip's
// kernels call it too): a dead unit runs the two passes over an empty range, so the cohort reductions between them are
// never taken under divergence.
// Every sum has a fixed order; there is no floating-point atomic and no host synchronisation.
//
// Backward from G = grad_out [N, H, C], saved: out, m, l (and the scores [N, H]):
//   pass T (in-edges)    t_e = <G[i,h], xp[j,h]>,  dot = <G[i,h], out[i,h]> (= sum alpha t: split rows need no merge),
//                        ds_e = alpha_e (t_e - dot),  da_e = ds_e leaky'(a_e),  grad_a_dst[i,h] = sum_e da_e,
//                        {alpha_e, da_e} written at the edge's CSC position
//   pass S (out-edges)   grad_xp[j,h,:] = sum_e alpha_e G[i,h,:],  grad_a_src[j,h] = sum_e da_e, and in the store
//                        grad_xp[j,h,:] += grad_a_src[j,h] att_src[h,:] + grad_a_dst[j,h] att_dst[h,:]
//   grad_att_src[h,c] = sum_j grad_a_src[j,h] xp[j,h,c] (grad_att_dst alike): per-workgroup partials in double,
//                        added in a fixed order by a reducer launch
#include "entry.h"
#include "row_walk.h"

namespace sngnn {

constexpr int GAT_MAX_HEADS = 16;
constexpr int GAT_ATT_BLOCKS = 512;      // most workgroups (= partial results) of the grad_att reduction

struct GatArgs : RowSide {         // the in-edges (forward, pass T) or the out-edges (pass S): row_walk.h
    const float *xp;               // [N, H, C]
    const float *gout;             // [N, H, C] backward: grad_out
    const float *fout;             // [N, H, C] backward: the forward's output
    float *out;                    // [N, H, C] forward: out; pass S: grad_xp (nullptr = not wanted)
    const float *asrc, *adst;      // [N, H]
    float *m, *l;                  // [N, H] written by the forward, read by pass T
    float *partial;                // [tasks, H, C]
    float *tm, *tl;                // [tasks, H] forward: m_t, l_t; backward: tm = the tasks' sums of da_e
    float *rec;                    // [E', H, 2] {alpha_e, da_e} in CSC order
    float *gasrc, *gadst;          // [N, H]
    const float *att_src, *att_dst;    // [H, C]
    float slope;
    int H, C, W, N;
    const int32_t *csc_pos;
};

// pass one of a row (or task): m = max a_e and l = sum exp(a_e - m) over its edges [e0, e1), shared by P lanes
template <int P>
__device__ __forceinline__ void gat_stats(const GatArgs &a, int h, int qs, int e0, int e1, float adst, int p, float &m,
                                          float &l)
{
    float mx = -INFINITY;
    for (int t = e0 + p; t < e1; t += P)
        mx = fmaxf(mx, leaky(a.asrc[(size_t)a.idx[qs + t] * a.H + h] + adst, a.slope));
    mx = cohort_max<P>(mx);
    float s = 0.f;
    for (int t = e0 + p; t < e1; t += P)
        s += expf(leaky(a.asrc[(size_t)a.idx[qs + t] * a.H + h] + adst, a.slope) - mx);
    m = mx;
    l = cohort_sum<P>(s);
}

// pass two: acc += exp(a_e - m) xp[j, h, :] over the edges first, first + stride, ... of [e0, e1)
template <int VEC, int G, int R>
__device__ __forceinline__ void gat_gather(const GatArgs &a, int h, int qs, int e0, int e1, int stride, int first, int lg,
                                           float adst, float m, Row<VEC, G, R> &acc)
{
    using RowT = Row<VEC, G, R>;
    constexpr int U = gather_unroll(R);
    const float *base = a.xp + h * a.C;
    for (int b = e0 + first; b < e1; b += stride * U) {
        RowT x[U];
        float w[U];
        bool act[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = b + u * stride;
            act[u] = t < e1;
            const int j = act[u] ? a.idx[qs + t] : 0;
            x[u].load(base + (size_t)j * a.W, a.C, lg);
            w[u] = expf(leaky(a.asrc[(size_t)j * a.H + h] + adst, a.slope) - m);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (act[u]) acc.axpy(w[u], x[u]);
    }
}

template <int VEC, int G, int R> __global__ __launch_bounds__(BLOCK) void k_gat_fwd(const GatArgs a)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    const int h = blockIdx.y;
    bool wide;
    const RowUnit u = row_unit<G>(a, a.N, blockIdx.x, wave, gid, wide);
    const float adst = a.adst[(size_t)u.seg * a.H + h];
    RowT acc;
    acc.zero();
    float m, l;
    if (wide) {
        gat_stats<64>(a, h, u.qs, u.e0, u.e1, adst, lane, m, l);
        gat_gather<VEC, G, R>(a, h, u.qs, u.e0, u.e1, NG, gid, lg, adst, m, acc);
        acc.reduce_across_groups();
    } else {
        gat_stats<G>(a, h, u.qs, u.e0, u.e1, adst, lg, m, l);
        gat_gather<VEC, G, R>(a, h, u.qs, u.e0, u.e1, 1, 0, lg, adst, m, acc);
    }
    if (!u.live || (wide && gid != 0)) return;
    if (u.task) {
        acc.store(a.partial + ((size_t)u.tq * a.H + h) * a.C, a.C, lg);
        if (lg == 0) {
            a.tm[(size_t)u.tq * a.H + h] = m;
            a.tl[(size_t)u.tq * a.H + h] = l;
        }
    } else {
        acc.div(l);                                        // l >= 1: the loop's term; + 1e-16 vanishes in fp32
        acc.store(a.out + (size_t)u.seg * a.W + h * a.C, a.C, lg);
        if (lg == 0) {
            a.m[(size_t)u.seg * a.H + h] = m;
            a.l[(size_t)u.seg * a.H + h] = l;
        }
    }
}

// split rows: the max-carrying merge of the tasks' (partial row, m_t, l_t) in task order
static __global__ __launch_bounds__(256) void k_gat_fwd_fin(const GatArgs a)
{
    const int p = blockIdx.x, h = blockIdx.y;
    const int r = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    float m = -INFINITY;
    for (int t = t0; t < t1; ++t) m = fmaxf(m, a.tm[(size_t)t * a.H + h]);
    float l = 0.f;
    for (int t = t0; t < t1; ++t) l += a.tl[(size_t)t * a.H + h] * expf(a.tm[(size_t)t * a.H + h] - m);
    for (int c = threadIdx.x; c < a.C; c += 256) {
        float s = 0.f;
        for (int t = t0; t < t1; ++t)
            s += a.partial[((size_t)t * a.H + h) * a.C + c] * expf(a.tm[(size_t)t * a.H + h] - m);
        a.out[(size_t)r * a.W + h * a.C + c] = s / l;
    }
    if (threadIdx.x == 0) {
        a.m[(size_t)r * a.H + h] = m;
        a.l[(size_t)r * a.H + h] = l;
    }
}

// pass T.  The loops' bounds are wave-uniform (an inactive slot loads row 0 and is discarded): the group sums are
// never taken under divergence.
template <int VEC, int G, int R> __global__ __launch_bounds__(BLOCK) void k_gat_bwd_t(const GatArgs a)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    constexpr int U = R >= 2 ? 1 : 2;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    const int h = blockIdx.y;
    bool wide;
    const RowUnit u = row_unit<G>(a, a.N, blockIdx.x, wave, gid, wide);
    const size_t sh = (size_t)u.seg * a.H + h;
    const float adst = a.adst[sh], m = a.m[sh], l = a.l[sh];
    RowT gi, oi;
    gi.load(a.gout + (size_t)u.seg * a.W + h * a.C, a.C, lg);
    oi.load(a.fout + (size_t)u.seg * a.W + h * a.C, a.C, lg);
    const float dot = group_sum<G>(gi.dot_partial(oi));
    const float *base = a.xp + h * a.C;
    const int stride = wide ? NG : 1, first = wide ? gid : 0;
    // (small rows: the longest row of the wave bounds the loop)
    const int e_end = wide ? u.e1 : wave_max_i(u.e1);
    float sda = 0.f;
    for (int b = u.e0; b < e_end; b += stride * U) {
        RowT x[U];
        bool act[U];
        int t[U], j[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            t[q] = b + first + q * stride;
            act[q] = t[q] < u.e1;
            j[q] = act[q] ? a.idx[u.qs + t[q]] : 0;
            x[q].load(base + (size_t)j[q] * a.W, a.C, lg);
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const float te = group_sum<G>(gi.dot_partial(x[q]));
            const float raw = a.asrc[(size_t)j[q] * a.H + h] + adst;
            const float alpha = expf(leaky(raw, a.slope) - m) / l;
            const float ds = alpha * (te - dot);
            const float da = raw > 0.f ? ds : ds * a.slope;
            if (act[q]) {
                sda += da;
                if (lg == 0) {
                    const size_t at = ((size_t)a.csc_pos[u.qs + t[q]] * a.H + h) * 2;
                    *reinterpret_cast<float2 *>(a.rec + at) = make_float2(alpha, da);
                }
            }
        }
    }
    if (wide) sda = cross_group_sum<G>(sda);
    if (!u.live || lg != 0 || (wide && gid != 0)) return;
    if (u.task) a.tm[(size_t)u.tq * a.H + h] = sda;
    else a.gadst[sh] = sda;
}

// split rows of pass T: grad_a_dst = the tasks' sums in task order
static __global__ void k_gat_bwd_t_fin(const GatArgs a)
{
    const int p = blockIdx.x, h = threadIdx.x;
    if (h >= a.H) return;
    const int r = a.perm[p];
    float s = 0.f;
    for (int t = a.split_task0[p]; t < a.split_task0[p + 1]; ++t) s += a.tm[(size_t)t * a.H + h];
    a.gadst[(size_t)r * a.H + h] = s;
}

// pass S over the out-edges (ptr / idx / perm are the CSC side's; the records are in its order)
template <int VEC, int G, int R> __global__ __launch_bounds__(BLOCK) void k_gat_bwd_s(const GatArgs a)
{
    using RowT = Row<VEC, G, R>;
    constexpr int NG = 64 / G;
    constexpr int U = gather_unroll(R);
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    const int h = blockIdx.y;
    bool wide;
    const RowUnit u = row_unit<G>(a, a.N, blockIdx.x, wave, gid, wide);
    const float *base = a.gout + h * a.C;
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
            act[q] = t < u.e1;
            const int e = act[q] ? u.qs + t : 0;
            x[q].load(base + (size_t)a.idx[e] * a.W, a.C, lg);
            rc[q] = *reinterpret_cast<const float2 *>(a.rec + ((size_t)e * a.H + h) * 2);
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
        acc.store(a.partial + ((size_t)u.tq * a.H + h) * a.C, a.C, lg);
        if (lg == 0) a.tm[(size_t)u.tq * a.H + h] = sda;
        return;
    }
    const size_t sh = (size_t)u.seg * a.H + h;
    if (lg == 0) a.gasrc[sh] = sda;
    if (a.out) {
        RowT w;
        w.load(a.att_src + h * a.C, a.C, lg);
        acc.axpy(sda, w);
        w.load(a.att_dst + h * a.C, a.C, lg);
        acc.axpy(a.gadst[sh], w);
        acc.store(a.out + (size_t)u.seg * a.W + h * a.C, a.C, lg);
    }
}

// split sources of pass S: the tasks' partial rows and sums in task order, then the store epilogue
static __global__ __launch_bounds__(256) void k_gat_bwd_s_fin(const GatArgs a)
{
    const int p = blockIdx.x, h = blockIdx.y;
    const int r = a.perm[p];
    const int t0 = a.split_task0[p], t1 = a.split_task0[p + 1];
    const size_t sh = (size_t)r * a.H + h;
    float sda = 0.f;
    for (int t = t0; t < t1; ++t) sda += a.tm[(size_t)t * a.H + h];
    if (threadIdx.x == 0) a.gasrc[sh] = sda;
    if (!a.out) return;
    const float gd = a.gadst[sh];
    for (int c = threadIdx.x; c < a.C; c += 256) {
        float s = 0.f;
        for (int t = t0; t < t1; ++t) s += a.partial[((size_t)t * a.H + h) * a.C + c];
        s += sda * a.att_src[h * a.C + c];
        s += gd * a.att_dst[h * a.C + c];
        a.out[(size_t)r * a.W + h * a.C + c] = s;
    }
}

// the score pass: a_src and a_dst [N, H] from one read of xp; the C products of a score are summed in double and
// rounded once.  Rows of xp are ld floats apart, rows of att_* lda (dense: H * C and C).
static __global__ __launch_bounds__(256) void k_gat_scores(const float *__restrict__ xp, int64_t ld,
                                                           const float *__restrict__ att_src,
                                                           const float *__restrict__ att_dst, int64_t lda, int64_t NH,
                                                           int H, int C, float *__restrict__ asrc,
                                                           float *__restrict__ adst)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NH) return;
    const int h = (int)(i % H);
    const float *row = xp + (i / H) * ld + (int64_t)h * C, *ws = att_src + h * lda, *wd = att_dst + h * lda;
    double s = 0.0, d = 0.0;
    for (int c = 0; c < C; ++c) {
        const double v = (double)row[c];
        s += v * (double)ws[c];
        d += v * (double)wd[c];
    }
    asrc[i] = (float)s;
    adst[i] = (float)d;
}

// grad_att: workgroup b's partial sums over its npb nodes, in double: part [B, 2, W]
static __global__ __launch_bounds__(256) void k_gat_att_part(const float *__restrict__ xp, int64_t ld,
                                                             const float *__restrict__ gasrc,
                                                             const float *__restrict__ gadst, int N, int H, int C, int npb,
                                                             double *__restrict__ part)
{
    const int W = H * C;
    const int n0 = blockIdx.x * npb, n1 = min(N, n0 + npb);
    for (int c = threadIdx.x; c < W; c += 256) {
        const int h = c / C;
        double s = 0.0, d = 0.0;
        for (int n = n0; n < n1; ++n) {
            const double v = (double)xp[(size_t)n * ld + c];
            s += (double)gasrc[(size_t)n * H + h] * v;
            d += (double)gadst[(size_t)n * H + h] * v;
        }
        part[((size_t)blockIdx.x * 2) * W + c] = s;
        part[((size_t)blockIdx.x * 2 + 1) * W + c] = d;
    }
}

// grad_att = the partials added in workgroup order: [2, H * C] (the source vector, then the target's), or - split - as
// WRGAT's atten [H, 2C], whose source half is [:, C:]
static __global__ __launch_bounds__(256) void k_gat_att_red(const double *__restrict__ part, int B, int H, int C,
                                                            int split, float *__restrict__ gatt)
{
    const int W = H * C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * W) return;
    const int which = i / W, c = i % W;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += part[((size_t)b * 2 + which) * W + c];
    gatt[split ? (size_t)(c / C) * 2 * C + (which == 0 ? C : 0) + c % C : i] = (float)s;
}

template <int VEC, int G, int R> int launch_gat_fwd(GatArgs a, hipStream_t st)
{
    const int nb = plan_side(a, a.N, 64 / G);
    if (nb > 0) k_gat_fwd<VEC, G, R><<<dim3(nb, a.H), BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_gat_fwd_fin<<<dim3(a.n_split, a.H), 256, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <int VEC, int G, int R> int launch_gat_bwd_t(GatArgs a, hipStream_t st)
{
    const int nb = plan_side(a, a.N, 64 / G);
    if (nb > 0) k_gat_bwd_t<VEC, G, R><<<dim3(nb, a.H), BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_gat_bwd_t_fin<<<a.n_split, 64, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <int VEC, int G, int R> int launch_gat_bwd_s(GatArgs a, hipStream_t st)
{
    const int nb = plan_side(a, a.N, 64 / G);
    if (nb > 0) k_gat_bwd_s<VEC, G, R><<<dim3(nb, a.H), BLOCK, 0, st>>>(a);
    if (a.n_split > 0) k_gat_bwd_s_fin<<<dim3(a.n_split, a.H), 256, 0, st>>>(a);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

SNGNN_DEFINE_DISPATCH(dispatch_gat_fwd, launch_gat_fwd, GatArgs)
SNGNN_DEFINE_DISPATCH(dispatch_gat_bwd_t, launch_gat_bwd_t, GatArgs)
SNGNN_DEFINE_DISPATCH(dispatch_gat_bwd_s, launch_gat_bwd_s, GatArgs)

static int gat_att_npb(int64_t N) { return (int)std::max<int64_t>(8, (N + GAT_ATT_BLOCKS - 1) / GAT_ATT_BLOCKS); }

// (common.h: the score pass, the grad_att partials on rows ld floats apart and their reducer - wrgat.hip enters them too)
int gat_att_blocks(int64_t N) { return ceil_div(std::max<int64_t>(N, 1), gat_att_npb(N)); }

int launch_gat_scores(const float *xp, int64_t ld, const float *att_src, const float *att_dst, int64_t lda, int64_t N,
                      int H, int C, float *a_src, float *a_dst, hipStream_t st)
{
    k_gat_scores<<<ceil_div(N * H, 256), 256, 0, st>>>(xp, ld, att_src, att_dst, lda, N * H, H, C, a_src, a_dst);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

int launch_gat_att_part(const float *xp, int64_t ld, const float *gasrc, const float *gadst, int64_t N, int H, int C,
                        double *part, hipStream_t st)
{
    k_gat_att_part<<<gat_att_blocks(N), 256, 0, st>>>(xp, ld, gasrc, gadst, (int)N, H, C, gat_att_npb(N), part);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

int launch_gat_att_red(const double *part, int64_t N, int H, int C, bool split, float *grad_att, hipStream_t st)
{
    k_gat_att_red<<<ceil_div(2 * H * C, 256), 256, 0, st>>>(part, gat_att_blocks(N), H, C, split, grad_att);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

// workspace regions (256-byte aligned): the tasks' partial rows | their two scalars per head | the edge records |
// grad_a_src | grad_a_dst | the grad_att partials
struct GatLayout { int64_t tml, rec, gasrc, gadst, att, total; };

static GatLayout gat_layout(const sngnn_graph_t *g, int H, int C)
{
    GatLayout L;
    const int64_t tasks = std::max(g->n_tasks, g->n_stasks);
    L.tml = up256(tasks * H * C * 4);
    L.rec = L.tml + up256(tasks * H * 2 * 4);
    L.gasrc = L.rec + up256(g->Ep * H * 2 * 4);
    L.gadst = L.gasrc + up256(g->N * H * 4);
    L.att = L.gadst + up256(g->N * H * 4);
    L.total = L.att + up256((int64_t)gat_att_blocks(g->N) * 2 * H * C * 8);
    return L;
}

}  // namespace sngnn

using namespace sngnn;

#define GAT_SHAPE(H, C)                                                                                                \
    SN_REQUIRE((H) >= 1 && (H) <= GAT_MAX_HEADS, SNGNN_ERANGE, "heads must be in [1, " + std::to_string(GAT_MAX_HEADS) + "]"); \
    SN_REQUIRE((C) >= 1 && (int64_t)(H) * (C) <= SNGNN_MAX_CHANNELS, SNGNN_ERANGE,                                     \
               "C must be at least 1 and heads * C at most " + std::to_string(SNGNN_MAX_CHANNELS));                    \
    RowCfg cfg;                                                                                                        \
    SN_REQUIRE(row_cfg((C), cfg), SNGNN_ERANGE, "unsupported channel layout")

#define GAT_GRAPH(g)                                                                                                   \
    SN_REQUIRE((g) != nullptr, SNGNN_EINVAL, "graph is NULL");                                                         \
    SN_REQUIRE(whole_graph_with_loops(g), SNGNN_EINVAL,                                                                \
               "the graph attention needs an unpartitioned graph built with add_loops = 1, remove_loops = "           \
               "SNGNN_LOOPS_REPLACE (GATConv's edge list)")

extern "C" int64_t sngnn_gat_workspace_bytes(const sngnn_graph_t *g, int H, int C)
{
    RowCfg cfg;
    if (g == nullptr || H < 1 || H > GAT_MAX_HEADS || C < 1 || (int64_t)H * C > SNGNN_MAX_CHANNELS || !row_cfg(C, cfg))
        return 0;
    return gat_layout(g, H, C).total;
}

extern "C" int sngnn_gat_scores(const float *xp, const float *att_src, const float *att_dst, int64_t N, int H, int C,
                                float *a_src, float *a_dst, void *stream)
{
    GAT_SHAPE(H, C);
    SN_REQUIRE(N >= 0 && N * (int64_t)H < (int64_t)1 << 31, SNGNN_ERANGE, "N * heads must fit 31 bits");
    if (N == 0) return SNGNN_OK;
    SN_REQUIRE(xp && att_src && att_dst && a_src && a_dst, SNGNN_EINVAL, "NULL argument");
    return launch_gat_scores(xp, (int64_t)H * C, att_src, att_dst, C, N, H, C, a_src, a_dst, (hipStream_t)stream);
}

extern "C" int sngnn_gat_forward(const sngnn_graph_t *g, const float *xp, const float *a_src, const float *a_dst, int H,
                                 int C, float negative_slope, float *out, float *ml, void *workspace, void *stream)
{
    GAT_GRAPH(g);
    GAT_SHAPE(H, C);
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(xp && a_src && a_dst && out && ml && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(rows_aligned(16, {xp, out, workspace}), SNGNN_EINVAL, "rows must be aligned to 16 bytes");
    const GatLayout L = gat_layout(g, H, C);
    GatArgs a = {};
    bind_softmax_side(g, false, a);
    a.xp = xp; a.asrc = a_src; a.adst = a_dst; a.out = out;
    a.m = ml; a.l = ml + g->N * (int64_t)H;
    a.partial = (float *)workspace;
    a.tm = (float *)((char *)workspace + L.tml); a.tl = a.tm + (int64_t)a.n_tasks * H;
    a.slope = negative_slope; a.H = H; a.C = C; a.W = H * C;
    return dispatch_gat_fwd(cfg, a, (hipStream_t)stream);
}

extern "C" int sngnn_gat_backward(const sngnn_graph_t *g, const float *grad_out, const float *xp, const float *out,
                                  const float *a_src, const float *a_dst, const float *ml, const float *att_src,
                                  const float *att_dst, int H, int C, float negative_slope, float *grad_xp,
                                  float *grad_att, void *workspace, void *stream)
{
    GAT_GRAPH(g);
    GAT_SHAPE(H, C);
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(grad_out && xp && out && a_src && a_dst && ml && att_src && att_dst && workspace, SNGNN_EINVAL,
               "NULL argument");
    SN_REQUIRE(rows_aligned(16, {grad_out, xp, out, att_src, att_dst, grad_xp, workspace}), SNGNN_EINVAL,
               "rows must be aligned to 16 bytes");
    hipStream_t st = (hipStream_t)stream;
    const GatLayout L = gat_layout(g, H, C);
    GatArgs a = {};
    a.xp = xp; a.gout = grad_out; a.fout = out; a.asrc = a_src; a.adst = a_dst;
    a.m = const_cast<float *>(ml); a.l = a.m + g->N * (int64_t)H;
    a.partial = (float *)workspace;
    a.tm = (float *)((char *)workspace + L.tml);
    a.rec = (float *)((char *)workspace + L.rec);
    a.gasrc = (float *)((char *)workspace + L.gasrc);
    a.gadst = (float *)((char *)workspace + L.gadst);
    a.att_src = att_src; a.att_dst = att_dst;
    a.slope = negative_slope; a.H = H; a.C = C; a.W = H * C;
    bind_softmax_side(g, false, a);
    int rc = dispatch_gat_bwd_t(cfg, a, st);
    if (rc != SNGNN_OK) return rc;
    bind_softmax_side(g, true, a);
    a.out = grad_xp;
    rc = dispatch_gat_bwd_s(cfg, a, st);
    if (rc != SNGNN_OK) return rc;
    if (grad_att) {
        double *part = (double *)((char *)workspace + L.att);
        rc = launch_gat_att_part(xp, (int64_t)H * C, a.gasrc, a.gadst, g->N, H, C, part, st);
        if (rc != SNGNN_OK) return rc;
        return launch_gat_att_red(part, g->N, H, C, false, grad_att, st);
    }
    return SNGNN_OK;
}

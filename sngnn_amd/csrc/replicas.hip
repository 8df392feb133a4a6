// R replicas of one 1-layer model trained together (sngnn_amd/splits.py): the reference's sweep
// scripts train every dataset once per geom-gcn split (train_script_SNGNN*.sh: part_id 0..9, and
// init_beta over five values for SNGNN++) - one process per run, each run almost all latency.  Here
// replica r's node i is row r N + i of a block-diagonal union graph, so the aggregation kernels run
// unchanged on it; what is specific to the replicas is this file:
//
//   sngnn_replica_unpack        the stacked lin output [N, R Cp] (x read once by one GEMM) -> the union
//                               table [R N, Cp] + bias, with the unit rows / norms / fp16 filter rows of
//                               k_normalize_rows from the same registers (replaces the normalisation pass)
//   sngnn_replica_wgrad         grad_W[r] = G_r^T x, grad_b[r] = sum_i G_r[i] for all replicas with x read
//                               once per 64 stacked channels; per element the summation order of
//                               sngnn_linear_wgrad's FMA path (k_wgrad_partial + k_sum_partials)
//   sngnn_replica_head_nll      log_softmax + masked mean NLL + correct count per replica (training: one
//                               split and d loss / d logits scaled by 1 / count_r; evaluation: two splits),
//                               optionally on SNGNN++'s blend with a per-replica beta formed in registers;
//                               per replica the workgroups, per-row arithmetic and summation tree of
//                               sngnn_head_nll / _nll2 / _nll_blend on that replica's rows
//   sngnn_replica_blend_*       the blend with beta[R]: forward, and backward with d beta[R], per replica
//                               the grid and reduction tree of sngnn_blend_backward
// Every sum is fixed-order: no float atomics.  Nothing here blocks the host.
#include "agg_fwd_filter.h"
#include "agg_fwd_select.h"
#include "entry.h"
#include "head_row.h"

namespace sngnn {

namespace {

// ---------------------------------------------------------------------------
// Unpack + bias + F.normalize: union row u = r N + i <- hs[i, r C .. r C + C) + bias[r].  The
// lane layout, loop and normalisation are k_normalize_rows' (agg_fwd_roles.h), so n / nrm / filt are
// the bits sngnn_normalize_rows_filter computes from the unpacked rows.
// ---------------------------------------------------------------------------
template <int VEC, int G, int R>
__global__ __launch_bounds__(BLOCK) void k_rep_unpack(const float *__restrict__ hs, const float *__restrict__ bias,
                                                      int64_t N, int NR, int C, float *__restrict__ h,
                                                      float *__restrict__ n, float *__restrict__ nrm,
                                                      uint2 *__restrict__ filt)
{
    using RowT = Row<VEC, G, R>;
    constexpr int RPW = 64 / G;
    constexpr int U = Unroll<R>::U >= 2 ? 2 : 1;
    const int lane = lane_id();
    const int gid = lane / G, lg = lane % G;
    const int64_t rows = N * NR;
    const int64_t stride = (int64_t)NR * C;
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    const int64_t w0 = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    for (int64_t base = w0 * RPW * U; base < rows; base += nw * RPW * U) {
        RowT x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t uu = base + u * RPW + gid;
            const int64_t q = uu < rows ? uu : rows - 1;
            const int64_t r = q / N, i = q - r * N;
            x[u].load(hs + i * stride + r * C, C, lg);
            if (bias != nullptr) {
                RowT b;
                b.load(bias + r * C, C, lg);
#pragma unroll
                for (int s = 0; s < R; ++s)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u].x[s][v] = x[u].x[s][v] + b.x[s][v];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t uu = base + u * RPW + gid;
            if (uu < rows) x[u].store(h + uu * C, C, lg);
            if (n == nullptr) continue;
            const float q = group_sum<G>(x[u].dot_partial(x[u]));
            const float d = fmaxf(ieee_sqrt(q), EPS_NORM);
            x[u].div_rn(d);
            if (uu < rows) {
                x[u].store(n + uu * C, C, lg);
                if (lg == 0) nrm[uu] = d;
                if constexpr (VEC == 4) {
                    if (filt) {
#pragma unroll
                        for (int s = 0; s < R; ++s)
                            filt[(size_t)uu * (G * R) + s * G + lg] =
                                make_uint2(pack_half2(x[u].x[s][0] * FILT_SCALE, x[u].x[s][1] * FILT_SCALE),
                                           pack_half2(x[u].x[s][2] * FILT_SCALE, x[u].x[s][3] * FILT_SCALE));
                    }
                }
            }
        }
    }
}

template <int VEC, int G, int R>
int launch_rep_unpack(const float *hs, const float *bias, int64_t N, int NR, int C, float *h, float *n, float *nrm,
                      void *filt, hipStream_t st)
{
    constexpr int RPW = 64 / G;
    constexpr int U = Unroll<R>::U >= 2 ? 2 : 1;
    const int64_t rows = N * NR;
    if (rows <= 0) return SNGNN_OK;
    const int64_t steps = (rows + RPW * U - 1) / (RPW * U);
    const int grid = (int)std::min<int64_t>(ceil_div(steps, WAVES), 256 * 8 * 4);
    if (filt && !(VEC == 4 && filter_row_bytes(C) == 8 * G * R)) {
        set_error("internal: filter rows need 16-byte row vectors");
        return SNGNN_EINVAL;
    }
    k_rep_unpack<VEC, G, R><<<grid, BLOCK, 0, st>>>(hs, bias, N, NR, C, h, n, nrm, (uint2 *)filt);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

int dispatch_rep_unpack(const RowCfg &cfg, const float *hs, const float *bias, int64_t N, int NR, int C, float *h,
                        float *n, float *nrm, void *filt, hipStream_t st)
{
    return dispatch_vec(cfg, [&](auto vec) {
        SNGNN_DISPATCH_GR(launch_rep_unpack, decltype(vec)::value, cfg, hs, bias, N, NR, C, h, n, nrm, filt, st)
    });
}

// ---------------------------------------------------------------------------
// Weight gradient over the stacked channels v = r C + c: k_wgrad_partial (head.hip) with the g tile
// read from the union layout G[(r N + i) C + c].  The order in which one output element accumulates
// depends on N only (WG_ROWS-row chunks, four 128-row quarters combined in fixed order, chunks summed
// by 16 strided threads then in order), so replica r's gradient is the single layer's bit for bit.
// ---------------------------------------------------------------------------
constexpr int RW_ROWS = 512, RW_FT = 128, RW_STEP = 16, RW_SUB = 4;

template <int KACC>
__global__ __launch_bounds__(256 * RW_SUB) void k_rep_wgrad_partial(const float *__restrict__ g,
                                                                    const float *__restrict__ x, int64_t N, int C,
                                                                    int RC, int F, float *__restrict__ part,
                                                                    float *__restrict__ part_b)
{
    constexpr int CT = 2 * KACC;
    static_assert(KACC % 4 == 0, "16-byte LDS reads");
    __shared__ __attribute__((aligned(16))) float sg[RW_SUB][RW_STEP][CT];
    __shared__ float sred[RW_SUB - 1][256];
    const int sub = threadIdx.x >> 8, tid = threadIdx.x & 255;
    const int fl = tid & (RW_FT - 1), half = tid >> 7;
    const int f = blockIdx.x * RW_FT + fl;
    const int ct0 = blockIdx.y * CT, c0 = ct0 + half * KACC;
    const int64_t rb = (int64_t)blockIdx.z * RW_ROWS + sub * (RW_ROWS / RW_SUB);
    const int64_t r1 = min(N, rb + RW_ROWS / RW_SUB);
    float acc[KACC], bacc[KACC];
#pragma unroll
    for (int k = 0; k < KACC; ++k) { acc[k] = 0.f; bacc[k] = 0.f; }
    const bool fok = f < F;
    const bool do_bias = part_b != nullptr && blockIdx.x == 0 && fl == 0;
    int64_t ib = rb;
    for (int it = 0; it < RW_ROWS / RW_SUB / RW_STEP; ib += RW_STEP, ++it) {
        float xv[RW_STEP];
#pragma unroll
        for (int r = 0; r < RW_STEP; ++r)
            xv[r] = (fok && ib + r < r1) ? x[(ib + r) * F + f] : 0.f;
        __syncthreads();
        for (int q = tid; q < RW_STEP * CT; q += 256) {
            const int r = q / CT, c = q % CT;
            const int v = ct0 + c;
            const int rep = v / C, cc = v - rep * C;
            sg[sub][r][c] = (ib + r < r1 && v < RC) ? g[((int64_t)rep * N + ib + r) * C + cc] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RW_STEP; ++r)
#pragma unroll
            for (int k4 = 0; k4 < KACC / 4; ++k4) {
                const float4 gv = *reinterpret_cast<const float4 *>(&sg[sub][r][half * KACC + 4 * k4]);
                acc[4 * k4 + 0] = fmaf(gv.x, xv[r], acc[4 * k4 + 0]);
                acc[4 * k4 + 1] = fmaf(gv.y, xv[r], acc[4 * k4 + 1]);
                acc[4 * k4 + 2] = fmaf(gv.z, xv[r], acc[4 * k4 + 2]);
                acc[4 * k4 + 3] = fmaf(gv.w, xv[r], acc[4 * k4 + 3]);
                if (do_bias) {
                    bacc[4 * k4 + 0] += gv.x; bacc[4 * k4 + 1] += gv.y;
                    bacc[4 * k4 + 2] += gv.z; bacc[4 * k4 + 3] += gv.w;
                }
            }
    }
#pragma unroll
    for (int k = 0; k < KACC; ++k) {
        __syncthreads();
        if (sub > 0) sred[sub - 1][tid] = acc[k];
        __syncthreads();
        if (sub == 0) acc[k] = ((acc[k] + sred[0][tid]) + sred[1][tid]) + sred[2][tid];
        if (part_b != nullptr && blockIdx.x == 0) {
            __syncthreads();
            if (sub > 0) sred[sub - 1][tid] = bacc[k];
            __syncthreads();
            if (sub == 0) bacc[k] = ((bacc[k] + sred[0][tid]) + sred[1][tid]) + sred[2][tid];
        }
    }
    if (sub != 0) return;
#pragma unroll
    for (int k = 0; k < KACC; ++k)
        if (c0 + k < RC) {
            if (fok) part[((size_t)blockIdx.z * RC + (c0 + k)) * F + f] = acc[k];
            if (do_bias) part_b[(size_t)blockIdx.z * RC + c0 + k] = bacc[k];
        }
}

// k_sum_partials (head.hip): 16 threads per output take every 16th chunk, then add in fixed order
template <typename ACC>
__global__ __launch_bounds__(256) void k_rep_sum_partials(const float *__restrict__ partA, int64_t lenA,
                                                          float *__restrict__ outA, int nbA,
                                                          const float *__restrict__ partB, int64_t lenB,
                                                          float *__restrict__ outB, int nchunks)
{
    __shared__ ACC s[16][16];
    const bool second = (int)blockIdx.x >= nbA;
    const float *part = second ? partB : partA;
    float *out = second ? outB : outA;
    const int64_t len = second ? lenB : lenA;
    const int blk = second ? blockIdx.x - nbA : blockIdx.x;
    const int o = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int64_t j = (int64_t)blk * 16 + o;
    ACC a = 0;
    if (j < len)
        for (int k = q; k < nchunks; k += 16) a += (ACC)part[(size_t)k * len + j];
    s[q][o] = a;
    __syncthreads();
    if (q == 0 && j < len) {
        ACC t = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += s[w][o];
        out[j] = (float)t;
    }
}

// ---------------------------------------------------------------------------
// Head over replicas.  blockIdx.y = replica; the x dimension is the single head's grid over that
// replica's N rows (same block count, same grid stride), so every per-block partial and the final
// double-precision tree of k_head_reduce are the single call's on that slice.  BLEND: the logits are
// beta[r] z + (1 - beta[r]) z1, each product and the sum rounded (k_blend_fwd's arithmetic).
// ---------------------------------------------------------------------------
constexpr int REP_HEAD_MAX_BLOCKS = 2048;      // HEAD_MAX_BLOCKS (head.hip)

__device__ __forceinline__ float rep_scale(const int64_t *counts, int j)
{
    const int64_t n = counts[j];
    return 1.0f / (float)(n > 0 ? n : 1);
}

// k_head_rows<false, TWO> (head.hip), lane per row, any C <= 64
template <bool TWO, bool BLEND>
__global__ __launch_bounds__(256) void k_rep_head_rows(const float *__restrict__ z0, const float *__restrict__ z1,
                                                       const float *__restrict__ beta, const int64_t *__restrict__ y,
                                                       const unsigned char *__restrict__ sel0,
                                                       const int64_t *__restrict__ counts, int64_t N, int C,
                                                       float *__restrict__ grad0, float *__restrict__ part0)
{
    __shared__ float s_loss[4], s_corr[4], s_lossb[4], s_corrb[4];
    const int rep = blockIdx.y;
    const float *z = z0 + (size_t)rep * N * C;
    const float *zb = BLEND ? z1 + (size_t)rep * N * C : nullptr;
    const unsigned char *sel = sel0 + (size_t)rep * N;
    float *grad = grad0 ? grad0 + (size_t)rep * N * C : nullptr;
    float *part = part0 + (size_t)rep * gridDim.x * (TWO ? 4 : 2);
    const float scale = TWO ? 0.f : rep_scale(counts, rep);
    float bb = 0.f, nbb = 0.f;
    if constexpr (BLEND) { bb = beta[rep]; nbb = 1.0f - bb; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float loss = 0.f, corr = 0.f, lossb = 0.f, corrb = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const unsigned char sv = sel[i];
        float *gi = grad ? grad + i * C : nullptr;
        if (sv == 0) {
            if (gi)
                for (int c = 0; c < C; ++c) gi[c] = 0.f;
            continue;
        }
        const float *zi = z + i * C;
        const int yi = (int)y[i];
        float v[64];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (4 * k < C) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = -INFINITY;
                    if (4 * k + e < C) {
                        t = zi[4 * k + e];
                        if constexpr (BLEND) t = bb * t + nbb * zb[i * C + 4 * k + e];
                    }
                    v[4 * k + e] = t;
                }
            }
        }
        float mx = -INFINITY, zy = 0.f;
        int arg = 0;
#pragma unroll
        for (int c = 0; c < 64; ++c)
            if (c < C) {
                if (v[c] > mx) { mx = v[c]; arg = c; }
                if (c == yi) zy = v[c];
            }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < 64; ++c)
            if (c < C) { v[c] = expf(v[c] - mx); se += v[c]; }
        const float row_loss = -(zy - mx - logf(se)), row_corr = (arg == yi) ? 1.f : 0.f;
        if constexpr (TWO) {
            if (sv & 1) { loss += row_loss; corr += row_corr; }
            if (sv & 2) { lossb += row_loss; corrb += row_corr; }
        } else {
            loss += row_loss;
            corr += row_corr;
        }
        if (gi) {
            const float inv = scale / se;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (4 * k < C) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * k + e < C) gi[4 * k + e] = v[4 * k + e] * inv - (4 * k + e == yi ? scale : 0.f);
                }
            }
        }
    }
    loss = wave_sum_f(loss);
    corr = wave_sum_f(corr);
    if constexpr (TWO) { lossb = wave_sum_f(lossb); corrb = wave_sum_f(corrb); }
    if (lane == 0) { s_loss[wave] = loss; s_corr[wave] = corr; s_lossb[wave] = lossb; s_corrb[wave] = corrb; }
    __syncthreads();
    if (threadIdx.x == 0 && TWO) {
        part[4 * blockIdx.x] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
        part[4 * blockIdx.x + 1] = (s_corr[0] + s_corr[1]) + (s_corr[2] + s_corr[3]);
        part[4 * blockIdx.x + 2] = (s_lossb[0] + s_lossb[1]) + (s_lossb[2] + s_lossb[3]);
        part[4 * blockIdx.x + 3] = (s_corrb[0] + s_corrb[1]) + (s_corrb[2] + s_corrb[3]);
    } else if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
        part[2 * blockIdx.x + 1] = (s_corr[0] + s_corr[1]) + (s_corr[2] + s_corr[3]);
    }
}

// k_head_groups<G, TWO> (head.hip), lane groups of 16-byte vectors, C % 4 == 0, C <= 64
template <int G, bool TWO, bool BLEND>
__global__ __launch_bounds__(256) void k_rep_head_groups(const float *__restrict__ z0, const float *__restrict__ z1,
                                                         const float *__restrict__ beta, const int64_t *__restrict__ y,
                                                         const unsigned char *__restrict__ sel0,
                                                         const int64_t *__restrict__ counts, int64_t N, int C,
                                                         float *__restrict__ grad0, float *__restrict__ part0)
{
    constexpr int RPW = 64 / G, U = 2;
    __shared__ float s_loss[4], s_corr[4], s_lossb[4], s_corrb[4];
    const int rep = blockIdx.y;
    const float *z = z0 + (size_t)rep * N * C;
    const float *zb = BLEND ? z1 + (size_t)rep * N * C : nullptr;
    const unsigned char *sel = sel0 + (size_t)rep * N;
    float *grad = grad0 ? grad0 + (size_t)rep * N * C : nullptr;
    float *part = part0 + (size_t)rep * gridDim.x * (TWO ? 4 : 2);
    const float scale = TWO ? 0.f : rep_scale(counts, rep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    const bool in = 4 * lg < C;
    const int c0 = in ? 4 * lg : 0;
    float loss = 0.f, corr = 0.f, lossb = 0.f, corrb = 0.f;
    const int64_t nw = (int64_t)gridDim.x * 4, w0 = (int64_t)blockIdx.x * 4 + wave;
    for (int64_t base = w0 * (RPW * U); base < N; base += nw * (RPW * U)) {
        float4 t[U];
        int yi[U];
        unsigned char sv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + u * RPW + gid;
            const int64_t ic = i < N ? i : N - 1;
            sv[u] = i < N ? sel[ic] : (unsigned char)0;
            t[u] = *reinterpret_cast<const float4 *>(z + ic * C + c0);
            yi[u] = (int)y[ic];
        }
        if constexpr (BLEND) {
            const float b = beta[rep], nb_ = 1.0f - b;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = base + u * RPW + gid;
                const int64_t ic = i < N ? i : N - 1;
                const float4 o1 = *reinterpret_cast<const float4 *>(zb + ic * C + c0);
                t[u] = make_float4(b * t[u].x + nb_ * o1.x, b * t[u].y + nb_ * o1.y, b * t[u].z + nb_ * o1.z,
                                   b * t[u].w + nb_ * o1.w);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + u * RPW + gid;
            if (i >= N) continue;
            float *gi = grad ? grad + i * C + c0 : nullptr;
            if (sv[u] == 0) {
                if (gi && in) *reinterpret_cast<float4 *>(gi) = make_float4(0.f, 0.f, 0.f, 0.f);
                continue;
            }
            const HeadRow hr = head_row<G>(t[u], in, c0, yi[u]);
            if (lg == 0) {
                if constexpr (TWO) {
                    if (sv[u] & 1) { loss += hr.loss; corr += hr.corr; }
                    if (sv[u] & 2) { lossb += hr.loss; corrb += hr.corr; }
                } else {
                    loss += hr.loss;
                    corr += hr.corr;
                }
            }
            if (gi && in) *reinterpret_cast<float4 *>(gi) = head_row_grad(hr, scale);
        }
    }
    loss = wave_sum_f(loss);
    corr = wave_sum_f(corr);
    if constexpr (TWO) { lossb = wave_sum_f(lossb); corrb = wave_sum_f(corrb); }
    if (lane == 0) { s_loss[wave] = loss; s_corr[wave] = corr; s_lossb[wave] = lossb; s_corrb[wave] = corrb; }
    __syncthreads();
    if (threadIdx.x == 0 && TWO) {
        part[4 * blockIdx.x] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
        part[4 * blockIdx.x + 1] = (s_corr[0] + s_corr[1]) + (s_corr[2] + s_corr[3]);
        part[4 * blockIdx.x + 2] = (s_lossb[0] + s_lossb[1]) + (s_lossb[2] + s_lossb[3]);
        part[4 * blockIdx.x + 3] = (s_corrb[0] + s_corrb[1]) + (s_corrb[2] + s_corrb[3]);
    } else if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
        part[2 * blockIdx.x + 1] = (s_corr[0] + s_corr[1]) + (s_corr[2] + s_corr[3]);
    }
}

// k_head_reduce (head.hip) per (replica, split): block (r, s) sums the pair at offset 2 s of the
// replica's `stride`-float partials; out row r at out + r * out_stride
__global__ __launch_bounds__(256) void k_rep_head_reduce(const float *__restrict__ part0, int nblocks,
                                                         const int64_t *__restrict__ counts, int sets,
                                                         float *__restrict__ out0, int64_t out_stride)
{
    __shared__ double s[2][256];
    const int rep = blockIdx.y, set = blockIdx.x;
    const int stride = 2 * sets;
    const float *part = part0 + (size_t)rep * nblocks * stride + 2 * set;
    float *out = out0 + rep * out_stride + 2 * set;
    const float scale = rep_scale(counts, rep * sets + set);
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) { a += part[(size_t)stride * i]; b += part[(size_t)stride * i + 1]; }
    s[0][threadIdx.x] = a;
    s[1][threadIdx.x] = b;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) { s[0][threadIdx.x] += s[0][threadIdx.x + m]; s[1][threadIdx.x] += s[1][threadIdx.x + m]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = (float)(s[0][0] * (double)scale); out[1] = (float)s[1][0]; }
}

// ---------------------------------------------------------------------------
// Blend with beta[R] (blend.hip's k_blend_fwd / k_blend_bwd / k_blend_reduce per replica slice of n
// elements; blockIdx.y = replica, the x dimension is blend_grid(n)).
// ---------------------------------------------------------------------------
constexpr int REP_BLEND_BLOCKS = 1024;       // BLEND_BLOCKS (blend.hip)

int rep_blend_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(REP_BLEND_BLOCKS, (n / 4 + 255) / 256)); }

__global__ __launch_bounds__(256) void k_rep_blend_fwd(const float *__restrict__ o0_, const float *__restrict__ o1_,
                                                       const float *__restrict__ beta, int64_t n4, int64_t n,
                                                       float *__restrict__ out_)
{
    const int rep = blockIdx.y;
    const float *o0 = o0_ + (size_t)rep * n, *o1 = o1_ + (size_t)rep * n;
    float *out = out_ + (size_t)rep * n;
    const float b = beta[rep], nb = 1.0f - b;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 x = reinterpret_cast<const float4 *>(o0)[i], y = reinterpret_cast<const float4 *>(o1)[i];
        reinterpret_cast<float4 *>(out)[i] = make_float4(b * x.x + nb * y.x, b * x.y + nb * y.y, b * x.z + nb * y.z,
                                                          b * x.w + nb * y.w);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        out[i] = b * o0[i] + nb * o1[i];
}

__global__ __launch_bounds__(256) void k_rep_blend_bwd(const float *__restrict__ g_, const float *__restrict__ o0_,
                                                       const float *__restrict__ o1_, const float *__restrict__ beta,
                                                       int64_t n4, int64_t n, float *__restrict__ g0_,
                                                       float *__restrict__ g1_, float *__restrict__ part_)
{
    __shared__ float s[256];
    const int rep = blockIdx.y;
    const size_t off = (size_t)rep * n;
    const float *g = g_ + off, *o0 = o0_ + off, *o1 = o1_ + off;
    float *g0 = g0_ + off, *g1 = g1_ + off;
    float *part = part_ + (size_t)rep * gridDim.x;
    const float b = beta[rep], nb = 1.0f - b;
    const int64_t stride = (int64_t)gridDim.x * 256;
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 x = reinterpret_cast<const float4 *>(o0)[i], y = reinterpret_cast<const float4 *>(o1)[i];
        const float4 d = reinterpret_cast<const float4 *>(g)[i];
        reinterpret_cast<float4 *>(g0)[i] = make_float4(b * d.x, b * d.y, b * d.z, b * d.w);
        reinterpret_cast<float4 *>(g1)[i] = make_float4(nb * d.x, nb * d.y, nb * d.z, nb * d.w);
        acc += (d.x * (x.x - y.x) + d.y * (x.y - y.y)) + (d.z * (x.z - y.z) + d.w * (x.w - y.w));
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float d = g[i];
        g0[i] = b * d;
        g1[i] = nb * d;
        acc += d * (o0[i] - o1[i]);
    }
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void k_rep_blend_reduce(const float *__restrict__ part_, int nblocks,
                                                          float *__restrict__ dbeta)
{
    __shared__ double s[256];
    const float *part = part_ + (size_t)blockIdx.x * nblocks;
    double a = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) a += part[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) dbeta[blockIdx.x] = (float)s[0];
}

}  // namespace

}  // namespace sngnn

using namespace sngnn;

extern "C" int sngnn_replica_unpack(const float *hs, const float *bias, int64_t N, int R, int C, float *h, float *n,
                                    float *nrm, void *filt, void *stream)
{
    SN_REQUIRE(N >= 0 && R >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(N * R < ((int64_t)1 << 31), SNGNN_ERANGE, "R N must stay below 2^31");
    if (N == 0) return SNGNN_OK;
    SN_REQUIRE(hs && h, SNGNN_EINVAL, "hs/h is NULL");
    SN_REQUIRE((n == nullptr) == (nrm == nullptr), SNGNN_EINVAL, "n and nrm go together");
    SN_REQUIRE(filt == nullptr || n != nullptr, SNGNN_EINVAL, "filter rows need the unit rows");
    RowCfg cfg;
    if (int rc = check_rows(C, 0, {hs, h, n, bias}, cfg)) return rc;
    SN_REQUIRE(filt == nullptr || filter_row_bytes(C) > 0, SNGNN_EINVAL,
               "no filter rows for this C (sngnn_filter_row_bytes(C) == 0)");
    SN_REQUIRE(((uintptr_t)filt % 16) == 0, SNGNN_EINVAL, "filt must be 16-byte aligned");
    return dispatch_rep_unpack(cfg, hs, bias, N, R, C, h, n, nrm, filt, (hipStream_t)stream);
}

extern "C" int64_t sngnn_replica_wgrad_workspace_bytes(int64_t N, int R, int C, int F)
{
    const int64_t chunks = (N + RW_ROWS - 1) / RW_ROWS;
    return chunks * (int64_t)R * C * (F + 1) * 4 + 256;
}

extern "C" int sngnn_replica_wgrad(const float *grad_out, const float *x, int64_t N, int R, int C, int F,
                                   float *grad_weight, float *grad_bias, void *workspace, void *stream)
{
    SN_REQUIRE(N >= 0 && R >= 1 && C >= 1 && F >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE((int64_t)R * C <= (1 << 20) && N * R < ((int64_t)1 << 31), SNGNN_ERANGE, "too many stacked rows");
    SN_REQUIRE(grad_out && x && grad_weight && workspace, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int RC = R * C;
    const int chunks = (int)((N + RW_ROWS - 1) / RW_ROWS);
    float *part = (float *)workspace;
    float *part_b = part + (size_t)chunks * RC * F;
    if (chunks > 0) {
        const int kacc = RC <= 16 ? 8 : RC <= 32 ? 16 : RC <= 40 ? 20 : RC <= 48 ? 24 : 32;
        dim3 grid((F + RW_FT - 1) / RW_FT, (RC + 2 * kacc - 1) / (2 * kacc), chunks);
        SN_REQUIRE(grid.y <= 65535u, SNGNN_ERANGE, "too many stacked channels");
        float *pb = grad_bias ? part_b : nullptr;
        switch (kacc) {
        case 8: k_rep_wgrad_partial<8><<<grid, 256 * RW_SUB, 0, st>>>(grad_out, x, N, C, RC, F, part, pb); break;
        case 16: k_rep_wgrad_partial<16><<<grid, 256 * RW_SUB, 0, st>>>(grad_out, x, N, C, RC, F, part, pb); break;
        case 20: k_rep_wgrad_partial<20><<<grid, 256 * RW_SUB, 0, st>>>(grad_out, x, N, C, RC, F, part, pb); break;
        case 24: k_rep_wgrad_partial<24><<<grid, 256 * RW_SUB, 0, st>>>(grad_out, x, N, C, RC, F, part, pb); break;
        default: k_rep_wgrad_partial<32><<<grid, 256 * RW_SUB, 0, st>>>(grad_out, x, N, C, RC, F, part, pb); break;
        }
    }
    const int64_t len = (int64_t)RC * F;
    const int nbA = (int)((len + 15) / 16), nbB = grad_bias ? (RC + 15) / 16 : 0;
    // (many partials: added in double - a lane's fp32 chain over 1 024 of them alone missed the float64 gate at 8.4 M rows)
    if (chunks > WGRAD_WIDE_SUM_CHUNKS)
        k_rep_sum_partials<double><<<nbA + nbB, 256, 0, st>>>(part, len, grad_weight, nbA, part_b, RC, grad_bias, chunks);
    else
        k_rep_sum_partials<float><<<nbA + nbB, 256, 0, st>>>(part, len, grad_weight, nbA, part_b, RC, grad_bias, chunks);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int64_t sngnn_replica_head_workspace_bytes(int R)
{
    return (int64_t)(R > 0 ? R : 1) * REP_HEAD_MAX_BLOCKS * 16 + 256;
}

extern "C" int sngnn_replica_head_nll(const float *logits, const float *logits1, const float *beta, const int64_t *y,
                                      const unsigned char *sel, const int64_t *counts, int64_t N, int R, int C, int sets,
                                      float *grad_logits, float *metrics, int64_t metrics_stride, void *workspace,
                                      void *stream)
{
    SN_REQUIRE(N >= 0 && R >= 1 && C >= 1 && C <= 64, SNGNN_EINVAL, "sngnn_replica_head_nll needs 1 <= C <= 64");
    SN_REQUIRE(R <= 65535, SNGNN_ERANGE, "at most 65535 replicas");
    SN_REQUIRE(sets == 1 || sets == 2, SNGNN_EINVAL, "sets must be 1 or 2");
    SN_REQUIRE(grad_logits == nullptr || sets == 1, SNGNN_EINVAL, "the gradient is one split's");
    SN_REQUIRE(logits && y && sel && counts && metrics && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((logits1 == nullptr) == (beta == nullptr), SNGNN_EINVAL, "the blend needs logits1 and beta");
    SN_REQUIRE(metrics_stride >= 2 * sets, SNGNN_EINVAL, "metrics rows overlap");
    hipStream_t st = (hipStream_t)stream;
    const bool blend = logits1 != nullptr;
    // sngnn_head_nll / _nll2 / _nll_blend's choice: 16-byte row vectors take the lane-group kernel
    const bool vec4 = C % 4 == 0 && ((uintptr_t)logits | (uintptr_t)logits1 | (uintptr_t)grad_logits) % 16 == 0;
    const int nb = (int)std::min<int64_t>(vec4 ? (N + 31) / 32 : (N + 255) / 256, REP_HEAD_MAX_BLOCKS);
    float *part = (float *)workspace;
    if (nb > 0) {
        dim3 grid(nb, R);
#define REP_HEAD(KERNEL, ...) KERNEL<__VA_ARGS__><<<grid, 256, 0, st>>>(logits, logits1, beta, y, sel, counts, N, C, grad_logits, part)
        if (vec4 && C <= 32) {
            if (sets == 2) { if (blend) REP_HEAD(k_rep_head_groups, 8, true, true); else REP_HEAD(k_rep_head_groups, 8, true, false); }
            else { if (blend) REP_HEAD(k_rep_head_groups, 8, false, true); else REP_HEAD(k_rep_head_groups, 8, false, false); }
        } else if (vec4) {
            if (sets == 2) { if (blend) REP_HEAD(k_rep_head_groups, 16, true, true); else REP_HEAD(k_rep_head_groups, 16, true, false); }
            else { if (blend) REP_HEAD(k_rep_head_groups, 16, false, true); else REP_HEAD(k_rep_head_groups, 16, false, false); }
        } else {
            if (sets == 2) { if (blend) REP_HEAD(k_rep_head_rows, true, true); else REP_HEAD(k_rep_head_rows, true, false); }
            else { if (blend) REP_HEAD(k_rep_head_rows, false, true); else REP_HEAD(k_rep_head_rows, false, false); }
        }
#undef REP_HEAD
    }
    k_rep_head_reduce<<<dim3(sets, R), 256, 0, st>>>(part, nb, counts, sets, metrics, metrics_stride);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int64_t sngnn_replica_blend_workspace_bytes(int R)
{
    return (int64_t)(R > 0 ? R : 1) * REP_BLEND_BLOCKS * 4 + 256;
}

extern "C" int sngnn_replica_blend_forward(const float *out0, const float *out1, const float *beta, int64_t n, int R,
                                           float *out, void *stream)
{
    SN_REQUIRE(n >= 0 && R >= 1 && R <= 65535, SNGNN_EINVAL, "bad shape");
    if (n == 0) return SNGNN_OK;
    SN_REQUIRE(out0 && out1 && beta && out, SNGNN_EINVAL, "NULL argument");
    // every replica's slice starts 16-byte aligned iff the base does and n % 4 == 0
    const bool al = ((uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)out) % 16 == 0 && n % 4 == 0;
    k_rep_blend_fwd<<<dim3(rep_blend_grid(n), R), 256, 0, (hipStream_t)stream>>>(out0, out1, beta, al ? n / 4 : 0, n, out);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_replica_blend_backward(const float *grad_out, const float *out0, const float *out1,
                                            const float *beta, int64_t n, int R, float *grad0, float *grad1,
                                            float *grad_beta, void *workspace, void *stream)
{
    SN_REQUIRE(n >= 0 && R >= 1 && R <= 65535, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(grad_beta && workspace, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    int nb = 0;
    if (n > 0) {
        SN_REQUIRE(grad_out && out0 && out1 && beta && grad0 && grad1, SNGNN_EINVAL, "NULL argument");
        const bool al = ((uintptr_t)grad_out | (uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)grad0 |
                         (uintptr_t)grad1) % 16 == 0 && n % 4 == 0;
        nb = rep_blend_grid(n);
        k_rep_blend_bwd<<<dim3(nb, R), 256, 0, st>>>(grad_out, out0, out1, beta, al ? n / 4 : 0, n, grad0, grad1,
                                                    (float *)workspace);
    }
    k_rep_blend_reduce<<<R, 256, 0, st>>>((const float *)workspace, nb, grad_beta);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

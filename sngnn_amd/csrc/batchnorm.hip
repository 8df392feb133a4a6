// Training-mode batch norm between two conv layers (models/models.py:204-209, 79-84, 296-301, 368-373): the conv's
// bias add, F.relu(x, inplace=True), BatchNorm1d on the batch's statistics and the dropout behind it,
//   z = x + bias,  r = max(z, 0),  mean_c = sum_i r / N,  var_c = sum_i (r - mean)^2 / N,  invstd = 1 / sqrt(var + eps),
//   xhat = (r - mean) * invstd,  out = (xhat * gamma + beta) * keep * keep_scale,
// which PyTorch runs as about nine passes over [N, C] forward and eleven backward.  Here: three launches each way
// (+ one tiny one for the conv bias' gradient), no hand-off between workgroups inside a launch.
//   1. partials: a workgroup walks row tiles of RB rows; a thread owns a fixed channel group (a float4 of channels
//      where C % 4 == 0 and every base is 16-byte aligned, one channel otherwise) and accumulates over its rows in
//      registers; the threads of one channel group combine through LDS in a fixed tree order: one partial per
//      workgroup and channel in the workspace.
//   2. one small reducer (a workgroup per channel) combines the partials in a fixed order, in double.
//   3. apply: re-reads x and writes the result.
// Nothing of size [N, C] is saved for the backward: it recomputes z, r, xhat and the keep mask from x.
//
// Summation: every accumulation is in double (gfx950 issues a v_add_f64 at the rate of a v_add_f32; the kernels are
// bound by their loads).  The statistics are NOT sum r, sum r^2 (a channel 100 +- 0.01 loses every digit of its
// variance that way): a thread sums d = r - K and d^2 with K the first value it met, turns that into (count, mean,
// M2 = sum (r - mean)^2) once, and from there on partials are combined by Chan's formula - thread to workgroup in
// LDS, workgroup to channel in the reducer.  A bad K (an outlier) costs digits only in that thread's few rows.
// No float atomics: the same inputs give the same bits on every run.  -ffp-contract=off: every product and sum in the
// apply passes is rounded separately, in the order written.
#include "common.h"
#include "device_utils.h"

namespace sngnn {

constexpr int BN_BLOCKS = 512;          // row-tile workgroups of a launch at most: the partials per channel
constexpr int BN_THREADS = 256;
constexpr int BN_NONE = 0, BN_MASK = 1, BN_SEED = 2;          // where keep comes from

// thread layout of a workgroup: GW channel groups of V channels side by side, RB rows of them; slab blockIdx.y
// covers the channel groups [blockIdx.y * GW, ...) of G
struct BnGeom { int G, GW, RB, slabs, nbx; };

static BnGeom bn_geom(int64_t N, int C, int V)
{
    BnGeom q;
    q.G = C / V;
    q.GW = std::min(q.G, BN_THREADS);
    q.RB = BN_THREADS / q.GW;
    q.slabs = (q.G + q.GW - 1) / q.GW;
    q.nbx = (int)std::min<int64_t>(BN_BLOCKS, (N + q.RB - 1) / q.RB);
    return q;
}

template <int V> __device__ __forceinline__ void bn_load(const float *__restrict__ p, int64_t i, float (&v)[V])
{
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[i];
    }
}

template <int V> __device__ __forceinline__ void bn_store(float *__restrict__ p, int64_t i, const float (&v)[V])
{
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    else p[i] = v[0];
}

// per-channel vector (bias, gamma, ...): scalar loads, once per thread; NULL reads as `dflt`
template <int V> __device__ __forceinline__ void bn_chan(const float *__restrict__ p, int c0, float dflt, float (&v)[V])
{
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = p ? p[c0 + j] : dflt;
}

// keep[j] of the V elements at flat index i (= row * C + c0): the caller's mask, or the aggregation epilogue's draw
template <int V, int KEEP>
__device__ __forceinline__ void bn_keep(const unsigned char *__restrict__ keep, unsigned long long seed, float p, int64_t i,
                                        bool (&k)[V])
{
    if constexpr (KEEP == BN_MASK) {
        if constexpr (V == 4) {
            const uchar4 m = *reinterpret_cast<const uchar4 *>(keep + i);
            k[0] = m.x != 0; k[1] = m.y != 0; k[2] = m.z != 0; k[3] = m.w != 0;
        } else {
            k[0] = keep[i] != 0;
        }
    } else if constexpr (KEEP == BN_SEED) {
#pragma unroll
        for (int j = 0; j < V; ++j) k[j] = sn_dropout_keep(seed, (unsigned long long)(i + j), p);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) k[j] = true;
    }
}

// (na, ma, qa) <- the union of two sets given as (count, mean, M2): Chan, Golub & LeVeque's update
__device__ __forceinline__ void bn_chan_merge(double &na, double &ma, double &qa, double nb, double mb, double qb)
{
    if (nb == 0.0) return;
    if (na == 0.0) { na = nb; ma = mb; qa = qb; return; }
    const double n = na + nb, d = mb - ma;
    ma = ma + d * (nb / n);
    qa = qa + qb + d * d * (na * nb / n);
    na = n;
}

struct BnThread { int rr, g, c0; bool active; };

template <int V> __device__ __forceinline__ BnThread bn_thread(int G, int GW, int RB)
{
    BnThread t;
    t.rr = threadIdx.x / GW;
    t.g = blockIdx.y * GW + threadIdx.x % GW;
    t.active = t.rr < RB && t.g < G;
    t.c0 = t.g * V;
    return t;
}

// smallest power of two >= RB (RB <= 256)
__device__ __forceinline__ int bn_pow2(int RB) { int p = 1; while (p < RB) p <<= 1; return p; }

// ---- forward 1: (count, mean, M2) of r per workgroup and channel --------------------------------------------------
// part: double [3][gridDim.x][C]
// RELU: the statistics of r = max(x + bias, 0) (the bias -> relu -> norm order); otherwise of x itself (norm -> relu)
template <int V, bool RELU>
__device__ __forceinline__ void bn_stats_rows(const float *__restrict__ x, const float *__restrict__ bias, int64_t N, int C,
                                              int G, int GW, int RB, double *__restrict__ part)
{
    __shared__ double sn[BN_THREADS], sm[BN_THREADS][V], sq[BN_THREADS][V];
    const BnThread t = bn_thread<V>(G, GW, RB);
    double cnt = 0.0, K[V], s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) K[j] = s1[j] = s2[j] = 0.0;
    if (t.active) {
        float b[V];
        bn_chan<V>(bias, t.c0, 0.f, b);
        const int64_t step = (int64_t)gridDim.x * RB;
#pragma unroll 2
        for (int64_t row = (int64_t)blockIdx.x * RB + t.rr; row < N; row += step) {
            float v[V];
            bn_load<V>(x, row * C + t.c0, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float z = v[j] + b[j];
                const double r = (!RELU || z > 0.f) ? z : 0.f;
                if (cnt == 0.0) K[j] = r;
                const double d = r - K[j];
                s1[j] += d;
                s2[j] += d * d;
            }
            cnt += 1.0;
        }
    }
    sn[threadIdx.x] = cnt;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        double m = 0.0, q = 0.0;
        if (cnt > 0.0) {
            m = K[j] + s1[j] / cnt;
            q = s2[j] - s1[j] * s1[j] / cnt;
            q = q > 0.0 ? q : 0.0;
        }
        sm[threadIdx.x][j] = m;
        sq[threadIdx.x][j] = q;
    }
    __syncthreads();
    for (int m = bn_pow2(RB) >> 1; m >= 1; m >>= 1) {
        if (t.active && t.rr < m && t.rr + m < RB) {
            const int o = threadIdx.x + m * GW;
            const double na = sn[threadIdx.x], nb = sn[o];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                double n = na, a = sm[threadIdx.x][j], q = sq[threadIdx.x][j];
                bn_chan_merge(n, a, q, nb, sm[o][j], sq[o][j]);
                sm[threadIdx.x][j] = a;
                sq[threadIdx.x][j] = q;
            }
            sn[threadIdx.x] = na + nb;
        }
        __syncthreads();
    }
    if (t.active && t.rr == 0) {
        const int64_t plane = (int64_t)gridDim.x * C, at = (int64_t)blockIdx.x * C + t.c0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            part[at + j] = sn[threadIdx.x];
            part[plane + at + j] = sm[threadIdx.x][j];
            part[2 * plane + at + j] = sq[threadIdx.x][j];
        }
    }
}

template <int V>
__global__ __launch_bounds__(BN_THREADS) void k_bn_stats(const float *__restrict__ x, const float *__restrict__ bias,
                                                         int64_t N, int C, int G, int GW, int RB, double *__restrict__ part)
{
    bn_stats_rows<V, true>(x, bias, N, C, G, GW, RB, part);
}

template <int V>
__global__ __launch_bounds__(BN_THREADS) void k_bn_post_stats(const float *__restrict__ x, int64_t N, int C, int G, int GW,
                                                              int RB, double *__restrict__ part)
{
    bn_stats_rows<V, false>(x, nullptr, N, C, G, GW, RB, part);
}

// ---- forward 2: the channel's statistics from its nb partials; a workgroup per channel -----------------------------
__global__ __launch_bounds__(BN_THREADS) void k_bn_reduce_stats(const double *__restrict__ part, int nb, int C, int64_t N,
                                                                double eps, double momentum, float *__restrict__ running_mean,
                                                                float *__restrict__ running_var, float *__restrict__ save_mean,
                                                                float *__restrict__ save_invstd)
{
    __shared__ double sn[BN_THREADS], sm[BN_THREADS], sq[BN_THREADS];
    const int c = blockIdx.x;
    const int64_t plane = (int64_t)nb * C;
    double n = 0.0, a = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < nb; i += BN_THREADS) {
        const int64_t at = (int64_t)i * C + c;
        bn_chan_merge(n, a, q, part[at], part[plane + at], part[2 * plane + at]);
    }
    sn[threadIdx.x] = n; sm[threadIdx.x] = a; sq[threadIdx.x] = q;
    __syncthreads();
    for (int m = BN_THREADS / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) {
            n = sn[threadIdx.x]; a = sm[threadIdx.x]; q = sq[threadIdx.x];
            bn_chan_merge(n, a, q, sn[threadIdx.x + m], sm[threadIdx.x + m], sq[threadIdx.x + m]);
            sn[threadIdx.x] = n; sm[threadIdx.x] = a; sq[threadIdx.x] = q;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mean = sm[0], var = sq[0] / (double)N;
        save_mean[c] = (float)mean;
        save_invstd[c] = (float)(1.0 / sqrt(var + eps));
        if (running_mean) {
            running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
            running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (sq[0] / (double)(N - 1)));
        }
    }
}

// ---- forward 3 -----------------------------------------------------------------------------------------------------
template <int V, int KEEP>
__global__ __launch_bounds__(BN_THREADS) void k_bn_apply(const float *__restrict__ x, const float *__restrict__ bias, int64_t N,
                                                         int C, int G, int GW, int RB, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, const float *__restrict__ mean,
                                                         const float *__restrict__ invstd, const unsigned char *__restrict__ keep,
                                                         const unsigned long long *__restrict__ seedp, float p, float scale,
                                                         float *__restrict__ out)
{
    const BnThread t = bn_thread<V>(G, GW, RB);
    if (!t.active) return;
    float b[V], ga[V], be[V], mu[V], is[V];
    bn_chan<V>(bias, t.c0, 0.f, b);
    bn_chan<V>(gamma, t.c0, 1.f, ga);
    bn_chan<V>(beta, t.c0, 0.f, be);
    bn_chan<V>(mean, t.c0, 0.f, mu);
    bn_chan<V>(invstd, t.c0, 1.f, is);
    unsigned long long seed = 0;
    if constexpr (KEEP == BN_SEED) seed = *seedp;
    const int64_t step = (int64_t)gridDim.x * RB;
#pragma unroll 2
    for (int64_t row = (int64_t)blockIdx.x * RB + t.rr; row < N; row += step) {
        const int64_t i = row * C + t.c0;
        float v[V], o[V];
        bool k[V];
        bn_load<V>(x, i, v);
        bn_keep<V, KEEP>(keep, seed, p, i, k);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float z = v[j] + b[j];
            const float r = z > 0.f ? z : 0.f;
            const float xh = (r - mu[j]) * is[j];
            float y = xh * ga[j] + be[j];
            if constexpr (KEEP != BN_NONE) y = k[j] ? y * scale : 0.f;
            o[j] = y;
        }
        bn_store<V>(out, i, o);
    }
}

// ---- backward 1: sum gz and sum gz * xhat per workgroup and channel; part: double [2][gridDim.x][C] ---------------
template <int V, int KEEP>
__global__ __launch_bounds__(BN_THREADS) void k_bn_bwd_stats(const float *__restrict__ g, const float *__restrict__ x,
                                                             const float *__restrict__ bias, int64_t N, int C, int G, int GW,
                                                             int RB, const float *__restrict__ mean,
                                                             const float *__restrict__ invstd,
                                                             const unsigned char *__restrict__ keep,
                                                             const unsigned long long *__restrict__ seedp, float p, float scale,
                                                             double *__restrict__ part)
{
    __shared__ double s0[BN_THREADS][V], s1[BN_THREADS][V];
    const BnThread t = bn_thread<V>(G, GW, RB);
    double a0[V], a1[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a0[j] = a1[j] = 0.0;
    if (t.active) {
        float b[V], mu[V], is[V];
        bn_chan<V>(bias, t.c0, 0.f, b);
        bn_chan<V>(mean, t.c0, 0.f, mu);
        bn_chan<V>(invstd, t.c0, 1.f, is);
        unsigned long long seed = 0;
        if constexpr (KEEP == BN_SEED) seed = *seedp;
        const int64_t step = (int64_t)gridDim.x * RB;
#pragma unroll 2
        for (int64_t row = (int64_t)blockIdx.x * RB + t.rr; row < N; row += step) {
            const int64_t i = row * C + t.c0;
            float v[V], d[V];
            bool k[V];
            bn_load<V>(x, i, v);
            bn_load<V>(g, i, d);
            bn_keep<V, KEEP>(keep, seed, p, i, k);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float z = v[j] + b[j];
                const float r = z > 0.f ? z : 0.f;
                const float xh = (r - mu[j]) * is[j];
                float gz = d[j];
                if constexpr (KEEP != BN_NONE) gz = k[j] ? gz * scale : 0.f;
                a0[j] += (double)gz;
                a1[j] += (double)gz * (double)xh;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { s0[threadIdx.x][j] = a0[j]; s1[threadIdx.x][j] = a1[j]; }
    __syncthreads();
    for (int m = bn_pow2(RB) >> 1; m >= 1; m >>= 1) {
        if (t.active && t.rr < m && t.rr + m < RB) {
            const int o = threadIdx.x + m * GW;
#pragma unroll
            for (int j = 0; j < V; ++j) { s0[threadIdx.x][j] += s0[o][j]; s1[threadIdx.x][j] += s1[o][j]; }
        }
        __syncthreads();
    }
    if (t.active && t.rr == 0) {
        const int64_t plane = (int64_t)gridDim.x * C, at = (int64_t)blockIdx.x * C + t.c0;
#pragma unroll
        for (int j = 0; j < V; ++j) { part[at + j] = s0[threadIdx.x][j]; part[plane + at + j] = s1[threadIdx.x][j]; }
    }
}

// ---- backward 2 (NS = 2): grad_beta = sum gz, grad_gamma = sum gz xhat, m12 = gamma * (both) / N; and backward 4
// (NS = 1): grad_bias = the column sums of grad_x.  part: double [NS][nb][C]; a workgroup per channel ---------------
template <int NS>
__global__ __launch_bounds__(BN_THREADS) void k_bn_reduce_sums(const double *__restrict__ part, int nb, int C, int64_t N,
                                                               const float *__restrict__ gamma, float *__restrict__ out0,
                                                               float *__restrict__ out1, float *__restrict__ m12)
{
    __shared__ double s[NS][BN_THREADS];
    const int c = blockIdx.x;
    const int64_t plane = (int64_t)nb * C;
    double a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.0;
    for (int i = threadIdx.x; i < nb; i += BN_THREADS)
#pragma unroll
        for (int k = 0; k < NS; ++k) a[k] += part[k * plane + (int64_t)i * C + c];
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int m = BN_THREADS / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m)
#pragma unroll
            for (int k = 0; k < NS; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out0[c] = (float)s[0][0];
        if constexpr (NS == 2) {
            out1[c] = (float)s[1][0];
            const double ga = (double)gamma[c];
            m12[c] = (float)(ga * s[0][0] / (double)N);
            m12[C + c] = (float)(ga * s[1][0] / (double)N);
        }
    }
}

// ---- backward 3: grad_x = invstd * (gamma gz - m1 - xhat m2) [z > 0]; BIAS: its column sums per workgroup ---------
// part: double [gridDim.x][C]
template <int V, int KEEP, bool BIAS>
__global__ __launch_bounds__(BN_THREADS) void k_bn_bwd_apply(const float *__restrict__ g, const float *__restrict__ x,
                                                             const float *__restrict__ bias, int64_t N, int C, int G, int GW,
                                                             int RB, const float *__restrict__ gamma,
                                                             const float *__restrict__ mean, const float *__restrict__ invstd,
                                                             const float *__restrict__ m12,
                                                             const unsigned char *__restrict__ keep,
                                                             const unsigned long long *__restrict__ seedp, float p, float scale,
                                                             float *__restrict__ gx, double *__restrict__ part)
{
    __shared__ double s0[BIAS ? BN_THREADS : 1][V];
    const BnThread t = bn_thread<V>(G, GW, RB);
    double a0[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a0[j] = 0.0;
    if (t.active) {
        float b[V], ga[V], mu[V], is[V], m1[V], m2[V];
        bn_chan<V>(bias, t.c0, 0.f, b);
        bn_chan<V>(gamma, t.c0, 1.f, ga);
        bn_chan<V>(mean, t.c0, 0.f, mu);
        bn_chan<V>(invstd, t.c0, 1.f, is);
        bn_chan<V>(m12, t.c0, 0.f, m1);
        bn_chan<V>(m12 + C, t.c0, 0.f, m2);
        unsigned long long seed = 0;
        if constexpr (KEEP == BN_SEED) seed = *seedp;
        const int64_t step = (int64_t)gridDim.x * RB;
#pragma unroll 2
        for (int64_t row = (int64_t)blockIdx.x * RB + t.rr; row < N; row += step) {
            const int64_t i = row * C + t.c0;
            float v[V], d[V], o[V];
            bool k[V];
            bn_load<V>(x, i, v);
            bn_load<V>(g, i, d);
            bn_keep<V, KEEP>(keep, seed, p, i, k);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float z = v[j] + b[j];
                const float r = z > 0.f ? z : 0.f;
                const float xh = (r - mu[j]) * is[j];
                float gz = d[j];
                if constexpr (KEEP != BN_NONE) gz = k[j] ? gz * scale : 0.f;
                float u = ga[j] * gz;
                u = u - m1[j];
                u = u - xh * m2[j];
                o[j] = z > 0.f ? is[j] * u : 0.f;
                if constexpr (BIAS) a0[j] += (double)o[j];
            }
            bn_store<V>(gx, i, o);
        }
    }
    if constexpr (BIAS) {
#pragma unroll
        for (int j = 0; j < V; ++j) s0[threadIdx.x][j] = a0[j];
        __syncthreads();
        for (int m = bn_pow2(RB) >> 1; m >= 1; m >>= 1) {
            if (t.active && t.rr < m && t.rr + m < RB) {
                const int o = threadIdx.x + m * GW;
#pragma unroll
                for (int j = 0; j < V; ++j) s0[threadIdx.x][j] += s0[o][j];
            }
            __syncthreads();
        }
        if (t.active && t.rr == 0) {
            const int64_t at = (int64_t)blockIdx.x * C + t.c0;
#pragma unroll
            for (int j = 0; j < V; ++j) part[at + j] = s0[threadIdx.x][j];
        }
    }
}

// ---- the other order: norm -> relu -> dropout (GCNII, models.py:1295-1298).  The statistics are those of x itself
// (k_bn_post_stats + k_bn_reduce_stats); y = xhat gamma + beta, out = max(y, 0) keep scale; the backward recomputes
// xhat, the relu mask [y > 0] and keep from x: gy = g keep scale [y > 0], then the sums and grad_x of the first order
// without its [z > 0] factor (k_bn_reduce_sums<2> between the two launches) ----------------------------------------
template <int V, int KEEP>
__global__ __launch_bounds__(BN_THREADS) void k_bn_post_apply(const float *__restrict__ x, int64_t N, int C, int G, int GW,
                                                              int RB, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, const float *__restrict__ mean,
                                                              const float *__restrict__ invstd,
                                                              const unsigned char *__restrict__ keep,
                                                              const unsigned long long *__restrict__ seedp, float p, float scale,
                                                              float *__restrict__ out)
{
    const BnThread t = bn_thread<V>(G, GW, RB);
    if (!t.active) return;
    float ga[V], be[V], mu[V], is[V];
    bn_chan<V>(gamma, t.c0, 1.f, ga);
    bn_chan<V>(beta, t.c0, 0.f, be);
    bn_chan<V>(mean, t.c0, 0.f, mu);
    bn_chan<V>(invstd, t.c0, 1.f, is);
    unsigned long long seed = 0;
    if constexpr (KEEP == BN_SEED) seed = *seedp;
    const int64_t step = (int64_t)gridDim.x * RB;
#pragma unroll 2
    for (int64_t row = (int64_t)blockIdx.x * RB + t.rr; row < N; row += step) {
        const int64_t i = row * C + t.c0;
        float v[V], o[V];
        bool k[V];
        bn_load<V>(x, i, v);
        bn_keep<V, KEEP>(keep, seed, p, i, k);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float xh = (v[j] - mu[j]) * is[j];
            float y = xh * ga[j] + be[j];
            y = y > 0.f ? y : 0.f;
            if constexpr (KEEP != BN_NONE) y = k[j] ? y * scale : 0.f;
            o[j] = y;
        }
        bn_store<V>(out, i, o);
    }
}

// FINAL = false: sum gy and sum gy * xhat per workgroup and channel, part: double [2][gridDim.x][C];
// FINAL = true: grad_x = invstd * (gamma gy - m1 - xhat m2)
template <int V, int KEEP, bool FINAL>
__global__ __launch_bounds__(BN_THREADS) void k_bn_post_bwd(const float *__restrict__ g, const float *__restrict__ x, int64_t N,
                                                            int C, int G, int GW, int RB, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const float *__restrict__ mean,
                                                            const float *__restrict__ invstd, const float *__restrict__ m12,
                                                            const unsigned char *__restrict__ keep,
                                                            const unsigned long long *__restrict__ seedp, float p, float scale,
                                                            float *__restrict__ gx, double *__restrict__ part)
{
    __shared__ double s0[FINAL ? 1 : BN_THREADS][V], s1[FINAL ? 1 : BN_THREADS][V];
    const BnThread t = bn_thread<V>(G, GW, RB);
    double a0[V], a1[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a0[j] = a1[j] = 0.0;
    if (t.active) {
        float ga[V], be[V], mu[V], is[V], m1[V], m2[V];
        bn_chan<V>(gamma, t.c0, 1.f, ga);
        bn_chan<V>(beta, t.c0, 0.f, be);
        bn_chan<V>(mean, t.c0, 0.f, mu);
        bn_chan<V>(invstd, t.c0, 1.f, is);
        bn_chan<V>(FINAL ? m12 : nullptr, t.c0, 0.f, m1);
        bn_chan<V>(FINAL ? m12 + C : nullptr, t.c0, 0.f, m2);
        unsigned long long seed = 0;
        if constexpr (KEEP == BN_SEED) seed = *seedp;
        const int64_t step = (int64_t)gridDim.x * RB;
#pragma unroll 2
        for (int64_t row = (int64_t)blockIdx.x * RB + t.rr; row < N; row += step) {
            const int64_t i = row * C + t.c0;
            float v[V], d[V], o[V];
            bool k[V];
            bn_load<V>(x, i, v);
            bn_load<V>(g, i, d);
            bn_keep<V, KEEP>(keep, seed, p, i, k);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float xh = (v[j] - mu[j]) * is[j];
                const float y = xh * ga[j] + be[j];
                float gy = d[j];
                if constexpr (KEEP != BN_NONE) gy = k[j] ? gy * scale : 0.f;
                gy = y > 0.f ? gy : 0.f;
                if constexpr (FINAL) {
                    float u = ga[j] * gy;
                    u = u - m1[j];
                    u = u - xh * m2[j];
                    o[j] = is[j] * u;
                } else {
                    a0[j] += (double)gy;
                    a1[j] += (double)gy * (double)xh;
                }
            }
            if constexpr (FINAL) bn_store<V>(gx, i, o);
        }
    }
    if constexpr (!FINAL) {
#pragma unroll
        for (int j = 0; j < V; ++j) { s0[threadIdx.x][j] = a0[j]; s1[threadIdx.x][j] = a1[j]; }
        __syncthreads();
        for (int m = bn_pow2(RB) >> 1; m >= 1; m >>= 1) {
            if (t.active && t.rr < m && t.rr + m < RB) {
                const int o = threadIdx.x + m * GW;
#pragma unroll
                for (int j = 0; j < V; ++j) { s0[threadIdx.x][j] += s0[o][j]; s1[threadIdx.x][j] += s1[o][j]; }
            }
            __syncthreads();
        }
        if (t.active && t.rr == 0) {
            const int64_t plane = (int64_t)gridDim.x * C, at = (int64_t)blockIdx.x * C + t.c0;
#pragma unroll
            for (int j = 0; j < V; ++j) { part[at + j] = s0[threadIdx.x][j]; part[plane + at + j] = s1[threadIdx.x][j]; }
        }
    }
}

// float4 / uchar4 accesses: C % 4 == 0 and every [N, C] base on a 16-byte boundary (a u8 mask then sits on 4 at least)
static int bn_vec(int C, std::initializer_list<const void *> ps)
{
    uintptr_t a = 0;
    for (const void *p : ps) a |= (uintptr_t)p;          // (NULL contributes nothing)
    return (C % 4 == 0 && a % 16 == 0) ? 4 : 1;
}

static int64_t bn_partial_doubles(int C) { return (int64_t)3 * BN_BLOCKS * C; }

#define BN_DISPATCH(V, mode, KERNEL, ...)                                                                  \
    do {                                                                                                   \
        if ((V) == 4) {                                                                                    \
            if ((mode) == BN_MASK) KERNEL(4, BN_MASK) __VA_ARGS__;                                         \
            else if ((mode) == BN_SEED) KERNEL(4, BN_SEED) __VA_ARGS__;                                    \
            else KERNEL(4, BN_NONE) __VA_ARGS__;                                                           \
        } else {                                                                                           \
            if ((mode) == BN_MASK) KERNEL(1, BN_MASK) __VA_ARGS__;                                         \
            else if ((mode) == BN_SEED) KERNEL(1, BN_SEED) __VA_ARGS__;                                    \
            else KERNEL(1, BN_NONE) __VA_ARGS__;                                                           \
        }                                                                                                  \
    } while (0)

}  // namespace sngnn

using namespace sngnn;

extern "C" int64_t sngnn_bn_train_workspace_bytes(int C)
{
    if (C < 1 || C > SNGNN_MAX_CHANNELS) return 0;
    return (bn_partial_doubles(C) * 8 + (int64_t)2 * C * 4 + 255) / 256 * 256;          // partials, then (m1, m2)
}

static int bn_check_common(const void *x, int64_t N, int C, float p, const void *keep, const void *seed)
{
    SN_REQUIRE(x != nullptr, SNGNN_EINVAL, "NULL argument (x)");
    SN_REQUIRE(N >= 2, SNGNN_EINVAL, "training-mode batch norm needs at least 2 rows (one value per channel has no variance)");
    SN_REQUIRE(C >= 1 && C <= SNGNN_MAX_CHANNELS, SNGNN_EINVAL, "C out of range");
    SN_REQUIRE(p >= 0.f && p < 1.f, SNGNN_EINVAL, "p must be in [0, 1)");
    SN_REQUIRE(!(keep && seed), SNGNN_EINVAL, "keep and seed exclude each other");
    return SNGNN_OK;
}

static int bn_keep_mode(const void *keep, const void *seed, float p) { return keep ? BN_MASK : (seed && p > 0.f) ? BN_SEED : BN_NONE; }

extern "C" int sngnn_bn_train_forward(const float *x, const float *bias, int64_t N, int C, const float *gamma, const float *beta,
                                      double eps, double momentum, float *running_mean, float *running_var,
                                      const unsigned char *keep, float keep_scale, const void *seed, float p, float *out,
                                      float *save_mean, float *save_invstd, void *workspace, void *stream)
{
    if (int rc = bn_check_common(x, N, C, p, keep, seed)) return rc;
    SN_REQUIRE(gamma && beta && out && save_mean && save_invstd && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), SNGNN_EINVAL,
               "running_mean and running_var go together (both NULL: no running statistics)");
    SN_REQUIRE(eps >= 0.0, SNGNN_EINVAL, "negative eps");
    hipStream_t st = (hipStream_t)stream;
    const int mode = bn_keep_mode(keep, seed, p);
    if (mode == BN_NONE) keep_scale = 1.f;
    const int V = bn_vec(C, {x, out, keep});
    const BnGeom q = bn_geom(N, C, V);
    const dim3 grid(q.nbx, q.slabs);
    double *part = (double *)workspace;
    if (V == 4) k_bn_stats<4><<<grid, BN_THREADS, 0, st>>>(x, bias, N, C, q.G, q.GW, q.RB, part);
    else k_bn_stats<1><<<grid, BN_THREADS, 0, st>>>(x, bias, N, C, q.G, q.GW, q.RB, part);
    k_bn_reduce_stats<<<C, BN_THREADS, 0, st>>>(part, q.nbx, C, N, eps, momentum, running_mean, running_var, save_mean,
                                                save_invstd);
#define BN_K(V_, M_) k_bn_apply<V_, M_>
    BN_DISPATCH(V, mode, BN_K, <<<grid, BN_THREADS, 0, st>>>(x, bias, N, C, q.G, q.GW, q.RB, gamma, beta, save_mean, save_invstd,
                                                            keep, (const unsigned long long *)seed, p, keep_scale, out));
#undef BN_K
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_bn_train_backward(const float *grad_out, const float *x, const float *bias, int64_t N, int C,
                                       const float *gamma, const float *save_mean, const float *save_invstd,
                                       const unsigned char *keep, float keep_scale, const void *seed, float p, float *grad_x,
                                       float *grad_gamma, float *grad_beta, float *grad_bias, void *workspace, void *stream)
{
    if (int rc = bn_check_common(x, N, C, p, keep, seed)) return rc;
    SN_REQUIRE(grad_out && gamma && save_mean && save_invstd && grad_x && grad_gamma && grad_beta && workspace, SNGNN_EINVAL,
               "NULL argument");
    SN_REQUIRE(!grad_bias || bias, SNGNN_EINVAL, "grad_bias without bias");
    hipStream_t st = (hipStream_t)stream;
    const int mode = bn_keep_mode(keep, seed, p);
    if (mode == BN_NONE) keep_scale = 1.f;
    const int V = bn_vec(C, {grad_out, x, grad_x, keep});
    const BnGeom q = bn_geom(N, C, V);
    const dim3 grid(q.nbx, q.slabs);
    double *part = (double *)workspace;
    float *m12 = (float *)(part + bn_partial_doubles(C));
    double *part_b = part + (int64_t)2 * BN_BLOCKS * C;          // (behind the two planes of the first launch)
    const unsigned long long *sd = (const unsigned long long *)seed;
#define BN_K(V_, M_) k_bn_bwd_stats<V_, M_>
    BN_DISPATCH(V, mode, BN_K, <<<grid, BN_THREADS, 0, st>>>(grad_out, x, bias, N, C, q.G, q.GW, q.RB, save_mean, save_invstd, keep,
                                                            sd, p, keep_scale, part));
#undef BN_K
    k_bn_reduce_sums<2><<<C, BN_THREADS, 0, st>>>(part, q.nbx, C, N, gamma, grad_beta, grad_gamma, m12);
    if (grad_bias) {
#define BN_K(V_, M_) k_bn_bwd_apply<V_, M_, true>
        BN_DISPATCH(V, mode, BN_K, <<<grid, BN_THREADS, 0, st>>>(grad_out, x, bias, N, C, q.G, q.GW, q.RB, gamma, save_mean,
                                                                save_invstd, m12, keep, sd, p, keep_scale, grad_x, part_b));
#undef BN_K
        k_bn_reduce_sums<1><<<C, BN_THREADS, 0, st>>>(part_b, q.nbx, C, N, nullptr, grad_bias, nullptr, nullptr);
    } else {
#define BN_K(V_, M_) k_bn_bwd_apply<V_, M_, false>
        BN_DISPATCH(V, mode, BN_K, <<<grid, BN_THREADS, 0, st>>>(grad_out, x, bias, N, C, q.G, q.GW, q.RB, gamma, save_mean,
                                                                save_invstd, m12, keep, sd, p, keep_scale, grad_x, nullptr));
#undef BN_K
    }
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_bn_post_forward(const float *x, int64_t N, int C, const float *gamma, const float *beta, double eps,
                                     double momentum, float *running_mean, float *running_var, const unsigned char *keep,
                                     float keep_scale, const void *seed, float p, float *out, float *save_mean,
                                     float *save_invstd, void *workspace, void *stream)
{
    if (int rc = bn_check_common(x, N, C, p, keep, seed)) return rc;
    SN_REQUIRE(gamma && beta && out && save_mean && save_invstd && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), SNGNN_EINVAL,
               "running_mean and running_var go together (both NULL: no running statistics)");
    SN_REQUIRE(eps >= 0.0, SNGNN_EINVAL, "negative eps");
    hipStream_t st = (hipStream_t)stream;
    const int mode = bn_keep_mode(keep, seed, p);
    if (mode == BN_NONE) keep_scale = 1.f;
    const int V = bn_vec(C, {x, out, keep});
    const BnGeom q = bn_geom(N, C, V);
    const dim3 grid(q.nbx, q.slabs);
    double *part = (double *)workspace;
    if (V == 4) k_bn_post_stats<4><<<grid, BN_THREADS, 0, st>>>(x, N, C, q.G, q.GW, q.RB, part);
    else k_bn_post_stats<1><<<grid, BN_THREADS, 0, st>>>(x, N, C, q.G, q.GW, q.RB, part);
    k_bn_reduce_stats<<<C, BN_THREADS, 0, st>>>(part, q.nbx, C, N, eps, momentum, running_mean, running_var, save_mean,
                                                save_invstd);
#define BN_K(V_, M_) k_bn_post_apply<V_, M_>
    BN_DISPATCH(V, mode, BN_K, <<<grid, BN_THREADS, 0, st>>>(x, N, C, q.G, q.GW, q.RB, gamma, beta, save_mean, save_invstd, keep,
                                                            (const unsigned long long *)seed, p, keep_scale, out));
#undef BN_K
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_bn_post_backward(const float *grad_out, const float *x, int64_t N, int C, const float *gamma,
                                      const float *beta, const float *save_mean, const float *save_invstd,
                                      const unsigned char *keep, float keep_scale, const void *seed, float p, float *grad_x,
                                      float *grad_gamma, float *grad_beta, void *workspace, void *stream)
{
    if (int rc = bn_check_common(x, N, C, p, keep, seed)) return rc;
    SN_REQUIRE(grad_out && gamma && beta && save_mean && save_invstd && grad_x && grad_gamma && grad_beta && workspace,
               SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int mode = bn_keep_mode(keep, seed, p);
    if (mode == BN_NONE) keep_scale = 1.f;
    const int V = bn_vec(C, {grad_out, x, grad_x, keep});
    const BnGeom q = bn_geom(N, C, V);
    const dim3 grid(q.nbx, q.slabs);
    double *part = (double *)workspace;
    float *m12 = (float *)(part + bn_partial_doubles(C));
    const unsigned long long *sd = (const unsigned long long *)seed;
#define BN_K(V_, M_) k_bn_post_bwd<V_, M_, false>
    BN_DISPATCH(V, mode, BN_K, <<<grid, BN_THREADS, 0, st>>>(grad_out, x, N, C, q.G, q.GW, q.RB, gamma, beta, save_mean, save_invstd,
                                                            nullptr, keep, sd, p, keep_scale, nullptr, part));
#undef BN_K
    k_bn_reduce_sums<2><<<C, BN_THREADS, 0, st>>>(part, q.nbx, C, N, gamma, grad_beta, grad_gamma, m12);
#define BN_K(V_, M_) k_bn_post_bwd<V_, M_, true>
    BN_DISPATCH(V, mode, BN_K, <<<grid, BN_THREADS, 0, st>>>(grad_out, x, N, C, q.G, q.GW, q.RB, gamma, beta, save_mean, save_invstd,
                                                            m12, keep, sd, p, keep_scale, grad_x, nullptr));
#undef BN_K
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

// LINKX's join (models/models.py:1135-1143), gfx950, fp32, row-local (no graph):
//     a = log_softmax(zA), x = log_softmax(zX)      (lsm = 0: a = zA, x = zX)
//     y = relu(a Wa^T + x Wx^T + b + a + x),        W = [Wa | Wx] row-major [H, 2H] (the reference's W.weight)
// for the last linears' outputs zA, zX [N, H] of mlpA and mlpX.  The reference runs two log_softmax, a cat, a Linear,
// two adds and a relu; here the rows are streamed once in 32- or 64-row tiles through LDS with the weight resident in LDS
// for the workgroup's lifetime (the layout of k_gcn2_map, gcn2.hip): the row's maximum and sum are taken in the tile before
// the product, [a | x] goes out as the ONE tensor the backward saves (it feeds the weight gradient as a single
// sngnn_linear_wgrad call with F = 2H), a thread owns 4 rows x CT columns and each dot product is four interleaved fma
// chains (k mod 4) added pairwise.  Per element, in this order: t = dotA + a, t = t + dotX, t = t + b, t = t + x,
// y = max(t, 0); every product and sum is rounded separately (-ffp-contract=off), fixed order, no atomics.
// H <= 96: both H x H halves of W are resident and a launch does everything (MODE 0).  97 <= H <= 128: both halves do
// not fit 160 KiB next to the tile, so they are resident one after the other, as two launches of the same kernel -
// MODE 1 leaves t = dotA + a in y, MODE 2 finishes it - with bit-identical arithmetic.
// The backward is the same tiling on g = grad_y [y > 0] (stored: the weight and bias gradients read it):
//     tA = g + g Wa,  grad_zA = tA - exp(a) sum_j tA_j      (lsm = 0: grad_zA = tA), and the same for X.
#include <algorithm>

#include "common.h"

namespace sngnn {

// NT threads a workgroup take NT / 8 rows a tile: NT / 32 row groups of 4 rows x 32 column lanes.  256 threads (32 rows)
// where several workgroups fit a CU's LDS side by side (H <= 64); 512 (64 rows) above, where W leaves room for one
// workgroup only and a second wave per SIMD hides the LDS latency of the product (measured at H = 128, 169 343 rows:
// forward 0.71 -> 0.46 ms, forward + backward 2.30 -> 1.68 ms; profiles/linkx.txt holds the latter)
constexpr int join_threads(int CT) { return CT <= 2 ? 256 : 512; }

// one H x H half of W into LDS as [contraction][output], CP x CP with zero padding.  Forward (by_out): the contraction
// runs over W's columns, sw[k][j] = W[j, half H + k]; backward: over its rows, sw[j][k] = W[j, half H + k].
template <int CT, int NT>
__device__ __forceinline__ void join_load_w(float *sw, const float *__restrict__ w, int H, int half, bool by_out, int tid)
{
    constexpr int CP = 32 * CT;
    for (int e = tid; e < CP * CP; e += NT) {
        const int c = e / CP, o = e % CP;
        float v = 0.f;
        if (c < H && o < H) v = by_out ? w[(size_t)o * (2 * H) + half * H + c] : w[(size_t)c * (2 * H) + half * H + o];
        sw[e] = v;
    }
}

// dot[i][q] = sum_k ss[rg 4 + i][k] sw[k][cl + 32 q]: four fma chains (k mod 4), added pairwise
template <int CT>
__device__ __forceinline__ void join_dot(const float *ss, const float *sw, int kend, int rg, int cl, float (&dot)[4][CT])
{
    constexpr int CP = 32 * CT, LD = CP + 4;
    float acc[4][CT][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < CT; ++q)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc[i][q][kk] = 0.f;
    for (int k0 = 0; k0 < kend; k0 += 4) {
        float4 sv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) sv[i] = *reinterpret_cast<const float4 *>(ss + (rg * 4 + i) * LD + k0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int q = 0; q < CT; ++q) {
                const float wv = sw[(k0 + kk) * CP + cl + 32 * q];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float xv = kk == 0 ? sv[i].x : kk == 1 ? sv[i].y : kk == 2 ? sv[i].z : sv[i].w;
                    acc[i][q][kk] = fmaf(xv, wv, acc[i][q][kk]);
                }
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < CT; ++q) dot[i][q] = (acc[i][q][0] + acc[i][q][1]) + (acc[i][q][2] + acc[i][q][3]);
}

// the sum of the 8 lanes of a row (lanes tid & 7 of one wave): a butterfly, the same bits in every lane
__device__ __forceinline__ float join_sum8(float v)
{
    v = v + __shfl_xor(v, 4);
    v = v + __shfl_xor(v, 2);
    return v + __shfl_xor(v, 1);
}

// One tile of z into ss (columns k >= H stay zero), log_softmax of its rows in place with lsm - 8 lanes a row, each
// over the columns k = lane (mod 8) in ascending order: max, sum of exp(z - max) in double, (z - max) - log(sum) - and
// the tile out to dst (rows ld floats apart).  Ends on a barrier: ss is ready to be read.
template <int CT, int NT>
__device__ __forceinline__ void join_stage(float *ss, const float *__restrict__ src, int nrows, int H, int lsm,
                                           float *__restrict__ dst, int ld, int tid)
{
    constexpr int LD = 32 * CT + 4;
    __syncthreads();                                   // the previous tile's reads are done
    for (int e = tid; e < nrows * H; e += NT) ss[(e / H) * LD + e % H] = src[e];
    __syncthreads();
    if (lsm) {
        const int r = tid >> 3, l = tid & 7;
        float *row = ss + r * LD;
        const bool live = r < nrows;
        float mx = -INFINITY;
        if (live)
            for (int k = l; k < H; k += 8) mx = fmaxf(mx, row[k]);
        mx = fmaxf(mx, __shfl_xor(mx, 4));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        // the sum and its logarithm in double: on rows that are log-probabilities already the sum is 1 + a little, and
        // an fp32 sum would round the little - all of a's largest element - away
        double sum = 0.0;
        if (live)
            for (int k = l; k < H; k += 8) sum = sum + (double)expf(row[k] - mx);
        sum = sum + __shfl_xor(sum, 4);
        sum = sum + __shfl_xor(sum, 2);
        sum = sum + __shfl_xor(sum, 1);
        const float ls = (float)log(sum);
        if (live)
            for (int k = l; k < H; k += 8) row[k] = (row[k] - mx) - ls;
        __syncthreads();
    }
    for (int e = tid; e < nrows * H; e += NT) dst[(size_t)(e / H) * ld + e % H] = ss[(e / H) * LD + e % H];
}

// MODE 0: both halves of W resident, everything.  MODE 1: the A half - writes ax[:, :H] and t = dotA + a into y.
// MODE 2: the X half - writes ax[:, H:] and finishes y from the t MODE 1 left there.
template <int CT, int MODE, int NT>
__global__ __launch_bounds__(NT) void k_linkx_join_fwd(const float *__restrict__ zA, const float *__restrict__ zX,
                                                        const float *__restrict__ w, const float *__restrict__ b,
                                                        int64_t N, int H, int lsm, float *__restrict__ ax,
                                                        float *y, int64_t ntiles)
{
    constexpr int CP = 32 * CT, LD = CP + 4, NW = MODE == 0 ? 2 : 1, JOIN_ROWS = NT / 8;
    __shared__ __align__(16) float sw[NW * CP * CP];
    __shared__ __align__(16) float ss[JOIN_ROWS * LD];
    const int tid = threadIdx.x, cl = tid & 31, rg = tid >> 5;
    if (MODE != 2) join_load_w<CT, NT>(sw, w, H, 0, true, tid);
    if (MODE != 1) join_load_w<CT, NT>(sw + (NW - 1) * CP * CP, w, H, 1, true, tid);
    for (int e = tid; e < JOIN_ROWS * LD; e += NT) ss[e] = 0.f;
    float bias[CT];
#pragma unroll
    for (int q = 0; q < CT; ++q) bias[q] = b[min(cl + 32 * q, H - 1)];
    const int kend = (H + 3) & ~3;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * JOIN_ROWS;
        const int nrows = N - row0 < JOIN_ROWS ? (int)(N - row0) : JOIN_ROWS;
        float t[4][CT], dot[4][CT];
        if (MODE != 2) {
            join_stage<CT, NT>(ss, zA + row0 * H, nrows, H, lsm, ax + row0 * (2 * H), 2 * H, tid);
            join_dot<CT>(ss, sw, kend, rg, cl, dot);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < CT; ++q) t[i][q] = dot[i][q] + ss[(rg * 4 + i) * LD + cl + 32 * q];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < CT; ++q) {
                    const int r = rg * 4 + i, j = cl + 32 * q;
                    t[i][q] = (r < nrows && j < H) ? y[(row0 + r) * H + j] : 0.f;
                }
        }
        if (MODE != 1) {
            join_stage<CT, NT>(ss, zX + row0 * H, nrows, H, lsm, ax + row0 * (2 * H) + H, 2 * H, tid);
            join_dot<CT>(ss, sw + (NW - 1) * CP * CP, kend, rg, cl, dot);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rg * 4 + i;
#pragma unroll
            for (int q = 0; q < CT; ++q) {
                const int j = cl + 32 * q;
                if (r < nrows && j < H) {
                    float v = t[i][q];
                    if (MODE != 1) {
                        v = ((v + dot[i][q]) + bias[q]) + ss[r * LD + j];
                        v = v > 0.f ? v : 0.f;
                    }
                    y[(row0 + r) * H + j] = v;
                }
            }
        }
    }
}

// MODE as above: 0 both halves, 1 the A half (stores g and grad_zA), 2 the X half (grad_zX; g is formed again, not stored)
template <int CT, int MODE, int NT>
__global__ __launch_bounds__(NT) void k_linkx_join_bwd(const float *__restrict__ gy, const float *__restrict__ y,
                                                        const float *__restrict__ ax, const float *__restrict__ w,
                                                        int64_t N, int H, int lsm, float *__restrict__ g,
                                                        float *__restrict__ gzA, float *__restrict__ gzX, int64_t ntiles)
{
    constexpr int CP = 32 * CT, LD = CP + 4, NW = MODE == 0 ? 2 : 1, JOIN_ROWS = NT / 8;
    __shared__ __align__(16) float sw[NW * CP * CP];
    __shared__ __align__(16) float ss[JOIN_ROWS * LD];          // the tile of g
    __shared__ __align__(16) float st[JOIN_ROWS * LD];          // the tile of tA / tX
    __shared__ float srow[JOIN_ROWS];                           // its row sums
    const int tid = threadIdx.x, cl = tid & 31, rg = tid >> 5;
    if (MODE != 2) join_load_w<CT, NT>(sw, w, H, 0, false, tid);
    if (MODE != 1) join_load_w<CT, NT>(sw + (NW - 1) * CP * CP, w, H, 1, false, tid);
    for (int e = tid; e < JOIN_ROWS * LD; e += NT) ss[e] = 0.f;
    const int kend = (H + 3) & ~3;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * JOIN_ROWS;
        const int nrows = N - row0 < JOIN_ROWS ? (int)(N - row0) : JOIN_ROWS;
        __syncthreads();                               // the previous tile's reads (and the fills above) are done
        for (int e = tid; e < nrows * H; e += NT) {
            const int64_t at = row0 * H + e;
            const float v = y[at] > 0.f ? gy[at] : 0.f;
            ss[(e / H) * LD + e % H] = v;
            if (MODE != 2) g[at] = v;
        }
        __syncthreads();
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if ((MODE == 1 && half == 1) || (MODE == 2 && half == 0)) continue;
            float *__restrict__ gz = half == 0 ? gzA : gzX;
            float dot[4][CT];
            join_dot<CT>(ss, sw + (MODE == 0 ? half : 0) * CP * CP, kend, rg, cl, dot);
            if (!lsm) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < CT; ++q) {
                        const int r = rg * 4 + i, j = cl + 32 * q;
                        if (r < nrows && j < H) gz[(row0 + r) * H + j] = ss[r * LD + j] + dot[i][q];
                    }
                continue;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < CT; ++q) {
                    const int r = rg * 4 + i, j = cl + 32 * q;
                    st[r * LD + j] = ss[r * LD + j] + dot[i][q];          // (columns j >= H: 0 + 0)
                }
            __syncthreads();
            {   // 8 lanes a row, each over the columns k = lane (mod 8) in ascending order
                const int r = tid >> 3, l = tid & 7;
                float sum = 0.f;
                if (r < nrows)
                    for (int k = l; k < H; k += 8) sum = sum + st[r * LD + k];
                sum = join_sum8(sum);
                if (l == 0) srow[r] = sum;
            }
            __syncthreads();
            for (int e = tid; e < nrows * H; e += NT) {
                const int r = e / H, k = e % H;
                const float p = expf(ax[(row0 + r) * (2 * H) + half * H + k]);
                gz[row0 * H + e] = st[r * LD + k] - p * srow[r];
            }
            __syncthreads();                           // st and srow are free again
        }
    }
}

// workgroups that fit a CU's 160 KiB of LDS side by side (8 at most), on 256 CUs
static int join_grid(int64_t ntiles, int64_t lds)
{
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / lds));
    return (int)std::min<int64_t>(ntiles, 256 * per_cu);
}

template <int CT>
static int launch_join_fwd(const float *zA, const float *zX, const float *w, const float *b, int64_t N, int H, int lsm,
                           float *ax, float *y, hipStream_t st)
{
    constexpr int CP = 32 * CT, NT = join_threads(CT), JOIN_ROWS = NT / 8, TILE = JOIN_ROWS * (CP + 4);
    const int64_t ntiles = (N + JOIN_ROWS - 1) / JOIN_ROWS;
    if constexpr (CT <= 3) {
        const int grid = join_grid(ntiles, (int64_t)(2 * CP * CP + TILE) * 4);
        k_linkx_join_fwd<CT, 0, NT><<<grid, NT, 0, st>>>(zA, zX, w, b, N, H, lsm, ax, y, ntiles);
    } else {
        const int grid = join_grid(ntiles, (int64_t)(CP * CP + TILE) * 4);
        k_linkx_join_fwd<CT, 1, NT><<<grid, NT, 0, st>>>(zA, zX, w, b, N, H, lsm, ax, y, ntiles);
        k_linkx_join_fwd<CT, 2, NT><<<grid, NT, 0, st>>>(zA, zX, w, b, N, H, lsm, ax, y, ntiles);
    }
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <int CT>
static int launch_join_bwd(const float *gy, const float *y, const float *ax, const float *w, int64_t N, int H, int lsm,
                           float *g, float *gzA, float *gzX, hipStream_t st)
{
    constexpr int CP = 32 * CT, NT = join_threads(CT), JOIN_ROWS = NT / 8, TILE = JOIN_ROWS * (CP + 4);
    const int64_t ntiles = (N + JOIN_ROWS - 1) / JOIN_ROWS;
    if constexpr (CT <= 3) {
        const int grid = join_grid(ntiles, (int64_t)(2 * CP * CP + 2 * TILE + JOIN_ROWS) * 4);
        k_linkx_join_bwd<CT, 0, NT><<<grid, NT, 0, st>>>(gy, y, ax, w, N, H, lsm, g, gzA, gzX, ntiles);
    } else {
        const int grid = join_grid(ntiles, (int64_t)(CP * CP + 2 * TILE + JOIN_ROWS) * 4);
        k_linkx_join_bwd<CT, 1, NT><<<grid, NT, 0, st>>>(gy, y, ax, w, N, H, lsm, g, gzA, gzX, ntiles);
        k_linkx_join_bwd<CT, 2, NT><<<grid, NT, 0, st>>>(gy, y, ax, w, N, H, lsm, g, gzA, gzX, ntiles);
    }
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

static bool join_shape_ok(int64_t N, int H, int &rc)
{
    rc = SNGNN_OK;
    if (N < 0) { set_error("bad shape"); rc = SNGNN_EINVAL; return false; }
    if (H < 1 || H > SNGNN_LINKX_MAX_H) {
        set_error("H must be in [1, " + std::to_string(SNGNN_LINKX_MAX_H) + "] (a wider join runs the plain op sequence)");
        rc = SNGNN_ERANGE;
        return false;
    }
    return true;
}

}  // namespace sngnn

using namespace sngnn;

extern "C" int sngnn_linkx_join_supported(int H) { return H >= 1 && H <= SNGNN_LINKX_MAX_H; }

extern "C" int sngnn_linkx_join_forward(const float *zA, const float *zX, const float *W, const float *b, int64_t N,
                                        int H, int lsm, float *ax, float *y, void *stream)
{
    int rc;
    if (!join_shape_ok(N, H, rc)) return rc;
    if (N == 0) return SNGNN_OK;
    SN_REQUIRE(zA && zX && W && b && ax && y, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(y != zA && y != zX && ax != zA && ax != zX && ax != y, SNGNN_EINVAL, "ax and y must not alias the inputs");
    hipStream_t st = (hipStream_t)stream;
    switch ((H + 31) / 32) {
    case 1: return launch_join_fwd<1>(zA, zX, W, b, N, H, lsm != 0, ax, y, st);
    case 2: return launch_join_fwd<2>(zA, zX, W, b, N, H, lsm != 0, ax, y, st);
    case 3: return launch_join_fwd<3>(zA, zX, W, b, N, H, lsm != 0, ax, y, st);
    default: return launch_join_fwd<4>(zA, zX, W, b, N, H, lsm != 0, ax, y, st);
    }
}

extern "C" int sngnn_linkx_join_backward(const float *grad_y, const float *y, const float *ax, const float *W, int64_t N,
                                         int H, int lsm, float *g, float *grad_zA, float *grad_zX, void *stream)
{
    int rc;
    if (!join_shape_ok(N, H, rc)) return rc;
    if (N == 0) return SNGNN_OK;
    SN_REQUIRE(grad_y && y && ax && W && g && grad_zA && grad_zX, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(g != grad_y && g != y && grad_zA != grad_y && grad_zA != y && grad_zX != grad_y && grad_zX != y &&
                   grad_zA != g && grad_zX != g && grad_zA != grad_zX,
               SNGNN_EINVAL, "g, grad_zA and grad_zX must not alias the inputs or each other");
    hipStream_t st = (hipStream_t)stream;
    switch ((H + 31) / 32) {
    case 1: return launch_join_bwd<1>(grad_y, y, ax, W, N, H, lsm != 0, g, grad_zA, grad_zX, st);
    case 2: return launch_join_bwd<2>(grad_y, y, ax, W, N, H, lsm != 0, g, grad_zA, grad_zX, st);
    case 3: return launch_join_bwd<3>(grad_y, y, ax, W, N, H, lsm != 0, g, grad_zA, grad_zX, st);
    default: return launch_join_bwd<4>(grad_y, y, ax, W, N, H, lsm != 0, g, grad_zA, grad_zX, st);
    }
}

// GGCN's layer transition (models/models.py:1544 + 1723-1736): the last line of GGCNlayer_SP,
//   y = scale * (prop + c2 * wh)                     (prop = c0 prop_pos + c1 prop_neg: the signed gather's output)
// and, between two layers, the model's elu and decayed residual behind it,
//   out = coeff * elu(y) + p,   p = prev | elu(prev) (the first transition: prev = fcn(x), coeff = 1).
// PyTorch runs these lines as about seven elementwise kernels forward and as many backward, each a full
// pass over [N, C]; here it is one pass each way over the flat n = N * C elements, with the reference's
// rounding (every product and sum rounded separately, in the order written; -ffp-contract=off).  The
// backward saves nothing: it re-reads prop and wh - which the two scalar gradients need anyway - and forms
// y again.  Those two sums follow the blend's scheme (blend.hip): per-block fp32 partials into the
// workspace, one block adds them in double in a fixed order - no float atomics, the same bits every run.
#include "common.h"
#include "device_utils.h"

namespace sngnn {

constexpr int GGCN_BLOCKS = 1024;
constexpr int GGCN_ACT = 1, GGCN_PREV_ELU = 2;

__device__ __forceinline__ float ggcn_elu(float v) { return v > 0.f ? v : expm1f(v); }

// SIGN: wh and cs = (c2, scale) are given; otherwise y = prop (use_sign=False, models.py:1546-1552)
template <bool ACT, bool PELU, bool SIGN>
__device__ __forceinline__ float ggcn_fwd1(float prop, float wh, float prev, float c2, float scale, float coeff)
{
    float y = prop;
    if constexpr (SIGN) y = scale * (prop + c2 * wh);
    if constexpr (ACT) {
        float p = prev;
        if constexpr (PELU) p = ggcn_elu(prev);
        return coeff * ggcn_elu(y) + p;
    }
    return y;
}

template <bool ACT, bool PELU, bool SIGN>
__global__ __launch_bounds__(256) void k_ggcn_fwd(const float *__restrict__ prop, const float *__restrict__ wh,
                                                  const float *__restrict__ cs, const float *__restrict__ prev,
                                                  float coeff, int64_t n4, int64_t n, float *__restrict__ out)
{
    float c2 = 0.f, scale = 1.f;
    if constexpr (SIGN) { c2 = cs[0]; scale = cs[1]; }
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 p = reinterpret_cast<const float4 *>(prop)[i];
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f), q = w;
        if constexpr (SIGN) w = reinterpret_cast<const float4 *>(wh)[i];
        if constexpr (ACT) q = reinterpret_cast<const float4 *>(prev)[i];
        reinterpret_cast<float4 *>(out)[i] =
            make_float4(ggcn_fwd1<ACT, PELU, SIGN>(p.x, w.x, q.x, c2, scale, coeff), ggcn_fwd1<ACT, PELU, SIGN>(p.y, w.y, q.y, c2, scale, coeff),
                        ggcn_fwd1<ACT, PELU, SIGN>(p.z, w.z, q.z, c2, scale, coeff), ggcn_fwd1<ACT, PELU, SIGN>(p.w, w.w, q.w, c2, scale, coeff));
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        float w = 0.f, q = 0.f;
        if constexpr (SIGN) w = wh[i];
        if constexpr (ACT) q = prev[i];
        out[i] = ggcn_fwd1<ACT, PELU, SIGN>(prop[i], w, q, c2, scale, coeff);
    }
}

// gy = d out / d y times g: coeff * g * elu'(y) (ACT) or g; grad_prop = scale * gy, grad_wh = c2 * grad_prop;
// acc0 += gy * wh, acc1 += gy * (prop + c2 * wh); under PELU grad_prev = g * elu'(prev)
template <bool ACT, bool PELU, bool SIGN>
__device__ __forceinline__ void ggcn_bwd1(float g, float prop, float wh, float prev, float c2, float scale, float coeff,
                                          float &gprop, float &gwh, float &gprev, float &acc0, float &acc1)
{
    float t = prop, gy = g;
    if constexpr (SIGN) t = prop + c2 * wh;
    if constexpr (ACT) {
        float y = t;
        if constexpr (SIGN) y = scale * t;
        gy = coeff * g;
        if (!(y > 0.f)) gy = gy * expf(y);
        if constexpr (PELU) gprev = prev > 0.f ? g : g * expf(prev);
    }
    if constexpr (SIGN) {
        gprop = scale * gy;
        gwh = c2 * gprop;
        acc0 += gy * wh;
        acc1 += gy * t;
    } else {
        gprop = gy;
    }
}

template <bool ACT, bool PELU, bool SIGN>
__global__ __launch_bounds__(256) void k_ggcn_bwd(const float *__restrict__ g, const float *__restrict__ prop,
                                                  const float *__restrict__ wh, const float *__restrict__ cs,
                                                  const float *__restrict__ prev, float coeff, int64_t n4, int64_t n,
                                                  float *__restrict__ gprop, float *__restrict__ gwh,
                                                  float *__restrict__ gprev, float *__restrict__ part)
{
    __shared__ float s0[256], s1[256];
    float c2 = 0.f, scale = 1.f;
    if constexpr (SIGN) { c2 = cs[0]; scale = cs[1]; }
    const int64_t stride = (int64_t)gridDim.x * 256;
    float acc0 = 0.f, acc1 = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 d = reinterpret_cast<const float4 *>(g)[i], p = reinterpret_cast<const float4 *>(prop)[i];
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f), q = w, gp, gw = w, gq = w;
        if constexpr (SIGN) w = reinterpret_cast<const float4 *>(wh)[i];
        if constexpr (PELU) q = reinterpret_cast<const float4 *>(prev)[i];
        ggcn_bwd1<ACT, PELU, SIGN>(d.x, p.x, w.x, q.x, c2, scale, coeff, gp.x, gw.x, gq.x, acc0, acc1);
        ggcn_bwd1<ACT, PELU, SIGN>(d.y, p.y, w.y, q.y, c2, scale, coeff, gp.y, gw.y, gq.y, acc0, acc1);
        ggcn_bwd1<ACT, PELU, SIGN>(d.z, p.z, w.z, q.z, c2, scale, coeff, gp.z, gw.z, gq.z, acc0, acc1);
        ggcn_bwd1<ACT, PELU, SIGN>(d.w, p.w, w.w, q.w, c2, scale, coeff, gp.w, gw.w, gq.w, acc0, acc1);
        reinterpret_cast<float4 *>(gprop)[i] = gp;
        if constexpr (SIGN) reinterpret_cast<float4 *>(gwh)[i] = gw;
        if constexpr (PELU) reinterpret_cast<float4 *>(gprev)[i] = gq;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        float w = 0.f, q = 0.f, gp, gw = 0.f, gq = 0.f;
        if constexpr (SIGN) w = wh[i];
        if constexpr (PELU) q = prev[i];
        ggcn_bwd1<ACT, PELU, SIGN>(g[i], prop[i], w, q, c2, scale, coeff, gp, gw, gq, acc0, acc1);
        gprop[i] = gp;
        if constexpr (SIGN) gwh[i] = gw;
        if constexpr (PELU) gprev[i] = gq;
    }
    if constexpr (SIGN) {
        s0[threadIdx.x] = acc0;
        s1[threadIdx.x] = acc1;
        __syncthreads();
        for (int m = 128; m >= 1; m >>= 1) {
            if (threadIdx.x < m) {
                s0[threadIdx.x] += s0[threadIdx.x + m];
                s1[threadIdx.x] += s1[threadIdx.x + m];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            part[blockIdx.x] = s0[0];
            part[GGCN_BLOCKS + blockIdx.x] = s1[0];
        }
    }
}

// grad_cs[0] = scale * sum gy wh, grad_cs[1] = sum gy (prop + c2 wh): the partials added in double, fixed order
__global__ __launch_bounds__(256) void k_ggcn_reduce(const float *__restrict__ part, int nblocks,
                                                     const float *__restrict__ cs, float *__restrict__ grad_cs)
{
    __shared__ double s0[256], s1[256];
    double a0 = 0.0, a1 = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        a0 += part[i];
        a1 += part[GGCN_BLOCKS + i];
    }
    s0[threadIdx.x] = a0;
    s1[threadIdx.x] = a1;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) {
            s0[threadIdx.x] += s0[threadIdx.x + m];
            s1[threadIdx.x] += s1[threadIdx.x + m];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        grad_cs[0] = (float)((double)cs[1] * s0[0]);
        grad_cs[1] = (float)s1[0];
    }
}

static int ggcn_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(GGCN_BLOCKS, (n / 4 + 255) / 256)); }

static bool ggcn_aligned(std::initializer_list<const void *> ps)
{
    uintptr_t a = 0;
    for (const void *p : ps) a |= (uintptr_t)p;          // (NULL contributes nothing)
    return a % 16 == 0;
}

}  // namespace sngnn

using namespace sngnn;

extern "C" int64_t sngnn_ggcn_transition_workspace_bytes(void) { return (int64_t)GGCN_BLOCKS * 2 * 4 + 256; }

// flags: 0 (combine), ACT, ACT | PREV_ELU
static bool ggcn_flags_ok(int flags) { return flags == 0 || flags == GGCN_ACT || flags == (GGCN_ACT | GGCN_PREV_ELU); }

#define GGCN_DISPATCH(KERNEL, flags, sign, ...)                                                          \
    do {                                                                                                 \
        if ((flags) == 0) {                                                                              \
            if (sign) KERNEL<false, false, true> __VA_ARGS__; else KERNEL<false, false, false> __VA_ARGS__; \
        } else if ((flags) == GGCN_ACT) {                                                                \
            if (sign) KERNEL<true, false, true> __VA_ARGS__; else KERNEL<true, false, false> __VA_ARGS__;   \
        } else {                                                                                         \
            if (sign) KERNEL<true, true, true> __VA_ARGS__; else KERNEL<true, true, false> __VA_ARGS__;     \
        }                                                                                                \
    } while (0)

extern "C" int sngnn_ggcn_transition_forward(const float *prop, const float *wh, const float *cs, const float *prev,
                                             float coeff, int flags, int64_t n, float *out, void *stream)
{
    SN_REQUIRE(n >= 0, SNGNN_EINVAL, "negative size");
    SN_REQUIRE(ggcn_flags_ok(flags), SNGNN_EINVAL, "flags must be 0, ACT or ACT | PREV_ELU");
    if (n == 0) return SNGNN_OK;          // (an empty tensor's pointer may be NULL: nothing is read)
    SN_REQUIRE((wh == nullptr) == (cs == nullptr), SNGNN_EINVAL, "wh and cs go together (both NULL: y = prop)");
    SN_REQUIRE(prop && out, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(!(flags & GGCN_ACT) || prev, SNGNN_EINVAL, "the transition needs prev");
    if (!(flags & GGCN_ACT)) prev = nullptr;
    const bool sign = wh != nullptr;
    const int64_t n4 = ggcn_aligned({prop, wh, prev, out}) ? n / 4 : 0;
    GGCN_DISPATCH(k_ggcn_fwd, flags, sign, <<<ggcn_grid(n), 256, 0, (hipStream_t)stream>>>(prop, wh, cs, prev, coeff, n4, n, out));
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_ggcn_transition_backward(const float *grad_out, const float *prop, const float *wh, const float *cs,
                                              const float *prev, float coeff, int flags, int64_t n, float *grad_prop,
                                              float *grad_wh, float *grad_prev, float *grad_cs, void *workspace,
                                              void *stream)
{
    SN_REQUIRE(n >= 0, SNGNN_EINVAL, "negative size");
    SN_REQUIRE(ggcn_flags_ok(flags), SNGNN_EINVAL, "flags must be 0, ACT or ACT | PREV_ELU");
    SN_REQUIRE(n == 0 || (wh == nullptr) == (cs == nullptr), SNGNN_EINVAL, "wh and cs go together (both NULL: y = prop)");
    const bool sign = cs != nullptr, pelu = (flags & GGCN_PREV_ELU) != 0;          // (n == 0: wh may be NULL)
    SN_REQUIRE(!sign || (grad_cs && workspace), SNGNN_EINVAL, "NULL argument (grad_cs / workspace)");
    if (n == 0 && !sign) return SNGNN_OK;
    hipStream_t st = (hipStream_t)stream;
    int nb = 0;
    if (n > 0) {
        SN_REQUIRE(grad_out && prop && grad_prop, SNGNN_EINVAL, "NULL argument");
        SN_REQUIRE(!sign || grad_wh, SNGNN_EINVAL, "NULL argument (grad_wh)");
        SN_REQUIRE(!pelu || (prev && grad_prev), SNGNN_EINVAL, "PREV_ELU needs prev and grad_prev");
        if (!pelu) { prev = nullptr; grad_prev = nullptr; }          // the gradient of prev is grad_out itself
        if (!sign) grad_wh = nullptr;
        const int64_t n4 = ggcn_aligned({grad_out, prop, wh, prev, grad_prop, grad_wh, grad_prev}) ? n / 4 : 0;
        nb = ggcn_grid(n);
        GGCN_DISPATCH(k_ggcn_bwd, flags, sign, <<<nb, 256, 0, st>>>(grad_out, prop, wh, cs, prev, coeff, n4, n, grad_prop,
                                                                   grad_wh, grad_prev, (float *)workspace));
    }
    if (sign) k_ggcn_reduce<<<1, 256, 0, st>>>((const float *)workspace, nb, cs, grad_cs);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

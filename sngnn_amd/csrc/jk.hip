// Jumping knowledge, 'max' (models/models.py:810, 840, 869, 897: PyG's JumpingKnowledge runs
// torch.stack(xs, -1).max(-1)[0]), gfx950, fp32, elementwise over L dense [N, C] tables:
//     forward    out[i] = max_l xs[l][i], which[i] = the layer it came from
//     backward   grads[l][i] = which[i] == l ? grad_out[i] : 0
// with torch's semantics exactly, as a scan over the layers in order: b = x_0, idx = 0; layer l replaces b iff
// x_l > b || (isnan(x_l) && !isnan(b)) - the FIRST maximal layer wins a tie, +0 and -0 tie (the first one's bits go
// out), the first NaN wins and sticks.  The reference's form is a stacked [N, C, L] copy, a reduction with an int64 index
// per element and, backward, a scatter into a zeroed [N, C, L] tensor whose per-layer views are stride-L; here every
// byte moves once: forward 4L + 4 + 1 bytes an element, backward 4 + 1 + 4L (every element of every wanted layer is
// stored, so nothing is zero-filled first).
// A flat streaming kernel: a lane takes 4 consecutive elements (16-byte row accesses, one packed 4-byte access of
// `which`) where every base pointer is 16-byte aligned, 1 element otherwise; the N C % 4 elements behind the last whole
// vector go to the first lanes of the grid as scalars.  L is a run-time loop over the pointer table in the kernel
// arguments (a uniform index: scalar loads).  No LDS, no atomics, no scratch.
#include <algorithm>

#include "common.h"

namespace sngnn {

struct JkTables { const float *p[SNGNN_JK_MAX_LAYERS]; };
struct JkGrads { float *p[SNGNN_JK_MAX_LAYERS]; };

constexpr int JK_BLOCK = 256, JK_MAX_GRID = 2048;

__device__ __forceinline__ void jk_scan(float x, int l, float &b, unsigned &idx)
{
    if (x > b || (x != x && b == b)) { b = x; idx = (unsigned)l; }
}

// `total` elements; VEC = 4: the first total / 4 vectors, then the tail as scalars by the grid's first lanes
template <int VEC>
__global__ __launch_bounds__(JK_BLOCK) void k_jk_max_fwd(JkTables xs, int L, int64_t total, float *__restrict__ out,
                                                          unsigned char *__restrict__ which)
{
    const int64_t tid = (int64_t)blockIdx.x * JK_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * JK_BLOCK;
    const int64_t nvec = VEC == 4 ? total / 4 : 0;          // whole vectors; everything behind them is scalar
    if constexpr (VEC == 4) {
        for (int64_t i = tid; i < nvec; i += step) {
            float4 b = reinterpret_cast<const float4 *>(xs.p[0])[i];
            unsigned i0 = 0, i1 = 0, i2 = 0, i3 = 0;
            for (int l = 1; l < L; ++l) {
                const float4 x = reinterpret_cast<const float4 *>(xs.p[l])[i];
                jk_scan(x.x, l, b.x, i0);
                jk_scan(x.y, l, b.y, i1);
                jk_scan(x.z, l, b.z, i2);
                jk_scan(x.w, l, b.w, i3);
            }
            reinterpret_cast<float4 *>(out)[i] = b;
            if (which) reinterpret_cast<unsigned *>(which)[i] = i0 | (i1 << 8) | (i2 << 16) | (i3 << 24);
        }
    }
    // scalars: everything (VEC == 1) or the tail behind the last whole vector
    for (int64_t i = nvec * 4 + tid; i < total; i += step) {
        float b = xs.p[0][i];
        unsigned idx = 0;
        for (int l = 1; l < L; ++l) jk_scan(xs.p[l][i], l, b, idx);
        out[i] = b;
        if (which) which[i] = (unsigned char)idx;
    }
}

template <int VEC>
__global__ __launch_bounds__(JK_BLOCK) void k_jk_max_bwd(const float *__restrict__ gout,
                                                          const unsigned char *__restrict__ which, int L, int64_t total,
                                                          JkGrads grads)
{
    const int64_t tid = (int64_t)blockIdx.x * JK_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * JK_BLOCK;
    const int64_t nvec = VEC == 4 ? total / 4 : 0;          // whole vectors; everything behind them is scalar
    if constexpr (VEC == 4) {
        for (int64_t i = tid; i < nvec; i += step) {
            const float4 g = reinterpret_cast<const float4 *>(gout)[i];
            const unsigned w = reinterpret_cast<const unsigned *>(which)[i];
            const unsigned i0 = w & 255u, i1 = (w >> 8) & 255u, i2 = (w >> 16) & 255u, i3 = w >> 24;
            for (int l = 0; l < L; ++l) {
                float *dst = grads.p[l];
                if (!dst) continue;
                const unsigned ul = (unsigned)l;
                reinterpret_cast<float4 *>(dst)[i] = make_float4(i0 == ul ? g.x : 0.f, i1 == ul ? g.y : 0.f,
                                                                 i2 == ul ? g.z : 0.f, i3 == ul ? g.w : 0.f);
            }
        }
    }
    for (int64_t i = nvec * 4 + tid; i < total; i += step) {
        const float g = gout[i];
        const unsigned idx = which[i];
        for (int l = 0; l < L; ++l) {
            float *dst = grads.p[l];
            if (dst) dst[i] = idx == (unsigned)l ? g : 0.f;
        }
    }
}

// min(ceil(work / block), 2048) workgroups, the rest by the grid-stride loops
static int jk_grid(int64_t total, int vec)
{
    const int64_t work = std::max<int64_t>(total / vec, vec > 1 ? total % vec : 0);
    return (int)std::min<int64_t>(std::max<int64_t>((work + JK_BLOCK - 1) / JK_BLOCK, 1), JK_MAX_GRID);
}

static bool jk_shape_ok(int L, int64_t N, int C, int &rc)
{
    rc = SNGNN_OK;
    if (L < 1 || L > SNGNN_JK_MAX_LAYERS) {
        set_error("L must be in [1, " + std::to_string(SNGNN_JK_MAX_LAYERS) + "] (more layers run the plain op sequence)");
        rc = SNGNN_ERANGE;
        return false;
    }
    if (N < 0 || C < 1) { set_error("bad shape"); rc = SNGNN_EINVAL; return false; }
    return true;
}

}  // namespace sngnn

using namespace sngnn;

extern "C" int sngnn_jk_max_forward(const float *const *xs, int L, int64_t N, int C, float *out, unsigned char *which,
                                    void *stream)
{
    int rc;
    if (!jk_shape_ok(L, N, C, rc)) return rc;
    SN_REQUIRE(xs && out, SNGNN_EINVAL, "NULL argument");
    JkTables t = {};
    uintptr_t bits = (uintptr_t)out | (uintptr_t)which;
    for (int l = 0; l < L; ++l) {
        SN_REQUIRE(xs[l], SNGNN_EINVAL, "NULL row pointer");
        SN_REQUIRE(xs[l] != out, SNGNN_EINVAL, "out must not alias an input");
        t.p[l] = xs[l];
        bits |= (uintptr_t)xs[l];
    }
    if (N == 0) return SNGNN_OK;
    const int64_t total = N * (int64_t)C;
    hipStream_t st = (hipStream_t)stream;
    if (bits % 16 == 0)
        k_jk_max_fwd<4><<<jk_grid(total, 4), JK_BLOCK, 0, st>>>(t, L, total, out, which);
    else
        k_jk_max_fwd<1><<<jk_grid(total, 1), JK_BLOCK, 0, st>>>(t, L, total, out, which);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_jk_max_backward(const float *grad_out, const unsigned char *which, int L, int64_t N, int C,
                                     float *const *grads, void *stream)
{
    int rc;
    if (!jk_shape_ok(L, N, C, rc)) return rc;
    SN_REQUIRE(grad_out && which && grads, SNGNN_EINVAL, "NULL argument");
    JkGrads t = {};
    uintptr_t bits = (uintptr_t)grad_out | (uintptr_t)which;
    bool any = false;
    for (int l = 0; l < L; ++l) {
        if (!grads[l]) continue;          // this layer wants no gradient
        SN_REQUIRE(grads[l] != grad_out, SNGNN_EINVAL, "a gradient must not alias grad_out");
        for (int m = 0; m < l; ++m)
            SN_REQUIRE(grads[m] != grads[l], SNGNN_EINVAL, "the gradients must not alias each other");
        t.p[l] = grads[l];
        bits |= (uintptr_t)grads[l];
        any = true;
    }
    if (N == 0 || !any) return SNGNN_OK;
    const int64_t total = N * (int64_t)C;
    hipStream_t st = (hipStream_t)stream;
    if (bits % 16 == 0)
        k_jk_max_bwd<4><<<jk_grid(total, 4), JK_BLOCK, 0, st>>>(grad_out, which, L, total, t);
    else
        k_jk_max_bwd<1><<<jk_grid(total, 1), JK_BLOCK, 0, st>>>(grad_out, which, L, total, t);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

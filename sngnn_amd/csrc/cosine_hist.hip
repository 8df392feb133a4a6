// Node-similarity distribution on fp32 tables: sngnn_cosine_hist (the kernels and the launch plan:
// cosine_hist_scan.h) and knob 10.
#include "cosine_hist_scan.h"

using namespace sngnn;

// knob 10: copies of the LDS counter table (0 = as many as fit, up to 16; 1 = the plain form; 2, 4, 8, 16)
static int g_hist_copies = 0;
namespace sngnn {
int set_hist_copies(int v)
{
    if (v != 0 && v != 1 && v != 2 && v != 4 && v != 8 && v != 16) return SNGNN_EINVAL;
    g_hist_copies = v;
    return SNGNN_OK;
}
int hist_copies_knob() { return g_hist_copies; }
}

// F in {32, 64, 96, 128} with 16-byte rows: the register-operand path (bf16 products: 256 rows x 64-column tiles)
static bool hist_regs(int64_t F, const float *x)
{
    return (F == 128 || F == 96 || F == 64 || F == 32) && (uintptr_t)x % 16 == 0;
}

extern "C" int64_t sngnn_cosine_hist_workspace_bytes(int64_t N, int64_t F, int bins, int groups)
{
    (void)F; (void)bins; (void)groups;
    if (N < 0) return 0;
    // inverse norms, then per workgroup min, max (f32) and sum (f64)
    return (N + 63) / 64 * 256 + (hist_parts(N) + 15) / 16 * 16 * 16 + 256;
}

extern "C" int sngnn_cosine_hist(const float *x, int64_t N, int64_t F, const int32_t *y, const float *edges, int bins,
                                 unsigned long long *counts, double *stats, void *workspace, void *stream)
{
    SN_REQUIRE(N >= 0 && F >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(bins >= 1 && bins <= CH_MAX_BINS, SNGNN_EINVAL, "bins must be in [1, " + std::to_string(CH_MAX_BINS) + "]");
    SN_REQUIRE(N < ((int64_t)1 << 31), SNGNN_EINVAL, "too many rows");
    SN_REQUIRE(edges && counts && stats, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(N == 0 || (x && workspace), SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int groups = y != nullptr ? 2 : 1;
    const int width = groups * (bins + 2);
    k_hist_zero<<<(width + 255) / 256, 256, 0, st>>>(counts, width);
    float *inv = (float *)workspace;
    const int64_t parts_cap = (hist_parts(N) + 15) / 16 * 16;
    float *pmin = (float *)((char *)workspace + (N + 63) / 64 * 256);
    float *pmax = pmin + parts_cap;
    double *psum = (double *)(pmax + parts_cap);
    int64_t nparts = 0;
    if (N >= 2) {
        const bool regs = hist_regs(F, x), bf3 = !sngnn::fp32_mfma_only();
        const bool wide = regs && bf3;
        const HistPlan p = hist_plan(N, wide ? 256 : KN_M, wide ? 64 : KN_M);
        nparts = p.nrb * p.ns;
        SN_REQUIRE(p.ns <= 65535, SNGNN_EINVAL, "internal: too many column ranges");
        const int ncopy = hist_copies(width, g_hist_copies);
        k_knn_inv_norm<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(x, N, F, inv);
        dim3 grid((unsigned)p.nrb, (unsigned)p.ns);
#define SN_HIST_GO(FH_, BF3_, NWV_, CB_)                                                                         \
        k_cosine_hist<FH_, BF3_, NWV_, CB_><<<grid, 64 * NWV_, 0, st>>>(x, N, F, inv, y, edges, bins, ncopy, p.tps, \
                                                                      counts, pmin, pmax, psum)
        if (wide && F == 128) SN_HIST_GO(64, true, 8, 2);
        else if (wide && F == 96) SN_HIST_GO(48, true, 8, 2);
        else if (wide && F == 64) SN_HIST_GO(32, true, 8, 2);
        else if (wide) SN_HIST_GO(16, true, 8, 2);
        else if (regs && F == 128) SN_HIST_GO(64, false, 4, 4);
        else if (regs && F == 96) SN_HIST_GO(48, false, 4, 4);
        else if (regs && F == 64) SN_HIST_GO(32, false, 4, 4);
        else if (regs) SN_HIST_GO(16, false, 4, 4);
        else SN_HIST_GO(0, false, 4, 4);
#undef SN_HIST_GO
    }
    k_hist_stats<<<1, 1024, 0, st>>>(pmin, pmax, psum, nparts, stats);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

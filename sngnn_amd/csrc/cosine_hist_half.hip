// Node-similarity distribution straight from an fp16 / bf16 table: sngnn_cosine_hist_half.  The scan of
// cosine_hist_scan.h on the engine's half forms (cosine_tiles.h, PL = 2 / 1; see knn_half.hip); counting, statistics,
// launch plan and workspace are sngnn_cosine_hist's.
#include "cosine_hist_scan.h"

using namespace sngnn;

namespace {

template <typename S, int PL>
void hist_go(const unsigned short *x, int64_t N, int64_t F, float *inv, const int32_t *y, const float *edges, int bins,
             int ncopy, const HistPlan &p, unsigned long long *counts, float *pmin, float *pmax, double *psum, hipStream_t st)
{
    k_knn_inv_norm_half<S><<<(unsigned)((N + 3) / 4), 256, 0, st>>>(x, N, F, inv);
    dim3 grid((unsigned)p.nrb, (unsigned)p.ns);
#define SN_HISTH_GO(FH_) k_cosine_hist<FH_, true, 8, 2, PL><<<grid, 512, 0, st>>>(x, N, F, inv, y, edges, bins, ncopy, p.tps, counts, pmin, pmax, psum)
    if (F == 128) SN_HISTH_GO(64);
    else if (F == 96) SN_HISTH_GO(48);
    else if (F == 64) SN_HISTH_GO(32);
    else SN_HISTH_GO(16);
#undef SN_HISTH_GO
}

}  // namespace

extern "C" int sngnn_cosine_hist_half(const void *x, int dtype, int64_t N, int64_t F, const int32_t *y, const float *edges,
                                      int bins, unsigned long long *counts, double *stats, void *workspace, void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    SN_REQUIRE(N >= 0 && F >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(bins >= 1 && bins <= CH_MAX_BINS, SNGNN_EINVAL, "bins must be in [1, " + std::to_string(CH_MAX_BINS) + "]");
    SN_REQUIRE(N < ((int64_t)1 << 31), SNGNN_EINVAL, "too many rows");
    SN_REQUIRE(sngnn_cosine_scan_half_supported(F, dtype), SNGNN_EINVAL,
               "no native half scan here: F must be 32, 64, 96 or 128, knob 5 off (bf16 products) and knob 6 not 3");
    SN_REQUIRE(edges && counts && stats, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(N == 0 || (x && workspace), SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((uintptr_t)x % 16 == 0, SNGNN_EINVAL, "the table's base must be 16-byte aligned");
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
        const HistPlan p = hist_plan(N, 256, 64);
        nparts = p.nrb * p.ns;
        SN_REQUIRE(p.ns <= 65535, SNGNN_EINVAL, "internal: too many column ranges");
        const int ncopy = hist_copies(width, sngnn::hist_copies_knob());
        const unsigned short *xs = static_cast<const unsigned short *>(x);
        if (dtype == SNGNN_DTYPE_F16) hist_go<__half, 2>(xs, N, F, inv, y, edges, bins, ncopy, p, counts, pmin, pmax, psum, st);
        else hist_go<__hip_bfloat16, 1>(xs, N, F, inv, y, edges, bins, ncopy, p, counts, pmin, pmax, psum, st);
    }
    k_hist_stats<<<1, 1024, 0, st>>>(pmin, pmax, psum, nparts, stats);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

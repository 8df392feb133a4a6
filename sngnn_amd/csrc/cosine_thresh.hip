// Threshold similarity graph on fp32 tables: sngnn_cosine_threshold_count / _fill (the kernels: cosine_thresh_scan.h).
// Engine variant and column ranges by sngnn_knn_query's rule (knn.hip): F, knobs 5 and 6, the 16-byte alignment of
// both tables - so every value is the one that entry forms, and the count and the fill of one call agree.
#include "cosine_thresh_scan.h"

using namespace sngnn;

namespace {

// one pass of the scan (FILL: the second).  sngnn_knn_query's dispatch.
template <bool FILL>
void thresh_scan(const float *xq, int64_t M, const float *xb, int64_t N, int64_t F, float thr, int64_t self_offset,
                 const ThreshWs &ws, const int64_t *rowptr, int64_t nnz, int32_t *out_col, float *out_val, int *ns_out,
                 hipStream_t st)
{
    const bool areg = (uintptr_t)xq % 16 == 0 && (uintptr_t)xb % 16 == 0;
    const bool bf3 = !sngnn::fp32_mfma_only();          // sngnn_tuning_set(5, 1): fp32 MFMAs
    const bool wide = areg && (F == 128 || F == 96 || F == 64 || F == 32) && bf3 && !sngnn::knn_no_wide_tiles();
    const KnnQueryPlan p = knn_query_plan(M, N, wide ? 256 : KN_M, wide ? 64 : KN_M);
    *ns_out = p.ns;
    dim3 grid((unsigned)p.nrb, (unsigned)p.ns);
#define SN_THRESH_GO(FH_, BF3_, NWV_, CB_)                                                                          \
    k_cosine_thresh<FH_, BF3_, NWV_, CB_, FILL><<<grid, 64 * NWV_, 0, st>>>(xq, M, ws.invq, xb, N, F, ws.invb, thr,    \
                                                                           self_offset, p.tps, ws.part, rowptr, nnz,  \
                                                                           out_col, out_val)
    if (wide && F == 128) SN_THRESH_GO(64, true, 8, 2);
    else if (wide && F == 96) SN_THRESH_GO(48, true, 8, 2);
    else if (wide && F == 64) SN_THRESH_GO(32, true, 8, 2);
    else if (wide) SN_THRESH_GO(16, true, 8, 2);
    else if (areg && F == 128) { if (bf3) SN_THRESH_GO(64, true, 4, 4); else SN_THRESH_GO(64, false, 4, 4); }
    else if (areg && F == 96) { if (bf3) SN_THRESH_GO(48, true, 4, 4); else SN_THRESH_GO(48, false, 4, 4); }
    else if (areg && F == 64) { if (bf3) SN_THRESH_GO(32, true, 4, 4); else SN_THRESH_GO(32, false, 4, 4); }
    else if (areg && F == 32) { if (bf3) SN_THRESH_GO(16, true, 4, 4); else SN_THRESH_GO(16, false, 4, 4); }
    else SN_THRESH_GO(0, false, 4, 4);
#undef SN_THRESH_GO
}

}  // namespace

extern "C" int64_t sngnn_cosine_threshold_workspace_bytes(int64_t M, int64_t N)
{
    if (M < 0 || N < 0) return 0;
    const int64_t ns = thresh_ranges_max(M, N);
    return (M + 63) / 64 * 256 + (N + 63) / 64 * 256 + (ns * M * 4 + 255) / 256 * 256 + 256;
}

extern "C" int sngnn_cosine_threshold_count(const float *xq, int64_t M, const float *xb, int64_t N, int64_t F, float thr,
                                            int64_t self_offset, int32_t *count, void *workspace, void *stream)
{
    if (const int rc = thresh_check(M, N, F, thr, self_offset)) return rc;
    if (M == 0) return SNGNN_OK;
    SN_REQUIRE(xq && count && workspace && (xb || N == 0), SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        k_thresh_zero<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(count, M);
        SN_HIP(hipGetLastError());
        return SNGNN_OK;
    }
    const ThreshWs ws = thresh_ws(workspace, M, N);
    k_knn_inv_norm<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(xq, M, F, ws.invq);
    k_knn_inv_norm<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(xb, N, F, ws.invb);
    int ns = 0;
    thresh_scan<false>(xq, M, xb, N, F, thr, self_offset, ws, nullptr, 0, nullptr, nullptr, &ns, st);
    k_thresh_ranges<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(ws.part, M, ns, count);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_cosine_threshold_fill(const float *xq, int64_t M, const float *xb, int64_t N, int64_t F, float thr,
                                           int64_t self_offset, const int64_t *rowptr, int64_t nnz, int32_t *out_col,
                                           float *out_val, void *workspace, void *stream)
{
    if (const int rc = thresh_check(M, N, F, thr, self_offset)) return rc;
    SN_REQUIRE(nnz >= 0, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(nnz <= (int64_t)0x7FFFFFFF, SNGNN_ERANGE, "more than 2^31 - 1 entries");
    if (M == 0) return SNGNN_OK;
    SN_REQUIRE(xq && rowptr && workspace && (xb || N == 0) && ((out_col && out_val) || nnz == 0), SNGNN_EINVAL,
               "NULL argument");
    if (N == 0 || nnz == 0) return SNGNN_OK;               // no entry to write
    hipStream_t st = (hipStream_t)stream;
    int ns = 0;
    thresh_scan<true>(xq, M, xb, N, F, thr, self_offset, thresh_ws(workspace, M, N), rowptr, nnz, out_col, out_val, &ns, st);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

// Threshold similarity graph straight from fp16 / bf16 tables: sngnn_cosine_threshold_count_half / _fill_half.  The
// two passes of cosine_thresh_scan.h on the engine's half forms (cosine_tiles.h, PL = 2 / 1; see knn_half.hip): the
// tables are read as stored - no fp32 copies - and only the products of the bf16 planes such a value has are issued,
// in BOTH passes.  One shape, 256 rows x 64-column tiles, F in {32, 64, 96, 128}; the column ranges, the workspace
// layout, the range prefix and the refusals are the fp32 entries'.  On finite tables the CSR is the fp32 entries' on
// the widened tables, bit for bit.
#include "cosine_thresh_scan.h"

using namespace sngnn;

namespace {

template <typename S> struct Planes;
template <> struct Planes<__half> { static constexpr int PL = 2; };
template <> struct Planes<__hip_bfloat16> { static constexpr int PL = 1; };

// one pass of the scan (FILL: the second)
template <typename S, bool FILL>
void thresh_go(const unsigned short *xq, int64_t M, const unsigned short *xb, int64_t N, int64_t F, float thr,
               int64_t self_offset, const ThreshWs &ws, const KnnQueryPlan &p, const int64_t *rowptr, int64_t nnz,
               int32_t *out_col, float *out_val, hipStream_t st)
{
    constexpr int PL = Planes<S>::PL;
    dim3 grid((unsigned)p.nrb, (unsigned)p.ns);
#define SN_THRESHH_GO(FH_)                                                                                           \
    k_cosine_thresh<FH_, true, 8, 2, FILL, PL><<<grid, 512, 0, st>>>(xq, M, ws.invq, xb, N, F, ws.invb, thr,         \
                                                                     self_offset, p.tps, ws.part, rowptr, nnz,       \
                                                                     out_col, out_val)
    if (F == 128) SN_THRESHH_GO(64);
    else if (F == 96) SN_THRESHH_GO(48);
    else if (F == 64) SN_THRESHH_GO(32);
    else SN_THRESHH_GO(16);
#undef SN_THRESHH_GO
}

template <typename S>
void count_go(const unsigned short *xq, int64_t M, const unsigned short *xb, int64_t N, int64_t F, float thr,
              int64_t self_offset, int32_t *count, void *workspace, hipStream_t st)
{
    const ThreshWs ws = thresh_ws(workspace, M, N);
    const KnnQueryPlan p = knn_query_plan(M, N, 256, 64);
    k_knn_inv_norm_half<S><<<(unsigned)((M + 3) / 4), 256, 0, st>>>(xq, M, F, ws.invq);
    k_knn_inv_norm_half<S><<<(unsigned)((N + 3) / 4), 256, 0, st>>>(xb, N, F, ws.invb);
    thresh_go<S, false>(xq, M, xb, N, F, thr, self_offset, ws, p, nullptr, 0, nullptr, nullptr, st);
    k_thresh_ranges<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(ws.part, M, p.ns, count);
}

// what the half entries refuse beyond thresh_check; the alignment is checked once the pointers are known to be there
int half_check(int dtype, int64_t F)
{
    SN_REQUIRE(sngnn_cosine_scan_half_supported(F, dtype), SNGNN_EINVAL,
               "no native half scan here: F must be 32, 64, 96 or 128, knob 5 off (bf16 products) and knob 6 not 3");
    return SNGNN_OK;
}

}  // namespace

extern "C" int sngnn_cosine_threshold_count_half(const void *xq, int64_t M, const void *xb, int dtype, int64_t N, int64_t F,
                                                 float thr, int64_t self_offset, int32_t *count, void *workspace,
                                                 void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    if (const int rc = thresh_check(M, N, F, thr, self_offset)) return rc;
    if (const int rc = half_check(dtype, F)) return rc;
    if (M == 0) return SNGNN_OK;
    SN_REQUIRE(xq && count && workspace && (xb || N == 0), SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((uintptr_t)xq % 16 == 0 && (uintptr_t)xb % 16 == 0, SNGNN_EINVAL, "both tables' bases must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        k_thresh_zero<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(count, M);
        SN_HIP(hipGetLastError());
        return SNGNN_OK;
    }
    const unsigned short *qs = static_cast<const unsigned short *>(xq), *bs = static_cast<const unsigned short *>(xb);
    if (dtype == SNGNN_DTYPE_F16) count_go<__half>(qs, M, bs, N, F, thr, self_offset, count, workspace, st);
    else count_go<__hip_bfloat16>(qs, M, bs, N, F, thr, self_offset, count, workspace, st);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

extern "C" int sngnn_cosine_threshold_fill_half(const void *xq, int64_t M, const void *xb, int dtype, int64_t N, int64_t F,
                                                float thr, int64_t self_offset, const int64_t *rowptr, int64_t nnz,
                                                int32_t *out_col, float *out_val, void *workspace, void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    if (const int rc = thresh_check(M, N, F, thr, self_offset)) return rc;
    SN_REQUIRE(nnz >= 0, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(nnz <= (int64_t)0x7FFFFFFF, SNGNN_ERANGE, "more than 2^31 - 1 entries");
    if (const int rc = half_check(dtype, F)) return rc;
    if (M == 0) return SNGNN_OK;
    SN_REQUIRE(xq && rowptr && workspace && (xb || N == 0) && ((out_col && out_val) || nnz == 0), SNGNN_EINVAL,
               "NULL argument");
    SN_REQUIRE((uintptr_t)xq % 16 == 0 && (uintptr_t)xb % 16 == 0, SNGNN_EINVAL, "both tables' bases must be 16-byte aligned");
    if (N == 0 || nnz == 0) return SNGNN_OK;               // no entry to write
    hipStream_t st = (hipStream_t)stream;
    const ThreshWs ws = thresh_ws(workspace, M, N);
    const KnnQueryPlan p = knn_query_plan(M, N, 256, 64);
    const unsigned short *qs = static_cast<const unsigned short *>(xq), *bs = static_cast<const unsigned short *>(xb);
    if (dtype == SNGNN_DTYPE_F16)
        thresh_go<__half, true>(qs, M, bs, N, F, thr, self_offset, ws, p, rowptr, nnz, out_col, out_val, st);
    else
        thresh_go<__hip_bfloat16, true>(qs, M, bs, N, F, thr, self_offset, ws, p, rowptr, nnz, out_col, out_val, st);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

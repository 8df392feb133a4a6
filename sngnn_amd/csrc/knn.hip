// kNN similarity-graph builder on fp32 tables: sngnn_knn_graph and sngnn_knn_query (the kernels: knn_scan.h), knob 6,
// and the two questions the half entries' callers ask - which route the square call takes, and whether the native
// half scan exists (knn_half.hip, cosine_hist_half.hip).
#include "knn_scan.h"

using namespace sngnn;

// 0 = by shape (default), 1 = the fused scan always, 2 = materialise + select always (measurement: sngnn_tuning_set(6, v))
// (value 3 / 4 - measurement: the fused scan with the 128 x 128 / the 256 x 64 tile shape whatever the width allows)
static int g_knn_route = 0, g_knn_shape = 0;
namespace sngnn {
int set_knn_route(int v)
{
    if (v < 0 || v > 4) return SNGNN_EINVAL;
    g_knn_shape = v == 3 ? 1 : 0;            // 1: never the <8, 2> shape
    g_knn_route = v >= 3 ? 1 : v;
    return SNGNN_OK;
}
bool knn_no_wide_tiles() { return g_knn_shape == 1; }
}

// (F in {32, 64, 96, 128} with 16-byte rows, bf16 products: the <8, 2> shape - 256 rows per workgroup, 64-column tiles,
// two waves per SIMD: 76 -> 58 ms at arxiv size)
static bool knn_wide(int64_t F, const float *x)
{
    return (F == 128 || F == 96 || F == 64 || F == 32) && (uintptr_t)x % 16 == 0 && !sngnn::fp32_mfma_only() && g_knn_shape != 1;
}

// the native scan of a half table exists in one form: the <8, 2> shape with bf16 products
extern "C" int sngnn_cosine_scan_half_supported(int64_t F, int dtype)
{
    return (dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16) && (F == 128 || F == 96 || F == 64 || F == 32) &&
           !sngnn::fp32_mfma_only() && g_knn_shape != 1;
}

static bool knn_dense_route(int64_t N)
{
    return g_knn_route == 2 || (g_knn_route == 0 && N <= KNN_DENSE_MAX_N && N >= 2);
}

extern "C" int sngnn_knn_graph_route(int64_t N) { return knn_dense_route(N) ? 2 : 1; }

extern "C" int64_t sngnn_knn_workspace_bytes(int64_t N, int k)
{
    const int ns = std::max(knn_splits(N), knn_splits(N, 256));       // (either tile shape)
    return (N + 63) / 64 * 256 + (ns > 1 ? (int64_t)ns * N * k * 8 : 0) + 256;
}

extern "C" int sngnn_knn_graph(const float *x, int64_t N, int64_t F, int k, int exclude_self,
                               int32_t *nbr_idx, float *nbr_sim, void *workspace, void *stream)
{
    SN_REQUIRE(N >= 0 && F >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(k >= 1 && k <= KNN_MAX_K, SNGNN_EINVAL, "k must be in [1, " + std::to_string(KNN_MAX_K) + "]");
    SN_REQUIRE(N < ((int64_t)1 << 31), SNGNN_EINVAL, "too many rows");
    if (N == 0) return SNGNN_OK;
    SN_REQUIRE(x && nbr_idx && nbr_sim && workspace, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    // (narrow features too: at 20 000 x 128 the fused scan's register-operand path takes 3.1 ms - few row
    // blocks, lists warmed up per column split - against ~1.2 ms for S + selection)
    if (knn_dense_route(N)) {
        // materialise + select (see k_row_topk); S lives in a stream-ordered allocation
        SN_REQUIRE(N <= 65535, SNGNN_EINVAL, "the dense route is for small graphs");
        // (outside the caller's allocator: up to 4.3 GB.  When the device cannot give it - the caller's pool holds
        // most of HBM - the fused scan below does the same job from the few MB of the workspace, unless the
        // dense route was forced)
        void *S = nullptr;
        const hipError_t got = hipMallocAsync(&S, (size_t)N * N * 4, st);
        if (got == hipSuccess) {
            int rc = sngnn_cosine_dense(x, N, F, (float *)S, stream);
            if (rc == SNGNN_OK) {
                int lowbits = 1;
                while (((int64_t)1 << lowbits) < N && lowbits < 31) ++lowbits;
                k_row_topk<<<(unsigned)((N + 3) / 4), 256, 0, st>>>((const float *)S, N, k, exclude_self, lowbits, nbr_idx, nbr_sim);
                if (hipGetLastError() != hipSuccess) rc = SNGNN_EHIP;
            }
            (void)hipFreeAsync(S, st);
            return rc;
        }
        (void)hipGetLastError();          // clear the allocation failure
        SN_REQUIRE(g_knn_route != 2, SNGNN_ENOMEM, "out of device memory for the dense route's N x N matrix");
    }
    float *inv = (float *)workspace;
    unsigned long long *part = (unsigned long long *)((char *)workspace + (N + 63) / 64 * 256);
    const bool wide = knn_wide(F, x);
    const int rows_wg = wide ? 256 : KN_M, cols_tile = wide ? 64 : KN_M;
    const int ns = knn_splits(N, rows_wg);
    const int64_t nrb = (N + rows_wg - 1) / rows_wg, nct = (N + cols_tile - 1) / cols_tile;
    const int tps = (int)((nct + ns - 1) / ns);          // column tiles per split
    const int ns_used = (int)((nct + tps - 1) / tps);
    k_knn_inv_norm<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(x, N, F, inv);
    dim3 grid((unsigned)nrb, (unsigned)ns_used);
    unsigned long long *pp = ns_used > 1 ? part : nullptr;
    const bool areg = (uintptr_t)x % 16 == 0;
    const bool bf3 = !sngnn::fp32_mfma_only();          // sngnn_tuning_set(5, 1): fp32 MFMAs
    if (wide && F == 128) k_knn_mfma<64, true, 8, 2><<<grid, 512, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim);
    else if (wide && F == 96) k_knn_mfma<48, true, 8, 2><<<grid, 512, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim);
    else if (wide && F == 64) k_knn_mfma<32, true, 8, 2><<<grid, 512, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim);
    else if (wide) k_knn_mfma<16, true, 8, 2><<<grid, 512, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim);
    else if (areg && F == 128) { if (bf3) k_knn_mfma<64, true><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim); else k_knn_mfma<64, false><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim); }
    else if (areg && F == 96) { if (bf3) k_knn_mfma<48, true><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim); else k_knn_mfma<48, false><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim); }
    else if (areg && F == 64) { if (bf3) k_knn_mfma<32, true><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim); else k_knn_mfma<32, false><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim); }
    else if (areg && F == 32) { if (bf3) k_knn_mfma<16, true><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim); else k_knn_mfma<16, false><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim); }
    else k_knn_mfma<0, false><<<grid, 256, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim);
    if (ns_used > 1) k_knn_merge<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(part, N, k, ns_used, nbr_idx, nbr_sim);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

// ---------------------------------------------------------------------------
// Two tables: the lists of M query rows against a base of N rows (see knn_scan).  The engine variant follows the
// square scan's rule - F, knob 5, and the 16-byte alignment of BOTH tables, so that a row range of an aligned base
// takes the variant the square scan takes on that base.  (The column splits: knn_query_plan, knn_scan.h.)
// ---------------------------------------------------------------------------
extern "C" int64_t sngnn_knn_query_workspace_bytes(int64_t M, int64_t N, int k)
{
    if (M < 0 || N < 0 || k < 1) return 0;
    const int ns = std::max(knn_query_plan(M, N, KN_M, KN_M).ns, knn_query_plan(M, N, 256, 64).ns);       // (either tile shape)
    // the inverse norms of the queries and of the base, then the column splits' partial lists
    return (M + 63) / 64 * 256 + (N + 63) / 64 * 256 + (ns > 1 ? (int64_t)ns * M * k * 8 : 0) + 256;
}

extern "C" int sngnn_knn_query(const float *xq, int64_t M, const float *xb, int64_t N, int64_t F, int k,
                               int64_t self_offset, int32_t *nbr_idx, float *nbr_sim, void *workspace, void *stream)
{
    SN_REQUIRE(M >= 0 && N >= 0 && F >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(k >= 1 && k <= KNN_MAX_K, SNGNN_EINVAL, "k must be in [1, " + std::to_string(KNN_MAX_K) + "]");
    SN_REQUIRE(M < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), SNGNN_EINVAL, "too many rows");
    SN_REQUIRE(self_offset >= -1 && (self_offset < 0 || self_offset + M <= N), SNGNN_EINVAL,
               "self_offset: the queries are not rows [self_offset, self_offset + M) of the base");
    if (M == 0) return SNGNN_OK;
    SN_REQUIRE(xq && nbr_idx && nbr_sim && workspace && (xb || N == 0), SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {                              // no base row: every slot is padding (a merge of no lists)
        k_knn_merge<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(nullptr, M, k, 0, nbr_idx, nbr_sim);
        SN_HIP(hipGetLastError());
        return SNGNN_OK;
    }
    float *invq = (float *)workspace;
    float *invb = (float *)((char *)workspace + (M + 63) / 64 * 256);
    unsigned long long *part = (unsigned long long *)((char *)invb + (N + 63) / 64 * 256);
    const bool areg = (uintptr_t)xq % 16 == 0 && (uintptr_t)xb % 16 == 0;
    const bool wide = areg && knn_wide(F, xb);
    const KnnQueryPlan p = knn_query_plan(M, N, wide ? 256 : KN_M, wide ? 64 : KN_M);
    k_knn_inv_norm<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(xq, M, F, invq);
    k_knn_inv_norm<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(xb, N, F, invb);
    dim3 grid((unsigned)p.nrb, (unsigned)p.ns);
    unsigned long long *pp = p.ns > 1 ? part : nullptr;
    const bool bf3 = !sngnn::fp32_mfma_only();          // sngnn_tuning_set(5, 1): fp32 MFMAs
    const KnnRows<true> rows = {xq, M, invq, self_offset};
#define SN_KNNQ_GO(FH_, BF3_, NWV_, CB_)                                                                           \
    k_knn_mfma<FH_, BF3_, NWV_, CB_, true><<<grid, 64 * NWV_, 0, st>>>(xb, N, F, invb, k, 0, p.tps, pp, nbr_idx,     \
                                                                       nbr_sim, rows)
    if (wide && F == 128) SN_KNNQ_GO(64, true, 8, 2);
    else if (wide && F == 96) SN_KNNQ_GO(48, true, 8, 2);
    else if (wide && F == 64) SN_KNNQ_GO(32, true, 8, 2);
    else if (wide) SN_KNNQ_GO(16, true, 8, 2);
    else if (areg && F == 128) { if (bf3) SN_KNNQ_GO(64, true, 4, 4); else SN_KNNQ_GO(64, false, 4, 4); }
    else if (areg && F == 96) { if (bf3) SN_KNNQ_GO(48, true, 4, 4); else SN_KNNQ_GO(48, false, 4, 4); }
    else if (areg && F == 64) { if (bf3) SN_KNNQ_GO(32, true, 4, 4); else SN_KNNQ_GO(32, false, 4, 4); }
    else if (areg && F == 32) { if (bf3) SN_KNNQ_GO(16, true, 4, 4); else SN_KNNQ_GO(16, false, 4, 4); }
    else SN_KNNQ_GO(0, false, 4, 4);
#undef SN_KNNQ_GO
    if (p.ns > 1) k_knn_merge<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(part, M, k, p.ns, nbr_idx, nbr_sim);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

#if defined(SNGNN_KNN_EXP) && SNGNN_KNN_EXP == 4
extern "C" int sngnn_knn_debug_counters(unsigned long long *out8, int reset)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (out8) SN_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(sngnn::g_knn_dbg), sizeof(z)));
    if (reset) SN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(sngnn::g_knn_dbg), z, sizeof(z)));
    return SNGNN_OK;
}
#endif

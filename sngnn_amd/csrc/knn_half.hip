// kNN similarity graph straight from an fp16 / bf16 table: sngnn_knn_graph_half and sngnn_knn_query_half.  The fused
// scan of knn_scan.h on the engine's half forms (cosine_tiles.h, PL = 2 / 1): the table is read as stored - no fp32
// copy - and only the products of the bf16 planes such a value has are issued (4 resp. 1 of the fp32 form's 8).  One
// shape, 256 rows x 64-column tiles, F in {32, 64, 96, 128}; the launch plans and the workspaces are the fp32
// entries'.  On finite tables the lists are the fp32 fused scan's on the widened table, bit for bit.
#include "knn_scan.h"

using namespace sngnn;

namespace {

template <typename S> struct Planes;
template <> struct Planes<__half> { static constexpr int PL = 2; };
template <> struct Planes<__hip_bfloat16> { static constexpr int PL = 1; };

// both tables' refusals that the fp32 entries do not have
bool half_dtype(int dtype) { return dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16; }
constexpr const char *NO_SCAN = "no native half scan here: F must be 32, 64, 96 or 128, knob 5 off (bf16 products) and knob 6 not 3";

template <typename S>
int graph_go(const unsigned short *x, int64_t N, int64_t F, int k, int exclude_self, int32_t *nbr_idx, float *nbr_sim,
             void *workspace, hipStream_t st)
{
    constexpr int PL = Planes<S>::PL;
    float *inv = (float *)workspace;
    unsigned long long *part = (unsigned long long *)((char *)workspace + (N + 63) / 64 * 256);
    const int ns = knn_splits(N, 256);
    const int64_t nrb = (N + 255) / 256, nct = (N + 63) / 64;
    const int tps = (int)((nct + ns - 1) / ns);          // column tiles per split
    const int ns_used = (int)((nct + tps - 1) / tps);
    k_knn_inv_norm_half<S><<<(unsigned)((N + 3) / 4), 256, 0, st>>>(x, N, F, inv);
    dim3 grid((unsigned)nrb, (unsigned)ns_used);
    unsigned long long *pp = ns_used > 1 ? part : nullptr;
#define SN_KNNH_GO(FH_) k_knn_mfma<FH_, true, 8, 2, false, PL><<<grid, 512, 0, st>>>(x, N, F, inv, k, exclude_self, tps, pp, nbr_idx, nbr_sim)
    if (F == 128) SN_KNNH_GO(64);
    else if (F == 96) SN_KNNH_GO(48);
    else if (F == 64) SN_KNNH_GO(32);
    else SN_KNNH_GO(16);
#undef SN_KNNH_GO
    if (ns_used > 1) k_knn_merge<<<(unsigned)((N + 3) / 4), 256, 0, st>>>(part, N, k, ns_used, nbr_idx, nbr_sim);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <typename S>
int query_go(const unsigned short *xq, int64_t M, const unsigned short *xb, int64_t N, int64_t F, int k, int64_t self_offset,
             int32_t *nbr_idx, float *nbr_sim, void *workspace, hipStream_t st)
{
    constexpr int PL = Planes<S>::PL;
    float *invq = (float *)workspace;
    float *invb = (float *)((char *)workspace + (M + 63) / 64 * 256);
    unsigned long long *part = (unsigned long long *)((char *)invb + (N + 63) / 64 * 256);
    const KnnQueryPlan p = knn_query_plan(M, N, 256, 64);
    k_knn_inv_norm_half<S><<<(unsigned)((M + 3) / 4), 256, 0, st>>>(xq, M, F, invq);
    k_knn_inv_norm_half<S><<<(unsigned)((N + 3) / 4), 256, 0, st>>>(xb, N, F, invb);
    dim3 grid((unsigned)p.nrb, (unsigned)p.ns);
    unsigned long long *pp = p.ns > 1 ? part : nullptr;
    const KnnRows<true> rows = {xq, M, invq, self_offset};
#define SN_KNNH_GO(FH_) k_knn_mfma<FH_, true, 8, 2, true, PL><<<grid, 512, 0, st>>>(xb, N, F, invb, k, 0, p.tps, pp, nbr_idx, nbr_sim, rows)
    if (F == 128) SN_KNNH_GO(64);
    else if (F == 96) SN_KNNH_GO(48);
    else if (F == 64) SN_KNNH_GO(32);
    else SN_KNNH_GO(16);
#undef SN_KNNH_GO
    if (p.ns > 1) k_knn_merge<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(part, M, k, p.ns, nbr_idx, nbr_sim);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

}  // namespace

extern "C" int sngnn_knn_graph_half(const void *x, int dtype, int64_t N, int64_t F, int k, int exclude_self,
                                    int32_t *nbr_idx, float *nbr_sim, void *workspace, void *stream)
{
    SN_REQUIRE(half_dtype(dtype), SNGNN_EINVAL, "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    SN_REQUIRE(N >= 0 && F >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(k >= 1 && k <= KNN_MAX_K, SNGNN_EINVAL, "k must be in [1, " + std::to_string(KNN_MAX_K) + "]");
    SN_REQUIRE(N < ((int64_t)1 << 31), SNGNN_EINVAL, "too many rows");
    SN_REQUIRE(sngnn_cosine_scan_half_supported(F, dtype), SNGNN_EINVAL, NO_SCAN);
    if (N == 0) return SNGNN_OK;
    SN_REQUIRE(x && nbr_idx && nbr_sim && workspace, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((uintptr_t)x % 16 == 0, SNGNN_EINVAL, "the table's base must be 16-byte aligned");
    const unsigned short *xs = static_cast<const unsigned short *>(x);
    if (dtype == SNGNN_DTYPE_F16) return graph_go<__half>(xs, N, F, k, exclude_self, nbr_idx, nbr_sim, workspace, (hipStream_t)stream);
    return graph_go<__hip_bfloat16>(xs, N, F, k, exclude_self, nbr_idx, nbr_sim, workspace, (hipStream_t)stream);
}

extern "C" int sngnn_knn_query_half(const void *xq, int64_t M, const void *xb, int dtype, int64_t N, int64_t F, int k,
                                    int64_t self_offset, int32_t *nbr_idx, float *nbr_sim, void *workspace, void *stream)
{
    SN_REQUIRE(half_dtype(dtype), SNGNN_EINVAL, "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    SN_REQUIRE(M >= 0 && N >= 0 && F >= 1, SNGNN_EINVAL, "bad shape");
    SN_REQUIRE(k >= 1 && k <= KNN_MAX_K, SNGNN_EINVAL, "k must be in [1, " + std::to_string(KNN_MAX_K) + "]");
    SN_REQUIRE(M < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), SNGNN_EINVAL, "too many rows");
    SN_REQUIRE(self_offset >= -1 && (self_offset < 0 || self_offset + M <= N), SNGNN_EINVAL,
               "self_offset: the queries are not rows [self_offset, self_offset + M) of the base");
    SN_REQUIRE(sngnn_cosine_scan_half_supported(F, dtype), SNGNN_EINVAL, NO_SCAN);
    if (M == 0) return SNGNN_OK;
    SN_REQUIRE(xq && nbr_idx && nbr_sim && workspace && (xb || N == 0), SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((uintptr_t)xq % 16 == 0 && (uintptr_t)xb % 16 == 0, SNGNN_EINVAL, "both tables' bases must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {                              // no base row: every slot is padding (a merge of no lists)
        k_knn_merge<<<(unsigned)((M + 3) / 4), 256, 0, st>>>(nullptr, M, k, 0, nbr_idx, nbr_sim);
        SN_HIP(hipGetLastError());
        return SNGNN_OK;
    }
    const unsigned short *qs = static_cast<const unsigned short *>(xq), *bs = static_cast<const unsigned short *>(xb);
    if (dtype == SNGNN_DTYPE_F16) return query_go<__half>(qs, M, bs, N, F, k, self_offset, nbr_idx, nbr_sim, workspace, st);
    return query_go<__hip_bfloat16>(qs, M, bs, N, F, k, self_offset, nbr_idx, nbr_sim, workspace, st);
}

// Launchers of the fused aggregation forward (gfx950) - the umbrella the per-layout translation units include
// (agg_fwd*_v*.hip, agg_fwd_v4e.hip: SNGNN_AGG_FWD_TU).  The kernels live one header per role:
//   agg_fwd_args.h    FwdArgs and its store epilogue; what the forward computes (the opening comment)
//   agg_fwd_head.h    the classification head's role
//   agg_fwd_select.h  scoring and top-k primitives
//   agg_fwd_src.h     how the work-item roles read what they gather: flat pointers, or buffer resources
//   agg_fwd_fin.h     the five forms of the split rows' finalize
//   agg_fwd_roles.h   the unit-row and filter passes, the three work-item roles, k_agg_fwd
// and every launch decision in fwd_plan.h (plain C++): the launchers below fill its input from FwdArgs, call it
// once, pick the template instantiations it names and launch.
#pragma once
#include "agg_fwd_roles.h"

namespace sngnn {

template <int VEC, int G, int R>
int launch_normalize_rows(const float *h, int64_t rows, int C, float *n, float *nrm, void *filt, hipStream_t st)
{
    constexpr int RPW = 64 / G;
    constexpr int U = Unroll<R>::U >= 2 ? 2 : 1;
    if (rows <= 0) return SNGNN_OK;
    // a streaming pass: short work items (one step per wave up to 8 resident workgroups per CU,
    // grid-stride beyond), so the launch drains evenly
    const int64_t steps = (rows + RPW * U - 1) / (RPW * U);
    const int grid = (int)std::min<int64_t>(ceil_div(steps, WAVES), CHIP_CUS * 8 * 4);
    if (filt && !(VEC == 4 && filter_row_bytes(C) == 8 * G * R)) {
        set_error("internal: filter rows need 16-byte row vectors");
        return SNGNN_EINVAL;
    }
    k_normalize_rows<VEC, G, R><<<grid, BLOCK, 0, st>>>(h, rows, C, n, nrm, (uint2 *)filt);
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

template <int VEC, int G, int R>
int launch_filter_rows(const float *n, int64_t rows, int C, void *filt, hipStream_t st)
{
    if constexpr (VEC == 4) {
        if (rows <= 0) return SNGNN_OK;
        if (filter_row_bytes(C) != 8 * G * R) { set_error("internal: filter row layout"); return SNGNN_EINVAL; }
        const int grid = (int)std::min<int64_t>(ceil_div(rows, (64 / G) * WAVES), CHIP_CUS * 8 * 4);
        k_filter_rows<G, R><<<grid, BLOCK, 0, st>>>(n, rows, C, (uint2 *)filt);
        SN_HIP(hipGetLastError());
        return SNGNN_OK;
    } else {
        set_error("internal: filter rows need 16-byte row vectors");
        return SNGNN_EINVAL;
    }
}

// what the launch decisions read of a call (fwd_plan.h)
template <int G, typename S>
FwdPlanIn fwd_plan_input(const FwdArgs &a, int max_split_deg)
{
    FwdPlanIn in;
    in.N = a.N; in.n_med_end = a.n_med_end; in.n_split = a.n_split; in.n_split_gt_wave = a.n_split_gt_wave;
    in.n_tasks = a.n_tasks; in.n_edges = a.n_edges; in.C = a.C; in.G = G; in.k = a.k;
    in.use_cand = a.use_cand != 0; in.head = a.head_sel != nullptr; in.half_rows = !std::is_same<S, float>::value;
    in.has_fin_done = a.fin_done != nullptr; in.role_mask = a.role_mask; in.max_split_deg = max_split_deg;
    in.fin_inline = g_fin_inline;
    return in;
}

// the head role as a launch of its own (finalize shapes that do not carry it; graphs without split rows)
template <int VEC, int G, int R>
int launch_head_rows(const FwdArgs &a, hipStream_t st)
{
    if (a.head_sel && a.head_nmain > 0) k_agg_head_rows<VEC, G, R><<<a.head_nmain, BLOCK, 0, st>>>(a);
    return SNGNN_OK;
}

// the candidate finalize's launches at NW waves per workgroup
template <int VEC, int G, int R, int NW, bool HEAD, typename S = float>
int launch_cand_finalize(const FwdArgs &a, const FwdPlan &p, hipStream_t st)
{
    if (!p.finc_fits) { set_error("internal: candidate finalize does not fit LDS"); return SNGNN_EINVAL; }
    if (p.finc_dyn > 48 * 1024)
        SN_HIP(hipFuncSetAttribute((const void *)k_agg_fin_cand<VEC, G, R, NW, HEAD, S>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.finc_dyn));
    if (p.fin.mixed) {
        // few moderate rows: one mixed launch
        if (p.finc_dyn_mixed > 48 * 1024)
            SN_HIP(hipFuncSetAttribute((const void *)k_agg_fin_mixed<VEC, G, R, NW, HEAD, S>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.finc_dyn_mixed));
        k_agg_fin_mixed<VEC, G, R, NW, HEAD, S><<<p.mixed_fin_blocks + (HEAD ? p.mixed_head_blocks : 0), NW * 64,
                                                  p.finc_dyn_mixed, st>>>(a, p.max_slots, p.fin.n_big_true, a.n_split,
                                                                          p.mixed_fin_blocks);
    } else {
        if constexpr (HEAD) launch_head_rows<VEC, G, R>(a, st);
        if (p.cand_blocks > 0) k_agg_fin_cand<VEC, G, R, NW, HEAD, S><<<p.cand_blocks, NW * 64, p.finc_dyn, st>>>(a, p.max_slots);
        if (p.wave_blocks > 0)
            k_agg_fin_wave<VEC, G, R, HEAD, S><<<p.wave_blocks, BLOCK, 0, st>>>(a, p.cand_blocks, a.n_split - p.cand_blocks);
    }
    return SNGNN_OK;
}

// launches of the split rows' finalize (after their tasks, same stream)
template <int VEC, int G, int R, typename S = float>
int launch_split_finalize(const FwdArgs &a, const FwdPlan &p, hipStream_t st)
{
    constexpr bool F32 = std::is_same<S, float>::value;         // (half rows: no head - the host refuses it)
    if (a.n_split > 0 && a.use_cand) {
        // streaming rows and candidate tournament
        if constexpr (F32 && VEC == 4 && R == 1 && (G == 8 || G == 16)) {
            if (p.finc_head) return launch_cand_finalize<VEC, G, R, 8, true>(a, p, st);
        }
        if (p.finc_waves == 16) return launch_cand_finalize<VEC, G, R, 16, false, S>(a, p, st);
        return launch_cand_finalize<VEC, G, R, 8, false, S>(a, p, st);
    } else if (a.n_split > 0) {
        if (p.topk_too_large) { set_error("top_k too large for the split-row finalize"); return SNGNN_EINVAL; }
        if (p.fin_dyn > 48 * 1024)
            SN_HIP(hipFuncSetAttribute((const void *)k_agg_fin<VEC, G, R, S>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.fin_dyn));
        k_agg_fin<VEC, G, R, S><<<a.n_split, FIN_BLOCK, p.fin_dyn, st>>>(a, p.lds_scores);      // (no head there: the host refuses)
    } else {
        if constexpr (F32) launch_head_rows<VEC, G, R>(a, st);
    }
    return SNGNN_OK;
}

template <int VEC, int G, int R, int EPI, typename S = float, bool BUF = false>
int launch_agg_fwd_impl(const FwdArgs &a0, int max_split_deg, hipEvent_t *ev, hipStream_t st)
{
    static_assert(!BUF || std::is_same<S, float>::value, "buffer-addressed reads: fp32 tables");
    constexpr bool F32 = std::is_same<S, float>::value;        // (half rows: on the fly only, launcher's check)
    const int reps = ev ? std::max(g_prof_reps, 1) : 1;
    const FwdPlan p = fwd_plan(fwd_plan_input<G, S>(a0, max_split_deg));
    FwdArgs a = a0;
    const bool fin_inline = p.fin_blocks > 0;
    const int grid = p.main_blocks + p.fin_blocks;
    a.main_blocks = p.main_blocks;
    g_last_fin_blocks = p.fin_blocks;
    if (fin_inline) a.fin_nonce = next_fin_nonce();
    a.head_nmain = p.head_nmain;
    // the lean kernel (agg_fwd_roles.h: k_agg_fwd, LEAN): a call that wants `out` and nothing else, where the plain
    // table-mode kernel would run (fp32 rows, no store epilogue; SNGNN_FWD_PLAIN below); sngnn_tuning_set(12, 1): never
    [[maybe_unused]] const bool lean = F32 && EPI == 0 && g_fwd_general_only == 0 && a.wsel == nullptr && a.inv_norm == nullptr &&
                      a.sel_src == nullptr && a.sel_w == nullptr && a.kbits == nullptr && a.head_sel == nullptr &&
                      a.row_flag == nullptr && a.epi_flags == 0;
    if (ev) SN_HIP(hipEventRecord(ev[0], st));
#define SNGNN_FWD_LAUNCH_L(FILTV, OTFV, FSV, LEANV)                                                            \
    do {                                                                                                       \
        if (fin_inline) k_agg_fwd<VEC, G, R, FILTV, OTFV, EPI, FSV, true, S, BUF, LEANV><<<grid, BLOCK, 0, st>>>(a); \
        else k_agg_fwd<VEC, G, R, FILTV, OTFV, EPI, FSV, false, S, BUF, LEANV><<<grid, BLOCK, 0, st>>>(a);           \
    } while (0)
#define SNGNN_FWD_LAUNCH(FILTV, OTFV, FSV) SNGNN_FWD_LAUNCH_L(FILTV, OTFV, FSV, false)
#define SNGNN_FWD_PLAIN()                                                                                      \
    do {                                                                                                       \
        if constexpr (F32 && EPI == 0) {                                                                       \
            if (lean) { SNGNN_FWD_LAUNCH_L(false, false, false, true); break; }                                \
        }                                                                                                      \
        SNGNN_FWD_LAUNCH(false, false, false);                                                                 \
    } while (0)
    for (int rep = 0; rep < reps && grid > 0; ++rep) {
        if (!F32 || a.nrm == nullptr) {                          // OTF: a.n holds the raw rows
            SNGNN_FWD_LAUNCH(false, true, false);
        } else if constexpr (F32 && VEC == 4 && G >= 16 && G * R <= 128) {     // the (G, R) that C in 36 .. 512 maps to
            if (a.filt && a.k >= 0 && a.filt_small) SNGNN_FWD_LAUNCH(true, false, true);
            else if (a.filt && a.k >= 0) SNGNN_FWD_LAUNCH(true, false, false);
            else SNGNN_FWD_PLAIN();
        } else if constexpr (F32) {
            SNGNN_FWD_PLAIN();
        }
    }
#undef SNGNN_FWD_PLAIN
#undef SNGNN_FWD_LAUNCH
#undef SNGNN_FWD_LAUNCH_L
    if (ev) SN_HIP(hipEventRecord(ev[1], st));
    for (int rep = 0; rep < reps && !fin_inline; ++rep)
        if (int rc = launch_split_finalize<VEC, G, R, S>(a, p, st)) return rc;
    if (ev) {
        SN_HIP(hipEventRecord(ev[2], st));
        SN_HIP(hipEventRecord(ev[3], st));       // empty interval: the cost of an event pair
    }
    SN_HIP(hipGetLastError());
    if (a.head_sel)
        return launch_head_reduce(a.head_part, a.head_nmain + a.n_split, a.head_scale, a.head_scale_b,
                                  (a.head_flags & 1) ? 2 : 1, 4, a.head_out, st);
    return SNGNN_OK;
}

// S = float, or the half path (sngnn_agg_forward_half): rows h stored as S = __half / __hip_bfloat16, scored on the fly,
// out stored as S.  The kernels are the fp32 ones with their row loads and output stores in S (device_utils.h: Row),
// so every register holds what it holds in the fp32 forward of h.float(): same lanes, same order, same bits.
template <int VEC, int G, int R, typename S = float>
int launch_agg_fwd(const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st)
{
    return launch_agg_fwd_impl<VEC, G, R, 0, S>(a, max_split_deg, ev, st);
}
template <int VEC, int G, int R>
int launch_agg_fwd_epi(const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st)
{
    return launch_agg_fwd_impl<VEC, G, R, 1>(a, max_split_deg, ev, st);
}
// the same two with the work-item roles in their buffer form (fp32 tables; fwd_plan.h: fwd_buffer_form)
template <int VEC, int G, int R>
int launch_agg_fwd_buf(const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st)
{
    return launch_agg_fwd_impl<VEC, G, R, 0, float, true>(a, max_split_deg, ev, st);
}
template <int VEC, int G, int R>
int launch_agg_fwd_epi_buf(const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st)
{
    return launch_agg_fwd_impl<VEC, G, R, 1, float, true>(a, max_split_deg, ev, st);
}

}  // namespace sngnn

#define SNGNN_AGG_FWD_TU(S, VEC)                                                                                       \
    template <>                                                                                                        \
    int sngnn::launch_agg_fwd_vec<S, VEC>(const RowCfg &cfg, const FwdArgs &a, int max_split_deg, hipEvent_t *ev,      \
                                          hipStream_t st)                                                              \
    {                                                                                                                  \
        SNGNN_DISPATCH_GRS(launch_agg_fwd, VEC, S, cfg, a, max_split_deg, ev, st)                                      \
    }
// the buffer form of the fp32 forward at VEC values per lane
#define SNGNN_AGG_FWD_BUF_TU(VEC)                                                                                      \
    template <>                                                                                                        \
    int sngnn::launch_agg_fwd_buf_vec<VEC>(const RowCfg &cfg, const FwdArgs &a, int max_split_deg, hipEvent_t *ev,     \
                                           hipStream_t st)                                                             \
    {                                                                                                                  \
        SNGNN_DISPATCH_GR(launch_agg_fwd_buf, VEC, cfg, a, max_split_deg, ev, st)                                      \
    }


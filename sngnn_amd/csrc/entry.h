// What the C-ABI entry points of the graph kernels share on the HOST: the row-class view of a graph side, the graph
// part of BwdArgs, the row checks, and the dispatch from (vector width, storage type) to a launcher.  No kernel here.
#pragma once
#include <initializer_list>
#include <type_traits>
#include <utility>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "common.h"

namespace sngnn {

// ---- row-class view of one side of a graph ---------------------------------------------------------------------------
template <class A, class = void> struct has_segments : std::false_type {};
template <class A>
struct has_segments<A, std::void_t<decltype(std::declval<A &>().ptr), decltype(std::declval<A &>().idx),
                                   decltype(std::declval<A &>().perm)>> : std::true_type {};

// Binds the structure a kernel walks: the in-edges (CSR by target; split / wave / small rows by in-degree) or, with
// `csc`, the out-edges (CSC by source, for A^T and the scatter passes).  Fills the row classes and their split tasks,
// and the segments themselves (ptr / idx / perm) where the args struct has them.
template <class A> void bind_side(const sngnn_graph_t *g, bool csc, A &a)
{
    if (!csc) {
        a.n_split = g->n_split; a.n_med_end = g->rows_gt(SMALL_T); a.n_tasks = g->n_tasks;
        a.task_slot = g->task_slot; a.task_chunk = g->task_chunk; a.split_task0 = g->split_task0;
    } else {
        a.n_split = g->n_ssplit; a.n_med_end = g->srcs_gt(SMALL_T); a.n_tasks = g->n_stasks;
        a.task_slot = g->stask_slot; a.task_chunk = g->stask_chunk; a.split_task0 = g->ssplit_task0;
    }
    if constexpr (has_segments<A>::value) {
        a.ptr = csc ? g->cscptr : g->rowptr;
        a.idx = csc ? g->csc_dst : g->col;
        a.perm = csc ? g->sperm : g->rperm;
    }
}

// bind_side for the edge-softmax families (gat.hip, wrgat.hip): their passes also need N and, to write an in-edge's record
// where the out-edge pass reads it, the CSR -> CSC positions
template <class A> void bind_softmax_side(const sngnn_graph_t *g, bool csc, A &a)
{
    a.N = (int)g->N;
    a.csc_pos = g->csc_pos;
    bind_side(g, csc, a);
}

// The graph part of BwdArgs (agg_bwd_impl.h; B = BwdArgs): both sides of the graph and the scratch regions of L
// inside the workspace.  What depends on the mode stays with the caller, set explicitly: the rows (h, gout, wsel,
// grad_h), wd / kmask / kmask_words / inv_deg / rec_dot, mode / top_k / role_mask / s_small_end, the fused-node
// lists (fdesc, trest, n_fused, n_trest) and the kept bits (kbits, csc_bit, kb_wbase, kb_tbase).
template <class B> void bind_bwd_graph(const sngnn_graph_t *g, int C, const BwdLayout &L, void *workspace, B &a)
{
    a.C = C; a.N = (int)g->N; a.Ntot = (int)g->Ntot; a.row_off = (int)g->row_off; a.Ep = g->Ep;
    a.rowptr = g->rowptr; a.col = g->col; a.rperm = g->rperm; a.rdesc = g->rdesc; a.sdesc = g->sdesc;
    a.cscptr = g->cscptr; a.csc_eid = g->csc_eid; a.csc_dst = g->csc_dst; a.csc_pos = g->csc_pos;
    a.sperm = g->sperm;
    a.dnT = (float *)((char *)workspace + L.dnT);
    a.partT = (float *)((char *)workspace + L.partT);
    a.partS = (float *)((char *)workspace + L.partS);
    bind_side(g, false, a);
    a.n_ssplit = g->n_ssplit; a.n_smed_end = g->srcs_gt(SMALL_T); a.n_stasks = g->n_stasks;
    a.stask_slot = g->stask_slot; a.stask_chunk = g->stask_chunk; a.ssplit_task0 = g->ssplit_task0;
    a.nbA = a.nbB = a.nbC = 0;
}

// the layouts of ws_layout.h for a graph
inline FwdLayout fwd_layout(const sngnn_graph_t *g, int C) { return fwd_layout(g->Ntot, g->split_edges, g->n_tasks, C); }
inline BwdLayout bwd_layout(const sngnn_graph_t *g, int C, bool attention)
{
    return bwd_layout(g->Ep, g->N, g->n_tasks, g->n_stasks, C, attention);
}

// ---- checks -----------------------------------------------------------------------------------------------------------
// gcn_norm's / GATConv's edge list: an unpartitioned graph whose self loops were replaced
inline bool whole_graph_with_loops(const sngnn_graph_t *g)
{
    return g->add_loops == 1 && g->remove_loops == SNGNN_LOOPS_REPLACE && g->N == g->Ntot && g->row_off == 0;
}

inline bool rows_aligned(uintptr_t bytes, std::initializer_list<const void *> rows)
{
    uintptr_t bits = 0;
    for (const void *p : rows) bits |= (uintptr_t)p;
    return bits % bytes == 0;
}

// Row configuration for C channels, and the alignment of feature tables to the row vector width: vec values of the
// storage type (dtype: 0 = fp32, SNGNN_DTYPE_F16 / SNGNN_DTYPE_BF16 = 2 bytes a value).  NULL passes.
inline int check_rows(int C, int dtype, std::initializer_list<const void *> rows, RowCfg &cfg)
{
    SN_REQUIRE(row_cfg(C, cfg), SNGNN_EINVAL, "C must be in [1, " + std::to_string(SNGNN_MAX_CHANNELS) + "]");
    SN_REQUIRE(rows_aligned((uintptr_t)cfg.vec * (dtype != 0 ? 2 : 4), rows), SNGNN_EINVAL,
               "rows must be aligned to the row vector width");
    return SNGNN_OK;
}

// a column slice: W columns at p of N rows ld floats apart; p == nullptr or W == 0: none
struct Slice { const float *p; int64_t N, ld, w; };

// whether two slices share an element.  Disjoint address intervals do not; neither do two column ranges of one
// row-strided table (equal strides, the second's first column d = (pb - pa) mod ld behind the first's last and its
// last in front of the stride's end) - MixHop's launches write slices of the table they also copy into.  Anything
// else whose intervals meet counts as sharing.
inline bool overlap(const Slice &a, const Slice &b)
{
    if (!a.p || !b.p || a.w <= 0 || b.w <= 0 || a.N <= 0) return false;
    const uintptr_t alo = (uintptr_t)a.p, ahi = alo + (uintptr_t)(((a.N - 1) * a.ld + a.w) * 4);
    const uintptr_t blo = (uintptr_t)b.p, bhi = blo + (uintptr_t)(((b.N - 1) * b.ld + b.w) * 4);
    if (ahi <= blo || bhi <= alo) return false;
    if (a.ld != b.ld) return true;
    const int64_t diff = ((int64_t)blo - (int64_t)alo) / 4;
    const int64_t d = ((diff % a.ld) + a.ld) % a.ld;
    return !(d >= a.w && d + b.w <= a.ld);
}

// ---- dispatch ---------------------------------------------------------------------------------------------------------
template <typename S> struct Storage { using type = S; };

// f(std::integral_constant<int, VEC>) for the row configuration's vector width
template <typename F> int dispatch_vec(const RowCfg &cfg, F &&f)
{
    switch (cfg.vec) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 4>{});
    }
}

// static int NAME(cfg, a, st): return FN<VEC, G, R>(a, st) for the row configuration (FN takes the ARGS by value)
#define SNGNN_DEFINE_DISPATCH(NAME, FN, ARGS)                                                                          \
    static int NAME(const RowCfg &cfg, const ARGS &a, hipStream_t st)                                                  \
    {                                                                                                                  \
        return dispatch_vec(cfg, [&](auto vec) { SNGNN_DISPATCH_GR(FN, decltype(vec)::value, cfg, a, st) });          \
    }

// f(VEC, G, R as integral constants) for a hop on a column slice: the lane layouts are row_cfg(W)'s, and - where the
// slice's alignment forces a narrower vector than W's own - the same groups with 2 or 4 times the steps
template <typename F> int dispatch_slice_layout(int vec, int g, int r, F &&f)
{
    using std::integral_constant;
    return dispatch_vec(RowCfg{vec, g, r}, [&](auto v) {
        constexpr int VEC = decltype(v)::value;
#define SN_GR_CASE(G_, R_) case G_ * 100 + R_: return f(v, integral_constant<int, G_>{}, integral_constant<int, R_>{});
        switch (g * 100 + r) {
            SN_GR_CASE(8, 1) SN_GR_CASE(16, 1) SN_GR_CASE(32, 1) SN_GR_CASE(64, 1) SN_GR_CASE(64, 2) SN_GR_CASE(64, 4)
            SN_GR_CASE(64, 8)
        default: break;
        }
        if constexpr (VEC < 4) {
            switch (g * 100 + r) {
                SN_GR_CASE(8, 2) SN_GR_CASE(16, 2) SN_GR_CASE(32, 2)
            default: break;
            }
        }
        if constexpr (VEC == 1) {
            switch (g * 100 + r) {
                SN_GR_CASE(8, 4) SN_GR_CASE(16, 4) SN_GR_CASE(32, 4)
            default: break;
            }
        }
#undef SN_GR_CASE
        set_error("unsupported channel layout");
        return (int)SNGNN_EINVAL;
    });
}

// f(Storage<S>, std::integral_constant<int, VEC>): the runtime pair (cfg.vec, dtype) as a compile-time pair.  The
// launchers `template <typename S, int VEC> int launch_..._vec(const RowCfg &, ...)` of the *_impl.h headers are
// defined one per translation unit (family x storage type x vector width); SNGNN_LAUNCH_VEC names one by family.
template <typename F> int dispatch_vec_dtype(const RowCfg &cfg, int dtype, F &&f)
{
    return dispatch_vec(cfg, [&](auto vec) {
        if (dtype == SNGNN_DTYPE_F16) return f(Storage<__half>{}, vec);
        if (dtype != 0) return f(Storage<__hip_bfloat16>{}, vec);
        return f(Storage<float>{}, vec);
    });
}
#define SNGNN_LAUNCH_VEC(FN, cfg, dtype, ...)                                                                           \
    sngnn::dispatch_vec_dtype(cfg, dtype, [&](auto s, auto vec) { return FN<typename decltype(s)::type, decltype(vec)::value>(cfg, __VA_ARGS__); })

}  // namespace sngnn

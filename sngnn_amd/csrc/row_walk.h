// The row-class walk (gfx950, wave = 64), in one place:
//   split segments (deg > WAVE_T)   CHUNK-edge tasks, one wave each, the lane groups striding the task's edges; the
//                                   tasks' partial rows are merged by the family's finalize kernel
//   wave segments  (deg > SMALL_T)  one wave each, the lane groups striding the edges
//   small segments                  one G-lane group each
// Two ways onto it.  The gather-sum hop kernels - k_adj, k_prop, k_gcn_hop, k_gcn2_hop, k_h2gcn_hop and k_acm - are
// walk_rows with a family's gather, partial store and epilogue (k_glo_hop shares the gather, the finalize sum and the
// launch plan, and spells the walk out: see glognn.hip).  The edge-softmax kernels of gat.hip and wrgat.hip pass over a
// unit twice and reduce across lanes in between: they call the decode row_unit and keep their own bodies.
// Contract ("The row-class walker"): every sum's order is fixed by G, CHUNK and the graph alone; no atomics.
#pragma once
#include "device_utils.h"

namespace sngnn {

// One side of a graph as a kernel walks it (bind_side, entry.h): the segments (CSR by target or CSC by source), the
// gathered ids, the degree order, the row classes with the split segments' tasks, and the launch's workgroup counts
// (plan_side).  The args struct of every kernel on walk_rows or row_unit derives from it.
struct RowSide {
    const int32_t *ptr, *idx, *perm;
    int n_split, n_med_end, n_tasks;
    const int32_t *task_slot, *task_chunk, *split_task0;
    int nbA, nbB;               // workgroups of split tasks and of wave segments, in front of the small segments'
};

// Which segment (or task) of a side with N segments a wave / lane group of workgroup b serves, for kernels that keep their
// own body.  G is the lane-group width of the SMALL segments only (a scalar pass calls it with the width it gives such a
// segment, whatever its rows' layout); gid = lane / G.
//   wide   wave-uniform: a task or a wave segment - all 64 lanes share [e0, e1); otherwise a small segment a group
//   task   the unit is task tq, the entries [e0, e1) of its segment; otherwise the whole segment, e0 = 0
//   qs     where the segment's entries start in idx: entry t is idx[qs + t]
// A dead unit (a wave past the tasks or wave segments, a group past the last segment) comes back as live = false, seg = 0,
// qs = ptr[0], e0 = e1 = 0: every lane then runs the caller's loops - over an empty range - and its shuffles, so a cross-
// lane reduction is never taken under divergence; `live` guards the stores alone.
struct RowUnit {
    bool live, task;
    int seg, tq, qs, e0, e1;
};

template <int G> __device__ __forceinline__ RowUnit row_unit(const RowSide &s, int N, int b, int wave, int gid, bool &wide)
{
    constexpr int NG = 64 / G;
    RowUnit u;
    u.tq = 0;
    wide = b < s.nbA + s.nbB;
    if (wide) {
        u.task = b < s.nbA;
        u.tq = b * WAVES + wave;
        const int slot = s.n_split + (b - s.nbA) * WAVES + wave;
        u.live = u.task ? u.tq < s.n_tasks : slot < s.n_med_end;               // (wave-uniform)
        u.seg = u.live ? s.perm[u.task ? s.task_slot[u.tq] : slot] : 0;
        u.e0 = u.live && u.task ? s.task_chunk[u.tq] * CHUNK : 0;
    } else {
        u.task = false;
        const int slot = s.n_med_end + ((b - s.nbA - s.nbB) * WAVES + wave) * NG + gid;
        u.live = slot < N;
        u.seg = u.live ? s.perm[slot] : 0;
        u.e0 = 0;
    }
    u.qs = s.ptr[u.seg];
    const int deg = u.live ? s.ptr[u.seg + 1] - u.qs : 0;
    u.e1 = u.task ? min(deg, u.e0 + CHUNK) : deg;
    return u;
}

// Workgroup b of a side with N segments, for a gather-sum.  It keeps its own decode, in which a lane without work calls
// nothing: written over row_unit it cost k_acm<4, 16, 1>, k_acm<4, 32, 1> and k_adj<2, 64, 8> a wave of occupancy
// (profiles/row_walk_resources.txt).  acc: the per-row state, any type with zero() and reduce_across_groups() (a
// Row, or ACM's pair of them).
//   gather(seg, qs, e0, e1, stride, first, lg, acc)   acc += the entries e0 + first, + stride, ... < e1 of segment seg,
//                                                     whose entries start at qs
//   store_task(tq, lg, acc)                           task tq's partial row
//   finish(seg, deg, lg, acc)                         the epilogue of segment seg (deg entries)
// Tasks and wave segments: all 64 lanes gather, the groups' sums are added across the wave, and the G lanes of group 0
// call store_task or finish.  Small segments: the G lanes of every group that has one call finish.  Lanes without work
// return from the walk having called nothing.
template <int G, class Acc, class Gather, class StoreTask, class Finish>
__device__ __forceinline__ void walk_rows(const RowSide &s, int b, int N, Acc &acc, Gather &&gather,
                                          StoreTask &&store_task, Finish &&finish)
{
    constexpr int NG = 64 / G;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int gid = lane / G, lg = lane % G;
    acc.zero();
    if (b < s.nbA + s.nbB) {
        // split task or one wave per segment
        const bool task = b < s.nbA;
        const int tq = b * WAVES + wave;
        const int slot = s.n_split + (b - s.nbA) * WAVES + wave;
        const bool live = task ? tq < s.n_tasks : slot < s.n_med_end;          // (wave-uniform)
        if (live) {
            const int seg = s.perm[task ? s.task_slot[tq] : slot];
            const int e0 = task ? s.task_chunk[tq] * CHUNK : 0;
            const int qs = s.ptr[seg];
            const int deg = s.ptr[seg + 1] - qs;
            const int e1 = task ? min(deg, e0 + CHUNK) : deg;
            gather(seg, qs, e0, e1, NG, gid, lg, acc);
            acc.reduce_across_groups();
            if (gid == 0) {
                if (task) store_task(tq, lg, acc);
                else finish(seg, deg, lg, acc);
            }
        }
    } else {
        const int slot = s.n_med_end + ((b - s.nbA - s.nbB) * WAVES + wave) * NG + gid;
        if (slot < N) {
            const int seg = s.perm[slot];
            const int qs = s.ptr[seg];
            const int deg = s.ptr[seg + 1] - qs;
            gather(seg, qs, 0, deg, 1, 0, lg, acc);
            finish(seg, deg, lg, acc);
        }
    }
}

// ---- the gather loop --------------------------------------------------------------------------------------------------
// the weight of a gathered row, a functor of (row, position qs + t in idx): none, dinv[row], or a per-entry value
struct NoWeight {
    __device__ __forceinline__ constexpr bool on() const { return false; }
    __device__ __forceinline__ float operator()(int, int) const { return 1.0f; }
};
struct RowWeight {               // dinv[row]
    const float *dinv;
    __device__ __forceinline__ constexpr bool on() const { return true; }
    __device__ __forceinline__ float operator()(int row, int) const { return dinv[row]; }
};
struct EntryWeight {             // w[t] for the entry at position t, or nullptr: none (a uniform test at run time)
    const float *w;
    __device__ __forceinline__ bool on() const { return w != nullptr; }
    __device__ __forceinline__ float operator()(int, int t) const { return w ? w[t] : 1.0f; }
};

// rows in flight per lane group: four registers' worth of steps
constexpr int gather_unroll(int R) { return 4 / (R >= 4 ? 4 : R); }

// acc += weight * table[idx[qs + t] + idx_shift, 0 .. W) over the entries t = e0 + first, + stride, ... < e1 of the
// segment at qs (table rows ld floats apart), U rows in flight.  The product is rounded, then added
// (-ffp-contract=off; a sparse mm's order).  A slot past e1 loads row 0 and drops it.
template <int VEC, int G, int R, int U, class Weight>
__device__ __forceinline__ void gather_rows(const float *table, int64_t ld, int W, const int32_t *idx, int qs, int e0,
                                            int e1, int stride, int first, int lg, Row<VEC, G, R> &acc, Weight weight,
                                            int idx_shift = 0)
{
    for (int base = e0 + first; base < e1; base += stride * U) {
        Row<VEC, G, R> x[U];
        float w[U];
        bool act[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = base + u * stride;
            act[u] = t < e1;
            const int row = act[u] ? idx[qs + t] + idx_shift : 0;
            w[u] = weight(row, qs + (act[u] ? t : base));
            x[u].load(table + (size_t)row * ld, W, lg);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (act[u]) {
                if (weight.on()) x[u].scale(w[u]);
                acc.add(x[u]);
            }
    }
}

// ---- the split segments' finalize -------------------------------------------------------------------------------------
// Thread (q, column c) of a 4 x 64 workgroup: the sum of column c of the partial rows t0 + q, + 4, ... < t1 (W floats
// apart) in four independent chains (the loads of a hub's ~100 tasks overlap), added pairwise; 0 for c >= W.
__device__ __forceinline__ float sum_task_partials(const float *__restrict__ partial, int W, int t0, int t1, int c, int q)
{
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (c < W) {
        int t = t0 + q;
        for (; t + 12 < t1; t += 16) {
            v0 += partial[(size_t)t * W + c];
            v1 += partial[(size_t)(t + 4) * W + c];
            v2 += partial[(size_t)(t + 8) * W + c];
            v3 += partial[(size_t)(t + 12) * W + c];
        }
        for (; t < t1; t += 4) v0 += partial[(size_t)t * W + c];
    }
    return (v0 + v1) + (v2 + v3);
}

// The four threads' sums of column lane cl, added pairwise in q order; every thread gets it.  All 256 threads call it
// (one barrier); a second call needs a barrier of the caller's in between.
__device__ __forceinline__ float combine_task_sums(float (&s)[4][64], float v, int q, int cl)
{
    s[q][cl] = v;
    __syncthreads();
    return (s[0][cl] + s[1][cl]) + (s[2][cl] + s[3][cl]);
}

// ---- host -------------------------------------------------------------------------------------------------------------
// Sets the side's workgroup counts and returns the main kernel's grid for N segments at NG = 64 / G lane groups a wave.
inline int plan_side(RowSide &s, int N, int NG)
{
    s.nbA = ceil_div(s.n_tasks, WAVES);
    s.nbB = ceil_div(s.n_med_end - s.n_split, WAVES);
    return s.nbA + s.nbB + ceil_div(N - s.n_med_end, (int64_t)WAVES * NG);
}

// bytes of the tasks' partial rows of W floats, for whichever side of g a launch walks
inline int64_t task_partial_bytes(const sngnn_graph_t *g, int64_t W)
{
    return up256((int64_t)std::max(g->n_tasks, g->n_stasks) * W * 4);
}

}  // namespace sngnn

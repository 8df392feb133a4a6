// Fused forward of the similarity-navigated aggregation (gfx950).
//
// A normalisation pass and the gather kernels compute, for every target row i of the
// CSR-by-target graph,
//     n_j   = h_j / nrm_j,  nrm_j = max(|h_j|_2, eps)      (F.normalize; k_normalize_rows)
//     s_e   = <n_i, n_j>                               per in-edge e = (j -> i)
//     keep  = top_k by (s desc, edge position asc) AND s >= thr    (or all, top_k < 0)
//     out_i = (1 / max(deg_i, 1)) * sum_{e kept} s_e * h_j
// i.e. models/models.py:122+132+139-158, :238-239+244-263, :325-326+331-334 of the
// reference without materialising any per-edge [E', C] tensor.
//
// Normalise-then-dot, in the reference's order (F.normalize first, then
// (norm_i * norm_j).sum(-1)), with IEEE square root and division per ROW: whenever two
// source rows normalise to the same bits in the reference (duplicates, power-of-two
// multiples, rows with one non-zero channel: exactly +-1 there) they do here, their
// cosines are the same bits, and the tie falls to the edge position, as in the reference.
// The gather reads the unit row n_j (4C bytes) and, for a kept edge, its 4-byte norm
// (h_j = n_j * nrm_j to half an ulp).  Measured alternatives: dividing each
// gathered h_j by its norm inside the gather (no unit-row table) costs the kernel 17 us of
// vector arithmetic; it is at its balance point between the vector pipes and the line rate
// of the memory system.
//
// Rows are processed in order of descending in-degree (graph.rperm) in three
// classes, all work items of one persistent launch:
//   A  split rows  (deg > WAVE_T): one wave per CHUNK-edge task scores its edges
//      (edge-balanced) and keeps its chunk-local top-k as candidates; a finalize launch
//      merges the candidates per row and gathers the winners;
//   B  wave rows   (SMALL_T < deg <= WAVE_T): one wave per row, its 64/G lane
//      groups stride over the row's edges;
//   C  small rows  (deg <= SMALL_T): one G-lane group per row, 64/G rows per wave.
// A row whose degree is <= top_k needs no ranking (only the threshold), so its
// weighted sum is accumulated in the same pass that scores it ("streaming");
// otherwise scores go to LDS (or HBM scratch for split rows), the row's top-k
// is selected, and only the <= top_k kept source rows are gathered again.
//
// The kernels are HBM/Infinity-Cache bound gathers of 4*C-byte rows; each lane
// group reads one whole source row per load (VEC*4 B per lane, coalesced).
//
// This header: FwdArgs - the one argument of every forward kernel - with its store epilogue, and the launchers and
// globals that the entry points (agg_fwd.hip) and the per-layout translation units (agg_fwd*_v*.hip) share.  Needs
// device_utils.h (Row, HalfRef, the dropout draw).  The kernels: agg_fwd_head.h, agg_fwd_select.h, agg_fwd_fin.h,
// agg_fwd_roles.h; the launch decisions: fwd_plan.h; the launchers: agg_fwd_impl.h.
#pragma once
#include "device_utils.h"

namespace sngnn {

struct FwdArgs {
    // TABLE mode: n = unit rows [Ntot, C] (k_normalize_rows), nrm = max(|h|_2, eps) [Ntot].
    // OTF mode (on the fly; nrm == nullptr): n = the RAW rows h themselves.  Every edge gets the
    // fast cosine <h_i, h_j> inv_i inv_j (device_utils.h: edge_score), which differs from the
    // reference-order value s = <h_i / d_i, h_j / d_j> by at most `delta`; wherever a decision
    // cannot be taken from the fast value - within delta of thr, within 2 delta of the top_k-th or
    // of another edge whose rank is asked for - the edge is scored again exactly (IEEE
    // normalisation of the two rows in registers, the table path's dot), so selections, ties
    // included, are those of the table path, bit for bit, without the normalisation pass.
    // (the half path, sngnn_agg_forward_half: n holds __half / __hip_bfloat16 rows and out is stored in that type -
    // the kernels' template parameter S; rows<S>() / outs<S>() / out_at<S>() below.  Everything else stays fp32.)
    const float *n;
    const float *nrm;
    // the table's size: Ntot rows, n_bytes = Ntot * C * (bytes per value) - what the buffer form of the work-item
    // roles builds its resources from (agg_fwd_src.h; n_bytes == 0: the table has 2 GiB or more and the call runs the
    // flat form, fwd_plan.h: fwd_buffer_form)
    int Ntot;
    unsigned n_bytes;
    float delta;          // OTF: bound on |fast - exact| (launcher: (4 C + 32) 2^-24)
    const uint4 *filt;    // [Ntot, filter_row_halfs(C)] fp16 filter rows (agg_fwd_filter.h) or nullptr
    int filt_small;       // the filter also in front of the SMALL rows (small_rows_set_filt): pays when a threshold
                          // prunes - then most rows fetch no fp32 row at all (arxiv size, top_k 16 / thr 0.9: main
                          // kernel 40.4 -> 36.2 us); with thr 0 it is a second dependent round trip per set for
                          // rows that keep something anyway (top_k 1: 49.3 -> 61.3 us), so the launcher sets it
                          // for thr >= 0.25 (and top_k >= 4) only
    int filt_min_deg;     // wave rows below this in-degree score their fp32 rows directly (two dependent round trips
                          // for a short row cost more than the second lines they save): launcher, agg_fwd.hip
    int C, N;             // N = owned target rows
    int row_off;          // row i's own feature row is n[row_off + i] (node-range partition)
    const int32_t *rowptr, *col, *rperm;
    const int32_t *col_s;       // col with the rows in slot order (rdesc.w = first entry)
    const int4 *rdesc;     // per degree-sorted slot: {row, first edge, in-degree, first entry in col_s}
    int k;            // < 0: no selection
    float thr;
    float *out, *wsel, *inv_norm;
    int32_t *sel_src;
    float *sel_w;
    int n_split, n_med_end;     // slots [0,n_split) split, [n_split,n_med_end) wave, rest small
    int n_tasks;
    const int32_t *task_slot, *task_chunk, *split_soff, *split_task0;
    const int32_t *task_order;      // position in the dealing order -> task (graph.hip 7b)
    float *scores, *partial;    // workspace
    unsigned long long *cand_key;   // [n_tasks, k]  chunk-local top-k keys of split rows
    int32_t *cand_src;              // [n_tasks, k]  their source ids (saves the finalize a dependent load)
    int use_cand;                   // split rows keep chunk-local candidates (k <= CAND_MAX_K and they fit LDS)
    int lowbits;                    // bits needed for a row-local edge index
    int n_split_gt_wave;        // split rows with more than 128 / k tasks (descending order: the first ones)
    // The split rows' finalize INSIDE the main launch (round 5; agg_fwd_fin.h: fin_block_pair / fin_group_batch / fin_stream_row): workgroups [main_blocks, gridDim.x)
    // take no work items - their waves finalize split rows, each as soon as the row's tasks have published their
    // candidates (fin_done[task] == fin_nonce).  main_blocks == gridDim.x: the finalize is the next launch.
    int main_blocks;
    unsigned long long *fin_done;   // [n_tasks] workspace; left zero by the wave that consumed them
    unsigned long long fin_nonce;   // this call's own value (never 0, never an earlier call's)
    unsigned k_magic;               // ceil(2^32 / k) for k >= 2: q / k = __umulhi(q, k_magic) for q < 2^32 / k (fin_slot)
    long long n_edges;              // E' of the call's graph (host side: the launcher's estimate of the launch's time)
    int role_mask;              // measurement aid (sngnn_tuning_set): bit 0 tasks, 1 wave rows, 2 small rows
    // row filter (sngnn_agg_forward_rows): only the target rows i with row_flag[i] == row_want are
    // computed and written; nullptr = all rows.  (A rank's interior rows - all sources local - run
    // while the halo rows of its boundary rows are still in flight, sngnn_amd/dist.py.)
    const uint8_t *row_flag;
    int row_want;
    __device__ __forceinline__ bool skip_row(int i) const { return row_flag != nullptr && row_flag[i] != row_want; }
    // n and out in their storage type S (float: the pointers themselves)
    template <typename S> __device__ __forceinline__ const S *rows() const { return reinterpret_cast<const S *>(n); }
    template <typename S> __device__ __forceinline__ S *outs() const { return reinterpret_cast<S *>(out); }
    // one value of out: `a.out_at<S>(idx) = v` (float: the plain element itself)
    template <typename S> __device__ __forceinline__ decltype(auto) out_at(size_t idx) const
    {
        if constexpr (std::is_same<S, float>::value) return (out[idx]);
        else return HalfRef<S>{outs<S>() + idx};
    }
    // store epilogue of a hidden layer (models.py:204-209: conv -> [+ bias] -> relu_ -> dropout), applied to
    // the finished mean row on its way out: out = keep ? max(mean + bias, 0) * scale : 0.
    // epi_flags: bit 0 relu, bit 1 bias, bit 2 keep mask; 0 = none (sngnn_agg_forward_epilogue).
    // Kept bits written by the forward itself (training calls; common.h "kbits" layout; nullptr = off, the
    // per-edge weights wsel are written instead): a small row stores its 16 bits as one halfword
    // at its row id, a wave row its 128 bits at its slot, a split-row task zeroes its 128 bits and
    // the finalize sets the winners' - plain stores of whole units each row owns: no atomics between
    // rows, no clearing pass, and the backward needs no k_pack_kept launch.  Host guarantees
    // 0 <= top_k <= SMALL_T (wave rows and tasks always rank) and the candidate finalize.
    unsigned *kbits;
    int kb_wbase, kb_tbase;
    // epi_flags: bit 0 relu, bit 1 bias, bit 2 keep mask given, bit 3 keep mask drawn here; 0 = none.
    int epi_flags;
    const float *epi_bias;          // [C]
    const uint8_t *epi_keep;        // [N, C] 1 = kept (the caller's own Bernoulli(1 - p) draw), or
    const unsigned long long *epi_seed;   // dev [1]: the mask is drawn here, keep = u(seed, i C + c) >= p
    float epi_p;
    float epi_scale;                // 1 / (1 - p) when something is dropped, else 1
    // The classification head of the LAST layer inside the forward's second launch (head_row.h;
    // sngnn_epilogue_t.head_*): the finished mean row (+ epi_bias) is the row of logits - its
    // log-softmax NLL term and arg-max hit are added to an entry of head_part ([entries][4] floats:
    // loss A, correct A, loss B, correct B) and, training, d loss / d logits replaces the row in `out`.
    // Split rows go through it in their finalize, while they are in registers (entry head_nmain + p);
    // all other rows are read back from `out` by extra workgroups of the SAME launch (head_rows_role;
    // entry = their wave id): the finalize is a latency chain of a few hundred workgroups on an
    // otherwise idle chip, the head a bandwidth-bound pass - one launch, the longer of the two.
    // (In the main kernel's stores instead: its 80-register budget spilled 15-39 registers, at 96
    // the kernel took 62 against 51 us - more than the head pass costs.)
    // head_flags: bit 0 two splits (head_sel is a bit set), bit 1 out = the gradient, else out = the logits.
    const int64_t *head_y;
    const uint8_t *head_sel;
    float *head_part;
    int head_flags, head_nmain;
    float head_scale;               // 1 / rows of split A (the gradient's factor, the mean's)
    float head_scale_b;             // 1 / rows of split B
    float *head_out;                // dev [2] or [4]: (mean NLL, correct count) per split, by launch_head_reduce
    __device__ __forceinline__ bool drawn_keep(int i, int c) const       // (device_utils.h: sn_dropout_keep)
    {
        return sn_dropout_keep(*epi_seed, (unsigned long long)i * (unsigned)C + (unsigned)c, epi_p);
    }
    __device__ __forceinline__ float epilogue(float v, int i, int c) const
    {
        if (epi_flags & 2) v += epi_bias[c];
        if (epi_flags & 1) v = fmaxf(v, 0.f);
        if (epi_flags & 4) v = epi_keep[(size_t)i * C + c] ? v * epi_scale : 0.f;
        if (epi_flags & 8) v = drawn_keep(i, c) ? v * epi_scale : 0.f;
        return v;
    }
};

// the same on a row held by a lane group (channels beyond C: untouched, never stored)
template <int VEC, int G, int R>
__device__ __forceinline__ void row_epilogue(const FwdArgs &a, Row<VEC, G, R> &acc, int i, int lg)
{
    if (a.epi_flags == 0) return;                         // (uniform)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c0 = (r * G + lg) * VEC;
        if (c0 < a.C) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc.x[r][v] = a.epilogue(acc.x[r][v], i, c0 + v);
        }
    }
}

// profiling (sngnn_profile_enable(reps)): every launch is issued `reps` times back to back
// between its two events, so the event pair's own cost is spread over reps launches
extern int g_prof_reps;
// sngnn_tuning_set(9, v): 0 = the split rows' finalize as a launch of its own (round 4's form), 1 = inside the main
// launch when it pays (fwd_plan.h: fwd_fin_blocks), v > 1 = inside it on v workgroups
extern int g_fin_inline, g_last_fin_blocks;
// sngnn_tuning_set(12, v): 0 = a call that wants `out` only runs the lean main kernel (agg_fwd_roles.h: k_agg_fwd,
// LEAN; launch_agg_fwd_impl has the rule), 1 = the general kernel always (the A/B of a measurement; the tests)
extern int g_fwd_general_only;
unsigned long long next_fin_nonce();

// The launchers the entry points call (agg_fwd.hip compiles none of the kernels behind them).
// Defined one per translation unit: storage type S (float, __half, __hip_bfloat16: agg_fwd[_f16|_bf16]_v*.hip) x VEC
// values per lane (entry.h: SNGNN_LAUNCH_VEC).  The unit-row passes and the store epilogue exist for fp32 rows only,
// the filter pass and the epilogue for 16-byte rows only (agg_fwd_v4.hip, agg_fwd_v4e.hip).
// fp32 rows have the forward in two forms (agg_fwd_src.h): launch_agg_fwd_buf_vec / launch_agg_fwd_epi_buf_v4 read
// through buffer resources (agg_fwd_v*.hip, agg_fwd_v4e.hip), launch_agg_fwd_vec<float, ..> / launch_agg_fwd_epi_v4
// are the flat form (agg_fwd_flat_v*.hip, agg_fwd_flat_v4e.hip); the caller picks by fwd_plan.h: fwd_buffer_form.
template <typename S, int VEC>
int launch_agg_fwd_vec(const RowCfg &cfg, const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st);
template <typename S, int VEC>
int launch_normalize_vec(const RowCfg &cfg, const float *h, int64_t rows, int C, float *n, float *nrm, void *filt,
                         hipStream_t st);
int launch_agg_fwd_epi_v4(const RowCfg &cfg, const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st);
template <int VEC>
int launch_agg_fwd_buf_vec(const RowCfg &cfg, const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st);
int launch_agg_fwd_epi_buf_v4(const RowCfg &cfg, const FwdArgs &a, int max_split_deg, hipEvent_t *ev, hipStream_t st);
int launch_filter_v4(const RowCfg &cfg, const float *n, int64_t rows, int C, void *filt, hipStream_t st);

}  // namespace sngnn

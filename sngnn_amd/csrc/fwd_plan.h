// The launch decisions of the fused aggregation forward, as plain C++ on plain counts (no HIP, no FwdArgs, no
// device): whether split rows keep candidates, how their finalize is shaped, its workgroup sizes and dynamic LDS,
// whether and on how many workgroups it rides inside the main launch, the persistent grid, the head role's
// workgroups.  The launchers (agg_fwd_impl.h) fill a FwdPlanIn from their arguments, call fwd_plan() once and then
// only pick template instantiations and launch; a host program can run the same code on any counts
// (tests/test_fwd_plan_cpu.py).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <algorithm>

#include "ws_layout.h"   // CAND_MAX_K, CHUNK, BLOCK, WAVES, FIN_BLOCK, ceil_div

namespace sngnn {

// ---- the chip, as the policy knows it (MI355X; not queried: a partitioned device keeps these figures) -------------
constexpr int CHIP_CUS = 256;
#ifndef SNGNN_FWD_WAVES
#define SNGNN_FWD_WAVES 6
#endif
constexpr int FWD_WAVES_PER_SIMD = SNGNN_FWD_WAVES;   // register budget of the main kernel (6: <= 80 VGPRs)
// workgroups of the main kernel (BLOCK threads: one wave per SIMD) the chip holds at that occupancy
constexpr int FWD_SLOTS = CHIP_CUS * FWD_WAVES_PER_SIMD;
constexpr int HEAD_ROLE_WAVES_MAX = CHIP_CUS * 32;    // waves of the head role as a launch of its own

// ---- the finalize inside the main launch: measured figures (us, MI355X; fwd_plan()'s comment) --------------------
constexpr int FIN_BLOCKS_MAX = 256;          // workgroups of the finalize role at most
constexpr double US_ITEM = 5.8;              // a wave of the main kernel per work item
constexpr double US_FIN_START = 6.0;         // the role starts this far in (the tasks are the first items)
constexpr double US_FIN_PAIR = 17.0;         // a workgroup per pair of big rows
constexpr double US_FIN_BATCH = 12.5;        // a wave per batch of 64 / G moderate rows (twice that at eight rows)
constexpr double US_FIN_STREAM_ROW = 4.0;    // no selection: a wave per row ..
constexpr double US_FIN_STREAM_16 = 2.5;     // .. + per sixteen tasks of the biggest row
constexpr double US_SEP_LAUNCH = 4.6;        // the finalize as a launch of its own: the launch ..
constexpr double US_SEP_BOUNDARY = 1.1;      // .. and the boundary in front of it
constexpr double US_SEP_BIG = 12.0;          // .. a big row's tournament (three workgroups per CU)
constexpr double FWD_BYTES_PER_US = 4.8e6;   // 4.8 TB/s: the rate the main kernel reaches on big graphs (x 0.8)

// ---- the candidate finalize (k_agg_fin_cand / k_agg_fin_mixed) -----------------------------------------------------
constexpr int FIN_WAVE_MIN_ROWS = 2048;   // fewer moderate split rows than this: one launch (k_agg_fin_cand) for all
// Waves per workgroup of the candidate finalize (template NW): 16 where the biggest row's tournament has more
// than 1 024 candidates to get through (its first level runs wide: arxiv size at top_k 16, 1 632 keys:
// 7.6 us against 8.5 with 8 waves), else 8 - a smaller workgroup is less launch to pay (top_k 1: 1.9
// against 2.7 us) - and 8 whenever the head role rides in the launch (75 registers: three 512-thread
// workgroups fit a CU, one of 1 024 threads).
constexpr int FINC_WAVES_MAX = 16;
constexpr size_t FINC_LDS_BUDGET = 150 * 1024;
// dynamic LDS of fin_cand_row: [FINC_WAVES_MAX * C] partial rows | two key and two source arrays of max_slots | count
inline size_t finc_lds_bytes(int C, int max_slots) { return ((size_t)FINC_WAVES_MAX * C + 1) * 4 + (size_t)max_slots * 24 + 16; }

// ---- the finalize from scores in HBM scratch (k_agg_fin) ----------------------------------------------------------
constexpr size_t FIN_LDS_SCORES_BUDGET = 120 * 1024;   // partial rows + kept list + as many scores as fit under this
constexpr size_t FIN_LDS_LIMIT = 150 * 1024;           // the kept list alone beyond this: top_k too large

// ---- how the work-item roles address what they gather (agg_fwd_src.h) ----------------------------------------------
// The buffer form - a resource per array and a 32-bit byte offset per load, out-of-range offsets for whatever nobody
// reads - iff the table has fewer than 2^31 bytes: an offset with bit 31 set must be beyond every array a resource
// names.  index_bytes: the largest of the graph's own arrays the roles read that way (column ids, 4 E'; the small
// rows' descriptors, 16 N) - below the table's size on every graph but degenerate ones, held to the same limit.
// addr_mode (sngnn_tuning_set(11, v)): 0 = this rule, 1 = the flat form always (64-bit pointers: the form for the
// tables beyond the limit, and the reference of an A/B measurement).
constexpr int64_t FWD_BUFFER_LIMIT = (int64_t)1 << 31;
inline bool fwd_buffer_form(int64_t table_bytes, int64_t index_bytes, int addr_mode)
{
    return addr_mode != 1 && table_bytes < FWD_BUFFER_LIMIT && index_bytes < FWD_BUFFER_LIMIT;
}

// whether split rows keep chunk-local candidates (else: scores to HBM scratch + k_agg_fin)
inline bool fwd_use_candidates(int top_k, int C, int max_split_deg)
{
    if (top_k < 0) return true;                 // no selection: partial rows, candidate launch shape
    if (top_k > CAND_MAX_K) return false;
    const int max_slots = std::max(1, ceil_div(max_split_deg, CHUNK) * std::max(top_k, 0));
    return finc_lds_bytes(C, max_slots) <= FINC_LDS_BUDGET;
}

// workgroups of the head role in a launch of `block` threads (head_part entry = the workgroup's index):
// enough waves to fill the chip, never more than the rows need
inline int head_role_blocks(int64_t N, int G, int block)
{
    // (inside the finalize launch the workgroups hold 75 registers - six waves per SIMD, three 512-thread
    // workgroups per CU - and the finalize's own workgroups sit beside them: ONE round of 2 per CU)
    const int64_t cap = block == BLOCK ? HEAD_ROLE_WAVES_MAX : (int64_t)CHIP_CUS * 2 * (block / 64);
    const int64_t waves = std::min<int64_t>(ceil_div(N, 2 * (64 / G)), cap);
    return ceil_div(waves, block / 64);
}

// what the policy reads of a call
struct FwdPlanIn {
    int N, n_med_end, n_split;   // owned rows; slots [0, n_split) split, [n_split, n_med_end) wave, the rest small
    int n_split_gt_wave;         // split rows with more than 128 / k tasks (no selection: more than 16)
    int n_tasks;
    long long n_edges;           // E' of the call's graph
    int C, G, k;                 // channels, lanes per row (RowCfg), top_k (< 0: no selection)
    bool use_cand;               // split rows keep chunk-local candidates (fwd_use_candidates, or forced off)
    bool head;                   // the classification head rides the call
    bool half_rows;              // rows stored as fp16 / bf16: no head role, whatever `head` says
    bool has_fin_done;           // the workspace has the tasks' done words
    int role_mask;               // sngnn_tuning_set(0, mask)
    int max_split_deg;           // in-degree of the biggest split row (0: none)
    int fin_inline;              // sngnn_tuning_set(9, v): 0 = finalize as a launch of its own, 1 = inside the main
                                 // launch when it pays, v > 1 = inside it on v workgroups
};

// how the split rows of a call are finalized (rows are in descending degree order: the first n_big_true
// need the workgroup tournament, the rest fit one wave-level selection)
struct FinShape { int n_wave, n_big, n_big_true; bool mixed; };

struct FwdPlan {
    // the main launch: workgroups [0, main_blocks) take work items, [main_blocks, main_blocks + fin_blocks) finalize
    // the split rows (fin_blocks == 0: the finalize is the launches below); head_part entries of the head role
    int main_blocks, fin_blocks, head_nmain;
    FinShape fin;
    // the candidate finalize (use_cand; all zero otherwise)
    int finc_waves;              // 8 or 16 waves per workgroup
    bool finc_head;              // its HEAD instantiation
    int max_slots;               // candidate slots of the biggest row
    size_t finc_dyn, finc_dyn_mixed;   // dynamic LDS bytes of k_agg_fin_cand / k_agg_fin_mixed
    bool finc_fits;              // finc_dyn <= FINC_LDS_BUDGET (else: "candidate finalize does not fit LDS")
    int mixed_fin_blocks, mixed_head_blocks;   // fin.mixed: the one launch's finalize and head workgroups
    int cand_blocks, wave_blocks;              // else: k_agg_fin_cand's and k_agg_fin_wave's workgroups
    // the scratch finalize (k_agg_fin)
    bool topk_too_large;         // the kept list alone does not fit LDS
    int lds_scores;              // scores of a row held in LDS (rows up to this in-degree)
    size_t fin_dyn;              // its dynamic LDS bytes
};

inline FinShape finalize_shape(const FwdPlanIn &a)
{
    FinShape f;
    f.n_wave = a.n_split - std::min(a.n_split, a.n_split_gt_wave);
    // (no selection, k < 0: the split is by the number of partial rows to add, > 16 tasks -> workgroup)
    f.n_big = a.k < 0 ? a.n_split - f.n_wave
                      : ((a.k > 0 && f.n_wave >= FIN_WAVE_MIN_ROWS) ? a.n_split - f.n_wave : (a.k > 0 ? a.n_split : 0));
    f.n_big_true = a.n_split - f.n_wave;         // rows that need the tournament
    // few moderate rows (arxiv-like graphs: a few hundred split rows in all; products-like ones have 10^5): ONE launch
    f.mixed = a.n_split > 0 && a.use_cand && a.k > 0 && f.n_big == a.n_split && f.n_wave > 0 && f.n_big_true < a.n_split;
    return f;
}

// Workgroups of the split rows' finalize INSIDE the main launch (agg_fwd_fin.h: fin_block_pair / fin_group_batch /
// fin_stream_row), 0 = it is the next launch: rows that rank from candidates, no head behind them - when it pays.
// All figures in us, measured on MI355X (tools/sweep_fwd.py FIN=.., arxiv and products size): a wave takes ~5.8 us per
// work item; the role starts ~6 us in (the tasks are the first items), a pair of big rows takes a workgroup ~17 us, a
// batch of 64 / G moderate rows a wave ~12.5.
//   * the role must end by 3/4 of the launch: the smallest number nb of workgroups that does;
//   * each of them is six waves' worth of slots the work items lose: the launch grows by nb / (slots - nb);
//   * against that, the launch it replaces: ~4.6 us + its rows over the whole chip, + the boundary (1.1).
// Arxiv size, C 40: 48 workgroups, +1.6 us against 7.1 saved (measured: 68.1 -> 62.0 us per forward, hot device).
// Products size: 64 workgroups, 4.65 -> 4.55 ms per forward.
// Small graphs, narrow rows (C 32: a 35 us launch): nothing ends the role in time - a launch.
//   Calls that select nothing (top_k < 0: fin_stream_row, one wave per row): ~4 us per row + 2.5 per sixteen tasks
// of the biggest row.
inline int fwd_fin_blocks(const FwdPlanIn &a, int64_t items)
{
    const int RPW = 64 / a.G;
    const bool fin_ok = a.fin_inline != 0 && a.n_split > 0 && a.use_cand && a.k != 0 && !a.head &&
                        a.has_fin_done && ((a.role_mask & 7) == 7 || a.fin_inline > 1);
    // (a forced role with the tasks masked out - knobs 9 and 0 - is the test of the bounded wait: the split rows come
    // back as NaN after FIN_SPIN_MAX polls, tests/test_fin_inline_gpu.py)
    if (!fin_ok) return 0;
    if (a.fin_inline > 1) return std::min(a.fin_inline, FIN_BLOCKS_MAX);      // (forced: tuning knob 9)
    const int fin_big = std::min(a.n_split, a.n_split_gt_wave);
    const int fin_batches = ceil_div(a.n_split - fin_big, RPW);
    // (eight rows per batch, C <= 32: sixteen keys per lane and eight partial sums - twice the time; measured at
    // arxiv size, C 32, top_k 1: the role on 32 workgroups 51.8 against 50.7 us as a launch)
    const double t_batch = RPW >= 8 ? 2 * US_FIN_BATCH : US_FIN_BATCH;
    for (int nb = 8; nb <= FIN_BLOCKS_MAX; nb += 8) {
        const int64_t main_waves = (int64_t)std::min<int64_t>(ceil_div(items, WAVES), FWD_SLOTS - nb) * WAVES;
        // the launch's time: work items at their latency-bound pace, or - big graphs, whose items are mostly
        // 128-edge tasks - the forward's bytes at the rate this kernel reaches (0.8 x B_fwd at 4.8 TB/s; products
        // size: 4.3 ms estimated, 4.1-4.2 measured; there 64 workgroups are the best count: 4.55 ms per forward
        // against 4.65 with the finalize as a launch, 4.64 with 48 or 128)
        const double b_fwd = (double)a.n_edges * (4.0 * a.C + 8.0) + (double)a.N * (8.0 * a.C + 8.0);
        const double t_main = std::max(US_ITEM * (double)ceil_div(items, main_waves), 0.8 * b_fwd / FWD_BYTES_PER_US);
        const double t_fin = a.k < 0
            ? US_FIN_START + US_FIN_STREAM_ROW * ceil_div(a.n_split, nb * WAVES) +
                  US_FIN_STREAM_16 * ceil_div(ceil_div(a.max_split_deg, CHUNK), 16)
            : US_FIN_START + US_FIN_PAIR * ceil_div(ceil_div(fin_big, 2), nb) + t_batch * ceil_div(fin_batches, nb * WAVES);
        if (t_fin > 0.75 * t_main) continue;
        const double t_sep = a.k < 0 ? US_SEP_LAUNCH + US_SEP_BOUNDARY + US_FIN_STREAM_ROW * a.n_split / (CHIP_CUS * 24.0)
                                     : US_SEP_LAUNCH + US_SEP_BOUNDARY + US_SEP_BIG * fin_big / (CHIP_CUS * 3.0) +
                                           US_FIN_BATCH * fin_batches / (CHIP_CUS * 24.0);
        const double loss = US_ITEM * (double)ceil_div(items, (int64_t)FWD_SLOTS * WAVES) * nb / (double)(FWD_SLOTS - nb);
        return loss + 1.0 < t_sep ? nb : 0;                   // (more workgroups only cost more)
    }
    return 0;
}

inline FwdPlan fwd_plan(const FwdPlanIn &a)
{
    FwdPlan p = {};
    const int RPW = 64 / a.G;
    const int n_small = a.N - a.n_med_end;
    const int64_t items = (int64_t)a.n_tasks + (a.n_med_end - a.n_split) + ceil_div(n_small, RPW);
    p.fin = finalize_shape(a);
    p.fin_blocks = fwd_fin_blocks(a, items);
    // persistent grid: what the chip holds at the kernel's occupancy, or less (the finalize role's workgroups
    // are resident from the start: they come out of the same budget)
    p.main_blocks = (int)std::min<int64_t>(ceil_div(items, WAVES), FWD_SLOTS - p.fin_blocks);
    // head_part: one entry per workgroup of the head role, then one per split row.  (The role rides in the
    // mixed finalize launch - 512 threads then - where there is one, else in a launch of its own.)
    p.head_nmain = a.head ? head_role_blocks(a.N, a.G, p.fin.mixed ? 512 : BLOCK) : 0;

    if (a.use_cand) {
        const int max_tasks = ceil_div(a.max_split_deg, CHUNK);
        const int64_t slots = (int64_t)max_tasks * std::max(a.k, 0);
        p.finc_waves = (!a.head && (a.k < 0 || slots > 1024)) ? 16 : 8;     // (FINC_WAVES_MAX's comment)
        p.finc_head = a.head && !a.half_rows;
        p.max_slots = std::max(1, max_tasks * std::max(a.k, 0));
        p.finc_dyn = finc_lds_bytes(a.C, p.max_slots);
        p.finc_fits = p.finc_dyn <= FINC_LDS_BUDGET;
        p.finc_dyn_mixed = std::max(p.finc_dyn, (size_t)p.finc_waves * CAND_MAX_K * 12);
        p.mixed_fin_blocks = p.fin.n_big_true + ceil_div(p.fin.n_wave, p.finc_waves);
        p.mixed_head_blocks = p.finc_head ? p.head_nmain : 0;
        p.cand_blocks = p.fin.n_big;
        p.wave_blocks = ceil_div(a.n_split - p.fin.n_big, WAVES);
    }
    // k_agg_fin: [C * FIN_BLOCK / 64] partial rows | [min(k, deg)] kept list | [lds_scores] scores
    const size_t fixed = (size_t)a.C * (FIN_BLOCK / 64) * 4 + (size_t)std::min(std::max(a.k, 0), a.max_split_deg) * 4;
    p.topk_too_large = fixed > FIN_LDS_LIMIT;
    if (fixed < FIN_LDS_SCORES_BUDGET)
        p.lds_scores = (int)std::min<size_t>((FIN_LDS_SCORES_BUDGET - fixed) / 4, (size_t)a.max_split_deg);
    p.fin_dyn = fixed + (size_t)p.lds_scores * 4;
    return p;
}

}  // namespace sngnn

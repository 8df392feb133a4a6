// The one definition of every region inside the workspace that sngnn_graph_workspace_bytes sizes.
// Plain C++ on plain counts (no HIP, no graph object): the size query (graph.hip) and every entry point that carves
// the buffer (agg_fwd.hip, agg_bwd.hip, attn.hip, signed.hip) read the same offsets, and a host program can check
// them (tests/test_workspace_layout_cpu.py).  All offsets and totals are BYTES from the start of the workspace.
// Also here, because the forward's launch plan (fwd_plan.h) is plain C++ too: the row classes and workgroup sizes.
#pragma once
#include <stdint.h>
#include <algorithm>

#include "sngnn_hip.h"

namespace sngnn {

// ---- row classes of the aggregation kernels (by in-degree) -----------------
constexpr int SMALL_T = 16;    // deg <= SMALL_T : one G-lane group per row
constexpr int WAVE_T = 128;    // deg <= WAVE_T  : one wave per row
constexpr int CHUNK = 128;     // deg >  WAVE_T  : split into CHUNK-edge wave tasks
constexpr int BLOCK = 256;     // threads per workgroup of the main kernels
constexpr int WAVES = BLOCK / 64;
constexpr int FIN_BLOCK = 1024;   // threads per workgroup of the split-row finalize
constexpr int CAND_MAX_K = 32;   // split rows: chunk-local candidates are kept for k <= this (fwd_plan.h)

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }
// bytes of `floats` fp32 values, rounded up to whole 16-byte vectors (what follows holds 16-byte aligned rows)
inline int64_t rows16(int64_t floats) { return (floats + 3) / 4 * 4 * 4; }

// bytes of one fp16 filter row (agg_fwd_filter.h): whole 128-byte lines; 0 = no filter for this C
// (it pays when a unit row is longer than one line and the rows are 16-byte vectors)
inline int64_t filter_row_bytes(int C)
{
    if (C % 4 != 0 || C <= 32 || C > SNGNN_MAX_CHANNELS) return 0;
    int64_t b = 128;                 // 2 bytes x (4 G R) channels of the row layout: 64, 128, 256 or 512
    while (b < 2 * (int64_t)C) b <<= 1;
    return b;
}

// forward (sngnn_agg_forward*): three 256-byte aligned tables in front of the split rows' scratch
//   unit rows [Ntot][C] | norms [Ntot] | fp16 filter rows [Ntot][filter_row_bytes(C)] |
//   scores of the split rows' edges | one partial row [C] per split task | CAND_MAX_K candidate keys per task |
//   CAND_MAX_K candidate source ids per task | one done word per task (the finalize role: agg_fwd_fin.h)
struct FwdLayout { int64_t unit, nrm, filt, scores, partial, cand_key, cand_src, fin_done, total; };

inline FwdLayout fwd_layout(int64_t Ntot, int64_t split_edges, int64_t n_tasks, int C)
{
    FwdLayout L;
    L.unit = 0;
    L.nrm = L.unit + up256(Ntot * (int64_t)C * 4);
    L.filt = L.nrm + up256(Ntot * 4);
    L.scores = L.filt + up256(Ntot * filter_row_bytes(C));
    L.partial = L.scores + rows16(split_edges);
    L.cand_key = L.partial + rows16(n_tasks * C);
    L.cand_src = L.cand_key + n_tasks * CAND_MAX_K * 8;
    L.fin_done = L.cand_src + n_tasks * CAND_MAX_K * 4;       // 8-byte aligned
    L.total = L.fin_done + n_tasks * 8;
    return L;
}

// backward, in its two shapes:
//   aggregation (sngnn_agg_backward*): {w, ds} record per edge, the kept-bit mask in its first words | dnT [N][C] |
//       partT [n_tasks][C] | partS [n_stasks][2 C]
//   attention and signed (sngnn_attn_backward*, sngnn_signed_backward*): records | dnT [N][C] |
//       partT [n_tasks][2 C + 4] | partS [n_stasks][2 C] | rec_dot [N] (dot_i per target: the attention mode only)
struct BwdLayout { int64_t rec, dnT, partT, partS, rec_dot, total; };

inline BwdLayout bwd_layout(int64_t Ep, int64_t N, int64_t n_tasks, int64_t n_stasks, int C, bool attention)
{
    BwdLayout L;
    L.rec = 0;
    L.dnT = L.rec + rows16(2 * Ep);
    L.partT = L.dnT + N * (int64_t)C * 4;
    L.partS = L.partT + n_tasks * (attention ? 2 * C + 4 : C) * 4;
    L.rec_dot = L.partS + n_stasks * C * 4 * 2;
    L.total = attention ? L.rec_dot + rows16(N) : L.rec_dot;
    return L;
}

// the attention and signed forwards keep only the split tasks' partial rows: [n_tasks][C + 4] and [n_tasks][C]
struct PartialLayout { int64_t partial, total; };

inline PartialLayout attn_fwd_layout(int64_t n_tasks, int C) { return {0, n_tasks * (C + 4) * 4}; }
inline PartialLayout signed_fwd_layout(int64_t n_tasks, int C) { return {0, n_tasks * C * 4}; }

// sngnn_graph_workspace_bytes: one buffer that serves every call above on a graph of these counts
inline int64_t graph_workspace_bytes(int64_t N, int64_t Ntot, int64_t Ep, int64_t n_tasks, int64_t n_stasks,
                                     int64_t split_edges, int C)
{
    return up256(std::max({fwd_layout(Ntot, split_edges, n_tasks, C).total,
                           bwd_layout(Ep, N, n_tasks, n_stasks, C, false).total,
                           bwd_layout(Ep, N, n_tasks, n_stasks, C, true).total,
                           attn_fwd_layout(n_tasks, C).total, signed_fwd_layout(n_tasks, C).total}));
}

}  // namespace sngnn

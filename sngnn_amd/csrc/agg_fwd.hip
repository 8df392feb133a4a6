// C-ABI entries of the fused aggregation forward (the kernels: agg_fwd_impl.h and the headers it lists; none is compiled here).
#include <atomic>
#include "agg_fwd_args.h"
#include "agg_fwd_filter.h"
#include "fwd_plan.h"
#include "head_row.h"
#include "entry.h"

using namespace sngnn;

// Optional in-library timing of the forward's launches (bench.py's roofline leg):
// HIP events recorded on the caller's stream around each launch.
//   ev[0] .. normalisation pass .. ev[1] .. main kernel .. ev[2] .. split-row finalize .. ev[3] .. (nothing) .. ev[4]
// The empty last interval measures what an event pair itself adds to an interval (a few
// microseconds on this stack); sngnn_profile_last_forward reports it so that the caller can
// take it off the three kernel figures.
static bool g_prof_on = false;
namespace sngnn { int g_prof_reps = 1; }
static hipEvent_t g_prof_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};

extern "C" int sngnn_profile_enable(int on)
{
    if (on && !g_prof_ev[0])
        for (auto &e : g_prof_ev) SN_HIP(hipEventCreate(&e));
    g_prof_on = on != 0;
    g_prof_reps = on > 1 ? on : 1;
    return SNGNN_OK;
}

extern "C" int sngnn_profile_last_forward(float *norm_ms, float *main_ms, float *fin_ms, float *empty_ms)
{
    SN_REQUIRE(g_prof_ev[0] != nullptr && norm_ms && main_ms && fin_ms && empty_ms, SNGNN_EINVAL,
               "profiling is not enabled");
    SN_HIP(hipEventSynchronize(g_prof_ev[4]));
    SN_HIP(hipEventElapsedTime(norm_ms, g_prof_ev[0], g_prof_ev[1]));
    SN_HIP(hipEventElapsedTime(main_ms, g_prof_ev[1], g_prof_ev[2]));
    SN_HIP(hipEventElapsedTime(fin_ms, g_prof_ev[2], g_prof_ev[3]));
    SN_HIP(hipEventElapsedTime(empty_ms, g_prof_ev[3], g_prof_ev[4]));
    *norm_ms /= (float)g_prof_reps;
    *main_ms /= (float)g_prof_reps;
    *fin_ms /= (float)g_prof_reps;
    return SNGNN_OK;
}

static __global__ void k_fill_sel(int32_t *__restrict__ src, float *__restrict__ w, int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        src[i] = -1;
        w[i] = 0.f;
    }
}

static int normalize_dispatch(const RowCfg &cfg, const float *h, int64_t rows, int C, float *n, float *nrm,
                              void *filt, hipStream_t st)
{
    return dispatch_vec(cfg, [&](auto vec) {
        return launch_normalize_vec<float, decltype(vec)::value>(cfg, h, rows, C, n, nrm, filt, st);
    });
}

// wave rows shorter than this score their fp32 rows directly: two dependent round trips for a short row cost more than
// the second lines they save (uniform in-degree 24, top_k 4: 213 us unfiltered, 273 filtered, 223 with this cut)
constexpr int FILT_MIN_DEG = 32;
constexpr double FILT_PRUNABLE_SHARE = 0.62;
// fp16 filter: 0 = never, 1 = when it is expected to pay (default), 2 = whenever it applies (small rows too),
// 3 = the rows above the small class (wave rows, split-row tasks) whenever it applies, at any threshold
static int g_filter_mode = 1;
// measurement aids: the fp16 filter can be switched off (the selections are the same either
// way); sngnn_tuning_set(0, mask) runs only some row classes of the main kernel (bit 0 split-row
// tasks, 1 wave rows, 2 small rows; results are then incomplete - timing only)
static int g_role_mask = 7;
// how sngnn_agg_forward scores: 0 = auto (on the fly from h when nothing is selected - top_k < 0,
// SNConv: 68 -> 58 us per forward at arxiv size, no normalisation pass, no table; the unit-row
// table otherwise: for ranking rows one cheap pass over table rows beats a fast pass plus the
// exact re-scoring of the candidates, 72.2 against 73.5 us at top_k 16 / thr 0), 1 = table
// always, 2 = on the fly always (same selections, bit for bit)
static int g_table_mode = 0;
// (sngnn_tuning_set(8, d): wave rows with fewer than d in-edges skip the fp16 filter; -1 = the library's rule)
static int g_filt_min_deg = -1;
int sngnn::g_fin_inline = 1;
// sngnn_tuning_set(11, v): how the work-item roles address their gathers - 0 = buffer resources where the table allows
// (fwd_plan.h: fwd_buffer_form), 1 = the flat form always
static int g_addr_mode = 0;
// sngnn_tuning_set(12, v): 0 = calls that want `out` only run the lean main kernel, 1 = the general kernel always
int sngnn::g_fwd_general_only = 0;
int sngnn::g_last_fin_blocks = 0;
extern "C" int sngnn_last_forward_finalize_workgroups(void) { return sngnn::g_last_fin_blocks; }
// a value no earlier call of this process has used (the finalize role: the tasks' done words)
unsigned long long sngnn::next_fin_nonce()
{
    static std::atomic<unsigned long long> counter{0};
    return 0xF1A0000000000000ull + counter.fetch_add(1) + 1;
}
bool sngnn::fwd_scores_on_the_fly_forced() { return g_table_mode == 2; }
extern "C" int sngnn_tuning_set(int which, int value)
{
    SN_REQUIRE(which == 0 || (which >= 2 && which <= 12), SNGNN_EINVAL, "unknown tuning knob");
    if (which == 12) { sngnn::g_fwd_general_only = value == 1 ? 1 : 0; return SNGNN_OK; }
    if (which == 11) { g_addr_mode = value == 1 ? 1 : 0; return SNGNN_OK; }
    if (which == 10) return sngnn::set_hist_copies(value);
    if (which == 9) { sngnn::g_fin_inline = value < 0 ? 0 : value; return SNGNN_OK; }
    if (which == 8) { g_filt_min_deg = value; return SNGNN_OK; }
    if (which == 7) return sngnn::set_cosine_split(value);
    if (which == 6) return sngnn::set_knn_route(value);
    if (which == 5) return sngnn::set_lin_mode(value);
    if (which == 3) return sngnn::set_bwd_mode(value);
    if (which == 4) return sngnn::set_bwd_roles(value);
    if (which == 0) g_role_mask = value & 7;
    else g_table_mode = value;
    return SNGNN_OK;
}

extern "C" int sngnn_filter_enable(int mode)
{
    SN_REQUIRE(mode >= 0 && mode <= 3, SNGNN_EINVAL,
               "filter mode must be 0 (off), 1 (auto), 2 (always) or 3 (wave rows and tasks always)");
    g_filter_mode = mode;
    return SNGNN_OK;
}

extern "C" int64_t sngnn_filter_row_bytes(int C) { return filter_row_bytes(C); }

extern "C" int sngnn_normalize_rows_filter(const float *h, int64_t rows, int C, float *n, float *nrm, void *filt,
                                           void *stream)
{
    SN_REQUIRE(rows >= 0, SNGNN_EINVAL, "negative row count");
    SN_REQUIRE(rows == 0 || (h && n && nrm), SNGNN_EINVAL, "h/n/nrm is NULL");
    RowCfg cfg;
    if (int rc = check_rows(C, 0, {h, n}, cfg)) return rc;
    SN_REQUIRE(filt == nullptr || filter_row_bytes(C) > 0, SNGNN_EINVAL,
               "no filter rows for this C (sngnn_filter_row_bytes(C) == 0)");
    SN_REQUIRE(((uintptr_t)filt % 16) == 0, SNGNN_EINVAL, "filt must be 16-byte aligned");
    return normalize_dispatch(cfg, h, rows, C, n, nrm, filt, (hipStream_t)stream);
}

extern "C" int sngnn_normalize_rows(const float *h, int64_t rows, int C, float *n, float *nrm, void *stream)
{
    return sngnn_normalize_rows_filter(h, rows, C, n, nrm, nullptr, stream);
}

// approximate cosine of node pairs straight from filter rows (the instruction sequence of the
// forward's filter pass) - lets a test check the error bound FILT_EPS on the hardware
template <int GF>
static __global__ __launch_bounds__(BLOCK) void k_filter_pair_scores(const uint4 *__restrict__ filt,
                                                                     const int64_t *__restrict__ pa,
                                                                     const int64_t *__restrict__ pb, int64_t n_pairs,
                                                                     float *__restrict__ out)
{
    constexpr int NGF = 64 / GF;
    const int lane = lane_id();
    const int gid = lane / GF, lf = lane % GF;
    const int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int64_t p = w * NGF + gid;
    const int64_t q = p < n_pairs ? p : n_pairs - 1;
    const uint4 fa = filt[(size_t)pa[q] * GF + lf], fb = filt[(size_t)pb[q] * GF + lf];
    const float s = group_sum<GF>(fdot8(fa, fb)) * FILT_UNSCALE;
    if (p < n_pairs && lf == 0) out[p] = s;
}

extern "C" int sngnn_filter_pair_scores(const void *filt, int C, const int64_t *pair_a, const int64_t *pair_b,
                                        int64_t n_pairs, float *out, void *stream)
{
    SN_REQUIRE(filter_row_bytes(C) > 0, SNGNN_EINVAL, "no filter rows for this C");
    SN_REQUIRE(n_pairs >= 0, SNGNN_EINVAL, "negative pair count");
    if (n_pairs == 0) return SNGNN_OK;
    SN_REQUIRE(filt && pair_a && pair_b && out, SNGNN_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int gf = (int)(filter_row_bytes(C) / 16);
    const int grid = ceil_div(n_pairs, (64 / gf) * WAVES);
    const uint4 *f = (const uint4 *)filt;
    switch (gf) {
    case 8: k_filter_pair_scores<8><<<grid, BLOCK, 0, st>>>(f, pair_a, pair_b, n_pairs, out); break;
    case 16: k_filter_pair_scores<16><<<grid, BLOCK, 0, st>>>(f, pair_a, pair_b, n_pairs, out); break;
    case 32: k_filter_pair_scores<32><<<grid, BLOCK, 0, st>>>(f, pair_a, pair_b, n_pairs, out); break;
    default: k_filter_pair_scores<64><<<grid, BLOCK, 0, st>>>(f, pair_a, pair_b, n_pairs, out); break;
    }
    SN_HIP(hipGetLastError());
    return SNGNN_OK;
}

// One forward call as its entry describes it (the seven extern "C" forwards below fill this and run it).
struct FwdCall {
    const sngnn_graph_t *g;
    const void *rows;               // raw rows h (fp32, or dtype's half type); with `prepared` the caller's unit rows
    int dtype = 0;                  // 0 = fp32 rows and out, else SNGNN_DTYPE_F16 / _BF16 (always scored on the fly)
    bool prepared = false;          // the caller holds the unit rows: rows | nrm | (optional) filt
    const float *nrm = nullptr;
    const void *filt = nullptr;
    bool by_rows = false;           // sngnn_agg_forward_rows: only the rows with row_flag == row_want
    const uint8_t *row_flag = nullptr;
    int row_want = 0;
    int C, top_k;
    float thr;
    const sngnn_epilogue_t *epi = nullptr;
    void *out;
    float *wsel, *inv_norm;
    int32_t *sel_src = nullptr;
    float *sel_w = nullptr;
    void *workspace, *stream;
};

// everything after the unit rows exist (nrm == NULL: n holds the raw rows and the kernels score on the fly)
static int launch_forward(const FwdCall &c, const RowCfg &cfg, const float *n, const float *nrm, const void *filt,
                          hipEvent_t *ev)
{
    const sngnn_graph_t *g = c.g;
    const sngnn_epilogue_t *epi = c.epi;
    const int C = c.C;
    const float thr = c.thr;
    hipStream_t st = (hipStream_t)c.stream;
    const int top_k = std::min(c.top_k, 1 << 20);     // more than any row can use

    if (c.sel_src && top_k > 0 && c.row_flag == nullptr) {
        // (a kernel, not hipMemsetAsync: inside a captured HIP graph a memset node was seen to
        // race with the kernel nodes behind it on this stack - see agg_bwd_impl.h)
        const int64_t nw = g->N * (int64_t)top_k;
        k_fill_sel<<<(int)std::min<int64_t>((nw + 255) / 256, 2048), 256, 0, st>>>(c.sel_src, c.sel_w, nw);
    }

    FwdArgs a;
    a.n = n; a.nrm = nrm; a.C = C; a.N = (int)g->N; a.row_off = (int)g->row_off;
    // fp32 tables below 2 GiB are read through buffer resources (agg_fwd_src.h); the half path keeps the flat form
    const int64_t table_bytes = g->Ntot * (int64_t)C * (c.dtype == 0 ? 4 : 2);
    const bool buf = c.dtype == 0 && fwd_buffer_form(table_bytes, std::max<int64_t>(4 * g->Ep, 16 * g->N), g_addr_mode);
    a.Ntot = (int)g->Ntot; a.n_bytes = buf ? (unsigned)table_bytes : 0u;
    a.filt = nrm ? (const uint4 *)filt : nullptr;
    // (sngnn_filter_enable(2) forces it at any threshold: the tests' and the fuzz runs' way in)
    // (top_k >= 4: at top_k 1 the small-row form gains 1.5 us where it prunes - 39.3 -> 37.6-38.8 us at thr
    // 0.99 - and costs 13.6 us per call where it does not: the reference scripts' own knobs)
    // (a pruning threshold: every ranking row takes the filter, as before; by the graph's prunable share: long rows only)
    a.filt_min_deg = g_filt_min_deg >= 0 ? g_filt_min_deg : (thr >= 0.25f ? 0 : FILT_MIN_DEG);
    a.filt_small = (a.filt != nullptr && top_k >= 0 && g_filter_mode != 0 &&
                    ((thr >= 0.25f && top_k >= 4) || g_filter_mode == 2)) ? 1 : 0;
    // OTF (nrm == NULL, n = raw rows): bound on |fast cosine - reference-order cosine|.  Either
    // value is within (2 C + 8) u of the real cosine (u = 2^-24: C products and sums of the dot,
    // C / 2 + 3 for each norm, the scalings), so they differ by less than (4 C + 16) u; twice
    // the margin on the constant term.
    a.delta = (float)(4 * C + 32) * 5.9604644775390625e-8f;
    a.role_mask = g_role_mask;
    a.row_flag = c.row_flag; a.row_want = c.row_want;
    a.epi_flags = 0; a.epi_bias = nullptr; a.epi_keep = nullptr; a.epi_seed = nullptr; a.epi_p = 0.f; a.epi_scale = 1.0f;
    a.head_y = nullptr; a.head_sel = nullptr; a.head_part = nullptr; a.head_flags = 0; a.head_nmain = 0;
    a.head_scale = a.head_scale_b = 0.f; a.head_out = nullptr;
    a.kbits = nullptr; a.kb_wbase = (int)g->kb_wbase; a.kb_tbase = (int)g->kb_tbase;
    if (epi && epi->kept_bits) {
        SN_REQUIRE(sngnn::kept_bits_path(g, top_k) && c.row_flag == nullptr && nrm != nullptr, SNGNN_EINVAL,
                   "no kept-bit path for this graph / top_k (sngnn_agg_kept_bits_supported)");
        a.kbits = (unsigned *)epi->kept_bits;
    }
    const bool head = epi != nullptr && epi->head_y != nullptr;
    if (head) {
        SN_REQUIRE(cfg.vec == 4 && cfg.r == 1 && cfg.g <= 16, SNGNN_EINVAL,
                   "the head epilogue needs C % 4 == 0 and C <= 64 (sngnn_agg_head_supported)");
        SN_REQUIRE(epi->head_sel && epi->head_metrics && epi->head_workspace, SNGNN_EINVAL,
                   "head_sel / head_metrics / head_workspace is NULL");
        SN_REQUIRE(epi->head_sets == 1 || epi->head_sets == 2, SNGNN_EINVAL, "head_sets must be 1 or 2");
        SN_REQUIRE((epi->head_out_mode == 1 || epi->head_out_mode == 2) && (epi->head_out_mode != 2 || epi->head_sets == 1),
                   SNGNN_EINVAL, "head_out_mode: 1 logits, 2 gradient (one split only)");
        SN_REQUIRE(c.out != nullptr, SNGNN_EINVAL, "out is NULL");
        SN_REQUIRE(!epi->relu && epi->keep == nullptr && epi->seed == nullptr, SNGNN_EINVAL,
                   "the head follows the LAST layer: no relu / dropout with it");
        SN_REQUIRE(c.row_flag == nullptr && c.sel_src == nullptr, SNGNN_EINVAL,
                   "the head epilogue covers all rows of a call and emits no selection lists");
        a.head_y = epi->head_y; a.head_sel = epi->head_sel;
        a.head_part = (float *)epi->head_workspace; a.head_out = epi->head_metrics;
        a.head_flags = (epi->head_sets == 2 ? 1 : 0) | (epi->head_out_mode == 2 ? 2 : 0);
        a.head_scale = 1.0f / (float)(epi->head_n_a > 0 ? epi->head_n_a : 1);
        a.head_scale_b = 1.0f / (float)(epi->head_n_b > 0 ? epi->head_n_b : 1);
    }
    if (epi) {
        a.epi_bias = epi->bias; a.epi_keep = epi->keep;
        a.epi_seed = (const unsigned long long *)epi->seed; a.epi_p = epi->p;
        const bool drops = epi->keep != nullptr || epi->seed != nullptr;
        a.epi_scale = drops ? epi->keep_scale : 1.0f;
        a.epi_flags = (epi->relu ? 1 : 0) | (epi->bias ? 2 : 0) | (epi->keep ? 4 : (epi->seed ? 8 : 0));
    }
    // row order: calls that stream the small rows (deg <= SMALL_T <= top_k, or no top_k) take the
    // bucket order, calls that rank inside them the exact degree order (graph.hip 5b)
    const bool stream_small = top_k < 0 || top_k >= SMALL_T;
    a.rowptr = g->rowptr; a.col = g->col;
    a.col_s = stream_small ? g->col_s_b : g->col_s;
    a.rperm = stream_small ? g->rperm_b : g->rperm;
    a.rdesc = stream_small ? g->rdesc_b : g->rdesc;
    a.k = top_k < 0 ? -1 : top_k; a.thr = thr;
    a.out = (float *)c.out; a.wsel = c.wsel; a.inv_norm = c.inv_norm;
    a.sel_src = top_k > 0 ? c.sel_src : nullptr; a.sel_w = top_k > 0 ? c.sel_w : nullptr;
    bind_side(g, false, a);
    a.task_order = g->task_order;
    a.split_soff = g->split_soff;
    // the split rows' scratch (a prepared call on a graph without split rows may bring no workspace)
    const FwdLayout L = fwd_layout(g, C);
    char *ws = (char *)c.workspace;
    a.scores = ws ? (float *)(ws + L.scores) : nullptr;
    a.partial = ws ? (float *)(ws + L.partial) : nullptr;
    a.cand_key = ws ? (unsigned long long *)(ws + L.cand_key) : nullptr;
    a.cand_src = ws ? (int32_t *)(ws + L.cand_src) : nullptr;
    a.fin_done = ws ? (unsigned long long *)(ws + L.fin_done) : nullptr;
    a.fin_nonce = 0ull; a.main_blocks = 0; a.n_edges = (long long)g->Ep;
    a.k_magic = top_k >= 2 ? (unsigned)(0xFFFFFFFFu / (unsigned)top_k + 1u) : 0u;
    const int max_split = g->n_split ? g->rdeg[0] : 0;
    a.use_cand = fwd_use_candidates(a.k, C, max_split) ? 1 : 0;
    SN_REQUIRE(a.kbits == nullptr || a.use_cand, SNGNN_EINVAL,
               "no kept-bit path: this graph's biggest row takes the scratch-score finalize");
    // split rows whose (tasks * top_k) candidates exceed one 128-key wave selection
    // (no selection: split rows with more than 16 partial rows to add)
    a.n_split_gt_wave = top_k > 0 ? g->rows_gt((int64_t)(128 / std::min(top_k, 128)) * CHUNK)
                                  : (top_k < 0 ? g->rows_gt((int64_t)16 * CHUNK) : 0);
    a.lowbits = 1;
    while ((1ll << a.lowbits) < g->max_in_deg && a.lowbits < 31) ++a.lowbits;
    if (head) {
        SN_REQUIRE(g->n_split == 0 || a.use_cand, SNGNN_EINVAL,
                   "no head epilogue: this graph's biggest row takes the scratch-score finalize (sngnn_agg_head_supported)");
        // (the plain kernels: the head rides in the second launch)
        return buf ? launch_agg_fwd_buf_vec<4>(cfg, a, max_split, ev, st)
                   : launch_agg_fwd_vec<float, 4>(cfg, a, max_split, ev, st);
    }
    if (a.epi_flags != 0) {
        SN_REQUIRE(cfg.vec == 4, SNGNN_EINVAL, "the store epilogue needs C % 4 == 0 (16-byte rows)");
        return buf ? launch_agg_fwd_epi_buf_v4(cfg, a, max_split, ev, st)
                   : launch_agg_fwd_epi_v4(cfg, a, max_split, ev, st);
    }
    if (buf)
        return dispatch_vec(cfg, [&](auto vec) { return launch_agg_fwd_buf_vec<decltype(vec)::value>(cfg, a, max_split, ev, st); });
    // (the half path: n = the raw half rows, nrm == NULL, no epilogue / head / kept bits)
    return SNGNN_LAUNCH_VEC(launch_agg_fwd_vec, cfg, c.dtype, a, max_split, ev, st);
}

// whether a call uses the filter region of the workspace: rows that rank (in-degree > top_k) above the small
// class must exist, otherwise nothing would read the table
static bool use_filter(const sngnn_graph_t *g, int C, int top_k, float thr)
{
    if (g_filter_mode == 0 || top_k < 0 || filter_row_bytes(C) == 0) return false;
    // a pruning threshold: the small rows read the table too (FwdArgs::filt_small) - any graph
    if ((thr >= 0.25f && top_k >= 4) || g_filter_mode == 2) return true;
    if (thr >= 0.25f || g_filter_mode == 3) return g->rows_gt(std::max(top_k, SMALL_T)) != 0;
    // No threshold to prune with, but top_k itself prunes: a row of `deg` in-edges keeps at most top_k of them, yet
    // the unfiltered pass fetches the fp32 unit row (two lines for C in 36 .. 60) of every in-edge.  Measured in round
    // 5 (tools/filter_gate_sweep.py, profiles/r05_filter_gate.txt): with the filter on the rows above the small
    // class at thr 0 the forward takes 0.73-0.92 of its time on products' degree law at every size tried (unit-row
    // table 23 MiB .. 470 MB: 5.54 -> 4.16 ms main kernel at full size), 0.79-0.84 at uniform in-degree 50, 0.89-0.93 on
    // arxiv's law at 4x its edges - and 1.01-1.03 at arxiv's own size (the extra table costs the normalisation pass
    // 3 us, the main kernel gains 1).  The rule is the graph's PRUNABLE share: edges beyond top_k in rows of at
    // least FILT_MIN_DEG in-edges (shorter rows skip the filter: FwdArgs::filt_min_deg), over E', at top_k 16 / 4:
    // products 0.72 / 0.77, uniform 50 0.68 / 0.92, arxiv x4 0.64 / 0.69, arxiv x2 0.58 / 0.62 (0.98 / 0.97 of its time)
    // | arxiv 0.53 / 0.57.
    if (g->Ep > 0 && (double)g->prunable_edges(top_k, FILT_MIN_DEG) >= FILT_PRUNABLE_SHARE * (double)g->Ep) return true;
    // No threshold to prune with: the filter could still skip, in rows much longer than top_k, the edges
    // far below the k-th - round 3's rule was "on for top_k <= 8" (-7 us per forward at top_k 1 then).
    // Re-measured in round 4 (same box, arxiv size, C = 40, thr 0; filter on / off): top_k 1: 70.7 / 69.5
    // us per call, top_k 4: 73.6 / 70.9, top_k 8: 75.0 / 72.6 - the main kernel gains ~1 us, the extra table
    // costs the normalisation pass 3; and a model's later layers (nearly parallel rows: every edge a
    // candidate) lose more: 2- / 3-layer hidden-64 top_k-1 epochs 0.711 / 1.099 ms with, 0.703 / 1.052
    // without.  Hence: a selective threshold only.
    return false;
}

// Checks a call, decides where its unit rows and filter rows come from, and launches it.
static int run_forward(const FwdCall &c)
{
    const sngnn_graph_t *g = c.g;
    const sngnn_epilogue_t *epi = c.epi;
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    SN_REQUIRE(g->N == 0 || (c.rows != nullptr && c.out != nullptr), SNGNN_EINVAL, "h/out is NULL");
    RowCfg cfg;
    if (int rc = check_rows(c.C, c.dtype, {c.rows, c.out}, cfg)) return rc;
    SN_REQUIRE((c.sel_src == nullptr) == (c.sel_w == nullptr), SNGNN_EINVAL, "sel_src and sel_w go together");
    SN_REQUIRE(c.sel_src == nullptr || c.top_k >= 0, SNGNN_EINVAL, "sel_src needs top_k >= 0");
    hipStream_t st = (hipStream_t)c.stream;
    if (g->N == 0) {        // no row: zero head metrics, nothing else
        if (epi != nullptr && epi->head_y != nullptr && epi->head_metrics != nullptr)
            return launch_head_reduce(nullptr, 0, 0.f, 0.f, epi->head_sets == 2 ? 2 : 1, 4, epi->head_metrics, st);
        return SNGNN_OK;
    }
    // raw fp32 rows go through the unit-row table unless the call scores on the fly from h itself: no normalisation
    // pass, no table - the kernels gather h (FwdArgs).  The half rows always do (knob 2 = 2's form: the table path
    // would need a unit-row table of the half rows' fp32 values - a pass, and 4 C bytes per row where the rows have 2 C).
    const bool table = !c.prepared && c.dtype == 0 && !(g_table_mode == 2 || (g_table_mode == 0 && c.top_k < 0));
    // the filter decision (sngnn_agg_forward_rows leaves it to its caller - sngnn_filter_wanted - who passes the rows
    // or NULL; a call that scores on the fly has no table to filter)
    const bool pays = (table || (c.prepared && !c.by_rows)) && use_filter(g, c.C, c.top_k, c.thr);
    const bool filter = pays && !(epi && epi->no_filter);
    if (c.by_rows) {
        // (nrm == NULL: rows holds the RAW rows h and the call scores on the fly, like sngnn_agg_forward)
        SN_REQUIRE(c.row_flag != nullptr && c.workspace != nullptr, SNGNN_EINVAL, "row_flag/workspace is NULL");
        SN_REQUIRE(c.nrm != nullptr || c.filt == nullptr, SNGNN_EINVAL, "filter rows go with unit rows + norms");
    } else if (c.prepared) {
        SN_REQUIRE(c.nrm != nullptr, SNGNN_EINVAL, "nrm is NULL");
        SN_REQUIRE(c.workspace != nullptr || (g->n_tasks == 0 && (c.filt != nullptr || !pays)), SNGNN_EINVAL,
                   "workspace is NULL");
    } else {
        SN_REQUIRE(c.workspace != nullptr, SNGNN_EINVAL, "workspace is NULL");
    }
    if (c.prepared) {
        SN_REQUIRE(c.filt == nullptr || filter_row_bytes(c.C) > 0, SNGNN_EINVAL,
                   "no filter rows for this C (sngnn_filter_row_bytes(C) == 0)");
        SN_REQUIRE(((uintptr_t)c.filt % 16) == 0, SNGNN_EINVAL, "filt must be 16-byte aligned");
    }
    // the same workspace layout for every entry; a prepared call leaves the unit-row region unused
    const FwdLayout L = fwd_layout(g, c.C);
    char *ws = (char *)c.workspace;
    hipEvent_t *ev = (g_prof_on && !c.by_rows) ? g_prof_ev : nullptr;
    if (ev) SN_HIP(hipEventRecord(ev[0], st));
    const float *n = (const float *)c.rows, *nrm = c.nrm;
    const void *filt = c.by_rows ? c.filt : nullptr;
    if (table) {
        // (sngnn_tuning_set(2, 1) forces it) the normalisation pass first
        float *unit = (float *)(ws + L.unit), *norms = (float *)(ws + L.nrm);
        void *wf = filter ? ws + L.filt : nullptr;
        for (int rep = 0; rep < (ev ? g_prof_reps : 1); ++rep)
            if (int rc = normalize_dispatch(cfg, n, g->Ntot, c.C, unit, norms, wf, st)) return rc;
        n = unit; nrm = norms; filt = wf;
    } else if (filter) {
        filt = c.filt;
        if (!filt) {       // the caller holds no filter rows: one more pass over its unit rows
            if (int rc = launch_filter_v4(cfg, n, g->Ntot, c.C, ws + L.filt, st)) return rc;
            filt = ws + L.filt;
        }
    }
    return launch_forward(c, cfg, n, nrm, filt, ev ? ev + 1 : nullptr);
}

extern "C" int sngnn_agg_forward(const sngnn_graph_t *g, const float *h, int C, int top_k,
                                 float thr, float *out, float *wsel, float *inv_norm,
                                 int32_t *sel_src, float *sel_w, void *workspace, void *stream)
{
    FwdCall c;
    c.g = g; c.rows = h; c.C = C; c.top_k = top_k; c.thr = thr; c.out = out; c.wsel = wsel; c.inv_norm = inv_norm;
    c.sel_src = sel_src; c.sel_w = sel_w; c.workspace = workspace; c.stream = stream;
    return run_forward(c);
}

// The half path: h and out stored as fp16 / bf16, always scored on the fly.
extern "C" int sngnn_agg_forward_half(const sngnn_graph_t *g, const void *h, int dtype, int C, int top_k, float thr,
                                      void *out, float *wsel, float *inv_norm, int32_t *sel_src, float *sel_w,
                                      void *workspace, void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    FwdCall c;
    c.g = g; c.rows = h; c.dtype = dtype; c.C = C; c.top_k = top_k; c.thr = thr; c.out = out; c.wsel = wsel;
    c.inv_norm = inv_norm; c.sel_src = sel_src; c.sel_w = sel_w; c.workspace = workspace; c.stream = stream;
    return run_forward(c);
}

extern "C" int64_t sngnn_agg_head_workspace_bytes(const sngnn_graph_t *g)
{
    // one 16-byte entry per wave of the head role and per split row
    return g ? ((int64_t)HEAD_ROLE_WAVES_MAX + g->n_split) * 16 + 256 : 0;
}

extern "C" int sngnn_agg_head_supported(const sngnn_graph_t *g, int C, int top_k)
{
    RowCfg cfg;
    if (g == nullptr || !row_cfg(C, cfg) || cfg.vec != 4 || cfg.r != 1 || cfg.g > 16) return 0;
    const int max_split = g->n_split ? g->rdeg[0] : 0;
    return (g->n_split == 0 || fwd_use_candidates(top_k < 0 ? -1 : top_k, C, max_split)) ? 1 : 0;
}

static int check_epilogue(const sngnn_epilogue_t *epi)
{
    SN_REQUIRE(epi != nullptr, SNGNN_EINVAL, "epilogue is NULL");
    SN_REQUIRE((epi->keep == nullptr && epi->seed == nullptr) || (epi->keep_scale > 0.f && epi->keep_scale < 1e30f),
               SNGNN_EINVAL, "keep_scale must be a positive finite number (1 / (1 - p))");
    SN_REQUIRE(epi->seed == nullptr || (epi->p >= 0.f && epi->p < 1.f), SNGNN_EINVAL, "p must be in [0, 1)");
    return SNGNN_OK;
}

extern "C" int sngnn_agg_forward_epilogue(const sngnn_graph_t *g, const float *h, int C, int top_k, float thr,
                                          const sngnn_epilogue_t *epi, float *out, float *wsel, float *inv_norm,
                                          void *workspace, void *stream)
{
    if (int rc = check_epilogue(epi)) return rc;
    FwdCall c;
    c.g = g; c.rows = h; c.C = C; c.top_k = top_k; c.thr = thr; c.epi = epi; c.out = out; c.wsel = wsel;
    c.inv_norm = inv_norm; c.workspace = workspace; c.stream = stream;
    return run_forward(c);
}

extern "C" int sngnn_agg_forward_prepared(const sngnn_graph_t *g, const float *n, const float *nrm,
                                          const void *filt, int C, int top_k, float thr, float *out, float *wsel,
                                          float *inv_norm, int32_t *sel_src, float *sel_w, void *workspace,
                                          void *stream)
{
    FwdCall c;
    c.g = g; c.rows = n; c.prepared = true; c.nrm = nrm; c.filt = filt; c.C = C; c.top_k = top_k; c.thr = thr;
    c.out = out; c.wsel = wsel; c.inv_norm = inv_norm; c.sel_src = sel_src; c.sel_w = sel_w;
    c.workspace = workspace; c.stream = stream;
    return run_forward(c);
}

extern "C" int sngnn_agg_forward_prepared_epilogue(const sngnn_graph_t *g, const float *n, const float *nrm,
                                                   const void *filt, int C, int top_k, float thr,
                                                   const sngnn_epilogue_t *epi, float *out, float *wsel,
                                                   float *inv_norm, void *workspace, void *stream)
{
    if (int rc = check_epilogue(epi)) return rc;
    FwdCall c;
    c.g = g; c.rows = n; c.prepared = true; c.nrm = nrm; c.filt = filt; c.C = C; c.top_k = top_k; c.thr = thr;
    c.epi = epi; c.out = out; c.wsel = wsel; c.inv_norm = inv_norm; c.workspace = workspace; c.stream = stream;
    return run_forward(c);
}

extern "C" int sngnn_agg_forward_rows(const sngnn_graph_t *g, const float *n, const float *nrm, const void *filt,
                                      int C, int top_k, float thr, const uint8_t *row_flag, int row_want,
                                      float *out, float *wsel, float *inv_norm, void *workspace, void *stream)
{
    FwdCall c;
    c.g = g; c.rows = n; c.prepared = true; c.nrm = nrm; c.filt = filt; c.by_rows = true; c.row_flag = row_flag;
    c.row_want = row_want; c.C = C; c.top_k = top_k; c.thr = thr; c.out = out; c.wsel = wsel; c.inv_norm = inv_norm;
    c.workspace = workspace; c.stream = stream;
    return run_forward(c);
}

// (the forward side of the question: split rows must take the candidate finalize, whose winners set their bits)
extern "C" int sngnn_agg_kept_bits_supported(const sngnn_graph_t *g, int C, int top_k)
{
    if (!sngnn::kept_bits_path(g, top_k)) return 0;
    return fwd_use_candidates(top_k, C, g->n_split ? g->rdeg[0] : 0) ? 1 : 0;
}

extern "C" int sngnn_filter_wanted(const sngnn_graph_t *g, int C, int top_k, float thr)
{
    return g != nullptr && use_filter(g, C, top_k, thr) ? 1 : 0;
}

extern "C" int sngnn_agg_forward_normalized(const sngnn_graph_t *g, const float *n, const float *nrm, int C,
                                            int top_k, float thr, float *out, float *wsel, float *inv_norm,
                                            int32_t *sel_src, float *sel_w, void *workspace, void *stream)
{
    return sngnn_agg_forward_prepared(g, n, nrm, nullptr, C, top_k, thr, out, wsel, inv_norm, sel_src, sel_w,
                                      workspace, stream);
}

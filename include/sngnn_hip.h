/*
 * sngnn_hip.h - C ABI of the MI355X (gfx950) implementation of SNGNN's
 * similarity-navigated aggregation path.
 *
 * The reference (MinhZou/SNGNN) is pure Python and has no FFI of its own; the
 * seam this library replaces is the body of the three conv layers'
 * ``forward(x, edge_index)`` after ``self.lin`` (models/models.py:116-137,
 * 233-242, 322-329) together with their ``message`` hooks (:139-158, :244-263,
 * :331-334) and the third-party calls underneath them (PyG propagate /
 * add_self_loops / remove_self_loops, torch_scatter.scatter_max / scatter(mean),
 * torch_sparse.SparseTensor) - plus the Sim-GFA toolbox's cosine statistics
 * (SimGFAToolbox/dense.py:138-179).  Each entry point cites the reference lines
 * it stands in for.  INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every pointer marked "dev" is a device (HBM) pointer; nothing here takes
 *     or returns a torch type;
 *   - fp32 values, row-major, dense (leading dimension == number of columns);
 *   - ``stream`` is a hipStream_t passed as void* (NULL = the null stream);
 *     forward/backward entry points only enqueue work: no allocation, no host
 *     synchronisation, safe to capture in a hipGraph;
 *   - every ``workspace`` (and ``head_workspace``) is dev scratch of the bytes the entry's ``*_workspace_bytes``
 *     function returns for the same arguments: the call reads and writes only inside those bytes, its contents on
 *     entry are unspecified (no result depends on them) and on return they mean nothing to the caller; one buffer
 *     must not be shared by calls that may run concurrently (two streams);
 *   - every function returns 0 on success or a negative SNGNN_E* code;
 *     sngnn_last_error() gives the message of the calling thread's last failure.
 */
#ifndef SNGNN_HIP_H
#define SNGNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNGNN_OK            0
#define SNGNN_EINVAL       -1   /* bad argument (NULL, negative size, C unsupported) */
#define SNGNN_ERANGE       -2   /* node id outside [0, N) in edge_index            */
#define SNGNN_EHIP         -3   /* a HIP runtime call failed                       */
#define SNGNN_ENOMEM       -4   /* allocation failed                               */

/* weight value stored for an edge that was NOT selected (training-mode output
 * of sngnn_agg_forward); a selected edge stores its cosine, which is > -1.1 */
#define SNGNN_UNSELECTED   (-4.0f)

/* largest supported number of channels per node row */
#define SNGNN_MAX_CHANNELS  512

const char *sngnn_last_error(void);
/* "gfx950;rocm-x.y;..." build identification */
const char *sngnn_build_info(void);

/* ------------------------------------------------------------------------
 * Graph structure (built once per edge_index / self-loop mode and cached by
 * the caller; the reference redoes this work on every forward).
 * ------------------------------------------------------------------------ */
typedef struct sngnn_graph sngnn_graph_t;

/*
 * Replaces: add_self_loops + remove_self_loops (models.py:117-120, 234-236,
 * 323) and the COO->per-target grouping that PyG's propagate / torch_scatter
 * perform implicitly on every call (models.py:132, 239, 326).
 *
 *   edge_index_dev  int64 [2, E] row-major (row 0 = source, row 1 = target),
 *                   exactly what the reference passes as ``edge_index``
 *   add_loops       append (v, v) for every v at the END of the list
 *   remove_loops    1: then drop EVERY edge with src == dst (so add+remove == remove)
 *                   2 (SNGNN_LOOPS_REPLACE): drop the ORIGINAL loops first, then
 *                   append - AGNNConv's order (models.py:393-395)
 *
 * The resulting list of E' edges keeps the reference's order; the library
 * stores it as CSR by target with the original relative order inside each row
 * (stable), which is what makes "first occurrence wins a tie" reproducible.
 * Synchronises the stream (one-time setup).
 */
#define SNGNN_LOOPS_REPLACE 2
int sngnn_graph_create(const int64_t *edge_index_dev, int64_t E, int64_t N,
                       int add_loops, int remove_loops, void *stream,
                       sngnn_graph_t **out_graph);
/*
 * Node-range partition of a larger graph (one process per GPU): this graph owns
 * the target rows [row_begin, row_end) of an N_total-node graph.  edge_index
 * holds GLOBAL node ids; edges whose target lies outside the owned range are
 * dropped, self-loops are appended for the owned nodes only.  Feature tables
 * handed to forward/backward then have N_total rows (the all-gathered h), the
 * outputs row_end - row_begin rows.  The reference has no counterpart (it is
 * single-device); with row range [0, N) this is sngnn_graph_create.
 */
int sngnn_graph_create_partition(const int64_t *edge_index_dev, int64_t E,
                                 int64_t N_total, int64_t row_begin,
                                 int64_t row_end, int add_loops, int remove_loops,
                                 void *stream, sngnn_graph_t **out_graph);
void sngnn_graph_destroy(sngnn_graph_t *g);

int64_t sngnn_graph_num_nodes(const sngnn_graph_t *g);       /* owned target rows */
int64_t sngnn_graph_num_total_nodes(const sngnn_graph_t *g); /* N_total            */
int64_t sngnn_graph_row_offset(const sngnn_graph_t *g);      /* row_begin          */
int64_t sngnn_graph_num_edges(const sngnn_graph_t *g);      /* E' */
int64_t sngnn_graph_max_in_degree(const sngnn_graph_t *g);
int64_t sngnn_graph_src_min(const sngnn_graph_t *g);         /* models.py:125 */
/* owned nodes with in-degree and out-degree <= 16: the one-work-item nodes of the node-centric
 * backward, which sngnn_agg_backward* takes when they are at least half of the owned nodes */
int64_t sngnn_graph_num_fused_nodes(const sngnn_graph_t *g);
/* bytes of device workspace sngnn_agg_forward/backward need for C channels */
int64_t sngnn_graph_workspace_bytes(const sngnn_graph_t *g, int C);

/* Copy one of the graph's arrays to host memory (tests / inspection).
 *   which: 0 rowptr   int32 [N+1]   CSR by target
 *          1 col      int32 [E']    source id of each CSR edge
 *          2 eid      int32 [E']    position of the CSR edge in the E' edge list
 *          3 cscptr   int32 [N_total+1]  CSC by source
 *          4 csc_eid  int32 [E']    CSR edge index of each CSC entry
 *          5 rperm    int32 [N]     rows sorted by in-degree, descending (stable)
 *          6 csc_dst  int32 [E']    local target row of each CSC entry
 *          7 csc_pos  int32 [E']    CSC position of each CSR edge (inverse of csc_eid)
 *          8 sperm    int32 [N_total]  sources by out-degree class, descending (stable): out-degree above 16,
 *                                   then the small sources that are not fused, then the fused nodes
 *          9 rdesc    int4  [N]     per slot of rperm: {row, first CSR edge, in-degree, first entry in col_s}
 *         10 col_s    int32 [E']    col with the rows in rperm's slot order
 *         11 rperm_b  int32 [N]     rows by in-degree above 16, else by bucket of 4 degrees; descending (stable)
 *         12 rdesc_b  int4  [N]     rdesc of that order (.w: first entry in col_s_b)
 *         13 col_s_b  int32 [E']    col with the rows in rperm_b's slot order
 *         14 sdesc    int4  [N_total]  per slot of sperm: {source, first CSC entry, out-degree, 0}
 *         15 fdesc    int4  [fused nodes]  natural order: {node, first CSR edge, first CSC entry,
 *                                   in-degree | out-degree << 8}
 *         16 trest    int4  [..]    owned rows with in-degree <= 16 and out-degree > 16, natural order:
 *                                   {row, first CSR edge, in-degree, 0}
 *         17 task_slot, 18 task_chunk  int32 [tasks]  one task per 128 edges of a row with in-degree > 128
 *                                   (slot of rperm, chunk inside the row), in slot order
 *         19 task_order int32 [tasks]  the order in which the forward deals those tasks (a permutation)
 *         20 split_soff, 21 split_task0  int32 [split rows + 1]  running edge / task counts of those rows
 *         22 stask_slot, 23 stask_chunk  int32 [source tasks]  the same for sources with out-degree > 128
 *         24 ssplit_task0  int32 [split sources + 1]
 *         25 csc_bit  int32 [E']    bit index of each CSC entry's edge in the kept-bit layout; length 0
 *                                   where the layout was not built (a partition, a graph without edges)
 *         26 inv_deg  float [N]     1 / max(in-degree, 1)
 * Ids 11..13 have length 0 for a graph without owned rows.
 */
int sngnn_graph_copy_array(const sngnn_graph_t *g, int which, void *host_dst);
/* device pointer to the same arrays (owned by the graph) */
const void *sngnn_graph_array_dev(const sngnn_graph_t *g, int which);
/* length of array `which` in 4-byte elements (an int4 descriptor counts as four); 0 for an array that
 * was not built, -1 for an unknown id */
int64_t sngnn_graph_array_len(const sngnn_graph_t *g, int which);

/* ------------------------------------------------------------------------
 * Fused aggregation:  F.normalize + per-edge cosine + top-k/threshold
 * selection + similarity-weighted scatter-mean.
 * ------------------------------------------------------------------------ */
/*
 * Replaces: models.py:122+132+139-158 (SNConv_plus_plus, the out_1 branch),
 * :238-239+244-263 (SNConv_plus), :325-326+331-334 (SNConv) and, underneath,
 * PyG propagate's four index_select gathers, torch_scatter.scatter_max (x top_k
 * rounds) and torch_scatter.scatter(reduce='mean').
 *
 *   h        dev f32 [N_total, C]  output of self.lin (NOT normalised); N_total == N
 *                             unless the graph is a partition
 *   top_k    < 0: SNConv - every edge weighted by its cosine, no selection
 *            >= 0: keep, per target, the top_k in-edges by (cosine descending,
 *            edge position ascending) and of those only the ones with
 *            cosine >= (float)thr; all other edges get weight 0
 *   out      dev f32 [N, C]   (1 / max(indeg', 1)) * sum_e weight_e * h[src_e]
 *                             (the mean divides by the FULL in-degree)
 * Optional outputs (NULL to skip):
 *   wsel     dev f32 [E']     per CSR edge: its cosine if selected, else
 *                             SNGNN_UNSELECTED (saved for backward)
 *   inv_norm dev f32 [N]      1 / max(||h_i||_2, 1e-12)
 *   sel_src  dev i32 [N, top_k]  selected source ids in rank order, -1 padded
 *   sel_w    dev f32 [N, top_k]  their cosines (0 padded)
 *   workspace dev, sngnn_graph_workspace_bytes(g, C) bytes (may be NULL when
 *            that is 0)
 */
int sngnn_agg_forward(const sngnn_graph_t *g, const float *h, int C, int top_k,
                      float thr, float *out, float *wsel, float *inv_norm,
                      int32_t *sel_src, float *sel_w, void *workspace,
                      void *stream);

/*
 * The two halves of sngnn_agg_forward, for a caller that already holds the unit rows
 * (e.g. produced by the epilogue of its own ``lin``) or wants them.
 *
 * sngnn_normalize_rows replaces F.normalize(x, p=2, dim=-1) (models.py:122,238,325):
 *   n[r, :] = h[r, :] / max(||h[r, :]||_2, 1e-12),  nrm[r] = that clamped norm,
 * IEEE square root and division, so rows that the reference normalises to the same
 * bits (duplicates, power-of-two multiples, rows with a single non-zero channel) get the
 * same bits here and their cosines tie exactly as in the reference.
 *   h, n  dev f32 [rows, C];  nrm dev f32 [rows]
 *
 * sngnn_agg_forward_normalized is sngnn_agg_forward on (n, nrm) of the N_total feature
 * rows: the per-edge cosine is <n_i, n_j>, a kept message is cosine * nrm_j * n_j
 * (= cosine * h_j to half an ulp).  Same workspace size and optional outputs.
 */
int sngnn_normalize_rows(const float *h, int64_t rows, int C, float *n, float *nrm,
                         void *stream);
/*
 * Filter rows (no reference counterpart; csrc/agg_fwd_filter.h).  For C % 4 == 0, C > 32 the
 * selecting forward first scores the edges of a row with more than top_k in-edges against an
 * fp16 copy of the unit rows, one 128-byte-aligned entry of sngnn_filter_row_bytes(C) bytes per
 * node, and fetches the fp32 unit row only of the edges that can still be among the top_k
 * (approximate cosine within a proven bound of the k-th); the selection itself is made on exact
 * fp32 cosines, so indices and weights are those of the unfiltered path, bit for bit.
 * sngnn_filter_row_bytes returns 0 when the filter is not used for this C.
 * sngnn_normalize_rows_filter is sngnn_normalize_rows that also writes the filter rows
 * (filt: dev, rows * sngnn_filter_row_bytes(C) bytes, 16-byte aligned; NULL to skip).
 * sngnn_agg_forward_prepared is sngnn_agg_forward_normalized for a caller that holds them
 * (filt == NULL: they are built inside the workspace by one more pass over n).
 * sngnn_filter_enable(mode): 0 = never, 1 = when it is expected to pay (default: a selective
 * threshold, thr >= 0.25; round 3 also switched it on for top_k <= 8: re-measured, it no longer pays there),
 * 2 = whenever it applies (the small rows' two-phase form too), 3 = for the rows above the small class
 * (wave rows, split-row tasks) at any threshold (measurement: the regime where the unit-row table does not
 * fit the Infinity Cache).  Results do not depend on it.
 */
int64_t sngnn_filter_row_bytes(int C);
int sngnn_normalize_rows_filter(const float *h, int64_t rows, int C, float *n, float *nrm,
                                void *filt, void *stream);
int sngnn_agg_forward_prepared(const sngnn_graph_t *g, const float *n, const float *nrm,
                               const void *filt, int C, int top_k, float thr, float *out,
                               float *wsel, float *inv_norm, int32_t *sel_src, float *sel_w,
                               void *workspace, void *stream);

/*
 * The forward with a hidden layer's store epilogue.  Replaces, on top of sngnn_agg_forward /
 * sngnn_agg_forward_prepared: the elementwise passes the reference runs between two conv layers
 * (models.py:204-209 / :79-84 / :296-301): `out + self.bias` (:135-136, 240-241, 327-328),
 * `F.relu(x, inplace=True)` and, in training, `self.dropout(x)` - applied to each finished mean row
 * on its way out instead of three more passes over [N, C]:
 *     out[i, c] = keep[i, c] ? max(mean[i, c] + bias[c], 0) * keep_scale : 0
 * bias NULL: none; relu 0: none; keep NULL and seed NULL: no dropout (evaluation, or p == 0).  keep
 * is the caller's own Bernoulli(1 - p) draw, uint8 [N, C]; or seed (a device counter) lets the
 * kernel draw it; keep_scale = 1 / (1 - p) either way.  C % 4 == 0.  The mask the backward
 * needs is out > 0 (times keep_scale): nothing else has to be saved (sngnn_linear_forward_masked).
 * (No batch norm in between: models.py:207-208's bn stays a layer of its own.)
 */
typedef struct sngnn_epilogue {
    const float *bias;
    const unsigned char *keep;
    float keep_scale;
    int relu;
    const void *seed;       /* dev uint64 [1] or NULL (with keep == NULL): draw the keep mask in the kernel, */
    float p;                /* keep[i, c] = u(seed, i * C + c) >= p, u a counter-based uniform: the same     */
                            /* seed gives the same mask; the caller advances the seed between forwards       */
    void *kept_bits;        /* dev, sngnn_graph_kept_bits_bytes(g) bytes, or NULL: training calls - the      */
                            /* forward writes WHICH edges it kept as packed bits (its own layout) for        */
                            /* sngnn_agg_backward_bits, instead of wsel + a packing launch in the backward;  */
                            /* only where sngnn_agg_kept_bits_supported(g, top_k); an all-zero struct with   */
                            /* this field set is a plain forward that saves the bits                         */
    /* The classification head of the LAST layer inside the forward's own launches (round 4; NULL
     * head_y = off): what the wrappers do to the last conv's output - log_softmax (models.py:86,211,
     * 303) - and what the harness does to that - nll_loss on a mask and the accuracy count
     * (train.py:81-84, 98-102, 112-116).  The rows go through it in the forward's SECOND launch: the
     * split rows in their finalize, all others read back by extra workgroups of that launch, which is
     * otherwise a latency chain on an idle chip - instead of two more launches behind it
     * (sngnn_head_nll / _nll2, which compute the same per-row bits).  `bias` (the conv's) is added
     * first; relu / keep / seed must be off.  Needs sngnn_agg_head_supported.                        */
    const int64_t *head_y;          /* dev int64 [N] labels                                                      */
    const unsigned char *head_sel;  /* dev u8 [N]: head_sets == 1: != 0 marks the split's rows; == 2: bit 0 = in */
                                    /* split A, bit 1 = in split B (validation and test off ONE forward)          */
    int head_sets;                  /* 1 or 2                                                                    */
    int head_out_mode;              /* what `out` holds afterwards: 1 the logits (mean rows + bias), 2 d(mean    */
                                    /* NLL of the split) / d logits, zero rows outside it (head_sets == 1):     */
                                    /* the tensor the backward starts from                                     */
    int64_t head_n_a, head_n_b;     /* rows in split A / B: the means' denominators                              */
    float *head_metrics;            /* dev f32 [2 * head_sets]: (mean NLL, correct count) per split              */
    void *head_workspace;           /* dev, sngnn_agg_head_workspace_bytes(g) bytes                              */
    int no_filter;                  /* != 0: this call does not use the fp16 filter whatever sngnn_filter_enable */
                                    /* would decide - the caller knows its rows (nearly parallel ones all pass   */
                                    /* the threshold: nothing to prune, the filter is a pass for nothing)       */
} sngnn_epilogue_t;
int64_t sngnn_agg_head_workspace_bytes(const sngnn_graph_t *g);
/* 1 if a forward on this graph at this width / top_k can take the head epilogue (C % 4 == 0, C <= 64, the
 * split rows on the candidate finalize), else 0 */
int sngnn_agg_head_supported(const sngnn_graph_t *g, int C, int top_k);
int sngnn_agg_forward_epilogue(const sngnn_graph_t *g, const float *h, int C, int top_k, float thr,
                               const sngnn_epilogue_t *epi, float *out, float *wsel, float *inv_norm,
                               void *workspace, void *stream);
int sngnn_agg_forward_prepared_epilogue(const sngnn_graph_t *g, const float *n, const float *nrm,
                                        const void *filt, int C, int top_k, float thr,
                                        const sngnn_epilogue_t *epi, float *out, float *wsel,
                                        float *inv_norm, void *workspace, void *stream);
int sngnn_filter_enable(int mode);
/* whether sngnn_agg_forward would use filter rows for this call (a caller that prepares the
 * rows itself writes them only then) */
int sngnn_filter_wanted(const sngnn_graph_t *g, int C, int top_k, float thr);
/*
 * sngnn_agg_forward_prepared restricted to the target rows i with row_flag[i] == row_want
 * (row_flag: dev u8 [N]); the other rows of out / wsel / inv_norm are not touched.  Two calls
 * with complementary flags equal one unrestricted call, bit for bit.  One rank of a node-range
 * partition aggregates its INTERIOR rows (all sources local) while the halo rows its other
 * rows need are still in flight (sngnn_amd/dist.py).  No reference counterpart.
 */
int sngnn_agg_forward_rows(const sngnn_graph_t *g, const float *n, const float *nrm,
                           const void *filt, int C, int top_k, float thr,
                           const uint8_t *row_flag, int row_want, float *out, float *wsel,
                           float *inv_norm, void *workspace, void *stream);
/* measurement aid: knob 0 = row classes the main forward kernel runs (bit 0 split-row tasks,
 * 1 wave rows, 2 small rows; default 7 - anything else leaves the output incomplete);
 * knob 2 = how sngnn_agg_forward scores: 0 (default) = on the fly from h when nothing is selected
 * (top_k < 0) and through the normalisation pass + unit-row table otherwise; 1 = table always;
 * 2 = on the fly always (fast cosine, exact normalise-then-dot wherever a decision is in doubt:
 * the same selections, bit for bit);
 * knob 3 = sngnn_agg_backward: 0 (default) = node-centric (a node small both as target and as
 * source does both passes in one work item; with a top_k hint every node) on graphs where such
 * nodes are at least half of the owned nodes, the two passes otherwise; 1 = the two passes for
 * every node (same bits without the hint; equal to rounding on split rows with it); 2 =
 * node-centric whatever the graph;
 * knob 4 = which items the hinted node-centric backward runs (bit 0 wave-per-node, bit 1 fused;
 * default 3 - anything else leaves grad_h incomplete: timing only);
 * knob 5 = sngnn_linear_forward*, sngnn_cosine_dense, sngnn_knn_graph, sngnn_knn_query: 0 (default) = products on the bf16 matrix
 * cores after an exact three-way split of both operands (fp32 accumulation, an fp32 contraction's
 * rounding), 1 = fp32 MFMAs;
 * knobs 6, 7, 8 = the kNN builder's route, the dense cosine's contraction split, the in-degree below which a wave row
 * skips the fp16 filter (csrc/knn.hip, toolbox.hip, agg_fwd.hip);
 * knob 9 = where the split rows (in-degree > 128) of sngnn_agg_forward* are finalized: 1 (default) = inside the main
 * launch - by its last workgroups, each row as soon as its tasks have published their candidates - when that
 * chain of round trips fits under the launch's own time (arxiv-sized graphs and up; calls that rank from
 * candidates, no head epilogue), else in a launch of its own; 0 = always a launch of its own; v > 1 = inside the
 * main launch on v workgroups.  Same selections and kept weights either way; the rows' sums agree bit for bit for
 * rows of at most 128 candidates and to rounding (another summation order) for the bigger ones;
 * knob 10 = copies of sngnn_cosine_hist's counter table in LDS (see there);
 * knob 11 = how the forward's work-item roles address what they gather (table rows, norms, column ids, filter rows):
 * 0 (default) = through buffer resources with 32-bit offsets when the fp32 table has fewer than 2^31 bytes (slots and
 * lanes nobody reads get an out-of-range offset: zeros, no request), the flat form otherwise; 1 = the flat form
 * (64-bit pointers) always.  The same bits either way - the A/B of a measurement, and the path of bigger tables;
 * knob 12 = which main kernel a forward that asks for `out` only runs (wsel, inv_norm, sel_src, sel_w and kept bits
 * NULL, no epilogue, no head, no row filter; fp32 rows scored from the unit-row table without the fp16 filter):
 * 0 (default) = the lean instantiation, which compiles the code of those outputs out of every role; 1 = the general
 * kernel always.  The same bits either way - the A/B of a measurement and of tests/test_fwd_lean_gpu.py. */
int sngnn_tuning_set(int which, int value);
/* how many workgroups of the last sngnn_agg_forward* launch on this process finalized split rows (0 = the
 * finalize was a launch of its own, or there was nothing to finalize) - measurement aid, see knob 9 */
int sngnn_last_forward_finalize_workgroups(void);
/* test aid: out[p] = the filter pass's approximate cosine of nodes pair_a[p], pair_b[p] (dev i64) */
int sngnn_filter_pair_scores(const void *filt, int C, const int64_t *pair_a, const int64_t *pair_b,
                             int64_t n_pairs, float *out, void *stream);
int sngnn_agg_forward_normalized(const sngnn_graph_t *g, const float *n, const float *nrm,
                                 int C, int top_k, float thr, float *out, float *wsel,
                                 float *inv_norm, int32_t *sel_src, float *sel_w,
                                 void *workspace, void *stream);

/*
 * Replaces: autograd through the op list above (triggered at train.py:86).
 * Deterministic: no floating-point atomics; every sum has a fixed order.
 *
 *   grad_out dev f32 [N, C]        dL/d out
 *   wsel                           as written by sngnn_agg_forward on the same h (only WHICH
 *                             edges were kept is read from it; the cosines are recomputed from
 *                             the rows the passes gather anyway)
 *   grad_h   dev f32 [N_total, C]  dL/d h through all three routes (message
 *                             value, norm_i, norm_j) and F.normalize's Jacobian.
 *                             For a partition this is the rank's PARTIAL gradient
 *                             (sum over ranks = reduce-scatter gives the total).
 */
int sngnn_agg_backward(const sngnn_graph_t *g, const float *h, int C,
                       const float *grad_out, const float *wsel, float *grad_h,
                       void *workspace, void *stream);
/* The same with the forward's top_k passed along (<= 0: unknown, == sngnn_agg_backward).  A
 * top_k in [1, 128] promises at most that many kept in-edges per row, which lets one wave take a
 * whole target row of any in-degree (kept edges found by scanning the packed kept bits): one
 * launch for all nodes, no split-row partial sums.  The result does not depend on the promise
 * being true (an over-full row is processed in pieces), only the speed does. */
int sngnn_agg_backward_topk(const sngnn_graph_t *g, const float *h, int C,
                            const float *grad_out, const float *wsel, int top_k, float *grad_h,
                            void *workspace, void *stream);
/* The same from the kept bits a forward wrote itself (sngnn_epilogue_t.kept_bits): no packing
 * launch in front.  sngnn_agg_kept_bits_supported: whole graph, 1 <= top_k <= 16, a graph on which
 * the backward is the node-centric one (most nodes small as target and as source) and whose
 * biggest row's candidates fit the finalize at this C.  The gradient
 * equals sngnn_agg_backward_topk's on the same forward, bit for bit. */
int sngnn_agg_kept_bits_supported(const sngnn_graph_t *g, int C, int top_k);
int64_t sngnn_graph_kept_bits_bytes(const sngnn_graph_t *g);
int sngnn_agg_backward_bits(const sngnn_graph_t *g, const float *h, int C, const float *grad_out,
                            const void *kept_bits, int top_k, float *grad_h, void *workspace, void *stream);

/*
 * Half-width feature rows: the aggregation on fp16 or bf16 h, forward and backward.
 * Replaces the same reference lines as sngnn_agg_forward / sngnn_agg_backward_topk (models.py:122+132+139-158,
 * :238-239+244-263, :325-326+331-334 and autograd through them, train.py:86) for a model cast to
 * torch.float16 / torch.bfloat16 - but NOT their eager arithmetic in that type, which would round the unit rows and
 * the cosines to 11 or 8 bits and create spurious ties.  Contract, with hf = h widened to fp32 (exact):
 *   forward:  the fp32 operator on hf, scoring on the fly (sngnn_tuning_set(2, 2): sngnn_agg_forward scores the
 *             raw rows, no unit-row table), with only `out` rounded once to the storage type (round to nearest
 *             even).  wsel, inv_norm, sel_src and sel_w stay fp32 and equal that call's bit for bit, exact ties
 *             included; the kept edges are those of the default sngnn_agg_forward on hf.
 *   backward: sngnn_agg_backward_topk(hf, grad_out widened, wsel, top_k) rounded once to the storage type.
 * The kernels are the fp32 ones with their row loads and output stores in the storage type (same lanes, same
 * summation order; norms, cosines and sums in fp32); deterministic, no floating-point atomics, no host sync.
 *   dtype    SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16: the type of h, out, grad_out and grad_h (anything else:
 *            SNGNN_EINVAL)
 *   h, out, grad_out, grad_h   dev, that type, rows of C values aligned to 2 * vec bytes (vec = 4, 2 or 1 for
 *            C % 4 == 0, C % 2 == 0, odd C: the fp32 layout's values per lane)
 *   workspace  sngnn_graph_workspace_bytes(g, C) bytes (an upper bound: the half path uses less)
 * No store epilogue, head, filter rows or kept bits: the caller runs those steps in torch.
 */
#define SNGNN_DTYPE_F16 1
#define SNGNN_DTYPE_BF16 2
int sngnn_agg_forward_half(const sngnn_graph_t *g, const void *h, int dtype, int C, int top_k, float thr,
                           void *out, float *wsel, float *inv_norm, int32_t *sel_src, float *sel_w,
                           void *workspace, void *stream);
int sngnn_agg_backward_half(const sngnn_graph_t *g, const void *h, int dtype, int C, const void *grad_out,
                            const float *wsel, int top_k, void *grad_h, void *workspace, void *stream);

/*
 * Cosine-attention mode of the same gather skeleton.
 * Replaces: AGNNConv.forward after ``lin`` + message + aggr='add'
 * (models.py:396-405): alpha_e = softmax over the in-edges of target i of
 * cos(h_i, h_j), out_i = sum_e alpha_e * h_j.  Build the graph with
 * add_loops = 1, remove_loops = SNGNN_LOOPS_REPLACE for AGNNConv's edge list.
 * A cosine lies in [-1, 1], so exp() is applied without the running maximum PyG's
 * softmax subtracts (identical up to rounding; the 1e-16 added to a sum >= e^-1 is
 * below fp32 resolution).
 *
 *   out    dev f32 [N, C]
 *   alpha  dev f32 [E'] or NULL  attention coefficients in CSR order (what
 *                                sngnn_attn_backward needs)
 */
int sngnn_attn_forward(const sngnn_graph_t *g, const float *h, int C, float *out,
                       float *alpha, void *workspace, void *stream);
/* autograd of the lines above; same conventions as sngnn_agg_backward */
int sngnn_attn_backward(const sngnn_graph_t *g, const float *h, int C,
                        const float *grad_out, const float *alpha, float *grad_h,
                        void *workspace, void *stream);

/*
 * Signed cosine attention of the same gather skeleton.
 * Replaces: GGCNlayer_SP.forward's use_sign branch after ``fcn`` (models.py:1512-1519 get_sparse_att,
 * :1529-1537 the two sparse products): with s_e = cos(Wh_i, Wh_j) for every entry e = (i, j),
 * i != j, of the adjacency and a_e = adj_e * softplus(deg_coeff_0 * degree_e + deg_coeff_1),
 *     out_i = sum_e a_e * (c_pos * relu(s_e) - c_neg * relu(-s_e)) * Wh_j
 *           = c_pos * prop_pos_i + c_neg * prop_neg_i            (coeff_0 / coeff_1 of :1541)
 * - the two propagations share every gathered row, so they are one gather.  Build the graph from
 * edge_index = [adj column; adj row] (source = column, target = row) with remove_loops = 1
 * (adj_remove_diag); per-edge arrays are in the graph's CSR order (array "eid" maps a CSR position
 * to its position in the loop-free entry list).
 *
 *   wh     dev f32 [N_total, C]
 *   coef   dev f32 [E']   a_e, CSR order
 *   c2     dev f32 [2]    c_pos, c_neg (device scalars: they are functions of a parameter)
 *   out    dev f32 [N, C]
 *   s      dev f32 [E'] or NULL   the cosines, CSR order (what sngnn_signed_backward needs)
 */
int sngnn_signed_forward(const sngnn_graph_t *g, const float *wh, int C, const float *coef,
                         const float *c2, float *out, float *s, void *workspace, void *stream);
/*
 * autograd of the lines above: grad_wh [N_total, C] through the message values, both rows of
 * every cosine and the normalisation's Jacobian (no floating-point atomics: two gather passes in
 * fixed order, like sngnn_attn_backward), and u [E'] (CSR order) = s_e * <grad_out_i, Wh_j>, from
 * which the caller finishes the small gradients: d a_e = kappa_e u_e with kappa_e = c_pos (s_e > 0)
 * | c_neg (s_e < 0) | 0, d c_pos = sum_{s_e > 0} a_e u_e, d c_neg = sum_{s_e < 0} a_e u_e.
 */
int sngnn_signed_backward(const sngnn_graph_t *g, const float *wh, int C, const float *grad_out,
                          const float *coef, const float *s, const float *c2, float *grad_wh, float *u,
                          void *workspace, void *stream);

/*
 * Half-width feature rows in the two attention modes: cosine attention and signed cosine attention on fp16 or
 * bf16 rows, forward and backward.
 * Replaces the same reference lines as the fp32 entries above (AGNNConv, models.py:396-405; GGCNlayer_SP's
 * use_sign branch, models.py:1512-1519 + :1529-1537; autograd through them) for a model cast to torch.float16 /
 * torch.bfloat16 - but NOT their eager arithmetic in that type: norms, cosines, exp, softmax sums and every
 * accumulation stay fp32.  Contract, with hf / whf = the rows widened to fp32 and gf = grad_out widened (exact):
 *   attention forward:  out == sngnn_attn_forward(hf).out rounded once to the storage type (round to nearest
 *                       even); alpha stays fp32 and equals that call's alpha bit for bit.
 *   attention backward: grad_h == sngnn_attn_backward(hf, gf, alpha) rounded once.
 *   signed forward:     out == sngnn_signed_forward(whf, coef, c2).out rounded once; s stays fp32 and equals that
 *                       call's s bit for bit, so every edge's sign and kappa are the fp32 call's.
 *   signed backward:    grad_wh == sngnn_signed_backward(whf, gf, coef, s, c2).grad_wh rounded once; u stays fp32
 *                       and equals that call's u bit for bit.
 * The kernels are the fp32 ones with their row loads and output stores in the storage type: same lanes, same
 * summation order.  coef, c2, alpha, s, u, the task partials, dnT / partT / partS / rec_dot and the per-edge records
 * are fp32 in the fp32 entries' workspace layout; a split row's out is the fp32 total (divided by l in the
 * attention mode) rounded once.  Deterministic, no floating-point atomics, no host synchronisation.
 *   dtype    SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16: the type of h / wh, out, grad_out and grad_h / grad_wh (anything
 *            else: SNGNN_EINVAL with "dtype" in sngnn_last_error(), before the graph or any pointer is looked at)
 *   h, wh, out, grad_out, grad_h, grad_wh   dev, that type, rows of C values aligned to 2 * vec bytes (vec = 4, 2
 *            or 1 for C % 4 == 0, C % 2 == 0, odd C: the fp32 layout's values per lane)
 *   workspace  sngnn_graph_workspace_bytes(g, C) bytes (an upper bound, as for the fp32 entries)
 * Everything else as in sngnn_attn_forward / sngnn_attn_backward / sngnn_signed_forward / sngnn_signed_backward.
 */
int sngnn_attn_forward_half(const sngnn_graph_t *g, const void *h, int dtype, int C, void *out,
                            float *alpha, void *workspace, void *stream);
int sngnn_attn_backward_half(const sngnn_graph_t *g, const void *h, int dtype, int C, const void *grad_out,
                             const float *alpha, void *grad_h, void *workspace, void *stream);
int sngnn_signed_forward_half(const sngnn_graph_t *g, const void *wh, int dtype, int C, const float *coef,
                              const float *c2, void *out, float *s, void *workspace, void *stream);
int sngnn_signed_backward_half(const sngnn_graph_t *g, const void *wh, int dtype, int C, const void *grad_out,
                               const float *coef, const float *s, const float *c2, void *grad_wh, float *u,
                               void *workspace, void *stream);

/*
 * Replaces: the SNGNN++ blend out = beta * out_0 + (1 - beta) * out_1  (models.py:134)
 * and its autograd, one pass over the n = N * C elements each way instead of five
 * elementwise launches.  beta: dev f32 [1] (the layer's Parameter).  Backward writes
 * grad0 = beta * grad_out, grad1 = (1 - beta) * grad_out and grad_beta [1] =
 * sum grad_out * (out_0 - out_1) (fixed-order sum).  workspace:
 * sngnn_blend_workspace_bytes().
 */
int64_t sngnn_blend_workspace_bytes(void);
int sngnn_blend_forward(const float *out0, const float *out1, const float *beta, int64_t n,
                        float *out, void *stream);
int sngnn_blend_backward(const float *grad_out, const float *out0, const float *out1,
                         const float *beta, int64_t n, float *grad0, float *grad1,
                         float *grad_beta, void *workspace, void *stream);
/* The blend with a hidden layer's relu + dropout behind it (models.py:81-84) in the same store:
 * sngnn_epilogue_t with relu and / or a seeded dropout (bias, keep and kept_bits must be NULL;
 * the keep draw is the aggregation epilogue's: seed, flat element index); and its backward from
 * the activated output `act`: d = act > 0 ? grad_out * scale : 0, then as above. */
int sngnn_blend_forward_epilogue(const float *out0, const float *out1, const float *beta, int64_t n,
                                 const sngnn_epilogue_t *epi, float *out, void *stream);
int sngnn_blend_backward_epilogue(const float *grad_out, const float *out0, const float *out1,
                                  const float *beta, int64_t n, const float *act, float scale,
                                  float *grad0, float *grad1, float *grad_beta, void *workspace,
                                  void *stream);

/*
 * Replaces: GGCN's layer transition - the last line of GGCNlayer_SP, `scale*(coeff[0]*prop_pos+coeff[1]*prop_neg+
 * coeff[2]*Wh)` (models.py:1544; prop = coeff[0]*prop_pos + coeff[1]*prop_neg is sngnn_signed_forward's output), and
 * between two layers the model's `act_fn`, `layer_inner + layer_previous` / `coeff*layer_inner + layer_previous`
 * (models.py:1720, 1726-1736) - and their autograd: about fifteen elementwise passes over [N, C] per layer as one pass
 * each way over the n = N * C elements.  cs dev f32 [2] = (c2, scale), coeff a host float.
 *   flags bit 0 (ACT) clear - combine, the last layer's output (prev, coeff unused):
 *     out = y = scale * (prop + c2 * wh)       every product and sum rounded separately, in this order: the torch
 *                                              expression scale * (prop + c[2] * Wh) bit for bit
 *   ACT set - transition:  out = coeff * elu(y) + p,  elu(v) = v > 0 ? v : expm1f(v),
 *     p = prev, or elu(prev) with bit 1 (PREV_ELU; needs ACT): the first transition, prev = fcn(x), coeff = 1
 *   wh == NULL && cs == NULL: y = prop (use_sign=False, models.py:1546-1552); one of them NULL alone is an error.
 * Backward (nothing saved by the forward: prop and wh are read again), g = grad_out:
 *   gy = coeff * g * (y > 0 ? 1 : expf(y))  (g itself without ACT),  grad_prop = scale * gy,  grad_wh = c2 * grad_prop,
 *   grad_cs [2] = (scale * sum gy * wh,  sum gy * (prop + c2 * wh))  - per-block partials, then one block adds them
 *   in double in a fixed order (no atomics);  PREV_ELU: grad_prev = g * (prev > 0 ? 1 : expf(prev)); otherwise the
 *   gradient of prev is grad_out itself and grad_prev (and prev) are not touched.  Without wh / cs, grad_wh, grad_cs
 *   and workspace are not touched.  workspace: sngnn_ggcn_transition_workspace_bytes().
 * n == 0 is SNGNN_OK whatever the tensors' pointers are (the backward then writes grad_cs = 0 if cs is given).
 * NULL where required, wh without cs, PREV_ELU without ACT or a negative n return SNGNN_EINVAL without a
 * launch.  float4 accesses when every pointer is 16-byte aligned, scalar ones otherwise.
 */
#define SNGNN_GGCN_ACT       1
#define SNGNN_GGCN_PREV_ELU  2
int64_t sngnn_ggcn_transition_workspace_bytes(void);
int sngnn_ggcn_transition_forward(const float *prop, const float *wh, const float *cs, const float *prev,
                                  float coeff, int flags, int64_t n, float *out, void *stream);
int sngnn_ggcn_transition_backward(const float *grad_out, const float *prop, const float *wh, const float *cs,
                                   const float *prev, float coeff, int flags, int64_t n, float *grad_prop,
                                   float *grad_wh, float *grad_prev, float *grad_cs, void *workspace, void *stream);

/*
 * Replaces: what the model wrappers run between two conv layers in TRAINING with bn=True (models.py:204-209, 79-84,
 * 296-301, 368-373): the conv's bias add (:135-136, 240-241, 327-328), `F.relu(x, inplace=True)`, `self.bns[i](x)` on the
 * batch's statistics and `self.dropout(x)` - about nine passes over [N, C] forward and eleven backward as three
 * launches each way (partials per workgroup, one small reducer, apply).  fp32, x / out / grad_* dense [N, C]:
 *   z = x + bias (bias NULL: z = x),  r = max(z, 0),  mean_c = sum_i r / N,  var_c = sum_i (r - mean)^2 / N (biased),
 *   invstd = 1 / sqrt(var + eps),  xhat = (r - mean) * invstd,  out = (xhat * gamma + beta) * keep * keep_scale
 * keep: the caller's u8 [N, C] mask, or drawn in the kernel from (seed, i * C + c) as sngnn_epilogue_t.seed documents
 * (seed: dev uint64 [1], used when p > 0), or neither: no dropout.  The relu is idempotent, so rows a producer already
 * stored as relu(conv + bias) go in with bias NULL.  The forward also writes save_mean / save_invstd [C] and, when
 * given, running_mean <- (1 - momentum) running_mean + momentum mean, running_var <- ... + momentum var N / (N - 1).
 * Nothing of size [N, C] is saved: the backward recomputes r, xhat and the mask from x.  With gz = grad_out * keep *
 * keep_scale:  grad_beta = sum_i gz,  grad_gamma = sum_i gz xhat,
 *   grad_x = invstd * (gamma gz - gamma grad_beta / N - xhat gamma grad_gamma / N) * [z > 0],
 * and grad_bias (optional; needs bias) = the column sums of grad_x.  Every sum is accumulated in double; the statistics
 * as (count, mean, M2) partials combined by Chan's formula, never as sum r^2.  No atomics: the same bits every run.
 * Only enqueues.  workspace: sngnn_bn_train_workspace_bytes(C) (0 for a C out of range).
 * NULL where required, N < 2, C < 1 or > SNGNN_MAX_CHANNELS, p outside [0, 1), keep together with seed, grad_bias
 * without bias, or one of running_mean / running_var alone return SNGNN_EINVAL without a launch.  float4 accesses
 * where C % 4 == 0 and every [N, C] base is 16-byte aligned, scalar ones otherwise.
 */
int64_t sngnn_bn_train_workspace_bytes(int C);
int sngnn_bn_train_forward(const float *x, const float *bias, int64_t N, int C, const float *gamma, const float *beta,
                           double eps, double momentum, float *running_mean, float *running_var,
                           const unsigned char *keep, float keep_scale, const void *seed, float p, float *out,
                           float *save_mean, float *save_invstd, void *workspace, void *stream);
int sngnn_bn_train_backward(const float *grad_out, const float *x, const float *bias, int64_t N, int C,
                            const float *gamma, const float *save_mean, const float *save_invstd,
                            const unsigned char *keep, float keep_scale, const void *seed, float p, float *grad_x,
                            float *grad_gamma, float *grad_beta, float *grad_bias, void *workspace, void *stream);
/*
 * The other order, norm -> relu -> dropout: what GCNII runs behind every GCN2Conv in TRAINING (models.py:1296-1298 and
 * the next layer's dropout, :1295): `self.bns[i](x)` on the batch's statistics, `x.relu()`, `F.dropout(x)`.
 *   mean_c = sum_i x / N,  var_c = sum_i (x - mean)^2 / N (biased),  invstd = 1 / sqrt(var + eps),
 *   xhat = (x - mean) * invstd,  y = xhat * gamma + beta,  out = max(y, 0) * keep * keep_scale
 * The same three launches each way, the same double / Chan summation, running statistics, keep / seed and workspace
 * (sngnn_bn_train_workspace_bytes) as the pair above; there is no conv bias.  Nothing of size [N, C] is saved: the
 * backward recomputes xhat, the relu mask [xhat * gamma + beta > 0] and the keep mask from x.  With
 * gy = grad_out * keep * keep_scale * [y > 0]:  grad_beta = sum_i gy,  grad_gamma = sum_i gy xhat,
 *   grad_x = invstd * (gamma gy - gamma grad_beta / N - xhat gamma grad_gamma / N).
 * The same argument errors as above.
 */
int sngnn_bn_post_forward(const float *x, int64_t N, int C, const float *gamma, const float *beta, double eps,
                          double momentum, float *running_mean, float *running_var, const unsigned char *keep,
                          float keep_scale, const void *seed, float p, float *out, float *save_mean,
                          float *save_invstd, void *workspace, void *stream);
int sngnn_bn_post_backward(const float *grad_out, const float *x, int64_t N, int C, const float *gamma,
                           const float *beta, const float *save_mean, const float *save_invstd,
                           const unsigned char *keep, float keep_scale, const void *seed, float p, float *grad_x,
                           float *grad_gamma, float *grad_beta, void *workspace, void *stream);

/*
 * The same two gather-sums on any graph, node-range partitions included (multi-GPU
 * SNGNN++; new - the reference is single-device).  A rank builds the partition of the
 * FLIPPED edge list (row 0 and row 1 of edge_index swapped), whose owned "targets" are
 * its own source nodes; then
 *   out0_local = sngnn_gather_sum_rows(g_flipped, wt_full, bias)      out[i] = bias + sum_{e in CSR row i} table[col_e]
 *   dwt_partial = sngnn_scatter_sum_rows(g_flipped, g0_local)         out[v] = sum_{q in CSC row v} vals[dst_q]
 * table / out of scatter have N_total rows, out of gather / vals have the owned rows.
 * Requires src_min == 0 (models.py:125's shift would cross partitions otherwise).
 */
int sngnn_gather_sum_rows(const sngnn_graph_t *g, const float *table, const float *bias,
                          int C, float *out, void *workspace, void *stream);
int sngnn_scatter_sum_rows(const sngnn_graph_t *g, const float *vals, int C, float *out,
                           void *workspace, void *stream);
/*
 * Replaces: GGCNlayer_SP's plain propagation `torch.sparse.mm(adj * sc, Wh)` (models.py:1544-1549,
 * use_sign=False) and its autograd - the same two gather-sums with one WEIGHT per entry:
 *   out[i]  = sum_{q in CSR row i} w_csr[q] * table[col_q]          (weights in the graph's CSR order)
 *   out[j]  = sum_{q in CSC row j} w_csc[q] * vals[dst_q]           (the transpose; weights in CSC order)
 * (value * row rounded, then added: a sparse mm's arithmetic; fixed order, no atomics), and the weights'
 * gradient out[p] = <a_rows[idx_a[p]], b_rows[idx_b[p]]> per entry (idx_*: dev i32 [n_pairs]).
 */
int sngnn_weighted_gather_sum_rows(const sngnn_graph_t *g, const float *table, const float *w_csr, int C,
                                   float *out, void *workspace, void *stream);
int sngnn_weighted_scatter_sum_rows(const sngnn_graph_t *g, const float *vals, const float *w_csc, int C,
                                    float *out, void *workspace, void *stream);
int sngnn_pair_dot_rows(const float *a_rows, const int32_t *idx_a, const float *b_rows, const int32_t *idx_b,
                        int64_t n_pairs, int C, float *out, void *stream);

/* ------------------------------------------------------------------------
 * Polynomial propagation with the GCN-normalised adjacency (GPRGNN, APPNP): csrc/prop.hip.
 * ------------------------------------------------------------------------ */
/*
 * A^ = D^-1/2 (A + I) D^-1/2 of PyG's gcn_norm(edge_index, None, N, add_self_loops=True): original self loops
 * dropped, one loop per node appended, duplicates counted - the graph built with add_loops = 1, remove_loops =
 * SNGNN_LOOPS_REPLACE, which every entry below requires (and an unpartitioned one: SNGNN_EINVAL otherwise) -,
 * deg_i = in-degree with the loop (>= 1), dinv = deg^-1/2, (A^ x)_i = sum_{e -> i} dinv_src dinv_i x_src, and
 * A^T the same sum over the out-edges (the CSC side; edge_index need not be symmetric).
 *
 * No weight is read per edge: the kernels carry the SCALED iterate u = dinv . x, so that (A^ x)_i = dinv_i S_i
 * with S_i = sum_{e -> i} u_src an unweighted gather-sum on the row classes of the other gather kernels (lane
 * group, wave, 128-edge tasks + finalize; fixed order, no atomics).  One hop is one launch sequence (main, +
 * finalize when the side has split rows) whose store epilogue is
 *     z_i = a x0_i + b (dinv_i S_i),   [acc_i += c z_i,]   [dot += <z_i, xd_i>,]   store dinv_i z_i | z_i (last hop)
 * with a, b, c read from device memory; every product and sum rounded separately.  Hops are separate launches.
 *
 * sngnn_prop_dinv replaces gcn_norm's degree pass (deg = scatter_add of ones, deg.pow(-0.5)): dinv dev f32 [N]
 * from the graph's own rowptr, once per graph.
 */
int sngnn_prop_dinv(const sngnn_graph_t *g, float *dinv, void *stream);
/* bytes of device workspace of the three entries below at C channels and K hops: two scaled iterates [N, C], the
 * split rows' task partials of either side and (K + 1) rows of per-workgroup dot partials (f64) */
int64_t sngnn_prop_workspace_bytes(const sngnn_graph_t *g, int C, int K);
/*
 * Replaces: models.py:1191-1208 - GPR_prop.forward after gcn_norm, hidden = sum_k gamma_k A^^k x (K propagate
 * calls with a 4-byte norm per edge and `hidden = hidden + gamma * x`, about five [N, C] passes per hop) - as K
 * hops in Horner form: h_K = gamma_K x, h_k = gamma_k x + A^ h_{k+1}, out = h_0; per hop the gather, one read of
 * x and one store.
 *   x      dev f32 [N, C]     rows aligned to 4 * vec bytes (vec = 4, 2, 1 for C % 4 == 0, C % 2 == 0, odd C)
 *   gamma  dev f32 [K + 1]    the coefficients rounded to fp32 (the parameter itself is float64: torch rounds a
 *                             0-dim float64 factor of an fp32 tensor the same way); K >= 1
 *   dinv   dev f32 [N]        sngnn_prop_dinv's output
 *   out    dev f32 [N, C]
 */
int sngnn_prop_gpr_forward(const sngnn_graph_t *g, const float *x, const float *gamma, int K, int C,
                           const float *dinv, float *out, void *workspace, void *stream);
/*
 * Replaces: autograd through models.py:1200-1204 (K saved iterates [N, C] and K transposed propagations).  Only
 * x is read: the power form on the transpose, t_0 = grad_out, t_{k+1} = A^T t_k,
 *   grad_x = sum_k gamma_k t_k   (accumulated in place by the hops' epilogues),
 *   grad_gamma_k = <t_k, x>      dev f64 [K + 1] - per-workgroup partial dots in double from the same launches,
 *                                added by one reducer launch in a fixed order: the same bits on every run.
 * grad_x (dev f32 [N, C]) or grad_gamma may be NULL (not wanted).
 */
int sngnn_prop_gpr_backward(const sngnn_graph_t *g, const float *grad_out, const float *x, const float *gamma,
                            int K, int C, const float *dinv, float *grad_x, double *grad_gamma,
                            void *workspace, void *stream);
/*
 * Replaces: PyG's APPNP.forward as models.py:1033 + 1048 use it (K, alpha; no dropout, no cache): x_0 = h,
 * x_{k+1} = (1 - alpha) A^ x_k + alpha h, out = x_K; and with transpose != 0 its autograd, the same recurrence on
 * A^T from h = grad_out (r <- alpha g + (1 - alpha) A^T r): nothing is saved by the forward.
 *   h      dev f32 [N, C]
 *   coef   dev f32 [2]       (alpha, 1 - alpha), each rounded to fp32
 */
int sngnn_prop_appnp(const sngnn_graph_t *g, const float *h, const float *coef, int K, int C, const float *dinv,
                     int transpose, float *out, void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * Graph attention (GAT): csrc/gat.hip.
 * ------------------------------------------------------------------------ */
/*
 * PyG 2.0.4's GATConv after its linear map, for xp = lin_src(x) viewed as [N, H, C] (H heads of C channels):
 *     a_src[n,h] = <xp[n,h,:], att_src[h,:]>,  a_dst[n,h] = <xp[n,h,:], att_dst[h,:]>
 *     per in-edge e = (j -> i) and head h:  a_e = leaky_relu(a_src[j,h] + a_dst[i,h], negative_slope)
 *     alpha_e = exp(a_e - max_i) / (sum_i exp(a - max_i) + 1e-16),   out[i,h,:] = sum_e alpha_e xp[j,h,:]
 * on the edge list of add_self_loops after remove_self_loops: the graph built with add_loops = 1, remove_loops =
 * SNGNN_LOOPS_REPLACE, unpartitioned (SNGNN_EINVAL otherwise).  Every row has its loop, so the sum is at least 1 and
 * the 1e-16 vanishes in fp32.  Limits: 1 <= H <= 16, C >= 1, H * C <= SNGNN_MAX_CHANNELS (SNGNN_ERANGE otherwise).
 * All rows are dev f32, dense, 16-byte aligned.  Row classes of the other gather kernels (lane group up to 16
 * in-edges, one wave up to 128, 128-edge tasks + a finalize for split rows), heads on the grid's second dimension;
 * fixed summation order, no floating-point atomics, no host synchronisation.
 */
/* bytes of device workspace of sngnn_gat_forward / sngnn_gat_backward: the split rows' task partials [tasks, H, C]
 * and two scalars per task and head, the backward's records [E', H, 2], grad_a_src and grad_a_dst [N, H] and the
 * per-workgroup partials of grad_att (f64); 0 outside the limits */
int64_t sngnn_gat_workspace_bytes(const sngnn_graph_t *g, int H, int C);
/*
 * Replaces: (x_src * att_src).sum(-1), (x_dst * att_dst).sum(-1) (gat_conv.py:197-198) - both from one read of xp,
 * each score's C products summed in double and rounded once.
 *   xp       dev f32 [N, H * C]      att_src, att_dst  dev f32 [H * C]      a_src, a_dst  dev f32 [N, H] (out)
 */
int sngnn_gat_scores(const float *xp, const float *att_src, const float *att_dst, int64_t N, int H, int C,
                     float *a_src, float *a_dst, void *stream);
/*
 * Replaces: GATConv.propagate - the gathers of alpha_j / alpha_i and x_j, leaky_relu, PyG's softmax (scatter max,
 * exp, scatter sum, division) and the weighted scatter-add: [E', H] and [E', H, C] intermediates.  Pass one settles
 * a row's maximum m and sum l per head from a 4-byte gather per edge and head; pass two gathers each head slice
 * once, weighted by exp(a_e - m), and divides by l in the store.  Split rows: every task writes its partial row,
 * m_t and l_t; the finalize merges them in task order, m = max m_t, l = sum l_t exp(m_t - m),
 * out = (sum_t exp(m_t - m) partial_t) / l.
 *   out      dev f32 [N, H * C]
 *   ml       dev f32 [2, N, H]       m then l per row and head: with out, all the backward needs saved
 */
int sngnn_gat_forward(const sngnn_graph_t *g, const float *xp, const float *a_src, const float *a_dst, int H, int C,
                      float negative_slope, float *out, float *ml, void *workspace, void *stream);
/*
 * Replaces: autograd through the sequence above and through the two score products.  With G = grad_out:
 *   pass T, in-edges:   t_e = <G[i,h], xp[j,h]>, dot = <G[i,h], out[i,h]>, ds_e = alpha_e (t_e - dot),
 *                       da_e = ds_e * (a_src[j,h] + a_dst[i,h] > 0 ? 1 : negative_slope),
 *                       grad_a_dst[i,h] = sum_e da_e; {alpha_e, da_e} stored at the edge's CSC position
 *   pass S, out-edges:  grad_xp[j,h,:] = sum_e alpha_e G[i,h,:] + grad_a_src[j,h] att_src[h,:]
 *                                        + grad_a_dst[j,h] att_dst[h,:],   grad_a_src[j,h] = sum_e da_e
 *   grad_att [2, H * C] (src then dst): grad_att_src[h,c] = sum_j grad_a_src[j,h] xp[j,h,c], dst alike -
 *                       per-workgroup partials in double added by one reducer launch in a fixed order.
 * grad_xp (dev f32 [N, H * C]) or grad_att may be NULL (not wanted).
 */
int sngnn_gat_backward(const sngnn_graph_t *g, const float *grad_out, const float *xp, const float *out,
                       const float *a_src, const float *a_dst, const float *ml, const float *att_src,
                       const float *att_dst, int H, int C, float negative_slope, float *grad_xp, float *grad_att,
                       void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * Weighted relational graph attention (WRGAT): csrc/wrgat.hip.
 * ------------------------------------------------------------------------ */
/*
 * WeightedRGATConv (models.py:1903-2014) after its linear maps, for P [N, R, C] with P[n,r,:] = x[n] weight[r] (R
 * relations of C channels), atten [R, 2C] = [target half | source half], edges e = (j -> i) of relation r_e and weight
 * w_e:
 *     s_dst[n,r] = <P[n,r], atten[r,:C]>,  s_src[n,r] = <P[n,r], atten[r,C:]>,  a_e = leaky_relu(s_dst[i,r] + s_src[j,r])
 *     per segment (i, r) of n_ir edges:  alpha_e = exp(a_e - m_ir) / (l_ir + 1e-16),  m_ir = max a_e, l_ir = sum exp(a_e - m_ir)
 *     out[i] = sum_r (1 / n_ir) sum_{e in (i,r)} w_e alpha_e P[j,r,:]  +  self_rows[i]  +  bias      (relu: max(., 0))
 * - a softmax per relation AND target, averaged over the relation's edges, all relations added into one row (the
 * reference: R masked propagate calls with [E_r, C] messages).  A non-empty segment holds its maximum, so l_ir >= 1 and
 * the 1e-16 vanishes in fp32; an empty segment adds exactly 0.
 *
 * The graph: the edge list sorted STABLY by relation, built with add_loops = 0, remove_loops = 0 (every edge kept,
 * duplicates count once each), unpartitioned (SNGNN_EINVAL otherwise).  Its CSR rows are then grouped by relation:
 *   rel_ptr  dev i32 [N, R + 1]   offsets inside the row: entries [rel_ptr[i,r], rel_ptr[i,r+1]) of row i carry relation r
 *   rel_csc  dev i32 [E]          the relation of every CSC entry (the backward's scatter pass; may be NULL when E == 0)
 *   w_csr    dev f32 [E]          the edge weights in CSR order, or NULL (= 1); data, no gradient
 * Limits: 1 <= R <= 16, C >= 1, R * C <= SNGNN_MAX_CHANNELS (SNGNN_ERANGE otherwise, nothing launched).
 * P, self_rows, grad_P and grad_self are row-strided (strides in floats, multiples of the row vector width 4 | 2 | 1
 * that divides C): slices of one [N, R * C + C] table.  Row classes of the other gather kernels; fixed summation
 * order, no floating-point atomics, no host synchronisation.
 */
/* bytes of device workspace of the two entries below; 0 outside the limits */
int64_t sngnn_wrgat_workspace_bytes(const sngnn_graph_t *g, int R, int C);
/*
 * Replaces: models.py:1975-1993 and :1997-2008 - per relation a masked edge list, a matmul, the gathers of x_i / x_j,
 * cat, leaky_relu, PyG's softmax, two [E_r, C] products, the scatter-mean and an add.  Launches: the score pass of
 * sngnn_gat_scores (H = R), the statistics m, l [N, R] from a 4-byte gather per edge (+ a finalize on [tasks, R]
 * scalars for split rows), and one weighted gather-sum that fetches only the slice P[j, r_e, :] per edge (+ a plain
 * finalize), root slice, bias and relu in its store.
 *   self_rows, bias  may be NULL       out  dev f32 [N, C] dense
 *   scores  dev f32 [2, N, R] (out)    s_src then s_dst       ml  dev f32 [2, N, R] (out)   m then l
 */
int sngnn_wrgat_forward(const sngnn_graph_t *g, const float *P, int64_t P_stride, const float *self_rows,
                        int64_t self_stride, const float *bias, const int32_t *rel_ptr, const float *w_csr,
                        const float *atten, int R, int C, float negative_slope, int relu, float *out, float *scores,
                        float *ml, void *workspace, void *stream);
/*
 * Replaces: autograd through the sequence above.  With G = grad_out, zeroed where relu gave out <= 0 (out is read
 * only then), t_e = <G_i, P[j,r]>, D_ir = sum_{(i,r)} alpha_e w_e t_e, ds_e = alpha_e (w_e t_e - D_ir) / n_ir,
 * da_e = ds_e leaky'(raw_e):
 *   grad_P[j,r,:] = sum_{e out of j, type r} (w_e alpha_e / n_ir) G_i + grad_s_src[j,r] atten[r,C:] + grad_s_dst[j,r] atten[r,:C]
 *   grad_atten [R, 2C] = [sum_n grad_s_dst[n,r] P[n,r,:] | sum_n grad_s_src[n,r] P[n,r,:]]  (f64 partials, fixed order)
 *   grad_self = G (masked), grad_bias = its column sums (f64 partials, fixed order)
 * Each of grad_P, grad_self, grad_atten, grad_bias may be NULL (not wanted).
 */
int sngnn_wrgat_backward(const sngnn_graph_t *g, const float *grad_out, const float *out, const float *P,
                         int64_t P_stride, const int32_t *rel_ptr, const int32_t *rel_csc, const float *w_csr,
                         const float *atten, const float *scores, const float *ml, int R, int C,
                         float negative_slope, int relu, float *grad_P, int64_t grad_P_stride, float *grad_self,
                         int64_t grad_self_stride, float *grad_atten, float *grad_bias, void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * ACM-GCN's low / high / identity filterbank with its three-way attention: csrc/acm.hip.
 * ------------------------------------------------------------------------ */
/*
 * GraphConvolution2.forward for model_type 'acmgcn' (relu != 0) / 'acmsgc' (relu == 0), variant = False, after its
 * three linear maps, P = X [W_low | W_high | W_mlp] = [Pl | Ph | Pm], dev f32 [N, 3C]:
 *     L = adj_low Pl,  H = adj_high Ph,  M = Pm,  o* = relu(L | H | M),
 *     d = (<ol, a_low>, <oh, a_high>, <om, a_mlp>),  att = softmax(sigmoid(d) att_vec / 3),
 *     out = 3 (att_0 ol + att_1 oh + att_2 om)
 * for the adjacency whose row i carries n_i entries (its diagonal among them) of weight 1 / n_i each, adj_high =
 * I - adj_low: the graph holds adj_low's pattern (source = column, target = row; loops kept, none added; every row
 * holds its diagonal; an unpartitioned graph, SNGNN_EINVAL otherwise), n_i is its rowptr's difference and no weight is
 * read per entry:
 *     L_i = S^l_i / n_i,  H_i = (1 - 1 / n_i) Ph_i - S^h_i / n_i,
 *     S^l_i = sum over row i of Pl[col],  S^h_i = sum over the off-diagonal entries of row i of Ph[col]
 * (the reference's own terms: Ph_i - Ph_i / n_i inside one sum would cancel what the reference never adds)
 * - one column id and one contiguous 8C-byte slice of P per entry on the row classes of the other gather kernels
 * (lane group up to 16 entries, one wave up to 128, 128-entry tasks + a finalize); fixed summation order, no
 * floating-point atomics, no host synchronisation.  Limits: 1 <= C, 2C <= SNGNN_MAX_CHANNELS (SNGNN_ERANGE
 * otherwise).  Rows aligned to 4 * vec bytes (vec = 4, 2, 1 for C % 4 == 0, C % 2 == 0, odd C).
 */
/* bytes of device workspace of the two entries below: the split rows' task partials [tasks, 2C] of either side, the
 * backward's scaled gradients [N, 2C] and the per-workgroup partials of the parameter gradients (f64); 0 outside
 * the limits */
int64_t sngnn_acm_workspace_bytes(const sngnn_graph_t *g, int C);
/*
 * Replaces: models.py:1787-1791 and 1809-1818 (1820-1830 with relu == 0) after the three mm - two spmm over COO
 * entries of 20 bytes each, three relu, three [N, C] x [C, 1] products, cat, sigmoid, the 3x3 mm, softmax, three
 * broadcasts and two adds, each an [N, C] or [N, 3] pass with its saved tensor: here one gather whose store
 * epilogue does the rest.
 *   a_low, a_high, a_mlp  dev f32 [C]     att_vec  dev f32 [3, 3]
 *   out   dev f32 [N, C]
 *   LH    dev f32 [N, 2C]   the pre-activations [L | H]   } all the backward needs saved next to P
 *   datt  dev f32 [N, 6]    (d_0..2, att_0..2) per row    }
 */
int sngnn_acm_forward(const sngnn_graph_t *g, const float *P, const float *a_low, const float *a_high,
                      const float *a_mlp, const float *att_vec, int C, int relu, float *out, float *LH, float *datt,
                      void *workspace, void *stream);
/*
 * Replaces: autograd through the sequence above.  Pass A, row-local: grad_out through the mix, the softmax, the
 * 3x3 product, the sigmoid, the three dots and relu' (the masks L > 0, H > 0, M > 0 of the stored fp32
 * pre-activations) gives gL, gH, gM; pass B, the transpose gather-sum over the other side of the graph:
 *     grad_P = [ sum_{i : j in row i} gL_i / n_i  |  (1 - 1 / n_j) gH_j - sum_{i != j : j in row i} gH_i / n_i  |  gM_j ]
 *   grad_P       dev f32 [N, 3C]
 *   grad_params  dev f64 [3C + 9]   grad a_low, a_high, a_mlp [C] each, then grad att_vec [3, 3] - per-workgroup
 *                                   partials in double added by one reducer launch in a fixed order
 */
int sngnn_acm_backward(const sngnn_graph_t *g, const float *grad_out, const float *P, const float *LH,
                       const float *datt, const float *a_low, const float *a_high, const float *a_mlp,
                       const float *att_vec, int C, int relu, float *grad_P, double *grad_params, void *workspace,
                       void *stream);

/* ------------------------------------------------------------------------
 * GCNII's layer, PyG 2.0.4's GCN2Conv (initial residual + identity mapping): csrc/gcn2.hip.
 * ------------------------------------------------------------------------ */
/*
 * GCN2Conv.forward with shared weights on the adjacency of sngnn_prop_* (A^ of gcn_norm: the unpartitioned graph
 * built with add_loops = 1, remove_loops = SNGNN_LOOPS_REPLACE; SNGNN_EINVAL otherwise):
 *     s = (1 - alpha) (A^ x) + alpha x0,     out = (1 - beta) s + beta (s W)
 * as two launches.  The scalars arrive as the fp32 values torch multiplies an fp32 tensor with.
 *
 * sngnn_gcn2_hop: s_i = a (dinv_i S_i) + b x0_i with S_i = sum_{e -> i} dinv_src x_src - the UNSCALED rows of x are
 * gathered and each is multiplied by dinv[src], loaded next to the column id (4 more bytes per edge instead of a
 * scaled copy of x per layer) - on the row classes of the other gather kernels (lane group, wave, 128-edge tasks +
 * a finalize; fixed summation order, no atomics); every product and sum rounded separately.  x0 NULL: no b x0 term
 * (alpha == 0, and the backward).  transpose != 0 walks the out-edges: a (A^T x), the backward's hop.
 *   x, x0, out  dev f32 [N, C]   rows aligned to 4 * vec bytes (vec = 4, 2, 1 for C % 4 == 0, C % 2 == 0, odd C)
 *   dinv        dev f32 [N]      sngnn_prop_dinv's output
 *   workspace   sngnn_gcn2_workspace_bytes(g, C): the split rows' task partials of either side
 *
 * sngnn_gcn2_map: out = c0 s + c1 (s W), W dev f32 [C, C] row-major ([in, out]; transpose_w != 0: s W^T, the
 * backward's g_s = (1 - beta) g + beta (g W^T)), 1 <= C <= SNGNN_GCN2_MAX_C (SNGNN_ERANGE otherwise).  s is
 * streamed once in 32-row tiles with W resident in LDS; a dot product is four interleaved fp32 fma chains added
 * pairwise.  rm != NULL (with invstd, gamma, beta_bn, all dev f32 [C]) adds the evaluation epilogue of the norm
 * and relu behind the layer: out = max(((out - rm) * invstd) * gamma + beta_bn, 0), each step rounded.
 * Both only enqueue.
 */
#define SNGNN_GCN2_MAX_C 128
int64_t sngnn_gcn2_workspace_bytes(const sngnn_graph_t *g, int C);
int sngnn_gcn2_hop(const sngnn_graph_t *g, const float *x, const float *x0, const float *dinv, float a, float b,
                   int C, int transpose, float *out, void *workspace, void *stream);
int sngnn_gcn2_map(const float *s, const float *w, float c0, float c1, int64_t N, int C, int transpose_w,
                   const float *rm, const float *invstd, const float *gamma, const float *beta_bn, float *out,
                   void *stream);

/* ------------------------------------------------------------------------
 * GCNConv, GCN / GCNJK and MixHop (models/models.py:539-580, 693-843): csrc/gcn.hip.
 * ------------------------------------------------------------------------ */
/*
 * One hop over A^ = D^-1/2 (A + I) D^-1/2 (the graph of sngnn_prop_* / sngnn_gcn2_*; any other: SNGNN_EINVAL) on a
 * COLUMN SLICE of a wider table, with a split store:
 *     z_i = dinv_i * sum_{e -> i} dinv_src * src[src_row, 0 .. W)
 * sngnn_gcn2_hop's skeleton (lane group up to 16 in-edges, wave up to 128, 128-edge tasks + a finalize; rows gathered
 * unscaled, dinv[src] loaded next to the column id; fixed summation order, no floating-point atomics, no host
 * synchronisation; every product and sum rounded separately).  The first W0 columns of z go to dst0, the other
 * W - W0 to dst1 (NULL iff W0 == W).  Wp > 0: Wp columns of row i of pass_src are copied to pass_dst by whoever
 * completes row i (MixHop's un-propagated slice).  Epilogue on the dst0 columns only, each step rounded:
 *     bias [W0]:                        z = z + bias
 *     rm, invstd, gamma, beta_bn [W0]:  z = ((z - rm) * invstd) * gamma + beta_bn      (all four or none)
 *     relu != 0:                        z = max(z, 0)
 * transpose != 0 walks the out-edges (A^T, the backward's hop).
 *
 * Every table pointer addresses column 0 of its slice; ld_* is its row stride in floats (>= the slice's width).
 * Limits: 1 <= W0 <= W <= SNGNN_MAX_CHANNELS, 0 <= Wp <= SNGNN_MAX_CHANNELS (SNGNN_ERANGE otherwise).  The lane
 * layout is that of W channels (so the summation order depends on W and the graph alone), the vector width vec is
 * the largest of 4, 2, 1 that divides W, W0, Wp, every stride and every table pointer's offset (in floats) from a
 * 16-byte boundary - a lane's vec channels never straddle the W0 boundary.  A narrower vec than W's own multiplies
 * the steps per lane; more than 8: SNGNN_ERANGE.  A destination (dst0, dst1, pass_dst) must not share an element with
 * the source, pass_src or another destination (SNGNN_EINVAL; nothing is launched): their address ranges
 * [p, p + (N - 1) ld + width) are disjoint, or they are disjoint column ranges of one table (equal strides) - a
 * MixHop launch writes one slice of the output and copies into another.
 *   workspace   sngnn_gcn_workspace_bytes(g, W): the split rows' task partials of either side (and the partial
 *               column sums of sngnn_gcn_bias_grad at C = W)
 *
 * sngnn_gcn_bias_grad: grad_bias[c] = sum_i g[i, c] (GCNConv's bias), accumulated in double in a fixed order
 * (per-workgroup partials, then one pass over them), rounded to fp32 once.  g dev f32 [N, C], dense.
 * Both only enqueue.
 */
typedef struct sngnn_gcn_hop {
    const float *src;       int64_t ld_src;
    int W, W0;
    float *dst0;            int64_t ld0;
    float *dst1;            int64_t ld1;
    const float *pass_src;  int64_t ld_ps;
    float *pass_dst;        int64_t ld_pd;
    int Wp;
    int relu;
    const float *bias, *rm, *invstd, *gamma, *beta_bn;
} sngnn_gcn_hop_t;
int64_t sngnn_gcn_workspace_bytes(const sngnn_graph_t *g, int W);
int sngnn_gcn_hop(const sngnn_graph_t *g, const sngnn_gcn_hop_t *a, const float *dinv, int transpose,
                  void *workspace, void *stream);
int sngnn_gcn_bias_grad(const float *g, int64_t N, int C, float *grad_bias, void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * H2GCN (models/models.py:903-1024): csrc/h2gcn.hip.
 * ------------------------------------------------------------------------ */
/*
 * The strict two-hop adjacency, replacing H2GCN.init_adj's torch_sparse / scipy passes on the host.  g is the
 * loop-free graph A1: unpartitioned, built with add_loops = 0, remove_loops = 1 (entry (i, j) per edge j -> i,
 * duplicates kept); anything else: SNGNN_EINVAL, nothing launched.  Row i of
 *     A2 = [(A1 A1 != 0) - diag - A1 > 0]
 * holds every k with k -> j -> i for some j, k != i, (i, k) not an entry of A1; multiplicities play no part.
 *   sngnn_two_hop_count   count dev i32 [N]: the exact number of entries of every row of A2
 *   sngnn_two_hop_fill    offsets dev i64 [N]: the exclusive scan of count (the caller's), E2 its total; edge_index dev
 *                         i64 [2, E2] in canonical order - row 1 the targets, ascending, row 0 the sources, ascending
 *                         within a target - which sngnn_graph_create takes.  E2 > 2^31 - 1: SNGNN_ERANGE.
 * One workgroup per row.  A row whose candidate bound sum_{j in N(i)} deg(j) is at most SNGNN_TWO_HOP_HASH_MAX goes
 * through an open-addressing table in LDS (sorted for the fill); a larger one through a bitmap of N bits in the
 * workspace, read in order.  Integer atomics only; exact and deterministic.
 *   workspace   sngnn_two_hop_workspace_bytes(g): the bitmaps (cleared by each call)
 * Both only enqueue.
 *
 * sngnn_h2gcn_dinv: dinv[i] = deg_i^-1/2 of a loop-free graph's row (in-)degree, 0 for an empty row (gcn_norm with
 * add_self_loops = False); dev f32 [N].  sngnn_prop_dinv keeps refusing such graphs.
 *
 * sngnn_h2gcn_hop: one H2GCNConv on A^s = D_s^-1/2 A_s D_s^-1/2 (s = 1, 2; g1 and g2 loop-free graphs of the same N,
 * dinv1 / dinv2 from sngnn_h2gcn_dinv; the row degree on BOTH sides of the product):
 *     transpose == 0   dst[:, 0:W] = A^1 src,  dst[:, W:2W] = A^2 src            src [N, W], dst [N, 2W]
 *     transpose != 0   dst[:, 0:W] = A^1T src[:, 0:W] + A^2T src[:, W:2W]        src [N, 2W], dst [N, W]
 * sngnn_gcn_hop's skeleton, arithmetic and slice rules (src / dst address column 0 of a column slice, ld_* its row
 * stride in floats; the lane layout is that of W channels, the vector width the largest of 4, 2, 1 that divides W, both
 * strides and both pointers' offsets from a 16-byte boundary; more than 8 steps per lane: SNGNN_ERANGE).  The forward is
 * one launch over the work lists of both graphs and one finalize where either has split rows; the transpose is that
 * sequence twice, the second adding into the first's stores (no floating-point atomics; each element's sum is
 * first + second).  A source whose dinv is 0 is multiplied, not skipped; a row without entries stores exact zeros.
 * Epilogue (transpose == 0 only; all four or none), on all 2W columns, each step rounded:
 *     rm, invstd, gamma, beta_bn [2W]:  z = ((z - rm) * invstd) * gamma + beta_bn
 * Limits: 1 <= W <= SNGNN_MAX_CHANNELS (SNGNN_ERANGE); dst must not share an element with src as in sngnn_gcn_hop,
 * partitioned graphs, graphs with loops added, mismatched N or NULL: SNGNN_EINVAL.  Refused calls launch nothing.
 *   workspace1 / workspace2   sngnn_h2gcn_workspace_bytes(g1 / g2, W): the split rows' task partials of either side
 * Only enqueues.
 */
#define SNGNN_TWO_HOP_HASH_MAX 1024
typedef struct sngnn_h2gcn_hop {
    const float *src;  int64_t ld_src;
    float *dst;        int64_t ld_dst;
    int W;
    const float *rm, *invstd, *gamma, *beta_bn;
} sngnn_h2gcn_hop_t;
int64_t sngnn_two_hop_workspace_bytes(const sngnn_graph_t *g);
int sngnn_two_hop_count(const sngnn_graph_t *g, int32_t *count, void *workspace, void *stream);
int sngnn_two_hop_fill(const sngnn_graph_t *g, const int64_t *offsets, int64_t E2, int64_t *edge_index,
                       void *workspace, void *stream);
int sngnn_h2gcn_dinv(const sngnn_graph_t *g, float *dinv, void *stream);
int64_t sngnn_h2gcn_workspace_bytes(const sngnn_graph_t *g, int W);
int sngnn_h2gcn_hop(const sngnn_graph_t *g1, const sngnn_graph_t *g2, const sngnn_h2gcn_hop_t *a, const float *dinv1,
                    const float *dinv2, int transpose, void *workspace1, void *workspace2, void *stream);

/* ------------------------------------------------------------------------
 * MLPNORM's norm layer (GloGNN, models/models.py:1389-1437) on the sparse graph: csrc/glognn.hip.
 * ------------------------------------------------------------------------ */
/*
 * Replaces: norm_func1 / norm_func2 with order_func1 / order_func2 on to_dense_adj's [N, N] matrix (about 25 torch
 * ops, norm_layers x orders dense N x N products, one torch.inverse) for fp32 rows of 1 <= C <= SNGNN_GLOGNN_MAX_C
 * channels (SNGNN_ERANGE otherwise).  With coe = 1/(alpha+beta), coe1 = 1-gamma, coe2 = 1/coe1, s = coe/coe1,
 * D = diag(diag) (I when diag is NULL), G = x^T x, V = (coe2^2 I + coe G)^-1:
 *     M = s V D,   T = s D G V D,   W = G V,   S = sum_k w_k A^k x,
 *     out = coe1 (x - gamma h0) T + beta S M + gamma h0
 * A is to_dense_adj's matrix, (A v)_i = sum over the edges with edge_index[0] == i of v[edge_index[1]] (duplicates
 * counted, loops kept): the CSC side of the unpartitioned graph built with add_loops = 0, remove_loops = 0
 * (SNGNN_EINVAL otherwise) - sngnn_adj_linear_forward's orientation.  orders_weight NULL is order_func1 (k = 0 .. orders,
 * w_k = 1), otherwise order_func2 (k = 1 .. orders, w_k = orders_weight[k - 1], dev f32 [orders]).  alpha, beta, gamma
 * act in double; alpha + beta == 0 or gamma == 1: SNGNN_EINVAL.  No floating-point atomics: the same bits on every
 * run.  Every entry only enqueues.
 *
 * sngnn_glognn_gram: out = (a - sub_scale a_sub)^T b and out2 = a2^T b, dev f64 [C, C], from one read of b; a_sub NULL:
 *   a^T b; a2 and out2 NULL together: one product.  a, a_sub, a2, b dev f32 [N, C].  32-row tiles through LDS,
 *   products and sums in double, per-workgroup partials added in workgroup order.
 *   workspace: sngnn_glognn_gram_workspace_bytes(C) (the first bytes of sngnn_glognn_workspace_bytes's buffer serve).
 * sngnn_glognn_solve: M, T, V, W dev f64 [C, C] and MT32 dev f32 [2, C, C] (M, then T, rounded) from G: one
 *   workgroup, Gauss-Jordan in double without pivoting (the matrix is SPD, smallest eigenvalue >= coe2^2).
 * sngnn_glognn_solve_backward: from gM = scale_m gM, gT = scale_t gT (dev f64 [C, C], the gradients of M and T):
 *   gV = s gM D + s G D gT D,  gG = s D gT D V - coe V gV V,  gG2 = gG + gG^T,
 *   grad_diag = s colsum(V o gM) + s rowsum((W D) o gT) + s colsum((D W) o gT)   (dev f64 [C]; NULL: not wanted).
 *   tmp dev f64 [2, C, C].
 * sngnn_glognn_forward: the hops t_k = A t_{k-1} (unweighted row gather-sums on the row classes of the other gather
 *   kernels: lane group, wave, 128-entry tasks + a finalize), S += w_k t_k in their stores, the mix in the last hop's
 *   store (M, T in LDS, each C x C product per row accumulated in double).  x, h0, S, out dev f32 [N, C], rows aligned
 *   to 4 * vec bytes; S is kept for the backward.
 * sngnn_glognn_backward: q = beta g M^T, grad_h0 = gamma g - gamma coe1 g T^T and grad_x = coe1 g T^T [+ q] in a row-
 *   local pass; r_0 = q, r_k = A^T r_{k-1} on the CSR side with grad_x += w_k r_k in the stores and x gG2 folded into
 *   the last one; grad_w dev f64 [orders] = <r_k, x> (NULL: not wanted) from per-workgroup partial dots in double,
 *   added by a reducer in a fixed order.  gG2 is sngnn_glognn_solve_backward's, from gM = beta S^T g and
 *   gT = coe1 (x - gamma h0)^T g (sngnn_glognn_gram).
 *   workspace: sngnn_glognn_workspace_bytes(g, C, orders) - the gram partials, two iterates [N, C], the split rows'
 *   task partials of either side and the dot partials.
 */
#define SNGNN_GLOGNN_MAX_C 64
int64_t sngnn_glognn_gram_workspace_bytes(int C);
int sngnn_glognn_gram(const float *a, const float *a_sub, double sub_scale, const float *a2, const float *b, int64_t N,
                      int C, double *out, double *out2, void *workspace, void *stream);
int sngnn_glognn_solve(const double *G, const float *diag, double alpha, double beta, double gamma, int C, double *M,
                       double *T, double *V, double *W, float *MT32, void *stream);
int sngnn_glognn_solve_backward(const double *gM, const double *gT, double scale_m, double scale_t, const double *G,
                                const double *V, const double *W, const float *diag, double alpha, double beta,
                                double gamma, int C, double *gG2, double *grad_diag, double *tmp, void *stream);
int64_t sngnn_glognn_workspace_bytes(const sngnn_graph_t *g, int C, int orders);
int sngnn_glognn_forward(const sngnn_graph_t *g, const float *x, const float *h0, const float *MT32,
                         const float *orders_weight, int orders, double beta, double gamma, int C, float *S, float *out,
                         void *workspace, void *stream);
int sngnn_glognn_backward(const sngnn_graph_t *g, const float *grad_out, const float *x, const float *MT32,
                          const double *gG2, const float *orders_weight, int orders, double beta, double gamma, int C,
                          float *grad_x, float *grad_h0, double *grad_w, void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * LINKX's join of the two embeddings (models/models.py:1098-1146): csrc/linkx.hip.
 * ------------------------------------------------------------------------ */
/*
 * Replaces: models.py:1135-1143 - the log_softmax at the end of mlpA's and mlpX's MLP.forward (:476), torch.cat,
 * self.W, the two adds and F.relu (inner_dropout and inner_activation off):
 *     a = log_softmax(zA), x = log_softmax(zX)     (lsm == 0: a = zA, x = zX)
 *     y = relu(a Wa^T + x Wx^T + b + a + x),       W = [Wa | Wx]
 * for the last linears' outputs zA, zX of the two MLPs.  Row-local, no graph: the rows are streamed once in 32-row
 * tiles (64 rows and 512 threads above H = 64) through LDS with W resident in LDS - both H x H halves for H <= 96, one after the other (two launches, the
 * same bits) above; the row's maximum and sum (of fp32 exponentials, added and logged in double) are taken in the tile
 * before the product; a dot product is four
 * interleaved fp32 fma chains added pairwise; per element t = dotA + a, t + dotX, + b, + x, max(., 0), every product
 * and sum rounded separately, fixed order, no atomics.
 *   zA, zX  dev f32 [N, H]      W  dev f32 [H, 2H] row-major (W.weight)      b  dev f32 [H]
 *   ax      dev f32 [N, 2H]     [a | x]: the one tensor the backward saves - sngnn_linear_wgrad(g, ax) with F = 2H
 *                               is the weight gradient
 *   y       dev f32 [N, H]
 * 1 <= H <= SNGNN_LINKX_MAX_H (sngnn_linkx_join_supported; SNGNN_ERANGE otherwise), any N >= 0; ax and y must not
 * alias the inputs (SNGNN_EINVAL).  Only enqueues.
 */
#define SNGNN_LINKX_MAX_H 128
int sngnn_linkx_join_supported(int H);
int sngnn_linkx_join_forward(const float *zA, const float *zX, const float *W, const float *b, int64_t N, int H, int lsm,
                             float *ax, float *y, void *stream);
/*
 * Replaces: autograd of the same lines w.r.t. the two embeddings, in one pass with the same tiling:
 *     g = grad_y [y > 0]                            (stored: the weight and bias gradients read it)
 *     tA = g + g Wa,  tX = g + g Wx
 *     grad_zA = tA - exp(a) sum_j tA_j              (lsm == 0: grad_zA = tA), the same for X, a and x read from ax
 *   grad_y, y  dev f32 [N, H]     ax  dev f32 [N, 2H]     W  dev f32 [H, 2H]
 *   g, grad_zA, grad_zX  dev f32 [N, H], distinct from the inputs and from each other (SNGNN_EINVAL)
 * Only enqueues.
 */
int sngnn_linkx_join_backward(const float *grad_y, const float *y, const float *ax, const float *W, int64_t N, int H,
                              int lsm, float *g, float *grad_zA, float *grad_zX, void *stream);

/* ------------------------------------------------------------------------
 * Jumping knowledge (models.py:810, 840, 869, 897): csrc/jk.hip.
 * ------------------------------------------------------------------------ */
/*
 * Replaces: JumpingKnowledge('max') - torch.stack(xs, -1).max(-1)[0] over the L layers' rows - without the stacked
 * [N, C, L] copy and the int64 index per element:
 *   out[i] = max_l xs[l][i], which[i] = the layer it came from, as a scan in layer order: b = x_0, idx = 0, layer l
 *   replaces b iff x_l > b || (isnan(x_l) && !isnan(b)).  These are torch's semantics exactly: the FIRST maximal layer
 *   wins a tie, +0 and -0 tie (the first one's bits are returned), the first NaN wins and sticks.
 *   xs      HOST array of L device pointers, each dev f32 [N, C] dense; read during the call (copied into the kernel's
 *           arguments): nothing is allocated, nothing synchronises
 *   out     dev f32 [N, C], must not alias an input (SNGNN_EINVAL)
 *   which   dev u8 [N, C], or NULL when no gradient is wanted
 * 1 <= L <= SNGNN_JK_MAX_LAYERS (SNGNN_ERANGE otherwise); C >= 1, N >= 0, no NULL row pointer (SNGNN_EINVAL);
 * N == 0 is a no-op.  16-byte accesses where every pointer is 16-byte aligned, scalar ones otherwise.  Only enqueues.
 */
#define SNGNN_JK_MAX_LAYERS 8
int sngnn_jk_max_forward(const float *const *xs, int L, int64_t N, int C, float *out, unsigned char *which, void *stream);
/*
 * Replaces: autograd of the same line - a scatter into a zeroed [N, C, L] tensor whose per-layer views are stride-L:
 *   grads[l][i] = which[i] == l ? grad_out[i] : 0 for every layer with a non-NULL grads[l] (a NULL entry: that layer
 *   wants no gradient).  Every element of every wanted layer is stored: no zero fill is needed before the call.
 *   grads   HOST array of L device pointers (or NULL), each dev f32 [N, C] dense, distinct from grad_out and from each
 *           other (SNGNN_EINVAL)
 * Only enqueues.
 */
int sngnn_jk_max_backward(const float *grad_out, const unsigned char *which, int L, int64_t N, int C, float *const *grads,
                          void *stream);

/*
 * Measurement aid (no reference counterpart): while enabled, sngnn_agg_forward
 * records HIP events on the caller's stream around its launches;
 * sngnn_profile_last_forward waits for the last call and returns the device time (ms)
 * of the normalisation pass, of the main kernel and of what follows it on the caller's
 * stream (the split-row finalize launches), and of an EMPTY interval between two events -
 * what an event pair itself adds to each of the three figures on this stack.
 * sngnn_profile_enable(reps) with reps > 1: every launch of the forward is issued reps times
 * back to back between its two events (the launches are idempotent) and the three figures are
 * the intervals divided by reps - the average launch duration with the event pair's own cost
 * spread over reps launches.
 */
int sngnn_profile_enable(int on);
int sngnn_profile_last_forward(float *norm_ms, float *main_ms, float *fin_ms, float *empty_ms);
/*
 * Measurement aid (no reference counterpart): the memory work of the aggregation forward
 * (models.py:239,244-263: the gathers of PyG's propagate + the scatter-mean's output) with NONE of
 * its arithmetic, over the caller's own graph and feature table - the floor bench.py prints beside
 * the main kernel's time (roofline.gather_floor_ms / kernel_over_floor).
 *   mode 0: one coalesced 4C-byte row read per entry of the graph's own column list (CSR order);
 *   mode 1: the same + per owned node its own row read and an output row written to `out`
 *           (dev f32 [N, C]; NULL in mode 0) - every byte of SURVEY.md 8d's B_fwd.
 * table: dev f32 [N_total, C], C % 4 == 0, C <= 256; workspace: sngnn_gather_floor_workspace_bytes().
 */
int64_t sngnn_gather_floor_workspace_bytes(void);
int sngnn_gather_floor(const sngnn_graph_t *g, const float *table, int C, int mode, float *out,
                       void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * SNGNN++ adjacency-linear branch and blend.
 * ------------------------------------------------------------------------ */
/*
 * Replaces: models.py:124-130 - SparseTensor(row - row.min(), col)
 * .to_torch_sparse_coo_tensor() followed by Linear(num_nodes, C) on it:
 *   out0[i] = b + sum over edges e with src_e - src_min == i of W[:, dst_e].
 *   wt   dev f32 [N, C]  the TRANSPOSE of the reference's w.weight ([C, N]);
 *                        row d is W[:, d] so every gather is one contiguous row
 *   bias dev f32 [C] or NULL
 *   workspace: sngnn_graph_workspace_bytes(g, C) bytes, as for the aggregation
 */
int sngnn_adj_linear_forward(const sngnn_graph_t *g, const float *wt,
                             const float *bias, int C, float *out0,
                             void *workspace, void *stream);
/*
 * Gradient of the above w.r.t. wt:  dwt[d] = sum over in-edges e of d of
 * g0[src_e - src_min]  (dense [N, C], like the reference's dense w.weight.grad).
 */
int sngnn_adj_linear_backward(const sngnn_graph_t *g, const float *g0, int C,
                              float *dwt, void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * The callers on either side of the aggregation inside one training epoch
 * (SURVEY.md 8f rank 1): classification head and self.lin's weight gradient.
 * ------------------------------------------------------------------------ */
/*
 * Replaces: F.log_softmax (models.py:86,211,303) + F.nll_loss on the masked rows +
 * the accuracy count (train.py:81-84, 98-102, 112-116) by one pass over the logits.
 *   logits   dev f32 [N, C]     the last conv's output (before log_softmax)
 *   y        dev i64 [N]        labels
 *   row_mask dev u8  [N]        1 for the rows of the split (train/val/test mask)
 *   n_masked                    number of ones in row_mask (the mean's denominator)
 *   grad_logits dev f32 [N, C] or NULL: d loss / d logits (zero rows outside the mask)
 *   loss_and_correct dev f32 [2]: mean NLL over the masked rows, number of correct rows
 *   workspace: sngnn_head_workspace_bytes(N) bytes.  Deterministic (fixed-order sums).
 */
int64_t sngnn_head_workspace_bytes(int64_t N);
int sngnn_head_nll(const float *logits, const int64_t *y, const unsigned char *row_mask,
                   int64_t N, int C, int64_t n_masked, float *grad_logits,
                   float *loss_and_correct, void *workspace, void *stream);
/*
 * The same for TWO splits read off one forward: validate_step and test_step (train.py:92-117)
 * run the same eval-mode forward and differ in their mask.  row_sets dev u8 [N]: bit 0 = the row
 * is in split A, bit 1 = in split B; out4 dev f32 [4] = {mean NLL A, correct A, mean NLL B,
 * correct B}.  C <= 64.  Same per-row arithmetic and summation order as sngnn_head_nll.
 */
int sngnn_head_nll2(const float *logits, const int64_t *y, const unsigned char *row_sets,
                    int64_t N, int C, int64_t n_a, int64_t n_b, float *out4, void *workspace,
                    void *stream);
/*
 * Replaces: SNGNN++'s last line `beta * out_0 + (1 - beta) * out_1` (models.py:134) followed by the wrapper's
 * log_softmax and the harness' nll_loss / accuracy (models.py:86; train.py:81-84, 98-102, 112-116) in ONE pass:
 * sngnn_head_nll / _nll2 on the blend of two tensors, which is formed in registers with sngnn_blend_forward's
 * rounding and never stored unless logits_out is given.  sets = 1: sel != 0 marks the split's rows, metrics[2];
 * sets = 2: bit 0 / bit 1, metrics[4].  grad_logits (sets == 1, or NULL): d (mean NLL) / d logits, zero rows
 * outside the split - the tensor sngnn_blend_backward starts from.  C % 4 == 0, C <= 64
 * (sngnn_head_nll_blend_supported); workspace: sngnn_head_workspace_bytes(N).
 */
int sngnn_head_nll_blend_supported(int C);
int sngnn_head_nll_blend(const float *out0, const float *out1, const float *beta, const int64_t *y,
                         const unsigned char *sel, int64_t N, int C, int sets, int64_t n_a, int64_t n_b,
                         float *grad_logits, float *logits_out, float *metrics, void *workspace, void *stream);
/*
 * Replaces: autograd of self.lin w.r.t. its parameters (models.py:121,237,324):
 *   grad_weight [C, F] = grad_out^T [C, N] . x [N, F],  grad_bias [C] = sum_i grad_out[i]
 * (grad_bias may be NULL).  workspace: sngnn_linear_wgrad_workspace_bytes(N, C, F).
 */
/*
 * Replaces: self.lin's forward for narrow layers, h = x W^T + b with C <= 64
 * (models.py:121,237,324).  x dev f32 [N, F], weight dev f32 [C, F], bias dev f32 [C]
 * or NULL, h dev f32 [N, C].  fp32 in, fp32 out, an fp32 dot product's rounding: for F in
 * {32, 64, 128} the products run on the bf16 matrix cores after an EXACT three-way split of both
 * operands, accumulated in fp32 (knob 5 of sngnn_tuning_set: fp32 MFMAs instead); HBM-bound (x
 * read once).  An infinity or NaN in a row of x makes that output row NaN.
 */
int sngnn_linear_forward(const float *x, const float *weight, const float *bias,
                         int64_t N, int F, int C, float *h, void *stream);
/*
 * h = act > 0 ? (x W^T + b) * act_scale : 0, act dev f32 [N, C]: the input gradient g W of a layer
 * (x = g, weight = W^T) whose input `act` was the epilogue'd output of the layer before
 * (sngnn_agg_forward_epilogue): autograd's threshold_backward and dropout backward
 * (models.py:206-209) folded into the store.  Any F, C <= 64.
 */
int sngnn_linear_forward_masked(const float *x, const float *weight, const float *bias, int64_t N,
                                int F, int C, const float *act, float act_scale, float *h, void *stream);
/* The same mask as a pass of its own (for a consumer that did not fold it into its store):
 * grad_pre[q] = act[q] > 0 ? grad[q] * scale : 0 over n = N * C elements (may alias grad). */
int sngnn_epilogue_backward(const float *grad, const float *act, float scale, int64_t n, float *grad_pre,
                            void *stream);
/*
 * Replaces: self.lin followed by F.normalize (models.py:237-238, :121-122, :324-325 - adjacent
 * lines of every conv forward): h as above AND, from the same launch's epilogue, the unit rows
 * n = h / max(||h||, 1e-12), the clamped norms and (filt != NULL, C > 32) the fp16 filter rows -
 * bit for bit what sngnn_normalize_rows_filter computes from h (same summation tree, IEEE
 * square root and division), so sngnn_agg_forward_prepared can follow without a normalisation
 * pass.  C % 4 == 0, C <= 64, F in {16, 32, 64, 128}, and x, h, the unit rows and the filter rows each
 * below 2^31 - 64 MiB bytes (sngnn_linear_normalized_supported); beyond: sngnn_linear_forward and a
 * normalisation pass.
 */
int sngnn_linear_normalized_supported(int64_t N, int F, int C);
int sngnn_linear_forward_normalized(const float *x, const float *weight, const float *bias,
                                    int64_t N, int F, int C, float *h, float *n, float *nrm,
                                    void *filt, void *stream);
int64_t sngnn_linear_wgrad_workspace_bytes(int64_t N, int C, int F);
int sngnn_linear_wgrad(const float *grad_out, const float *x, int64_t N, int C, int F,
                       float *grad_weight, float *grad_bias, void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * Sim-GFA toolbox (SimGFAToolbox/dense.py).
 * ------------------------------------------------------------------------ */
/* dense.py:138-141: S = normalize(x) normalize(x)^T, dev f32 [N, N]. */
int sngnn_cosine_dense(const float *x, int64_t N, int64_t F, float *S, void *stream);
/*
 * Fused statistics of S without materialising it (dense.py:9-30, 104-130,
 * 144-149, 167-179): class_sum dev f64 [n_classes, n_classes] receives the sum
 * of S over every (class_i, class_j) block INCLUDING the diagonal, diag_sum dev
 * f64 [1] the sum of S's diagonal.  y dev int32 [N] (all zeros for the global
 * mean).  Both outputs must be zeroed by the caller.
 */
int sngnn_cosine_class_sums(const float *x, int64_t N, int64_t F, const int32_t *y,
                            int n_classes, double *class_sum, double *diag_sum,
                            void *stream);
/*
 * The distribution the reference's toolbox draws (plot.py:61: `sns.distplot(sim, bins=200)` on the `sim` of
 * dense.py:144-149) at any N - where dense.py:9-30 returns `None, mean` and nothing can be drawn: the histogram of
 * the N (N - 1) off-diagonal entries of S = normalize(x) normalize(x)^T in one scan of x, S never stored (the tile
 * engine of sngnn_knn_graph on the upper triangle, each pair counted twice; fp32 rounding: exact bf16 split or
 * fp32 MFMAs, knob 5).
 *   y       dev i32 [N] or NULL.  With y the counters have two rows: row 0 pairs with y_i == y_j, row 1 pairs
 *           with y_i != y_j; a NEGATIVE label is "unlabelled" and every pair with such a node counts in row 1.
 *   edges   dev f32 [bins + 1], ascending (not checked here); 1 <= bins <= 1024.  Value s belongs to bin b with
 *           edges[b] <= s < edges[b + 1], the last bin closed on the right (numpy's rule) - decided against this
 *           table itself, not against a formula.
 *   counts  dev u64 [groups][bins + 2], groups = y ? 2 : 1: slot 0 = values below edges[0], slots 1 .. bins the
 *           bins, slot bins + 1 = values above edges[bins].  Ordered pairs: a row block sums to the number of
 *           its pairs, all of them to N (N - 1).
 *   stats   dev f64 [3]: min, max (fp32 values) and sum (f64) of the counted entries.
 * Both outputs are overwritten (no zeroing by the caller); N <= 1: counts 0, stats = +inf, -inf, 0.  Only
 * enqueues on `stream`; integer atomics and fixed-order reductions: the same bits on every run.
 *   workspace: sngnn_cosine_hist_workspace_bytes(N, F, bins, groups)
 * Knob 10 of sngnn_tuning_set (measurement): copies of the per-workgroup counter table in LDS, 0 (default) = as
 * many as fit up to 16, 1 = one (plain same-address LDS atomics), 2 / 4 / 8 / 16.
 */
int64_t sngnn_cosine_hist_workspace_bytes(int64_t N, int64_t F, int bins, int groups);
int sngnn_cosine_hist(const float *x, int64_t N, int64_t F, const int32_t *y, const float *edges, int bins,
                      unsigned long long *counts, double *stats, void *workspace, void *stream);
/*
 * dense.py:152-164: per-edge cosine of raw features for an arbitrary COO edge
 * list: sim[e] = <n[a_e], n[b_e]>, a = edge_index[0], b = edge_index[1].
 */
int sngnn_edge_cosine(const float *x, int64_t N, int64_t F,
                      const int64_t *edge_index_dev, int64_t E, float *sim,
                      void *stream);
/*
 * dense.py:163 `scatter_mean(sim, edge_index[0], dim=0)` (torch_scatter) and
 * the per-node means of dense.py:85-96 / sparse.py:98-115: mean[m] = (sum of val[e] over the
 * entries with index[e] == m, added in ENTRY ORDER in fp32) / max(count, 1); an empty group
 * reads 0.  No atomics: the same additions in the same order as the CPU's serial scatter, on
 * every run.  val dev f32 [E], index dev int64 [E] with values in [0, M), mean dev f32 [M],
 * count dev int32 [M] or NULL.
 */
int sngnn_segment_mean(const float *val, const int64_t *index, int64_t E, int64_t M, float *mean,
                       int32_t *count, void *stream);
/*
 * sparse.py:8-14 without forming the product: entries (pair_a[p], pair_b[p]) of
 * M_n^T M_n, M_n = the column-normalised sparse input in CSC form (colptr int64
 * [n_cols + 1], rowidx int32 ascending inside a column, vals = the NORMALISED values).
 * What sparse.py's linked / neighbourhood statistics read out of the scipy product
 * row by row (sparse.py:45-120).  Synchronises the stream (range check of the pairs).
 */
int sngnn_sparse_pair_dot(const int64_t *colptr, const int32_t *rowidx, const float *vals,
                          int64_t n_cols, const int64_t *pair_a, const int64_t *pair_b,
                          int64_t n_pairs, float *out, void *stream);
/*
 * sparse.py:8-14 with the product kept SPARSE, at any number of columns (csrc/sparse_cosine.hip): S = M_n^T M_n,
 * M_n the column-normalised [rows, cols] input, coalesced, explicit zeros dropped, in BOTH layouts - by column
 * (colptr i64 [cols + 1], rowidx i32 ascending inside a column, vals f32) and by row (rowptr i64 [rows + 1],
 * colidx i32 ascending inside a row, rvals f32); all dev.  Row i of S holds every j that shares a row of M_n with
 * column i - the structural pattern: the diagonal is an ordinary entry, a sum that cancels to 0.0 stays, a zero
 * column gives an empty row - column ids ascending, and
 *     S[i, j] = sum_k M_n[k, i] * M_n[k, j]      k ascending, each product rounded, then added (fp32)
 * so a value's bits depend on the matrix alone.  One workgroup per row: a row whose candidate bound
 * sum_{k in col i} deg_row(k) is at most SNGNN_SPARSE_COSINE_HASH_MAX keeps keys and sums in LDS tables (sorted by
 * key), a larger one in a per-workgroup accumulator of `cols` floats and a bitmap in the workspace.  No
 * floating-point atomics; the same bits on every run.
 *   sngnn_sparse_cosine_count   count dev i32 [cols]: the exact number of entries of every row of S
 *   sngnn_sparse_cosine_fill    offsets dev i64 [cols]: the exclusive scan of count (the caller's), nnz its total;
 *                               out_col dev i32 [nnz], out_val dev f32 [nnz].  nnz > 2^31 - 1: SNGNN_ERANGE.
 *   sngnn_sparse_cosine_hist    the same rows, counted instead of stored - the distribution of ALL cols^2 entries of
 *                               S (diagonal != 0) or of its cols (cols - 1) off-diagonal ones (diagonal == 0), with
 *                               edges / bins / counts [bins + 2] / stats [3] as in sngnn_cosine_hist (one group):
 *                               numpy's bin rule against the table itself, on exactly the fp32 values the fill
 *                               stores; the entries outside the pattern are exact zeros, added arithmetically to
 *                               the slot that holds 0.0 and counted in min and max.  No limit on nnz.
 *   sngnn_sparse_cosine_topk    the same rows, selected instead of stored - the structural kNN graph, sngnn_knn_graph's
 *                               sibling: for every column i the k best of the entries the fill would store for row
 *                               i (the pattern only: a column outside it is no candidate, whatever the sign of the
 *                               entries; a sum that cancelled to 0.0 is one; (i, i) is one unless exclude_self != 0),
 *                               in the order (value descending, column id ascending), with the fill's fp32 values
 *                               bit for bit.  nbr_idx dev i32 [cols, k], nbr_sim dev f32 [cols, k]; a row with
 *                               fewer than k candidates is padded with -1 / 0.0 (a zero column: k pads).
 *                               1 <= k <= 32, else SNGNN_EINVAL.  A stored value is never -0.0 (the sums start at
 *                               +0.0), so the order of the values is the order of the floats.
 *   workspace, workspace_bytes  the matching sngnn_sparse_cosine_*_workspace_bytes(rows, cols[, bins | k]) at least
 *                               (less: SNGNN_EINVAL); cleared by each call.
 * rows, cols < 2^31 - 1 (SNGNN_ERANGE); NULL or a bad shape: SNGNN_EINVAL.  Refused calls launch nothing.  All
 * four only enqueue.
 */
#define SNGNN_SPARSE_COSINE_HASH_MAX 2048
int64_t sngnn_sparse_cosine_count_workspace_bytes(int64_t rows, int64_t cols);
int64_t sngnn_sparse_cosine_fill_workspace_bytes(int64_t rows, int64_t cols);
int64_t sngnn_sparse_cosine_hist_workspace_bytes(int64_t rows, int64_t cols, int bins);
int64_t sngnn_sparse_cosine_topk_workspace_bytes(int64_t rows, int64_t cols, int k);
int sngnn_sparse_cosine_count(const int64_t *colptr, const int32_t *rowidx, const int64_t *rowptr,
                              const int32_t *colidx, int64_t rows, int64_t cols, int32_t *count, void *workspace,
                              int64_t workspace_bytes, void *stream);
int sngnn_sparse_cosine_fill(const int64_t *colptr, const int32_t *rowidx, const float *vals, const int64_t *rowptr,
                             const int32_t *colidx, const float *rvals, int64_t rows, int64_t cols,
                             const int64_t *offsets, int64_t nnz, int32_t *out_col, float *out_val, void *workspace,
                             int64_t workspace_bytes, void *stream);
int sngnn_sparse_cosine_hist(const int64_t *colptr, const int32_t *rowidx, const float *vals, const int64_t *rowptr,
                             const int32_t *colidx, const float *rvals, int64_t rows, int64_t cols, const float *edges,
                             int bins, int diagonal, unsigned long long *counts, double *stats, void *workspace,
                             int64_t workspace_bytes, void *stream);
int sngnn_sparse_cosine_topk(const int64_t *colptr, const int32_t *rowidx, const float *vals, const int64_t *rowptr,
                             const int32_t *colidx, const float *rvals, int64_t rows, int64_t cols, int k,
                             int exclude_self, int32_t *nbr_idx, float *nbr_sim, void *workspace,
                             int64_t workspace_bytes, void *stream);

/*
 * kNN similarity graph (the north star's "Node-Similarity build"):
 * for every node the k most cosine-similar nodes, without storing the N x N similarity
 * the reference materialises (dense.py:138-141) - tiled matrix-core products (fp32 rounding:
 * exact bf16 split or fp32 MFMAs, knob 5) with a fused per-row top-k.  Order (cosine desc, node id asc), k <= 32.
 *   nbr_idx dev i32 [N, k]   neighbour ids in rank order, -1 padded when N - 1 < k
 *   nbr_sim dev f32 [N, k]   their cosines (0 padded)
 *   exclude_self             a node is not its own neighbour
 *   workspace: sngnn_knn_workspace_bytes(N, k)
 */
int64_t sngnn_knn_workspace_bytes(int64_t N, int k);
int sngnn_knn_graph(const float *x, int64_t N, int64_t F, int k, int exclude_self,
                    int32_t *nbr_idx, float *nbr_sim, void *workspace, void *stream);
/*
 * The same scan with two tables: for every QUERY row i of xq [M, F] the k rows j of the BASE xb [N, F] of largest
 * cosine <xq_i, xb_j> / (max(|xq_i|, eps) max(|xb_j|, eps)) - a rank's node range against all N nodes, held-out
 * nodes against a fixed base, the lists of some rows only.  Always the fused scan (no M x N matrix, no allocation,
 * only enqueues: capturable); engine variant by sngnn_knn_graph's rule - F, knobs 5 and 6 (3 / 4 pin the tile
 * shape; 0, 1, 2: by the rule), the 16-byte alignment of BOTH tables - and every value formed as there, so a row
 * range xq = xb + r0 F, self_offset = r0 returns rows [r0, r0 + M) of the fused square scan bit for bit.
 *   nbr_idx dev i32 [M, k]   base ids in rank order (cosine desc, base id asc), -1 padded when fewer than k are eligible
 *   nbr_sim dev f32 [M, k]   their cosines (0 padded)
 *   self_offset >= 0         base row self_offset + i is not eligible for query i (self_offset + M <= N);
 *               == -1        every base row is eligible
 *   xq may point into xb; both are read-only and the outputs must not overlap them.  M == 0: nothing is launched;
 *   N == 0: every slot is padding.  k in [1, 32], M, N < 2^31.
 *   workspace: sngnn_knn_query_workspace_bytes(M, N, k) - both tables' inverse norms and, few query rows against many
 *   base rows being cut into up to 320 column ranges, their partial lists (M = 128, k = 32: ~10 MB)
 */
int64_t sngnn_knn_query_workspace_bytes(int64_t M, int64_t N, int k);
int sngnn_knn_query(const float *xq, int64_t M, const float *xb, int64_t N, int64_t F, int k, int64_t self_offset,
                    int32_t *nbr_idx, float *nbr_sim, void *workspace, void *stream);
/*
 * The threshold (epsilon-neighbourhood) graph of the same two tables: for every query row i EVERY eligible base row j
 * with cosine s_ij >= thr, as CSR - a row has as many entries as the cut gives it, none or thousands, where the kNN
 * lists stop at 32.  No M x N matrix: the scan of sngnn_knn_query runs twice, a count pass and a fill pass around the
 * caller's exclusive scan (csrc/cosine_thresh_scan.h).
 *   Entry rule: (i, j) is an entry iff base row j is eligible for query i - sngnn_knn_query's rule: self_offset = r >= 0
 *   excludes base row r + i, -1 excludes nothing - and s_ij >= thr in fp32 (a cosine of exactly thr IS an entry; a NaN
 *   value is none; thr = -inf keeps every eligible pair).  s_ij is the value sngnn_knn_query forms for the same tables
 *   and knob state - acc * (inv_i * inv_j) + 0.0f on the same engine variant (F, knobs 5 and 6, the 16-byte alignment
 *   of both tables) - so a stored value is never -0.0 and a row range has the square call's rows bit for bit.
 *   Non-finite table entries are outside the contract.
 * sngnn_cosine_threshold_count   count dev i32 [M]: the exact number of entries of every row (overwritten; the caller
 *                                zeroes nothing).
 * sngnn_cosine_threshold_fill    rowptr dev i64 [M + 1]: the caller's exclusive scan of count, nnz its total.  Row i's
 *                                entries go to [rowptr[i], rowptr[i + 1]) of out_col dev i32 [nnz] / out_val dev f32
 *                                [nnz], column ids ASCENDING.  nnz > 2^31 - 1: SNGNN_ERANGE.
 *                                The fill RELIES on what the matching count call left in the workspace - both tables'
 *                                inverse norms and, per column range, the number of a row's entries in the ranges
 *                                before it: call it with the count's arguments (tables, shapes, thr, self_offset, knob
 *                                state) and the count's workspace, with nothing else using that workspace in between.
 * NaN thr, NULL, a bad shape, self_offset + M > N, M or N >= 2^31: SNGNN_EINVAL; a refused call launches nothing.
 * M == 0 launches nothing; N == 0: every count is 0.  No atomics: the same bits on every run.  Both only enqueue on
 * `stream` (capturable).
 *   workspace: sngnn_cosine_threshold_workspace_bytes(M, N) - the inverse norms and 4 bytes per row and column range
 *   (up to 320 ranges when there are few query rows)
 */
int64_t sngnn_cosine_threshold_workspace_bytes(int64_t M, int64_t N);
int sngnn_cosine_threshold_count(const float *xq, int64_t M, const float *xb, int64_t N, int64_t F, float thr,
                                 int64_t self_offset, int32_t *count, void *workspace, void *stream);
int sngnn_cosine_threshold_fill(const float *xq, int64_t M, const float *xb, int64_t N, int64_t F, float thr,
                                int64_t self_offset, const int64_t *rowptr, int64_t nnz, int32_t *out_col,
                                float *out_val, void *workspace, void *stream);
/*
 * The cosine scans straight from an fp16 / bf16 table (2 F bytes a row, read as stored - no fp32 copy): the kNN graph,
 * the two-table query and the histogram above on the tile engine's half forms.  A value of such a table has two
 * (fp16) resp. one (bf16) of the three bf16 planes the fp32 scan splits a float into; the planes it has are used as
 * they are and only their products are issued - 4 resp. 1 of the 8 matrix instructions per product - in the fp32
 * scan's order.  Inverse norms, selection, counting and statistics are the fp32 entries'.  On a table of finite
 * values the outputs are those of the fp32 fused scan on the widened table, bit for bit (the planes left out are
 * exactly +0.0 there; csrc/cosine_tiles.h).  A non-finite entry is outside that statement.
 *   dtype   SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16, the type of every table of the call (anything else: SNGNN_EINVAL
 *           with "dtype" in sngnn_last_error(), before any pointer is looked at)
 *   sngnn_cosine_scan_half_supported   1 iff the native scan exists for the knobs as they stand: dtype as above, F in
 *           {32, 64, 96, 128}, knob 5 off (bf16 products) and knob 6 not 3 (the half forms have the 256 x 64 tile only)
 *   sngnn_knn_graph_route              1: sngnn_knn_graph would run the fused scan on N rows (knob 6 as it stands),
 *           2: it would materialise S and select.  sngnn_knn_graph_half ALWAYS runs the fused scan; a caller that
 *           wants the fp32 call's route on small tables asks here first.
 * Refused with SNGNN_EINVAL, nothing launched: what sngnn_cosine_scan_half_supported refuses, a table whose base is
 * not 16-byte aligned, and whatever the fp32 entry refuses (k, shapes, NULL, self_offset).  The empty shapes behave
 * as in the fp32 entries.  Only enqueue on `stream`.
 *   workspace: sngnn_knn_workspace_bytes(N, k) / sngnn_knn_query_workspace_bytes(M, N, k) /
 *              sngnn_cosine_hist_workspace_bytes(N, F, bins, groups) - the fp32 entries' sizes
 */
int sngnn_cosine_scan_half_supported(int64_t F, int dtype);
int sngnn_knn_graph_route(int64_t N);
int sngnn_knn_graph_half(const void *x, int dtype, int64_t N, int64_t F, int k, int exclude_self,
                         int32_t *nbr_idx, float *nbr_sim, void *workspace, void *stream);
int sngnn_knn_query_half(const void *xq, int64_t M, const void *xb, int dtype, int64_t N, int64_t F, int k,
                         int64_t self_offset, int32_t *nbr_idx, float *nbr_sim, void *workspace, void *stream);
int sngnn_cosine_hist_half(const void *x, int dtype, int64_t N, int64_t F, const int32_t *y, const float *edges,
                           int bins, unsigned long long *counts, double *stats, void *workspace, void *stream);
/*
 * The threshold graph straight from two fp16 / bf16 tables: sngnn_cosine_threshold_count / _fill on the same half
 * forms (csrc/cosine_thresh_half.hip).  BOTH passes read the tables as stored and issue 4 (fp16) resp. 1 (bf16) of the
 * 8 matrix instructions per product; inverse norms (the fp32 chain on the widened values), entry rule, value
 * expression, column ranges and the range prefix are the fp32 pair's.  On tables of finite values count, out_col and
 * out_val are those of the fp32 pair on the widened tables, bit for bit; a non-finite entry is outside that statement.
 *   dtype   SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16, the type of BOTH tables
 * Refused, nothing launched and no output or workspace byte written: everything the fp32 pair refuses (shapes, NaN
 * thr, self_offset, nnz - SNGNN_ERANGE past 2^31 - 1 -, NULL), a dtype that is neither half type, what
 * sngnn_cosine_scan_half_supported(F, dtype) refuses, and a table whose base is not 16-byte aligned (SNGNN_EINVAL).
 * M == 0, N == 0 and nnz == 0 behave as in the fp32 pair.  The count / fill contract is the fp32 pair's: the fill of
 * THIS pair is called with the arguments and the workspace of the count of THIS pair, nothing in between on that
 * workspace (the fp32 count's column ranges may differ).  Both only enqueue on `stream` (capturable).
 *   workspace: sngnn_cosine_threshold_workspace_bytes(M, N) - the fp32 pair's size and layout
 */
int sngnn_cosine_threshold_count_half(const void *xq, int64_t M, const void *xb, int dtype, int64_t N, int64_t F,
                                      float thr, int64_t self_offset, int32_t *count, void *workspace, void *stream);
int sngnn_cosine_threshold_fill_half(const void *xq, int64_t M, const void *xb, int dtype, int64_t N, int64_t F,
                                     float thr, int64_t self_offset, const int64_t *rowptr, int64_t nnz,
                                     int32_t *out_col, float *out_val, void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * R replicas of one 1-layer model trained together (sngnn_amd/splits.py): the sweep scripts'
 * ten geom-gcn splits (train_script_SNGNN{,_plus,_plus_plus}.sh: part_id 0..9, one process each)
 * and SNGNN++'s init_beta grid in one job.  Replica r's node i is row r N + i of a block-diagonal
 * union graph (the aggregation entries above run on it unchanged); the entries below are the
 * per-replica parts of lin, the head and the blend.  Every sum is fixed-order; none blocks the host.
 * ------------------------------------------------------------------------ */
/*
 * Replaces: R separate `self.lin(x)` bias adds and F.normalize passes (models.py:121-122, 237-238,
 * 324-325, one process per split).  hs dev f32 [N, R C] = x W_stacked^T (one GEMM over the stacked
 * [R C, F] weights: x read once); bias dev f32 [R, C] or NULL.  Writes the union table
 * h [R N, C] (row r N + i = hs[i, r C .. r C + C) + bias[r]) and, n / nrm non-NULL, the unit rows,
 * the clamped norms and (filt non-NULL) the fp16 filter rows - bit for bit what
 * sngnn_normalize_rows_filter computes from h - in the same pass.
 */
int sngnn_replica_unpack(const float *hs, const float *bias, int64_t N, int R, int C, float *h, float *n,
                         float *nrm, void *filt, void *stream);
/*
 * Replaces: R calls of sngnn_linear_wgrad (autograd of self.lin, models.py:121,237,324 - one per split's
 * process): grad_weight [R C, F] (block r = G_r^T x), grad_bias [R C] (may be NULL), G = grad_out dev f32
 * [R N, C] in the union layout, x read once per 64 stacked channels.  Per element the summation order of
 * sngnn_linear_wgrad's FMA path (the one it takes unless F is 16, 32, 64 or 128 and N >= 1024):
 * replica r's result equals that call on G_r bit for bit there.
 * workspace: sngnn_replica_wgrad_workspace_bytes(N, R, C, F).
 */
int64_t sngnn_replica_wgrad_workspace_bytes(int64_t N, int R, int C, int F);
int sngnn_replica_wgrad(const float *grad_out, const float *x, int64_t N, int R, int C, int F,
                        float *grad_weight, float *grad_bias, void *workspace, void *stream);
/*
 * Replaces: per split's process, log_softmax (models.py:86,211,303) + nll_loss on the split's rows +
 * the accuracy count (train.py:81-84, 98-102, 112-116).  logits dev f32 [R N, C] (C <= 64); with
 * logits1 / beta dev f32 [R] non-NULL the logits are SNGNN++'s blend beta[r] logits + (1 - beta[r])
 * logits1 (models.py:134) formed in registers.  y dev i64 [N] (shared); sel dev u8 [R, N]: sets = 1,
 * nonzero = the replica's split; sets = 2, bit 0 / bit 1 = splits A / B.  counts dev i64 [R sets]: the
 * rows of each split (the mean's divisor).  metrics row r (at metrics + r metrics_stride) = {loss,
 * correct} per split.  grad_logits (sets == 1, or NULL) [R N, C]: d (mean NLL_r) / d logits.
 * Replica r's results equal sngnn_head_nll / _nll2 / _nll_blend on its rows bit for bit.
 * workspace: sngnn_replica_head_workspace_bytes(R).
 */
int64_t sngnn_replica_head_workspace_bytes(int R);
int sngnn_replica_head_nll(const float *logits, const float *logits1, const float *beta, const int64_t *y,
                           const unsigned char *sel, const int64_t *counts, int64_t N, int R, int C, int sets,
                           float *grad_logits, float *metrics, int64_t metrics_stride, void *workspace,
                           void *stream);
/*
 * Replaces: R calls of sngnn_blend_forward / _backward (models.py:134) with one beta per replica:
 * n elements per replica, replica r's slice at offset r n; grad_beta dev f32 [R].  Per replica the grid
 * and reduction tree of the single call (bit for bit when n % 4 == 0).
 * workspace: sngnn_replica_blend_workspace_bytes(R).
 */
int64_t sngnn_replica_blend_workspace_bytes(int R);
int sngnn_replica_blend_forward(const float *out0, const float *out1, const float *beta, int64_t n, int R,
                                float *out, void *stream);
int sngnn_replica_blend_backward(const float *grad_out, const float *out0, const float *out1,
                                 const float *beta, int64_t n, int R, float *grad0, float *grad1,
                                 float *grad_beta, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNGNN_HIP_H */

// C-ABI entry of the aggregation backward (kernels: agg_bwd_impl.h).
#include "agg_bwd_impl.h"
#include "entry.h"

using namespace sngnn;

// sngnn_tuning_set(3, v): 0 = node-centric backward when most nodes are fused work items (default),
// 1 = the two passes for every node, 2 = node-centric whatever the graph (the same bits;
// measurement / test aid)
static int g_bwd_mode = 0, g_bwd_roles = 3;
int sngnn::set_bwd_mode(int v) { g_bwd_mode = (v == 1 || v == 2) ? v : 0; return SNGNN_OK; }
int sngnn::set_bwd_roles(int v) { g_bwd_roles = v & 7; return SNGNN_OK; }

extern "C" int sngnn_agg_backward(const sngnn_graph_t *g, const float *h, int C,
                                  const float *grad_out, const float *wsel, float *grad_h,
                                  void *workspace, void *stream)
{
    return sngnn_agg_backward_topk(g, h, C, grad_out, wsel, -1, grad_h, workspace, stream);
}

// whether a forward with this top_k can write the kept bits itself AND the backward that would read
// them is the hinted node-centric one (agg_fwd.hip asks the same question)
static bool node_centric(const sngnn_graph_t *g)
{
    const bool mostly_fused = (int64_t)g->n_fused * 2 >= g->N;
    return g_bwd_mode == 2 || (g_bwd_mode == 0 && mostly_fused);
}
bool sngnn::kept_bits_path(const sngnn_graph_t *g, int top_k)
{
    return g != nullptr && g->csc_bit != nullptr && g->N == g->Ntot && top_k >= 1 && top_k <= SMALL_T && node_centric(g) &&
           !fwd_scores_on_the_fly_forced();       // (the forward writes the bits in table mode only)
}

static int backward_impl(const sngnn_graph_t *g, const float *h, int C, const float *grad_out, const float *wsel,
                         const unsigned *kbits, int top_k, float *grad_h, void *workspace, void *stream,
                         int dtype = 0);

extern "C" int sngnn_agg_backward_topk(const sngnn_graph_t *g, const float *h, int C,
                                       const float *grad_out, const float *wsel, int top_k,
                                       float *grad_h, void *workspace, void *stream)
{
    SN_REQUIRE(g == nullptr || wsel != nullptr || g->Ep == 0, SNGNN_EINVAL, "wsel is NULL");
    return backward_impl(g, h, C, grad_out, wsel, nullptr, top_k, grad_h, workspace, stream);
}

extern "C" int sngnn_agg_backward_bits(const sngnn_graph_t *g, const float *h, int C, const float *grad_out,
                                       const void *kept_bits, int top_k, float *grad_h, void *workspace,
                                       void *stream)
{
    SN_REQUIRE(g != nullptr && kept_bits != nullptr, SNGNN_EINVAL, "graph / kept_bits is NULL");
    SN_REQUIRE(kept_bits_path(g, top_k), SNGNN_EINVAL,
               "no kept-bit path for this graph / top_k (sngnn_agg_kept_bits_supported)");
    return backward_impl(g, h, C, grad_out, nullptr, (const unsigned *)kept_bits, top_k, grad_h, workspace, stream);
}

// the half path: h, grad_out and grad_h stored as fp16 / bf16 (everything else as in sngnn_agg_backward_topk)
extern "C" int sngnn_agg_backward_half(const sngnn_graph_t *g, const void *h, int dtype, int C, const void *grad_out,
                                       const float *wsel, int top_k, void *grad_h, void *workspace, void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    SN_REQUIRE(g == nullptr || wsel != nullptr || g->Ep == 0, SNGNN_EINVAL, "wsel is NULL");
    return backward_impl(g, (const float *)h, C, (const float *)grad_out, wsel, nullptr, top_k, (float *)grad_h,
                         workspace, stream, dtype);
}

static int backward_impl(const sngnn_graph_t *g, const float *h, int C, const float *grad_out, const float *wsel,
                         const unsigned *kbits, int top_k, float *grad_h, void *workspace, void *stream, int dtype)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    if (g->Ntot == 0) return SNGNN_OK;
    SN_REQUIRE(h && grad_h && workspace && (grad_out || g->N == 0), SNGNN_EINVAL, "NULL argument");
    RowCfg cfg;
    if (int rc = check_rows(C, dtype, {h, grad_out, grad_h}, cfg)) return rc;
    const BwdLayout L = bwd_layout(g, C, false);
    BwdArgs a;
    bind_bwd_graph(g, C, L, workspace, a);
    a.h = h; a.gout = grad_out; a.wsel = wsel; a.grad_h = grad_h;
    // (the kept-bit mask lives in the first words of the records' region; the attention mode keeps records there)
    a.wd = nullptr; a.rec_dot = nullptr;
    a.kmask = (unsigned *)((char *)workspace + L.rec);
    a.kmask_words = (g->Ep + 31) / 32;
    a.inv_deg = g->inv_deg;
    // The node-centric path pays when most nodes are FUSED work items (small both as target and as
    // source: four nodes per wave, both passes in one go) - 95 % at arxiv's degree law, where it wins
    // at every size tried (x1 .. x32: 1.2 M .. 37 M edges, 60 vs 77 us .. 2.26 vs 2.72 ms).  Where
    // nodes mostly have 17..128 out-edges (products' degree law: no fused node at all) every node
    // would be a wave-per-node item, one node per wave with a longer dependent chain than either
    // pass has: 4.9 ms against the two passes' 4.2 ms at products size.  So: node-centric when at
    // least half of the owned nodes are fused.
    a.mode = node_centric(g) ? 0 : 1;   // (knob 3 = 2: node-centric whatever the graph - measurement)
    a.top_k = top_k;
    a.role_mask = g_bwd_roles;
    a.fdesc = g->fdesc; a.trest = g->trest;
    a.n_fused = g->n_fused; a.n_trest = g->n_trest;
    a.kbits = kbits; a.csc_bit = g->csc_bit; a.kb_wbase = (int)g->kb_wbase; a.kb_tbase = (int)g->kb_tbase;
    a.s_small_end = a.mode == 0 ? g->srcs_gt(SMALL_T - 1) : (int)g->Ntot;
    return SNGNN_LAUNCH_VEC(launch_agg_bwd_vec, cfg, dtype, a, (hipStream_t)stream);
}

// C-ABI entries of the cosine-attention mode (kernels: attn_impl.h).
#include "attn_impl.h"
#include "entry.h"

using namespace sngnn;

// dtype: 0 = fp32 rows, else SNGNN_DTYPE_F16 / SNGNN_DTYPE_BF16 (2 bytes a value)
// h and out are float rows for dtype 0, else rows of the half type behind the same pointers
static int forward_impl(const sngnn_graph_t *g, const float *h, int dtype, int C, float *out, float *alpha,
                        void *workspace, void *stream)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(h && out, SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(workspace != nullptr || g->n_tasks == 0, SNGNN_EINVAL, "workspace is NULL");
    RowCfg cfg;
    if (int rc = check_rows(C, dtype, {h, out}, cfg)) return rc;
    AttnArgs a;
    a.h = h; a.C = C; a.N = (int)g->N; a.row_off = (int)g->row_off;
    a.col = g->col; a.rdesc = g->rdesc;
    a.out = out; a.alpha = alpha;
    bind_side(g, false, a);
    a.partial = workspace ? (float *)((char *)workspace + attn_fwd_layout(g->n_tasks, C).partial) : nullptr;
    a.nbA = a.nbB = 0;
    return SNGNN_LAUNCH_VEC(launch_attn_fwd_vec, cfg, dtype, a, (hipStream_t)stream);
}

extern "C" int sngnn_attn_forward(const sngnn_graph_t *g, const float *h, int C, float *out,
                                  float *alpha, void *workspace, void *stream)
{
    return forward_impl(g, h, 0, C, out, alpha, workspace, stream);
}

// the half path: h and out stored as fp16 / bf16 (alpha and the workspace as in sngnn_attn_forward)
extern "C" int sngnn_attn_forward_half(const sngnn_graph_t *g, const void *h, int dtype, int C, void *out,
                                       float *alpha, void *workspace, void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    return forward_impl(g, (const float *)h, dtype, C, (float *)out, alpha, workspace, stream);
}

static int backward_impl(const sngnn_graph_t *g, const float *h, int dtype, int C, const float *grad_out,
                         const float *alpha, float *grad_h, void *workspace, void *stream)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    if (g->Ntot == 0) return SNGNN_OK;
    SN_REQUIRE(h && grad_h && workspace && (grad_out || g->N == 0), SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(alpha != nullptr || g->Ep == 0, SNGNN_EINVAL, "alpha is NULL");
    RowCfg cfg;
    if (int rc = check_rows(C, dtype, {h, grad_out, grad_h}, cfg)) return rc;
    const BwdLayout L = bwd_layout(g, C, true);
    BwdArgs a;
    bind_bwd_graph(g, C, L, workspace, a);
    a.h = h; a.gout = grad_out; a.wsel = alpha; a.grad_h = grad_h;
    a.wd = (float2 *)((char *)workspace + L.rec);
    a.rec_dot = (float *)((char *)workspace + L.rec_dot);
    a.kmask = nullptr; a.kmask_words = 0; a.inv_deg = nullptr;
    a.mode = 1; a.top_k = -1; a.role_mask = 3; a.s_small_end = (int)g->Ntot;
    a.fdesc = nullptr; a.trest = nullptr; a.n_fused = a.n_trest = 0;
    a.kbits = nullptr; a.csc_bit = nullptr; a.kb_wbase = a.kb_tbase = 0;
    return SNGNN_LAUNCH_VEC(launch_attn_bwd_vec, cfg, dtype, a, (hipStream_t)stream);
}

extern "C" int sngnn_attn_backward(const sngnn_graph_t *g, const float *h, int C,
                                   const float *grad_out, const float *alpha, float *grad_h,
                                   void *workspace, void *stream)
{
    return backward_impl(g, h, 0, C, grad_out, alpha, grad_h, workspace, stream);
}

// the half path: h, grad_out and grad_h stored as fp16 / bf16 (alpha, the records and every scratch row stay fp32)
extern "C" int sngnn_attn_backward_half(const sngnn_graph_t *g, const void *h, int dtype, int C, const void *grad_out,
                                        const float *alpha, void *grad_h, void *workspace, void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    return backward_impl(g, (const float *)h, dtype, C, (const float *)grad_out, alpha, (float *)grad_h, workspace,
                         stream);
}

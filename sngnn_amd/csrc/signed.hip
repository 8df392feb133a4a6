// C-ABI entries of the signed cosine-attention mode (kernels: signed_impl.h).
#include "signed_impl.h"
#include "entry.h"

using namespace sngnn;

// dtype: 0 = fp32 rows, else SNGNN_DTYPE_F16 / SNGNN_DTYPE_BF16 (2 bytes a value)
// wh and out are float rows for dtype 0, else rows of the half type behind the same pointers
static int forward_impl(const sngnn_graph_t *g, const float *wh, int dtype, int C, const float *coef, const float *c2,
                        float *out, float *s, void *workspace, void *stream)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    if (g->N == 0) return SNGNN_OK;
    SN_REQUIRE(wh && out && c2 && (coef || g->Ep == 0), SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE(workspace != nullptr || g->n_tasks == 0, SNGNN_EINVAL, "workspace is NULL");
    RowCfg cfg;
    if (int rc = check_rows(C, dtype, {wh, out}, cfg)) return rc;
    SignedArgs a;
    a.h = wh; a.coef = coef; a.c2 = c2; a.C = C; a.N = (int)g->N; a.row_off = (int)g->row_off;
    a.col = g->col; a.rdesc = g->rdesc;
    a.out = out; a.s = s;
    bind_side(g, false, a);
    a.partial = workspace ? (float *)((char *)workspace + signed_fwd_layout(g->n_tasks, C).partial) : nullptr;
    a.nbA = a.nbB = 0;
    return SNGNN_LAUNCH_VEC(launch_signed_fwd_vec, cfg, dtype, a, (hipStream_t)stream);
}

extern "C" int sngnn_signed_forward(const sngnn_graph_t *g, const float *wh, int C, const float *coef,
                                    const float *c2, float *out, float *s, void *workspace, void *stream)
{
    return forward_impl(g, wh, 0, C, coef, c2, out, s, workspace, stream);
}

// the half path: wh and out stored as fp16 / bf16 (coef, c2, s and the workspace as in sngnn_signed_forward)
extern "C" int sngnn_signed_forward_half(const sngnn_graph_t *g, const void *wh, int dtype, int C, const float *coef,
                                         const float *c2, void *out, float *s, void *workspace, void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    return forward_impl(g, (const float *)wh, dtype, C, coef, c2, (float *)out, s, workspace, stream);
}

static int backward_impl(const sngnn_graph_t *g, const float *wh, int dtype, int C, const float *grad_out,
                         const float *coef, const float *s, const float *c2, float *grad_wh, float *u,
                         void *workspace, void *stream)
{
    SN_REQUIRE(g != nullptr, SNGNN_EINVAL, "graph is NULL");
    if (g->Ntot == 0) return SNGNN_OK;
    SN_REQUIRE(wh && grad_wh && workspace && c2 && (grad_out || g->N == 0), SNGNN_EINVAL, "NULL argument");
    SN_REQUIRE((coef && s && u) || g->Ep == 0, SNGNN_EINVAL, "coef / s / u is NULL");
    RowCfg cfg;
    if (int rc = check_rows(C, dtype, {wh, grad_out, grad_wh}, cfg)) return rc;
    const BwdLayout L = bwd_layout(g, C, true);
    BwdArgs a;
    bind_bwd_graph(g, C, L, workspace, a);
    a.h = wh; a.gout = grad_out; a.wsel = s; a.grad_h = grad_wh;
    a.wd = (float2 *)((char *)workspace + L.rec); a.rec_dot = nullptr;       // (final records)
    a.kmask = nullptr; a.kmask_words = 0; a.inv_deg = nullptr;
    a.mode = 1; a.top_k = -1; a.role_mask = 3; a.s_small_end = (int)g->Ntot;
    a.fdesc = nullptr; a.trest = nullptr; a.n_fused = a.n_trest = 0;
    a.kbits = nullptr; a.csc_bit = nullptr; a.kb_wbase = a.kb_tbase = 0;
    SignedBwdExtra x;
    x.coef = coef; x.c2 = c2; x.u = u;
    return SNGNN_LAUNCH_VEC(launch_signed_bwd_vec, cfg, dtype, a, x, (hipStream_t)stream);
}

extern "C" int sngnn_signed_backward(const sngnn_graph_t *g, const float *wh, int C, const float *grad_out,
                                     const float *coef, const float *s, const float *c2, float *grad_wh, float *u,
                                     void *workspace, void *stream)
{
    return backward_impl(g, wh, 0, C, grad_out, coef, s, c2, grad_wh, u, workspace, stream);
}

// the half path: wh, grad_out and grad_wh stored as fp16 / bf16 (coef, s, c2, u, the records and every scratch row
// stay fp32)
extern "C" int sngnn_signed_backward_half(const sngnn_graph_t *g, const void *wh, int dtype, int C,
                                          const void *grad_out, const float *coef, const float *s, const float *c2,
                                          void *grad_wh, float *u, void *workspace, void *stream)
{
    SN_REQUIRE(dtype == SNGNN_DTYPE_F16 || dtype == SNGNN_DTYPE_BF16, SNGNN_EINVAL,
               "dtype must be SNGNN_DTYPE_F16 or SNGNN_DTYPE_BF16");
    return backward_impl(g, (const float *)wh, dtype, C, (const float *)grad_out, coef, s, c2, (float *)grad_wh, u,
                         workspace, stream);
}

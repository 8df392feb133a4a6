"""CPU: the workspace layouts of ``sngnn_amd/csrc/ws_layout.h`` as a host compiler computes them.

A stand-alone program includes the header (plain C++, no HIP) and prints every offset and total for a grid of
counts.  They must equal the expressions the entry points and ``sngnn_graph_workspace_bytes`` carried inline before
the layouts had one definition (restated below in Python; the Python side caches buffers by the returned size, so
the totals may not move), keep their regions ordered, disjoint and aligned, and fit every consumer into the size
``sngnn_graph_workspace_bytes`` returns for the same counts.

Alignment: the regions that the layout itself rounds (unit rows, the forward's partial rows, dnT, the attention and
signed forwards' partial rows) start on 16 bytes, key and done-word regions on 8, the tables on 256.  partT, partS and
rec_dot follow whole rows of C floats without padding (their offsets are fixed by the sizes above), so they are
aligned to the row vector width - 4 bytes times the largest of 1, 2, 4 dividing C, which is what the kernels load -
and to 16 bytes whenever C % 4 == 0."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CHANNELS, CAND_MAX_K = 512, 32

PROGRAM = r"""
#include <stdio.h>
#include "ws_layout.h"
using namespace sngnn;
int main()
{
    long long in[7];       // binary records on stdin and stdout: the grid has 50 000 points
    while (fread(in, sizeof in, 1, stdin) == 1) {
        const long long N = in[0], Ntot = in[1], Ep = in[2], nt = in[3], ns = in[4], se = in[5];
        const int C = (int)in[6];
        const FwdLayout f = fwd_layout(Ntot, se, nt, C);
        const BwdLayout b = bwd_layout(Ep, N, nt, ns, C, false), t = bwd_layout(Ep, N, nt, ns, C, true);
        const PartialLayout pa = attn_fwd_layout(nt, C), ps = signed_fwd_layout(nt, C);
        const long long v[] = {f.unit, f.nrm, f.filt, f.scores, f.partial, f.cand_key, f.cand_src, f.fin_done, f.total,
                               b.rec, b.dnT, b.partT, b.partS, b.rec_dot, b.total,
                               t.rec, t.dnT, t.partT, t.partS, t.rec_dot, t.total,
                               pa.partial, pa.total, ps.partial, ps.total,
                               graph_workspace_bytes(N, Ntot, Ep, nt, ns, se, C), filter_row_bytes(C), CAND_MAX_K};
        fwrite(v, sizeof v, 1, stdout);
    }
    return 0;
}
"""
COLUMNS = ("f_unit f_nrm f_filt f_scores f_partial f_cand_key f_cand_src f_fin_done f_total "
           "b_rec b_dnT b_partT b_partS b_rec_dot b_total t_rec t_dnT t_partT t_partS t_rec_dot t_total "
           "pa_partial pa_total ps_partial ps_total ws frb cand_max_k").split()


def grid():
    """[points, 7] int64: N, Ntot, Ep, n_tasks, n_stasks, split_edges, C."""
    rows = []
    for c in (1, 2, 3, 4, 36, 40, 64, 512):
        counts = (0, 1, 3, 1026, 2 ** 31 // c + 1)       # 1026 % 4 == 2; the last makes count * C pass 2^31
        for ep, n, nt, ns, se in itertools.product(counts, repeat=5):
            for ntot in (n, n + 7):
                rows.append((n, ntot, ep, nt, ns, se, c))
    rows.append((5, 5, 9, 0, 2, 0, 40))                  # split sources but no split row, and the other way round
    rows.append((5, 5, 9, 2, 0, 300, 40))
    return np.array(rows, dtype=np.int64)


def up256(v):
    return (v + 255) // 256 * 256


def test_workspace_layouts_match_the_inline_expressions_they_replaced(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "sngnn_amd", "csrc"), str(src), "-o", str(exe)])
    g = grid()
    out = subprocess.run([str(exe)], input=g.tobytes(), capture_output=True, check=True).stdout
    got = np.frombuffer(out, dtype=np.int64).reshape(len(g), len(COLUMNS))
    L = {name: got[:, i] for i, name in enumerate(COLUMNS)}
    N, Ntot, Ep, nt, ns, se, C = (g[:, i] for i in range(7))
    assert ((nt == 0) & (ns > 0)).any() and ((nt > 0) & (ns == 0)).any()
    assert (L["cand_max_k"] == CAND_MAX_K).all()

    # bytes of one filter row (common.h before; the forward's third table)
    frb = np.zeros_like(C)
    for c in np.unique(C).tolist():
        if c % 4 == 0 and 32 < c <= MAX_CHANNELS:
            b = 128
            while b < 2 * c:
                b <<= 1
            frb[C == c] = b
    assert (L["frb"] == frb).all()

    # ---- the parent's expressions --------------------------------------------------------------------------------
    # common.h fwd_table_bytes; agg_fwd.hip: nrm in agg_forward_impl, ws_filter, forward_normalized's carve
    units = up256(Ntot * C * 4)
    table = units + up256(Ntot * 4) + up256(Ntot * frb)
    want = {"f_unit": 0 * C, "f_nrm": units, "f_filt": units + up256(Ntot * 4), "f_scores": table}
    want["f_partial"] = want["f_scores"] + (se + 3) // 4 * 4 * 4
    want["f_cand_key"] = want["f_partial"] + (nt * C + 3) // 4 * 4 * 4
    want["f_cand_src"] = want["f_cand_key"] + nt * CAND_MAX_K * 8
    want["f_fin_done"] = want["f_cand_src"] + nt * CAND_MAX_K * 4
    # graph.hip sngnn_graph_workspace_bytes (its literal 32 is CAND_MAX_K)
    fwd = table + (se + 3) // 4 * 4 * 4 + (nt * C + 3) // 4 * 4 * 4 + nt * 32 * 8 + nt * 32 * 4 + nt * 8
    bwd = (2 * Ep + 3) // 4 * 4 * 4 + N * C * 4 + nt * (2 * C + 4) * 4 + ns * C * 4 * 2 + (N + 3) // 4 * 4 * 4
    want["f_total"] = fwd
    want["ws"] = up256(np.maximum(fwd, bwd))
    # agg_bwd.hip: ws | dnT = ws + ds_len | partT = dnT + N C | partS = partT + n_tasks C   (floats)
    ds_len = (2 * Ep + 3) // 4 * 4
    want.update(b_rec=0 * C, b_dnT=ds_len * 4, b_partT=(ds_len + N * C) * 4, b_partS=(ds_len + N * C + nt * C) * 4)
    # attn.hip / signed.hip: partT rows of 2 C + 4, then partS [n_stasks][2 C], then (attn.hip) rec_dot
    want.update(t_rec=0 * C, t_dnT=ds_len * 4, t_partT=(ds_len + N * C) * 4,
                t_partS=(ds_len + N * C + nt * (2 * C + 4)) * 4,
                t_rec_dot=(ds_len + N * C + nt * (2 * C + 4) + ns * 2 * C) * 4, t_total=bwd)
    # attn.hip:33 / signed.hip:33: the partial rows start the buffer
    want.update(pa_partial=0 * C, ps_partial=0 * C)
    for name, w in want.items():
        bad = np.nonzero(L[name] != w)[0]
        assert bad.size == 0, (name, g[bad[0]].tolist(), int(L[name][bad[0]]), int(w[bad[0]]))

    # ---- order, no overlap: every region ends at or before the next one starts ------------------------------------
    def chain(regions, total):
        for (a, size), (b, _) in zip(regions, regions[1:] + [(total, None)]):
            assert (L[a] >= 0).all() and (L[a] + size <= (L[b] if isinstance(b, str) else b)).all(), (a, b)

    chain([("f_unit", Ntot * C * 4), ("f_nrm", Ntot * 4), ("f_filt", Ntot * frb), ("f_scores", se * 4),
           ("f_partial", nt * C * 4), ("f_cand_key", nt * CAND_MAX_K * 8), ("f_cand_src", nt * CAND_MAX_K * 4),
           ("f_fin_done", nt * 8)], L["f_total"])
    chain([("b_rec", Ep * 8), ("b_dnT", N * C * 4), ("b_partT", nt * C * 4), ("b_partS", ns * 2 * C * 4)], L["b_total"])
    chain([("t_rec", Ep * 8), ("t_dnT", N * C * 4), ("t_partT", nt * (2 * C + 4) * 4), ("t_partS", ns * 2 * C * 4),
           ("t_rec_dot", N * 4)], L["t_total"])
    assert (L["b_rec_dot"] == L["b_total"]).all()        # (the aggregation keeps no rec_dot)
    assert (L["pa_total"] == nt * (C + 4) * 4).all() and (L["ps_total"] == nt * C * 4).all()

    # ---- alignment (module docstring) -----------------------------------------------------------------------------
    for name in ("f_unit", "f_partial", "b_rec", "b_dnT", "t_rec", "t_dnT", "pa_partial", "ps_partial"):
        assert (L[name] % 16 == 0).all(), name
    for name in ("f_cand_key", "f_fin_done"):
        assert (L[name] % 8 == 0).all(), name
    for name in ("f_unit", "f_nrm", "f_filt", "f_scores"):
        assert (L[name] % 256 == 0).all(), name
    vec_bytes = np.where(C % 4 == 0, 16, np.where(C % 2 == 0, 8, 4))
    for name in ("b_partT", "b_partS", "t_partT", "t_partS"):
        assert (L[name] % vec_bytes == 0).all(), name
    assert (L["f_cand_src"] % 4 == 0).all() and (L["t_rec_dot"] % 4 == 0).all()

    # ---- every consumer ends inside sngnn_graph_workspace_bytes of the same counts --------------------------------
    ends = {"forward": L["f_fin_done"] + nt * 8, "aggregation backward": L["b_partS"] + ns * 2 * C * 4,
            "attention backward": L["t_rec_dot"] + N * 4, "signed backward": L["t_partS"] + ns * 2 * C * 4,
            "attention forward [n_tasks][C + 4]": nt * (C + 4) * 4, "signed forward [n_tasks][C]": nt * C * 4}
    for who, end in ends.items():
        assert (end <= L["ws"]).all(), who
    assert (L["ws"] % 256 == 0).all()

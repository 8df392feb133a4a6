"""CPU: the forward's launch decisions of ``sngnn_amd/csrc/fwd_plan.h`` as a host compiler computes them.

A stand-alone program includes the header (plain C++, no HIP), reads binary records of inputs and writes every field
of the plan.  Each integer field must equal, on every grid point, the expression that the launchers of
``agg_fwd_impl.h`` carried inline at commit c78c21b (restated below in Python with that file's line numbers; Python
and numpy floats are IEEE doubles and the operation order is kept, and the program is compiled with
``-O0 -ffp-contract=off``, so the placement rule's doubles agree bit for bit).

The grid is the product the decisions depend on (channel widths with the lane layout ``row_cfg`` gives them, top_k,
head, half rows, candidates as ``fwd_use_candidates`` decides and forced off, tuning knob 9, role masks, and count
tuples from no split row to products size).  Two outcomes cannot occur inside that product and get a few points of
their own beside it, as do three scans across the placement rule's thresholds: ``top_k too large`` needs a kept list of more than 150 KiB (top_k > 30 000; the product stops
at 64), and ``does not fit LDS`` needs candidates forced ON where ``fwd_use_candidates`` says no (inside the product
they are only ever forced off).  The test asserts that every outcome it names is reached."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAND_MAX_K, CHUNK, BLOCK, WAVES, FIN_BLOCK = 32, 128, 256, 4, 1024
FWD_WAVES_PER_SIMD, FIN_BLOCKS_MAX, FIN_WAVE_MIN_ROWS = 6, 256, 2048
FINC_WAVES_MAX, FINC_LDS_BUDGET = 16, 150 * 1024

INPUTS = ("N n_med_end n_split n_split_gt_wave n_tasks n_edges C G k use_cand head half_rows has_fin_done role_mask "
          "max_split_deg fin_inline").split()
OUTPUTS = ("main_blocks fin_blocks head_nmain n_wave n_big n_big_true mixed finc_waves finc_head max_slots finc_dyn "
           "finc_dyn_mixed finc_fits mixed_fin_blocks mixed_head_blocks cand_blocks wave_blocks topk_too_large "
           "lds_scores fin_dyn use_candidates head_blocks_256 head_blocks_512 chip_cus fwd_slots").split()

PROGRAM = r"""
#include <stdio.h>
#include "fwd_plan.h"
using namespace sngnn;
int main()
{
    long long in[%d];
    while (fread(in, sizeof in, 1, stdin) == 1) {
        FwdPlanIn a;
        a.N = (int)in[0]; a.n_med_end = (int)in[1]; a.n_split = (int)in[2]; a.n_split_gt_wave = (int)in[3];
        a.n_tasks = (int)in[4]; a.n_edges = in[5]; a.C = (int)in[6]; a.G = (int)in[7]; a.k = (int)in[8];
        a.use_cand = in[9] != 0; a.head = in[10] != 0; a.half_rows = in[11] != 0; a.has_fin_done = in[12] != 0;
        a.role_mask = (int)in[13]; a.max_split_deg = (int)in[14]; a.fin_inline = (int)in[15];
        const FwdPlan p = fwd_plan(a);
        const long long v[] = {p.main_blocks, p.fin_blocks, p.head_nmain, p.fin.n_wave, p.fin.n_big, p.fin.n_big_true,
                               p.fin.mixed, p.finc_waves, p.finc_head, p.max_slots, (long long)p.finc_dyn,
                               (long long)p.finc_dyn_mixed, p.finc_fits, p.mixed_fin_blocks, p.mixed_head_blocks,
                               p.cand_blocks, p.wave_blocks, p.topk_too_large, p.lds_scores, (long long)p.fin_dyn,
                               fwd_use_candidates(a.k, a.C, a.max_split_deg), head_role_blocks(a.N, a.G, BLOCK),
                               head_role_blocks(a.N, a.G, 512), CHIP_CUS, FWD_SLOTS};
        fwrite(v, sizeof v, 1, stdout);
    }
    return 0;
}
""" % len(INPUTS)


def ceil_div(a, b):
    """common.h:54 at the parent (int64 operands, non-negative here)."""
    return (a + b - 1) // b


def row_group(c):
    """common.h row_cfg: lanes per row for C channels."""
    vec = 4 if c % 4 == 0 else (2 if c % 2 == 0 else 1)
    g = 8
    while g < c // vec and g < 64:
        g <<= 1
    return g


def use_candidates(k, c, max_split_deg):
    """agg_fwd_impl.h:2294-2300 (finc_lds_bytes: 1948)."""
    if k < 0:
        return True
    if k > CAND_MAX_K:
        return False
    max_slots = max(1, ceil_div(max_split_deg, CHUNK) * max(k, 0))
    return (FINC_WAVES_MAX * c + 1) * 4 + max_slots * 24 + 16 <= FINC_LDS_BUDGET


# N, n_med_end, n_split, n_split_gt_wave, n_tasks, n_edges, max_split_deg
COUNTS = (
    (2708, 40, 0, 0, 0, 10556, 0),                                   # no split row
    (20000, 900, 5, 0, 14, 150000, 420),                             # a few split rows, all under 128 / k tasks
    (169343, 9000, 825, 94, 3100, 1163820, 13155),                   # a few hundred of both kinds, ~10^5 work items
    (2449029, 700000, 100000, 3000, 260000, 30000000, 100000),       # ~10^5 split rows, 10^7s of edges
    # n_wave just below FIN_WAVE_MIN_ROWS and at it (64 tasks in the biggest row: 1 024 candidates at top_k 16, the
    # last count that takes the candidate finalize on 8 waves)
    (400000, 30000, 2047 + 60, 60, 7000, 4000000, 8192),
    (400000, 30000, 2048 + 60, 60, 7000, 4000000, 8192),
)


def grid():
    rows = []
    for c, k, head, half, forced_off, knob, mask, cnt in itertools.product(
            (1, 7, 24, 32, 40, 64, 100, 200, 512), (-1, 0, 1, 3, 16, 32, 33, 64), (0, 1), (0, 1), (0, 1),
            (0, 1, 3, 64, 1000), (7, 3), COUNTS):
        n, med, ns, gt, nt, ne, msd = cnt
        uc = 0 if forced_off else int(use_candidates(k, c, msd))
        rows.append((n, med, ns, gt, nt, ne, c, row_group(c), k, uc, head, half, 1, mask, msd, knob))
    product = len(rows)
    # beside the product (module docstring): the workspace without done words; a kept list beyond 150 KiB;
    # candidates forced on where they do not fit
    n, med, ns, gt, nt, ne, msd = COUNTS[2]
    for c in (40, 64):
        rows.append((n, med, ns, gt, nt, ne, c, row_group(c), 16, 1, 0, 0, 0, 7, msd, 1))
        rows.append((n, med, ns, gt, nt, ne, c, row_group(c), 40000, 0, 0, 0, 1, 7, 100000, 1))
        rows.append((n, med, ns, gt, nt, ne, c, row_group(c), 32, 1, 0, 0, 1, 7, 1000000, 1))
    # scans across the placement rule's thresholds, wherever they lie: the launch's bytes (n_edges), the big rows
    # (n_split_gt_wave) and, with a few split rows only, the work items the role's wave slots are taken from (N)
    for c, k in itertools.product((32, 40, 64), (-1, 1, 16)):
        tail = (c, row_group(c), k, 1, 0, 0, 1, 7)
        for e in np.linspace(2e5, 4e6, 150).astype(np.int64).tolist():
            rows.append((n, med, ns, gt, nt, e) + tail + (msd, 1))
        for big in range(0, 400, 3):
            rows.append((n, med, ns, big, nt, ne) + tail + (msd, 1))
        for nn in np.linspace(2e5, 8e6, 150).astype(np.int64).tolist():
            rows.append((nn, 2000, 5, 0, 14, 5 * nn) + tail + (420, 1))
    return np.array(rows, dtype=np.int64), product


def expected(g):
    """The parent's expressions (agg_fwd_impl.h at c78c21b), vectorised over the grid."""
    a = {name: g[:, i] for i, name in enumerate(INPUTS)}
    N, med, ns, gt, nt, ne, C, G, k = (a[x] for x in INPUTS[:9])
    uc, head, half, fin_done = a["use_cand"] != 0, a["head"] != 0, a["half_rows"] != 0, a["has_fin_done"] != 0
    mask, msd, knob = a["role_mask"], a["max_split_deg"], a["fin_inline"]
    w = {}
    # :2305-2316 finalize_shape
    n_wave = ns - np.minimum(ns, gt)
    n_big = np.where(k < 0, ns - n_wave, np.where((k > 0) & (n_wave >= FIN_WAVE_MIN_ROWS), ns - n_wave,
                                                  np.where(k > 0, ns, 0)))
    n_big_true = ns - n_wave
    mixed = (ns > 0) & uc & (k > 0) & (n_big == ns) & (n_wave > 0) & (n_big_true < ns)
    w.update(n_wave=n_wave, n_big=n_big, n_big_true=n_big_true, mixed=mixed)
    # :2408-2410 work items
    RPW = 64 // G
    items = nt + (med - ns) + ceil_div(N - med, RPW)
    # :2424-2425 fin_ok, :2428-2433
    fin_ok = (knob != 0) & (ns > 0) & uc & (k != 0) & ~head & fin_done & (((mask & 7) == 7) | (knob > 1))
    fin_big = np.minimum(ns, gt)
    fin_batches = ceil_div(ns - fin_big, RPW)
    SLOTS = 256 * FWD_WAVES_PER_SIMD
    t_batch = np.where(RPW >= 8, 25.0, 12.5)
    fin_blocks = np.zeros_like(ns)
    forced = fin_ok & (knob > 1)
    fin_blocks[forced] = np.minimum(knob, FIN_BLOCKS_MAX)[forced]                       # :2435
    rule = fin_ok & ~forced
    open_ = rule.copy()                                                                 # :2437 the loop still runs
    with np.errstate(divide="ignore", invalid="ignore"):
        for nb in range(8, FIN_BLOCKS_MAX + 1, 8):
            main_waves = np.minimum(ceil_div(items, WAVES), SLOTS - nb) * WAVES         # :2438
            b_fwd = ne.astype(np.float64) * (4.0 * C + 8.0) + N.astype(np.float64) * (8.0 * C + 8.0)      # :2443
            per_wave = ceil_div(items, np.where(open_, main_waves, 1))
            t_main = np.maximum(5.8 * per_wave.astype(np.float64), 0.8 * b_fwd / 4.8e6)                    # :2444
            t_fin = np.where(                                                                              # :2445-2447
                k < 0,
                6.0 + 4.0 * ceil_div(ns, nb * WAVES) + 2.5 * ceil_div(ceil_div(msd, CHUNK), 16),
                6.0 + 17.0 * ceil_div(ceil_div(fin_big, 2), nb) + t_batch * ceil_div(fin_batches, nb * WAVES))
            ends = open_ & ~(t_fin > 0.75 * t_main)                                                        # :2448
            t_sep = np.where(k < 0, 4.6 + 1.1 + 4.0 * ns / (256.0 * 24),                                   # :2449-2450
                             4.6 + 1.1 + 12.0 * fin_big / (256.0 * 3) + 12.5 * fin_batches / (256.0 * 24))
            loss = 5.8 * ceil_div(items, SLOTS * WAVES).astype(np.float64) * nb / float(SLOTS - nb)         # :2451
            fin_blocks[ends & (loss + 1.0 < t_sep)] = nb                                                   # :2452
            open_ &= ~ends                                                                                 # :2453 break
    w["fin_blocks"] = fin_blocks
    w["main_blocks"] = np.minimum(ceil_div(items, WAVES), 256 * FWD_WAVES_PER_SIMD - fin_blocks)           # :2459
    # :289-296 head_role_blocks, :2466 head_nmain
    def head_blocks(block):
        cap = 256 * 32 if block == BLOCK else 256 * 2 * (block // 64)
        return ceil_div(np.minimum(ceil_div(N, 2 * (64 // G)), cap), block // 64)
    w["head_blocks_256"], w["head_blocks_512"] = head_blocks(BLOCK), head_blocks(512)
    w["head_nmain"] = np.where(head, np.where(mixed, head_blocks(512), head_blocks(BLOCK)), 0)
    # the candidate finalize: :2330-2331 finc_waves, :2338-2341, :2349, :2353-2354, :2359-2361; :2374 the HEAD
    # instantiation is taken for fp32 rows only.  A call without candidates never gets there: zeros.
    max_tasks = ceil_div(msd, CHUNK)
    kk = np.maximum(k, 0)
    finc_waves = np.where(~head & ((k < 0) | (max_tasks * kk > 1024)), 16, 8)
    max_slots = np.maximum(1, max_tasks * kk)
    finc_dyn = (FINC_WAVES_MAX * C + 1) * 4 + max_slots * 24 + 16                                          # :1948
    finc_head = head & ~half
    cand = dict(finc_waves=finc_waves, finc_head=finc_head, max_slots=max_slots, finc_dyn=finc_dyn,
                finc_fits=finc_dyn <= FINC_LDS_BUDGET,
                finc_dyn_mixed=np.maximum(finc_dyn, finc_waves * CAND_MAX_K * 12),
                mixed_fin_blocks=n_big_true + ceil_div(n_wave, finc_waves),
                mixed_head_blocks=np.where(finc_head, w["head_nmain"], 0),
                cand_blocks=n_big, wave_blocks=np.where(ns > n_big, ceil_div(ns - n_big, WAVES), 0))
    for name, v in cand.items():
        w[name] = np.where(uc, v, 0)
    # :2379-2384 the scratch finalize
    fixed = C * (FIN_BLOCK // 64) * 4 + np.minimum(kk, msd) * 4
    w["topk_too_large"] = fixed > 150 * 1024
    w["lds_scores"] = np.where(fixed < 120 * 1024, np.minimum((120 * 1024 - fixed) // 4, msd), 0)
    w["fin_dyn"] = fixed + w["lds_scores"] * 4
    w["use_candidates"] = (k < 0) | ((k <= CAND_MAX_K) & (finc_dyn <= FINC_LDS_BUDGET))                    # :2294-2300
    w["chip_cus"], w["fwd_slots"] = np.full_like(ns, 256), np.full_like(ns, 256 * FWD_WAVES_PER_SIMD)
    return w, dict(rule=rule, forced=forced, fin_ok=fin_ok, uc=uc, knob=knob, msd=msd)


def test_forward_plan_matches_the_inline_expressions_it_replaced(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "sngnn_amd", "csrc"), str(src), "-o", str(exe)])
    g, product = grid()
    out = subprocess.run([str(exe)], input=g.tobytes(), capture_output=True, check=True).stdout
    got = np.frombuffer(out, dtype=np.int64).reshape(len(g), len(OUTPUTS))
    P = {name: got[:, i] for i, name in enumerate(OUTPUTS)}
    want, why = expected(g)
    assert sorted(want) == sorted(OUTPUTS)
    for name in OUTPUTS:
        bad = np.nonzero(P[name] != want[name].astype(np.int64))[0]
        assert bad.size == 0, (name, dict(zip(INPUTS, g[bad[0]].tolist())), int(P[name][bad[0]]),
                               int(want[name][bad[0]]), bad.size)

    # ---- the grid reaches every outcome (of the product alone, except the two the docstring names) ---------------
    inside = np.arange(len(g)) < product
    rule, forced, uc = why["rule"] & inside, why["forced"] & inside, why["uc"] & inside
    fb = P["fin_blocks"]
    assert (fb[rule] == 0).any()
    assert np.unique(fb[rule & (fb > 0)]).size >= 2, np.unique(fb[rule])
    assert (fb[forced] == FIN_BLOCKS_MAX).any() and (why["knob"][forced & (fb == FIN_BLOCKS_MAX)] > FIN_BLOCKS_MAX).all()
    assert (fb[forced] == 3).any() and (fb[forced] == 64).any()
    assert (fb[inside & ~why["fin_ok"]] == 0).all() and (fb[~inside & (g[:, INPUTS.index("has_fin_done")] == 0)] == 0).all()
    assert (P["mixed"][inside] == 1).any() and (P["mixed"][inside & (g[:, 2] > 0)] == 0).any()
    assert (P["finc_waves"][uc] == 8).any() and (P["finc_waves"][uc] == 16).any()
    scratch = inside & ~why["uc"] & (g[:, 2] > 0)
    assert (P["lds_scores"][scratch] < why["msd"][scratch]).any()
    assert ((P["lds_scores"][scratch] == why["msd"][scratch]) & (why["msd"][scratch] > 0)).any()
    assert not P["topk_too_large"][inside].any() and (P["topk_too_large"][~inside] == 1).any()
    assert P["finc_fits"][uc].all() and ((P["finc_fits"] == 0) & why["uc"] & ~inside).any()
    assert (P["use_candidates"][inside] == 1).any() and (P["use_candidates"][inside] == 0).any()

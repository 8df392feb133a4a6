#!/usr/bin/env python3
"""The half path against fp32: forward, backward and forward + backward of the aggregation in ms, per form.

Forms: fp32 (the library's default scoring), fp32 with knob 2 = 2 (on the fly, what the half path runs), bf16,
fp16, and bf16 / fp16 with the rows padded by zero channels to the width their 16-byte lane layout spans anyway
(conv.HALF_PAD: 40 -> 64, 48 -> 64 - the same bits, whole 128-byte lines).  Cases:
  arxiv     config 4's graph (arxiv size), SNGNN_Plus's operator, top_k 16, thr 0 and 0.9, C 40
  parallel  the same graph with nearly parallel rows (a deep layer's input: every cosine close to 1, most
            decisions in doubt and re-scored exactly) - the on-the-fly form's worst case
  products  config 5's graph (products size), one SNGNN_Plus_Plus layer's aggregation, top_k 16, thr 0, C 48;
            plus the adjacency branch as the half layer runs it (ops.adj_linear on an fp32 copy of w)
  attention config 4's graph (arxiv size), C 40: the cosine attention (AGNNConv's operator) and the signed cosine
            attention (GGCNlayer_SP's), forward and backward, fp32 / bf16 / fp16 on the same two graph objects in
            this process; the forms alternate over --rounds rounds (median and spread per form, half / fp32 ratio)
Warm-up as bench.py: an untimed preheat of the same step (--preheat-ms), W warm-up steps, K timed steps.
Per form: algorithmic bytes (bench.algorithmic_bytes / backward_bytes with 2-byte rows for the half forms)
and their fraction of 8 TB/s.  One JSON line per (case, form, pass); --json FILE writes them all.

    python tools/bench_half.py [--cases arxiv,parallel,products,attention] [--steps 50] [--warmup 10]
Kernel figures: run it under ``rocprofv3 --kernel-trace --stats``; counters (FETCH_SIZE) in a run of their own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from sngnn_amd import _lib, conv, ops  # noqa: E402
from sngnn_amd.graph import LOOPS_REPLACE, Graph  # noqa: E402

PEAK = 8.0e12


def pad_width(c):
    old = conv.HALF_PAD
    conv.HALF_PAD = True
    try:
        return conv.half_width(c)
    finally:
        conv.HALF_PAD = old


def timed(step, steps, warmup, preheat_ms):
    """ms per step: preheat (untimed, until the device has been busy preheat_ms), warmup, K timed steps"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    t_one = max(time.perf_counter() - t0, 1e-6)
    for _ in range(int(min(5000, max(1, preheat_ms * 1e-3 / t_one)))):
        step()
    dt, _ = bench.time_loop(step, warmup, steps, torch.cuda.synchronize)
    return dt / steps * 1e3


def run_case(name, g, h32, k, thr, args, records, extra=None):
    n, c = h32.shape
    e_prime = g.num_edges
    forms = [("fp32", torch.float32, 0, c), ("fp32_otf", torch.float32, 2, c),
             ("bf16", torch.bfloat16, 0, c), ("fp16", torch.float16, 0, c)]
    cp = pad_width(c)
    if cp != c:
        forms += [(f"bf16_pad{cp}", torch.bfloat16, 0, cp), (f"fp16_pad{cp}", torch.float16, 0, cp)]
    for form, D, knob2, width in forms:
        h = h32.to(D)
        if width != c:
            h = torch.nn.functional.pad(h, (0, width - c))
        h = h.contiguous()
        go = torch.randn(n, width, device=h.device).to(D)
        _lib.load().sngnn_tuning_set(2, knob2)
        try:
            out, wsel, _, _, _ = ops.aggregate_forward(g, h, k, thr, save_for_backward=True)
            n_sel = int((wsel != _lib.UNSELECTED).sum())
            t_f = timed(lambda: ops.aggregate_forward(g, h, k, thr, save_for_backward=True), args.steps,
                        args.warmup, args.preheat_ms)
            t_b = timed(lambda: ops.aggregate_backward(g, h, go, wsel, k), args.steps, args.warmup, args.preheat_ms)

            def fb():
                o, w, _, _, _ = ops.aggregate_forward(g, h, k, thr, save_for_backward=True)
                return ops.aggregate_backward(g, h, go, w, k)
            t_fb = timed(fb, args.steps, args.warmup, args.preheat_ms)
        finally:
            _lib.load().sngnn_tuning_set(2, 0)
        rb = h.element_size()
        # bench.py's models with rows of rb-byte values (their 4-byte terms are fp32 row bytes)
        b_f = e_prime * (rb * width + 8) + n * (2 * rb * width + 8)
        b_b = e_prime * 8 + n_sel * (3 * rb * width + 8) + n * 4 * rb * width
        rec = dict(case=name, form=form, dtype=str(D).replace("torch.", ""), C=c, width=width, top_k=k, thr=thr,
                   n=n, e_prime=e_prime, kept=n_sel, fwd_ms=round(t_f, 4), bwd_ms=round(t_b, 4),
                   fwd_bwd_ms=round(t_fb, 4), fwd_bytes=b_f, bwd_bytes=b_b,
                   fwd_frac_8tbs=round(b_f / (t_f * 1e-3) / PEAK, 4),
                   bwd_frac_8tbs=round(b_b / (t_b * 1e-3) / PEAK, 4), steps=args.steps, warmup=args.warmup)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del h, go
    if extra:
        extra(records)


def run_attention(n, ei, h32, args, records):
    """The two attention modes, half against fp32: same graph objects, same process; per pass the forms are timed
    in turn, --rounds times over (a drift of the machine hits every form alike), median per form."""
    c = h32.size(1)
    dev = h32.device
    g_attn = Graph(ei, n, True, LOOPS_REPLACE)                # as AGNNConv builds it
    g_sign = Graph(ei, n, False, True)                        # as GGCNlayer_SP builds it (adj_remove_diag)
    gen = torch.Generator(device=dev).manual_seed(9)
    go32 = torch.randn(n, c, device=dev, generator=gen)
    coef = torch.randn(g_sign.num_edges, device=dev, generator=gen)
    c2 = torch.tensor([0.7, 0.2], device=dev)
    forms = [("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)]
    steps = {}
    for form, D in forms:
        h, go = h32.to(D).contiguous(), go32.to(D).contiguous()
        _, alpha = ops.attention_forward(g_attn, h, True)
        _, s = ops.signed_forward(g_sign, h, coef, c2)
        steps[form] = {
            "attn_fwd": (lambda h=h: ops.attention_forward(g_attn, h, True)),
            "attn_bwd": (lambda h=h, go=go, alpha=alpha: ops.attention_backward(g_attn, h, go, alpha)),
            "signed_fwd": (lambda h=h: ops.signed_forward(g_sign, h, coef, c2)),
            "signed_bwd": (lambda h=h, go=go, s=s: ops.signed_backward(g_sign, h, go, coef, s, c2)),
        }
    for pas in ("attn_fwd", "attn_bwd", "signed_fwd", "signed_bwd"):
        ms = {form: [] for form, _ in forms}
        for _ in range(args.rounds):
            for form, _ in forms:
                ms[form].append(timed(steps[form][pas], args.steps, args.warmup, args.preheat_ms))
        med = {form: float(np.median(v)) for form, v in ms.items()}
        e_prime = (g_attn if pas.startswith("attn") else g_sign).num_edges
        for form, D in forms:
            rec = dict(case="attention", op=pas, form=form, C=c, n=n, e_prime=e_prime,
                       ms_median=round(med[form], 4), ms_min=round(min(ms[form]), 4), ms_max=round(max(ms[form]), 4),
                       ratio_to_fp32=round(med[form] / med["fp32"], 4), rounds=args.rounds, steps=args.steps,
                       warmup=args.warmup)
            print(json.dumps(rec), flush=True)
            records.append(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="arxiv,parallel,products,attention")
    ap.add_argument("--rounds", type=int, default=3, help="attention case: alternating rounds per form")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--preheat-ms", type=float, default=60.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    records = []
    cases = args.cases.split(",")
    if "arxiv" in cases or "parallel" in cases or "attention" in cases:
        n, c, ei, x, h, lin = bench.make_rank_inputs("arxiv", 0, 1, 1234, dev)
        if "attention" in cases:
            run_attention(n, ei, h, args, records)
        g = Graph(ei, n, True, True)
        if "arxiv" in cases:
            for thr in (0.0, 0.9):
                run_case("arxiv", g, h, 16, thr, args, records)
        if "parallel" in cases:
            gen = torch.Generator(device=dev).manual_seed(5)
            base = torch.randn(1, c, device=dev, generator=gen)
            hp = base + 1e-2 * torch.randn(n, c, device=dev, generator=gen)
            run_case("parallel", g, hp.contiguous(), 16, 0.0, args, records)
        del g, ei, x, h
    if "products" in cases:
        n, c, ei, x, h, lin = bench.make_rank_inputs("products", 0, 1, 1234, dev, channels=48)
        del x
        g = Graph(ei, n, True, True)

        def adj_branch(records):
            torch.manual_seed(3)
            w = (torch.randn(n, 48, device=dev) * 0.01).t()            # [C, N] column-major, as _AdjLinearParams
            b = torch.zeros(48, device=dev)
            wh, bh = w.to(torch.bfloat16), b.to(torch.bfloat16)
            t32 = timed(lambda: ops.adj_linear(w, b, g), args.steps, args.warmup, args.preheat_ms)
            t16 = timed(lambda: ops.adj_linear(wh.float(), bh.float(), g).to(torch.bfloat16), args.steps,
                        args.warmup, args.preheat_ms)
            tcp = timed(lambda: wh.float(), args.steps, args.warmup, args.preheat_ms)
            rec = dict(case="products", form="adj_branch", fp32_ms=round(t32, 4), bf16_via_fp32_copy_ms=round(t16, 4),
                       of_which_copy_ms=round(tcp, 4), w_bytes_fp32=int(w.numel() * 4))
            print(json.dumps(rec), flush=True)
            records.append(rec)
        run_case("products", g, h, 16, 0.0, args, records, adj_branch)
    if args.json:
        with open(args.json, "w") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Kernel gate of the four-plane (early-fusion RGB-D) stem at b=16, 450x800: rd_stem_fwd_split and rd_stem_wgrad_split_bn_t at 4 -> 64
against the 3 -> 64 launches of the same library, the two sides alternating over --rounds repeats in one process, plus the fp32-MFMA
siblings (rd_stem_fwd, rd_stem_wgrad_t) and the 1 -> 64 shapes.  Pass: t(4->64) / t(3->64) <= work ratio x (1 + s), the work ratio from
the code (forward 4/3: input bytes and staging, MFMA steps 14/11; weight gradient 7/5: row tiles) and s the relative spread
(max - min over median) of the 3 -> 64 timings across the repeats.

    python tools/bench_stem4.py [--rounds 7] [--iters 20]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ops import timeit  # noqa: E402
from radar_depth_amd._lib import check, current_stream, lib, ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    L = lib()
    n, cout, h, w = 16, 64, 450, 800
    hw = h * w
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    m = n * ho * wo
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, 4, h, w, generator=gen).cuda()
    raw = (torch.randn(n, ho, wo, cout, generator=gen) * 1.5 + 0.3).cuda()
    g = (torch.randn(n, ho, wo, cout, generator=gen) * (torch.rand(n, ho, wo, cout, generator=gen) < 0.3)).cuda()
    out = torch.empty(n, ho, wo, cout, device="cuda")
    stat = torch.zeros(L.rd_stem_stat_tiles(n, h, w), 2, cout, device="cuda")
    gamma = torch.ones(cout, device="cuda")
    mean = raw.mean((0, 1, 2))
    invstd = 1.0 / torch.sqrt(raw.var((0, 1, 2), unbiased=False) + 1e-5)
    tiles = L.rd_bn_bwd_tiles(C.c_int64(m), cout)
    red = torch.zeros(tiles, 3, cout, device="cuda")
    check(L.rd_bn_bwd_reduce_t(0, ptr(g), cout, None, 0, ptr(raw), cout, ptr(mean), None, 0, None, None, 0, C.c_int64(m), cout, 0, ptr(red),
                               current_stream()), "rd_bn_bwd_reduce_t")
    dg, db, coef = torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda"), torch.zeros(3 * cout, device="cuda")
    ops = {}
    for cin in (3, 4, 1):
        planes = (C.c_void_p * 4)(*[x.data_ptr() + 4 * hw * c if c < cin else None for c in range(4)])
        strides = (C.c_int64 * 4)(*[4 * hw if c < cin else 0 for c in range(4)])
        wp = torch.randn(49, cin, cout, device="cuda") * 0.1
        gw = torch.empty(cout, cin, 7, 7, device="cuda")
        ws = torch.empty(int(L.rd_stem_wgrad_workspace_floats(n, h, w, cin, cout)), device="cuda")
        keep = (planes, strides, wp, gw, ws)

        def fwd(fn, name, k=keep, cin=cin):
            return lambda: check(fn(k[0], k[1], cin, n, h, w, ptr(k[2]), cout, ptr(out), ptr(stat), current_stream()), name)
        ops["fwd_split %d->64" % cin] = fwd(L.rd_stem_fwd_split, "rd_stem_fwd_split")
        ops["fwd_fp32  %d->64" % cin] = fwd(L.rd_stem_fwd, "rd_stem_fwd")
        ops["wgrad_split_bn %d->64" % cin] = lambda k=keep, cin=cin: check(L.rd_stem_wgrad_split_bn_t(
            0, k[0], k[1], cin, n, h, w, ptr(g), ptr(raw), ptr(red), tiles, ptr(gamma), ptr(mean), ptr(invstd), ptr(dg), ptr(db), ptr(coef),
            cout, ptr(k[3]), ptr(k[4]), current_stream()), "rd_stem_wgrad_split_bn_t")
        ops["wgrad_split %d->64" % cin] = lambda k=keep, cin=cin: check(L.rd_stem_wgrad_split_t(
            0, k[0], k[1], cin, n, h, w, ptr(g), cout, ptr(k[3]), ptr(k[4]), current_stream()), "rd_stem_wgrad_split_t")
        ops["wgrad_fp32  %d->64" % cin] = lambda k=keep, cin=cin: check(L.rd_stem_wgrad_t(
            0, k[0], k[1], cin, n, h, w, ptr(g), cout, ptr(k[3]), ptr(k[4]), current_stream()), "rd_stem_wgrad_t")
    times = {k: [] for k in ops}
    for _ in range(a.rounds):          # the sides alternate inside every round
        for k, fn in ops.items():
            times[k].append(timeit(fn, iters=a.iters) * 1e6)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("%-24s median %7.1f us   min %7.1f   max %7.1f   spread %.3f" % (k, med[k], min(v), max(v), (max(v) - min(v)) / med[k]))
    for fam, ratio, sib in (("fwd_split", 4.0 / 3.0, "fwd_fp32 "), ("wgrad_split_bn", 7.0 / 5.0, "wgrad_fp32 ")):
        base = times["%s 3->64" % fam]
        s = (max(base) - min(base)) / med["%s 3->64" % fam]
        r = med["%s 4->64" % fam] / med["%s 3->64" % fam]
        print("gate %-15s t(4->64)/t(3->64) = %.3f   bound %.3f x (1 + %.3f) = %.3f   %s   (fp32-MFMA sibling at 4->64: %.1f us)"
              % (fam, r, ratio, s, ratio * (1 + s), "PASS" if r <= ratio * (1 + s) else "MISS", med["%s 4->64" % sib]))


if __name__ == "__main__":
    main()

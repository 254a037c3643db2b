#!/usr/bin/env python3
"""Kernel gate of rd_gemm_taps_split (csrc/gemm_taps_split.hip) against rd_gconv_split on the same descriptors, one process, one GPU
(rd_gconv_split with rd_gconv_split_plan_all(1): the planner leaves these shapes to the pre-split form, rd_gconv_split_pre, which the
plan runs today and which is timed too -- its operand split into piece planes outside the timing, as the producer pass does in a step):
deconv3's forward and deconv2's input gradient on decoder layers 1-3 at b=16 450x800 (the gate: >= 1.15x on the summed time admits
the kernel to the decoder plan through rd_gemm_taps_split_preferred), and -- to size the follow-up that would move them -- the
encoder's stride-2 3x3 input gradients with >= 32 channels.  Both kernels with BatchNorm partial sums, as in the plan.

    python tools/bench_taps_split.py [--reps 50]
"""
import argparse
import os
import sys

import ctypes as C

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radar_depth_amd import convdesc as cd, ops  # noqa: E402
from radar_depth_amd._lib import lib  # noqa: E402

B = 16
# (name, descriptor, weight slabs) -- decoder layer l: 256 / 2^(l-1) -> half the channels, input map 15x25 * 2^(l-1)
GATE = [("deconv3.fwd L%d" % l, cd.deconv_fwd(B, 15 << (l - 1), 25 << (l - 1), 256 >> (l - 1), 128 >> (l - 1), 3), 9) for l in (1, 2, 3)] + \
       [("deconv2.dgrad L%d" % l, cd.deconv_dgrad(B, 15 << (l - 1), 25 << (l - 1), 256 >> (l - 1), 128 >> (l - 1), 2), 4) for l in (1, 2, 3)]
# encoder stride-2 3x3 conv1 of the first block of layer2..4 (RGB) and layer3..4 (depth; layer2_depth's 16 output channels are not served)
ENC = [("enc layer2.0.conv1.dgrad", cd.conv_dgrad(B, 113, 200, 64, 128, 3, 2, 1)[0], 9),
       ("enc layer3.0.conv1.dgrad", cd.conv_dgrad(B, 57, 100, 128, 256, 3, 2, 1)[0], 9),
       ("enc layer4.0.conv1.dgrad", cd.conv_dgrad(B, 29, 50, 256, 512, 3, 2, 1)[0], 9),
       ("enc layer3_depth.0.conv1.dgrad", cd.conv_dgrad(B, 57, 100, 32, 64, 3, 2, 1)[0], 9),
       ("enc layer4_depth.0.conv1.dgrad", cd.conv_dgrad(B, 29, 50, 64, 128, 3, 2, 1)[0], 9)]


def time_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def run(rows, reps):
    tot = [0.0, 0.0, 0.0]
    for name, d, slabs in rows:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(d.N, d.Hi, d.Wi, d.ldi, generator=g).cuda()
        w = ops.pack_weights_split((torch.randn(d.Cout, d.Cin, slabs, 1, generator=g) * d.Cin ** -0.5).cuda())
        out_a = torch.empty(d.N, d.Ho, d.Wo, d.ldo, device="cuda")
        out_b = torch.empty_like(out_a)
        assert ops.gconv_split_supported(d) and ops.gemm_taps_split_supported(d), name
        st_a = torch.zeros(ops.gconv_split_stat_tiles(d), 2, d.Cout, device="cuda")
        st_b = torch.zeros(ops.gemm_taps_split_stat_tiles(d), 2, d.Cout, device="cuda")
        ta = time_us(lambda: ops.gconv_split(d, x, w, out_a, stat=st_a), reps)
        tb = time_us(lambda: ops.gemm_taps_split(d, x, w, out_b, stat=st_b), reps)
        tp = float("nan")
        if ops.gconv_split_pre_supported(d):
            pc = ops.split_pieces(x)
            out_p = torch.empty_like(out_a)
            st_p = torch.zeros(ops.gconv_split_pre_stat_tiles(d), 2, d.Cout, device="cuda")
            tp = time_us(lambda: ops.gconv_split_pre(d, pc, w, out_p, stat=st_p), reps)
        diff = ((out_a - out_b).abs().max() / out_a.abs().max()).item()
        taps = "/".join(str(d.phase[i].n_taps) for i in range(d.n_phases))
        gmac = sum(d.N * d.phase[i].lh * d.phase[i].lw * d.phase[i].n_taps for i in range(d.n_phases)) * d.Cin * d.Cout / 1e9
        print("%-32s taps %-8s %4d->%-4d  gconv_split %7.1f us  gconv_split_pre %7.1f us  gemm_taps_split %7.1f us  x%.2f / x%.2f  "
              "(useful TFLOP/s %.0f / %.0f / %.0f; max rel diff %.1e)"
              % (name, taps, d.Cin, d.Cout, ta, tp, tb, ta / tb, tp / tb, 2e3 * gmac / ta, 2e3 * gmac / tp, 2e3 * gmac / tb, diff), flush=True)
        tot[0] += ta
        tot[1] += tb
        tot[2] += tp
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    prev = lib().rd_gconv_split_plan_all(1)
    try:
        g = run(GATE, a.reps)
        e = run(ENC, a.reps)
    finally:
        lib().rd_gconv_split_plan_all(prev)
    print("GATE deconv3 fwd + deconv2 dgrad, layers 1-3, b=16: gconv_split %.1f us, gconv_split_pre %.1f us, gemm_taps_split %.1f us, "
          "speed-up x%.3f / x%.3f (admit at >= 1.15)" % (g[0], g[2], g[1], g[0] / g[1], g[2] / g[1]), flush=True)
    print("ENCODER stride-2 3x3 input gradients (5 launches per step): gconv_split %.1f us, gconv_split_pre %.1f us, gemm_taps_split %.1f us, "
          "x%.3f / x%.3f" % (e[0], e[2], e[1], e[0] / e[1], e[2] / e[1]), flush=True)


if __name__ == "__main__":
    main()

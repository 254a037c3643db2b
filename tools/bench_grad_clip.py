"""Gradient-norm clipping against the plain SGD launch, one job on one MI355X:
  (a) on the config-2 arena (the late-fusion model's st["total"] floats): rd_sgd_step, rd_grad_sumsq, rd_sgd_step_clip and a
      device-to-device copy of the arena's bytes;
  (b) the fused config-2 training step (resnet18_latefusion b = 16, 450x800, split operands) without and with max_grad_norm, the two
      steps timed in alternating groups of five of the same job.
Every line is the median of REPS timed groups on the device timeline with the fastest and slowest group next to it.  Three conditions are
checked and reported, not tuned:
  kernels  t(rd_grad_sumsq) + t(rd_sgd_step_clip) <= t(rd_sgd_step) + t(copy)
  step 1   the stand-alone time of the added work, t(rd_grad_sumsq) + t(rd_sgd_step_clip) - t(rd_sgd_step), is under 0.1 of the step
  step 2   the clipped step stays within the job's own run-to-run spread of  plain step + that stand-alone time
    python tools/bench_grad_clip.py [--no-step] [--reverse]      (--reverse: the clipped step is built and timed first)"""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_berhu import B, H, REPS, W, group, groups, line, stats  # noqa: E402


def main():
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    from radar_depth_amd.main import HipTrainStep, create_model
    from radar_depth_amd.synthetic import make_batch
    L = lib()
    torch.manual_seed(0)
    model = create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), [H, W]).cuda()
    n = model._ensure_arenas()["total"]
    print("gradient clipping: arena of %d floats (%.1f MB); median of %d groups [fastest .. slowest]" % (n, 4 * n / 1e6, REPS))
    gen = torch.Generator(device="cuda").manual_seed(1)
    p, g, buf = (torch.randn(n, generator=gen, device="cuda") * s for s in (1.0, 1e-2, 1e-2))
    dst = torch.empty_like(g)
    k = L.rd_grad_sumsq_partials(n)
    part = torch.zeros(k, dtype=torch.float64, device="cuda")
    st4 = torch.zeros(4, dtype=torch.float64, device="cuda")
    st = current_stream()
    hp = (1e-6, 0.9, 1e-4, 1.0)          # (a small lr: the arenas stay finite over the thousands of timed updates)

    def sgd():
        check(L.rd_sgd_step(ptr(p), ptr(g), ptr(buf), n, *hp, 0, st), "rd_sgd_step")

    def sumsq():
        check(L.rd_grad_sumsq(ptr(g), n, ptr(part), st), "rd_grad_sumsq")

    def clip():
        check(L.rd_sgd_step_clip(ptr(p), ptr(g), ptr(buf), n, *hp, 1.0, 1, ptr(part), k, ptr(st4), st), "rd_sgd_step_clip")

    def copy():
        dst.copy_(g)

    sumsq()
    t = {name: stats(groups(fn, 50, 10)) for name, fn in (("sgd", sgd), ("sumsq", sumsq), ("clip", clip), ("copy", copy))}
    print("total_norm %.6g, clip_coef %.6g, skipped %d" % tuple(st4[:3].tolist()))
    line("(a) rd_sgd_step", t["sgd"], "  %.0f GB/s over five arena passes" % (20 * n / t["sgd"][0] / 1e3))
    bw_copy, bw_red = 8 * n / t["copy"][0] / 1e3, 4 * n / t["sumsq"][0] / 1e3
    line("(a) rd_grad_sumsq (%d partials)" % k, t["sumsq"], "  %.0f GB/s = %.2f of the copy's" % (bw_red, bw_red / bw_copy))
    line("(a) rd_sgd_step_clip", t["clip"], "  %.0f GB/s, x%.3f of rd_sgd_step" % (20 * n / t["clip"][0] / 1e3, t["clip"][0] / t["sgd"][0]))
    line("(a) device-to-device copy of the arena", t["copy"], "  %.0f GB/s read + written" % bw_copy)
    lhs, rhs = t["sumsq"][0] + t["clip"][0], t["sgd"][0] + t["copy"][0]
    print("    rd_grad_sumsq + rd_sgd_step_clip = %.1f us; rd_sgd_step + copy = %.1f us (%s the kernel condition)"
          % (lhs, rhs, "meets" if lhs <= rhs else "MISSES"))
    extra = lhs - t["sgd"][0]
    print("    stand-alone time of the added work = %.1f us" % extra)
    if "--no-step" in sys.argv:
        return
    del p, g, buf, dst
    xs, tg = make_batch(B, H, W, 1234)
    xs, tg = xs.cuda(), tg.cuda()
    steps = {}
    order = ("clip", "plain") if "--reverse" in sys.argv else ("plain", "clip")      # which step is built, and timed, first
    for kind in order:
        torch.manual_seed(0)
        m = model if kind == order[0] else create_model(
            types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), [H, W]).cuda()
        kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if kind == "clip" else {}
        steps[kind] = HipTrainStep(m, B, H, W, lr=0.01, momentum=0.9, weight_decay=1e-4, operands="split", **kw)
        for _ in range(5):
            steps[kind].step(xs, tg)
    torch.cuda.synchronize()
    out = {"plain": [], "clip": []}
    for _ in range(REPS):                                   # alternating groups: both steps see the same drift of the machine
        for kind in order:
            out[kind].append(group(lambda: steps[kind].step(xs, tg), 5))
    s0, s1 = stats(out["plain"]), stats(out["clip"])
    c = steps["clip"]
    print("clipped step: total_norm %.6g, clip_coef %.6g, skipped %d" % (c.grad_norm, c.clip_coef, c.skipped))
    line("(b) fused step", s0, "  %.0f samples/s" % (B / s0[0] * 1e6))
    line("(b) fused step, max_grad_norm=1, skip_nonfinite", s1, "  %.0f samples/s" % (B / s1[0] * 1e6))
    print("    condition 1: added work %.1f us = %.4f of the step (%s the 0.1 bar)" % (extra, extra / s0[0], "meets" if extra < 0.1 * s0[0] else "MISSES"))
    spread = max(s0[2] - s0[1], s1[2] - s1[1])
    over = s1[0] - (s0[0] + extra)
    print("    condition 2: clipped step - (plain step + %.1f us) = %+.1f us; run-to-run spread of the job %.1f us (%s the condition)"
          % (extra, over, spread, "meets" if abs(over) <= spread else "MISSES"))


if __name__ == "__main__":
    main()

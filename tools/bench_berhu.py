"""MaskedBerHuLoss against the MaskedL1Loss kernels it sits next to, one job on one MI355X, b = 16 at 450x800:
  (a) rd_masked_l1_sums and rd_masked_berhu_sums on the same planes (the loss forward: one streaming pass against two);
  (b) rd_masked_l1_bwd and rd_masked_berhu_bwd;
  (c) the fused config-2 training step (resnet18_latefusion b = 16, split operands) with criterion="l1" and with criterion="berhu", the
      two steps timed in alternating groups of the same job.
Every line is the median of REPS timed groups on the device timeline with the fastest and slowest group next to it.  Two conditions are
checked and reported, not tuned: the BerHu forward takes at most 3x the L1 forward, and the BerHu step stays within the job's own
run-to-run spread of  l1 step + (berhu loss launches - l1 loss launches).
    python tools/bench_berhu.py [--no-step] [--reverse]      (--reverse: the berhu step is built and timed first)"""
import ctypes as C
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, H, W = 16, 450, 800
REPS = 15


def groups(fn, inner, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        out.append(group(fn, inner))
    return out


def group(fn, inner):
    """us per call of one group of ``inner`` calls, on the device timeline"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def stats(out):
    return float(np.median(out)), min(out), max(out)


def line(name, t, extra=""):
    print("%-58s %10.1f us  [%.1f .. %.1f]%s" % (name, t[0], t[1], t[2], extra), flush=True)


def main():
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    from radar_depth_amd.synthetic import make_batch
    L = lib()
    print("BerHu against L1: b=%d %dx%d; median of %d groups [fastest .. slowest]" % (B, H, W, REPS))
    xs, t = make_batch(B, H, W, 1234)
    xs, t = xs.cuda(), t.cuda()
    pred = (t + torch.randn_like(t) * 3).contiguous()
    n = pred.numel()
    f64 = lambda k: torch.zeros(k, dtype=torch.float64, device="cuda")      # noqa: E731
    ws = f64((int(L.rd_berhu_workspace_floats(n)) + 1) // 2)
    s_l1, s_bh = f64(4), f64(4)
    coef = torch.ones(1, device="cuda")
    dpred = torch.empty_like(pred)
    st = current_stream()

    def l1_fwd():
        check(L.rd_masked_l1_sums(ptr(pred), ptr(t), C.c_int64(n), ptr(ws), ptr(s_l1), st), "l1 sums")

    def bh_fwd():
        check(L.rd_masked_berhu_sums(ptr(pred), ptr(t), n, 0.2, ptr(ws), ptr(s_bh), st), "berhu sums")

    def l1_bwd():
        check(L.rd_masked_l1_bwd(ptr(pred), ptr(t), C.c_int64(n), ptr(s_l1), ptr(coef), ptr(dpred), 0, st), "l1 bwd")

    def bh_bwd():
        check(L.rd_masked_berhu_bwd(ptr(pred), ptr(t), n, ptr(s_bh), ptr(coef), ptr(dpred), 0, st), "berhu bwd")

    k = {name: stats(groups(fn, 50, 10)) for name, fn in (("l1_fwd", l1_fwd), ("bh_fwd", bh_fwd), ("l1_bwd", l1_bwd), ("bh_bwd", bh_bwd))}
    valid = int(s_bh[1].item())
    print("%d of %d pixels valid; delta = %.6g, max |t - p| = %.6g; loss l1 %.6g, berhu %.6g"
          % (valid, n, s_bh[2].item(), s_bh[3].item(), (s_l1[0] / s_l1[1]).item(), (s_bh[0] / s_bh[1]).item()))
    line("(a) rd_masked_l1_sums (2 launches)", k["l1_fwd"], "  %.0f GB/s" % (8 * n / k["l1_fwd"][0] / 1e3))
    ratio = k["bh_fwd"][0] / k["l1_fwd"][0]
    line("(a) rd_masked_berhu_sums (3 launches)", k["bh_fwd"], "  %.0f GB/s over two passes" % (16 * n / k["bh_fwd"][0] / 1e3))
    print("    berhu forward / l1 forward = %.2f (%s the 3x condition)" % (ratio, "meets" if ratio <= 3.0 else "MISSES"))
    line("(b) rd_masked_l1_bwd", k["l1_bwd"])
    line("(b) rd_masked_berhu_bwd", k["bh_bwd"], "  x%.2f" % (k["bh_bwd"][0] / k["l1_bwd"][0]))
    extra = (k["bh_fwd"][0] + k["bh_bwd"][0]) - (k["l1_fwd"][0] + k["l1_bwd"][0])
    print("    berhu loss launches - l1 loss launches = %.1f us" % extra)
    if "--no-step" in sys.argv:
        return
    from radar_depth_amd.main import HipTrainStep, create_model
    steps = {}
    order = ("berhu", "l1") if "--reverse" in sys.argv else ("l1", "berhu")      # which step is built, and timed, first
    for crit in order:
        torch.manual_seed(0)
        model = create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), [H, W]).cuda()
        steps[crit] = HipTrainStep(model, B, H, W, lr=0.01, momentum=0.9, weight_decay=1e-4, operands="split", criterion=crit)
        for _ in range(5):
            steps[crit].step(xs, t)
    torch.cuda.synchronize()
    out = {"l1": [], "berhu": []}
    for _ in range(REPS):                                   # alternating groups: both criteria see the same drift of the machine
        for crit in order:
            out[crit].append(group(lambda: steps[crit].step(xs, t), 5))
    s1, sb = stats(out["l1"]), stats(out["berhu"])
    line("(c) fused step, criterion=l1", s1, "  %.0f samples/s" % (B / s1[0] * 1e6))
    line("(c) fused step, criterion=berhu", sb, "  %.0f samples/s" % (B / sb[0] * 1e6))
    spread = max(s1[2] - s1[1], sb[2] - sb[1])
    over = sb[0] - (s1[0] + extra)
    print("    berhu step - (l1 step + %.1f us) = %+.1f us; run-to-run spread of the job %.1f us (%s the condition)"
          % (extra, over, spread, "meets" if abs(over) <= spread else "MISSES"))


if __name__ == "__main__":
    main()

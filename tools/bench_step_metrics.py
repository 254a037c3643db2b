"""What the reference's per-step metric bookkeeping (main.py:449-452: Result().evaluate + average_meter.update after every step)
costs the fused training step, and what the on-device meters cost instead.
    python tools/bench_step_metrics.py [--steps 50] [--warmup 10] [--reps 3] [--out FILE]

Config 2 of BASELINE.json: resnet18_latefusion, upproj, rgbd, b = 16, 450x800, split plan, plain launches.  Three legs:
  A  the fused step alone                                                   (what bench.py times)
  B  the fused step + Result().evaluate(pred, target) + AverageMeter.update every step: two launches and a blocking 80-byte
     readback per step -- the only way to these numbers without the device meters
  C  HipTrainStep(metrics=True): sums in the loss pass, one small launch per step, ONE average() at the end
Wall-clock time over --steps steps after --warmup warm-up steps with one final synchronise (the effect is host-side: event timing
alone would hide it); --reps repetitions per leg, interleaved (A B C A B C ...) in one process; median and spread (max - min) per leg.
On a checkout without the `metrics` keyword leg C is skipped, so the same file measures A and B on the parent commit."""
import argparse
import inspect
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radar_depth_amd.evaluation.metrics import AverageMeter, Result  # noqa: E402
from radar_depth_amd.main import HipTrainStep, create_model  # noqa: E402
from radar_depth_amd.synthetic import make_batch  # noqa: E402

B, H, W = 16, 450, 800


def make_step(**kw):
    torch.manual_seed(0)
    model = create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), [H, W]).cuda()
    return HipTrainStep(model, B, H, W, lr=0.01, momentum=0.9, weight_decay=1e-4, **kw)


def kernel_times(iters=200):
    """Device time (events around `iters` back-to-back calls) of the loss pass at the step's size, with and without the metric sums."""
    import ctypes as C
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    L = lib()
    if not hasattr(L, "rd_meter_update"):
        return ["  loss-pass kernels: this checkout has no fused entry points"]
    n = B * H * W
    x, t = make_batch(B, H, W, 1234)
    t = t.cuda()
    o = (t + torch.rand_like(t) * 3 + 0.5).contiguous()
    f64 = lambda k: torch.zeros(k, dtype=torch.float64, device="cuda")
    tiles = L.rd_loss_tiles(C.c_int64(n))
    ws, sums, msums, meter, last, w = f64(12 * tiles), f64(2), f64(10), f64(12), f64(10), torch.full((1,), 16.0, dtype=torch.float64, device="cuda")
    s = current_stream()
    cases = [("rd_masked_l1_sums", lambda: L.rd_masked_l1_sums(ptr(o), ptr(t), C.c_int64(n), ptr(ws), ptr(sums), s)),
             ("rd_masked_l1_sums_metrics", lambda: L.rd_masked_l1_sums_metrics(ptr(o), ptr(t), C.c_int64(n), ptr(ws), ptr(sums), ptr(msums), s)),
             ("rd_depth_metrics", lambda: L.rd_depth_metrics(ptr(o), ptr(t), C.c_int64(n), ptr(ws), ptr(msums), s)),
             ("rd_meter_update", lambda: L.rd_meter_update(ptr(msums), 1, ptr(w), None, 1, ptr(meter), ptr(last), s))]
    lines = []
    for name, call in cases:
        for _ in range(10):
            check(call(), name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            check(call(), name)
        e1.record()
        torch.cuda.synchronize()
        lines.append("  %-28s %7.2f us per call (n = %d, %d back-to-back calls)" % (name, e0.elapsed_time(e1) / iters * 1e3, n, iters))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--kernels", action="store_true", help="also time the loss-pass kernels on their own (device events)")
    ap.add_argument("--label", default="", help="a word for the report's first line (e.g. the commit measured)")
    args = ap.parse_args()
    has_metrics = "metrics" in inspect.signature(HipTrainStep.__init__).parameters
    x, t = make_batch(B, H, W, 1234)
    x, t = x.cuda(), t.cuda()
    plain = make_step()
    fused = make_step(metrics=True) if has_metrics else None
    host_meter = AverageMeter()

    def leg_a():
        plain.step(x, t)

    def leg_b():
        _, pred = plain.step(x, t)
        r = Result()
        r.evaluate(pred, t)
        host_meter.update(r, 0, 0, B)

    def leg_c():
        fused.step(x, t)

    legs = [("A fused step", leg_a, None), ("B step + Result.evaluate + AverageMeter.update", leg_b, host_meter.average)]
    if has_metrics:
        legs.append(("C metrics=True, one average() at the end", leg_c, lambda: fused.meter.average()))
    ms = {name: [] for name, _, _ in legs}
    for _ in range(args.reps):
        for name, body, finish in legs:
            for _ in range(args.warmup):
                body()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                body()
            if finish is not None:
                finish()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    lines = ["step metrics %s: resnet18_latefusion upproj rgbd b=%d %dx%d, split plan, plain launches; wall ms/step over %d steps after %d "
             "warm-up, %d interleaved repetitions" % (args.label, B, H, W, args.steps, args.warmup, args.reps)]
    med = {}
    for name, _, _ in legs:
        v = ms[name]
        med[name[0]] = (statistics.median(v), max(v) - min(v))
        lines.append("  %-52s median %8.3f ms  spread %6.3f ms  (%s)" % (name, med[name[0]][0], med[name[0]][1], ", ".join("%.3f" % q for q in v)))
    lines.append("  B - A = %+.3f ms/step" % (med["B"][0] - med["A"][0]))
    if has_metrics:
        lines.append("  C - A = %+.3f ms/step (A's spread %.3f)" % (med["C"][0] - med["A"][0], med["A"][1]))
        lines.append("  C <= B + spread(B): %s (%.3f vs %.3f)" % (med["C"][0] <= med["B"][0] + med["B"][1], med["C"][0], med["B"][0] + med["B"][1]))
        a, c = host_meter.average(), fused.meter.average()
        lines.append("  rmse of the averages: host %.6f, device %.6f (different steps enter them: the legs train separate replicas)" % (a.rmse, c.rmse))
    else:
        lines.append("  leg C skipped: this checkout's HipTrainStep has no `metrics` keyword")
    if args.kernels:
        lines += kernel_times()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

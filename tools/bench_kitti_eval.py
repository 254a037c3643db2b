"""The KITTI devkit evaluation (radar_depth_amd.evaluation.kitti, csrc/kitti_eval.hip) against the work it sits next to, one job on one
MI355X, frames of 450x800, B = 1 and B = 16, ground truth 0.8 % and 100 % valid, predictions with 30 % holes:
  (a) every entry point on its own through the C ABI (preallocated buffers, no Python allocation): interpolate (two launches), errors
      (two launches), error_image (one), stats_update (one), each next to
  (b) a device-to-device copy of the bytes it reads and writes, with the fraction of the copy's rate;
  (c) the whole per-frame evaluation through the Python module -- fill, errors, error image, stats update -- against
  (d) a HipInference frame (b = 1, hipGraph) of the same job.  The condition checked: (c) at B = 1 stays below a tenth of (d).
Every line is the median of REPS timed groups on the device timeline with the fastest and slowest group next to it.
    python tools/bench_kitti_eval.py [--out profiles/r22_kitti_eval.txt] [--no-model]"""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, ".")

H, W = 450, 800
REPS = 15
LINES = []


def timed(fn, inner=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner * 1e3)
    return float(np.median(out)), min(out), max(out)


def say(text):
    print(text, flush=True)
    LINES.append(text)


def line(name, t, extra=""):
    say("%-64s %9.1f us  [%.1f .. %.1f]%s" % (name, t[0], t[1], t[2], extra))


def copy_time(nbytes):
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    return timed(lambda: dst.copy_(src))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r22_kitti_eval.txt"))
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    from radar_depth_amd.evaluation import kitti
    L = lib()
    say("KITTI devkit evaluation: %dx%d frames; median of %d groups [fastest .. slowest]" % (H, W, REPS))
    table = kitti.log_colormap().ctypes.data
    whole = {}
    for B in (1, 16):
        n = H * W
        g = torch.Generator(device="cuda").manual_seed(B)
        pred = torch.rand((B, 1, H, W), device="cuda", generator=g) * 80 + 1
        pred[torch.rand((B, 1, H, W), device="cuda", generator=g) < 0.3] = -1
        filled = torch.empty_like(pred)
        ws = torch.empty(int(L.rd_kitti_workspace_bytes(B, H, W)), dtype=torch.uint8, device="cuda")
        errs = torch.empty((B, 10), dtype=torch.float64, device="cuda")
        img = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
        state = torch.zeros((9, 4), dtype=torch.float64, device="cuda")
        s = current_stream()
        t = timed(lambda: check(L.rd_kitti_interpolate(ptr(pred), n, ptr(filled), n, B, H, W, ptr(ws), s), "interpolate"))
        c = copy_time(B * n * 4)
        line("(a) interpolate, B=%d (30 %% holes)" % B, t, "  copy of %.1f MB read + written: %.1f us, %.2f of its rate"
             % (2 * B * n * 4 / 1e6, c[0], c[0] / t[0]))
        for frac in (0.008, 1.0):
            gt = torch.rand((B, 1, H, W), device="cuda", generator=g) * 80 + 1
            if frac < 1:
                gt[torch.rand((B, 1, H, W), device="cuda", generator=g) >= frac] = -1
            tag = "B=%d, %.1f %% valid" % (B, 100 * frac)
            t = timed(lambda: check(L.rd_kitti_errors(ptr(gt), n, ptr(filled), n, B, H, W, 0, ptr(ws), ptr(errs), s), "errors"))
            c = copy_time(B * n * 4)                      # (a copy of n bytes reads n and writes n: the two planes read)
            line("(a) errors, " + tag, t, "  copy moving %.1f MB: %.1f us, %.2f of its rate" % (2 * B * n * 4 / 1e6, c[0], c[0] / t[0]))
            t = timed(lambda: check(L.rd_kitti_error_image(ptr(gt), n, ptr(filled), n, B, H, W, 0, table, ptr(img), 3 * n, 3 * W, s), "image"))
            c = copy_time(B * n * 11 // 2)                # 8 bytes read and 3 written per pixel
            line("(a) error_image, " + tag, t, "  copy moving %.1f MB: %.1f us, %.2f of its rate" % (B * n * 11 / 1e6, c[0], c[0] / t[0]))
            meter = kitti.KittiDepthMeter()

            def frame():
                meter.update(pred, gt)
                kitti.error_image(gt, filled, out=img)
            whole[(B, frac)] = timed(frame)
            line("(c) fill + errors + error image + stats update, " + tag, whole[(B, frac)], "  %.1f us per frame" % (whole[(B, frac)][0] / B))
        t = timed(lambda: check(L.rd_kitti_stats_update(ptr(errs), B, ptr(state), s), "stats"))
        line("(a) stats_update, B=%d" % B, t)
    if not args.no_model:
        from radar_depth_amd.main import HipInference, create_model
        from radar_depth_amd.synthetic import make_batch
        torch.manual_seed(0)
        model = create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), [H, W]).cuda()
        infer = HipInference(model, 1, H, W, use_graph=True)
        x1 = make_batch(1, H, W, 1)[0].cuda()
        frame_t = timed(lambda: infer(x1), inner=10, warmup=5)
        line("(d) HipInference frame (resnet18_latefusion b=1, hipGraph)", frame_t)
        for frac in (0.008, 1.0):
            r = whole[(1, frac)][0] / frame_t[0]
            say("(c) B=1, %.1f %% valid / inference frame = %.4f (%s the 0.1 condition)" % (100 * frac, r, "meets" if r < 0.1 else "MISSES"))
            say("(c) B=16, %.1f %% valid, per frame / inference frame = %.4f" % (100 * frac, whole[(16, frac)][0] / 16 / frame_t[0]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

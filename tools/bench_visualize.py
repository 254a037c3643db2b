"""The comparison rows (radar_depth_amd.utils.merge_into_row_with_gt) against the work they sit next to, one job on one MI355X, frames of
450x800:
  (a) merge_into_row_with_gt for one frame and for B = 16, on channel slices of one [B,4,H,W] tensor, into a preallocated tensor;
  (b) the reference's algorithm on the same tensors as restated in tests/visualize_ref.py, its blocking .cpu() copies included (the
      restatement replaces matplotlib's float64 colormap call by a table lookup, so it is FASTER than the reference; B = 16 is sixteen
      calls, as the reference asserts batch 1);
  (c) a HipInference frame (b = 1, hipGraph) and the fused config-2 training step (b = 16) in the same job;
  (d) a device-to-device copy of the bytes (a) moves: the fp32 planes read plus the uint8 rows written.
Every GPU line is the median of REPS timed groups with the fastest and slowest group next to it.  The condition checked: (a) stays below
a tenth of the inference frame at B = 1 and below a tenth of the fused step at B = 16.  The ratio to (b) and the fraction of (d)'s
bandwidth are reported, not gated.
    python tools/bench_visualize.py [--no-step]"""
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

H, W = 450, 800
REPS = 15


def timed(fn, inner=20, warmup=3):
    """us per call on the device timeline: (median, fastest, slowest) of REPS groups of ``inner`` calls."""
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


def wall_timed(fn, reps=5):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), min(out), max(out)


def line(name, t, extra=""):
    print("%-66s %10.1f us  [%.1f .. %.1f]%s" % (name, t[0], t[1], t[2], extra), flush=True)


def tensors(B):
    from radar_depth_amd.synthetic import make_batch
    x, t = make_batch(B, H, W, 77)
    x, t = x.cuda(), t.cuda()
    x[:, :3] = torch.rand(B, 3, H, W, device="cuda")                # the rgb panel wants 0..1
    pred = (t + torch.randn_like(t)).contiguous()
    return x, t, pred


def main():
    import visualize_ref as V
    from radar_depth_amd import utils
    print("comparison rows: %dx%d frames, 4 panels; median of %d groups [fastest .. slowest]" % (H, W, REPS))
    table = utils.viridis_table()
    ours, copies = {}, {}
    for B in (1, 16):
        x, t, pred = tensors(B)
        out = torch.empty((H, 4 * W, 3) if B == 1 else (B, H, 4 * W, 3), dtype=torch.uint8, device="cuda")
        got = utils.merge_into_row_with_gt(x[:, :3], x[:, 3:4], t, pred, out=out).cpu().numpy().reshape(B, H, 4 * W, 3)

        def reference():
            return [V.merge_row(x[b, :3].cpu().numpy(), [x[b, 3].cpu().numpy(), t[b, 0].cpu().numpy(), pred[b, 0].cpu().numpy()], table)
                    for b in range(B)]
        assert np.array_equal(got, np.stack(reference())), "the GPU rows are not the restatement's"
        ours[B] = timed(lambda: utils.merge_into_row_with_gt(x[:, :3], x[:, 3:4], t, pred, out=out))
        line("(a) merge_into_row_with_gt, B=%d" % B, ours[B], "  %.1f us per frame" % (ours[B][0] / B))
        ref = wall_timed(reference)
        line("(b) restated reference with its .cpu() copies, B=%d (wall clock)" % B, ref, "  x%.0f of (a)" % (ref[0] / ours[B][0]))
        nbytes = B * H * W * (6 * 4 + 4 * 3)
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        copies[B] = timed(lambda: dst.copy_(src))
        line("(d) device copy of %.1f MB, B=%d" % (nbytes / 1e6, B), copies[B],
             "  %.0f GB/s; (a) runs at %.2f of it" % (2 * nbytes / copies[B][0] / 1e3, copies[B][0] / ours[B][0]))
    from radar_depth_amd.main import HipInference, HipTrainStep, create_model
    from radar_depth_amd.synthetic import make_batch
    torch.manual_seed(0)
    model = create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), [H, W]).cuda()
    infer = HipInference(model, 1, H, W, use_graph=True)
    x1 = make_batch(1, H, W, 1)[0].cuda()
    frame = timed(lambda: infer(x1), inner=10, warmup=5)
    line("(c) HipInference frame (resnet18_latefusion b=1, hipGraph)", frame)
    ratio = ours[1][0] / frame[0]
    print("(a) B=1 / inference frame = %.4f (%s the 0.1 condition)" % (ratio, "meets" if ratio < 0.1 else "MISSES"))
    if "--no-step" in sys.argv:
        return
    ts = HipTrainStep(model, 16, H, W, lr=0.01, momentum=0.9, weight_decay=1e-4, operands="split")
    xs, t = make_batch(16, H, W, 1234)
    xs, t = xs.cuda(), t.cuda()
    step = timed(lambda: ts.step(xs, t), inner=5, warmup=5)
    line("(c) fused step (config 2: resnet18_latefusion b=16, split)", step, "  %.0f samples/s" % (16 / step[0] * 1e6))
    ratio = ours[16][0] / step[0]
    print("(a) B=16 / fused step = %.4f (%s the 0.1 condition)" % (ratio, "meets" if ratio < 0.1 else "MISSES"))


if __name__ == "__main__":
    main()

"""Training-input staging (rd_stage_frames_train) against the step it has to feed, in one job at BASELINE.json's config-2 geometry
(b=16, 450x800): stage_train_batch (with the tables prepared ahead, and with their host preparation inside the call), stage_val_batch
(the validation kernel, same frames) and the fused training step, plus a device-to-device copy as the bandwidth yardstick.
Algorithmic bytes per frame of the training path: 3*H0*W0 (min / max pass over the rotated frame) + ch*cw * (3 read + 4 written:
resample) + ch*cw * (4 + 2*2 read, 20 written: jitter, depth and the planar stores); validation: 7 read + 20 written per output
pixel.  The condition this tool checks: staging a batch takes less than a tenth of the step, so that on a side stream it cannot
become the step's bottleneck.
    python tools/bench_staging_train.py [--no-step]"""
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, ".")
from radar_depth_amd.dataset import draw_train_params, prepare_train_params, stage_train_batch, stage_val_batch  # noqa: E402

B, H0, W0, CROP = 16, 450, 800, (450, 800)


def timed(fn, warmup=3, iters=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    h0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    host = (time.perf_counter() - h0) / iters * 1e6
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, host          # us per call on the device timeline, us of host time per call


def main():
    img = torch.randint(0, 256, (B, H0, W0, 3), dtype=torch.uint8, device="cuda")
    lid = torch.randint(0, 20000, (B, H0, W0), dtype=torch.int16, device="cuda")
    rad = torch.randint(0, 20000, (B, H0, W0), dtype=torch.int16, device="cuda")
    p = draw_train_params(B, CROP, rng=np.random.RandomState(0))
    src, dst = torch.empty(1 << 28, dtype=torch.uint8, device="cuda"), torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    copy_us, _ = timed(lambda: dst.copy_(src))
    copy_tbs = 2 * (1 << 28) / copy_us / 1e6
    print("device copy 256 MiB: %.1f us, %.2f TB/s (read + write)" % (copy_us, copy_tbs))
    px = CROP[0] * CROP[1]
    rows = {}
    prep = prepare_train_params(p, H0, W0, CROP)
    train_bytes = B * (3 * H0 * W0 + px * (7 + 28))
    for name, fn, by in (("stage_train_batch", lambda: stage_train_batch(img, lid, rad, prep, CROP, 80.0), train_bytes),
                         ("stage_train_batch + host preparation", lambda: stage_train_batch(img, lid, rad, p, CROP, 80.0), train_bytes),
                         ("stage_val_batch", lambda: stage_val_batch(img, lid, rad, CROP, 80.0), B * px * 27)):
        us, host = timed(fn)
        rows[name] = us
        print("%s b=%d %dx%d -> %dx%d: %.1f us/batch (host %.0f us/call), %.0f frames/s, %.1f MB algorithmic, %.2f TB/s = %.0f %% of the copy rate"
              % (name, B, H0, W0, CROP[0], CROP[1], us, host, B / us * 1e6, by / 1e6, by / us / 1e6, 100 * by / us / 1e6 / copy_tbs))
    if "--no-step" in sys.argv:
        return
    from radar_depth_amd.main import HipTrainStep, create_model
    from radar_depth_amd.synthetic import make_batch
    torch.manual_seed(0)
    model = create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), [H0, W0]).cuda()
    ts = HipTrainStep(model, B, H0, W0, lr=0.01, momentum=0.9, weight_decay=1e-4, operands="split")
    x, t = make_batch(B, H0, W0, 1234)
    x, t = x.cuda(), t.cuda()
    step_us, _ = timed(lambda: ts.step(x, t), warmup=5, iters=20)
    ratio = rows["stage_train_batch"] / step_us
    print("fused step (config 2: resnet18_latefusion b=%d %dx%d, split operands): %.1f us, %.0f samples/s" % (B, H0, W0, step_us, B / step_us * 1e6))
    print("stage_train_batch / step = %.4f (%s the 0.1 condition); stage_train_batch / stage_val_batch = %.1f"
          % (ratio, "meets" if ratio < 0.1 else "MISSES", rows["stage_train_batch"] / rows["stage_val_batch"]))
    # and with staging queued on a side stream while the step runs: what the step loses to it
    side = torch.cuda.Stream()

    def both():
        with torch.cuda.stream(side):
            stage_train_batch(img, lid, rad, prep, CROP, 80.0)
        ts.step(x, t)
    both_us, _ = timed(both, warmup=3, iters=20)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    print("fused step with stage_train_batch on a side stream: %.1f us (%.1f %% over the step alone)" % (both_us, 100 * (both_us / step_us - 1)))


if __name__ == "__main__":
    main()

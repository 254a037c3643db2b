"""The lidar sparsifiers (lidar_radar, uniform) against the step they have to feed, one job on one MI355X: b=16 frames of 900x1600 with 3000
lidar and 130 radar points each, crop 450x800.  Per batch: stage_train_batch alone, stage_train_batch followed by lidar_radar_sparse_depth,
by uniform_sparse_depth with uploaded draws (the 46 MB upload from pinned memory included) and by uniform_sparse_depth with the device
generator, each writing inputs[:, 3:4], and the fused config-2 training step (b=16, 450x800) in the same job.  Every line is the median
of REPS timed groups with the fastest and slowest group next to it.  The condition checked: what a sparsifier adds to a staged training
batch stays below a tenth of the step.
The CPU lines run on one core of whatever host runs the tool: with --reference PATH the reference checkout's own dense_to_sparse on one
450x800 frame of the same densities.
    python tools/bench_lidar_sparsifiers.py [--no-step] [--cpu-only] [--reference PATH]"""
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, ".")

B, H0, W0, CROP, NL, NR = 16, 900, 1600, (450, 800), 3000, 130
NUM_SAMPLES, MAX_DEPTH = 100, 80.0
REPS = 15


def timed(fn, inner=10, warmup=3):
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


def cpu_timed(fn, reps=5):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), min(out), max(out)


def line(name, t, extra=""):
    print("%-62s %10.1f us  [%.1f .. %.1f]%s" % (name, t[0], t[1], t[2], extra), flush=True)


def cpu_lines():
    """The reference's own classes on one 450x800 frame with NL lidar and NR radar pixels, one core."""
    if "--reference" not in sys.argv:
        return
    sys.path.insert(0, sys.argv[sys.argv.index("--reference") + 1])
    torch.set_num_threads(1)
    from dataset.dense_to_sparse import LidarRadarSampling, UniformSampling
    rng = np.random.RandomState(2)
    h, w = CROP
    lidar, radar = np.zeros(h * w, np.float32), np.zeros(h * w, np.float32)
    lidar[rng.choice(h * w, NL, replace=False)] = rng.uniform(2, 100, NL)
    radar[rng.choice(h * w, NR, replace=False)] = rng.uniform(2, 100, NR)
    lt, rt = torch.from_numpy(lidar.reshape(1, h, w)), torch.from_numpy(radar.reshape(1, h, w))
    lr, un = LidarRadarSampling(NUM_SAMPLES, MAX_DEPTH), UniformSampling(NUM_SAMPLES, MAX_DEPTH)
    line("reference LidarRadarSampling.dense_to_sparse, one frame, one core", cpu_timed(lambda: lr.dense_to_sparse(lt, rt)))
    line("reference UniformSampling.dense_to_sparse, one frame, one core", cpu_timed(lambda: un.dense_to_sparse(lt)))


def main():
    print("lidar sparsifiers: b=%d, %dx%d frames, %d lidar / %d radar points per frame, crop %dx%d; median of %d groups [fastest .. slowest]"
          % (B, H0, W0, NL, NR, CROP[0], CROP[1], REPS))
    if "--cpu-only" in sys.argv:
        return cpu_lines()
    from radar_depth_amd.dataset import (draw_train_params, lidar_radar_sparse_depth, prepare_train_params, stage_train_batch,
                                         uniform_sparse_depth)
    rng = np.random.RandomState(11)
    img = torch.randint(0, 256, (B, H0, W0, 3), dtype=torch.uint8, device="cuda")
    lid, rad = np.zeros((B, H0 * W0), np.int16), np.zeros((B, H0 * W0), np.int16)
    for b in range(B):                                               # four times the points in the frame: about NL / NR inside the crop
        lid[b, rng.choice(H0 * W0, 4 * NL, replace=False)] = rng.randint(2 * 256, 100 * 256, 4 * NL)
        rad[b, rng.choice(H0 * W0, 4 * NR, replace=False)] = rng.randint(2 * 256, 100 * 256, 4 * NR)
    lid, rad = torch.from_numpy(lid.reshape(B, H0, W0)).cuda(), torch.from_numpy(rad.reshape(B, H0, W0)).cuda()
    prep = prepare_train_params(draw_train_params(B, CROP, rng=np.random.RandomState(0)), H0, W0, CROP)
    draws_host = torch.from_numpy(rng.uniform(0, 1, (B, 1) + CROP)).pin_memory()
    x, y = stage_train_batch(img, lid, rad, prep, CROP)
    print("pixels per frame inside the crop: lidar %.0f, radar %.0f" % ((y > 0).sum().item() / B, (x[:, 3] > 0).sum().item() / B))

    def stage():
        return stage_train_batch(img, lid, rad, prep, CROP)

    def with_lidar_radar():
        x, y = stage()
        lidar_radar_sparse_depth(y, x[:, 3:4], out=x[:, 3:4])

    def with_uniform_draws():
        x, y = stage()
        uniform_sparse_depth(y, NUM_SAMPLES, MAX_DEPTH, draws=draws_host.to("cuda", non_blocking=True), out=x[:, 3:4])

    def with_uniform_seed():
        x, y = stage()
        uniform_sparse_depth(y, NUM_SAMPLES, MAX_DEPTH, seed=1, offset=0, out=x[:, 3:4])

    rows = {}
    for name, fn in (("stage_train_batch", stage), ("stage_train_batch + lidar_radar", with_lidar_radar),
                     ("stage_train_batch + uniform, uploaded draws (upload included)", with_uniform_draws),
                     ("stage_train_batch + uniform, device generator", with_uniform_seed)):
        rows[name] = timed(fn)
        line(name, rows[name])
    base = rows.pop("stage_train_batch")[0]
    added = {name: t[0] - base for name, t in rows.items()}
    for name, a in added.items():
        print("%-62s adds %.1f us to a staged training batch (%.1f us per frame)" % (name, a, a / B))
    cpu_lines()
    if "--no-step" in sys.argv:
        return
    from radar_depth_amd.main import HipTrainStep, create_model
    from radar_depth_amd.synthetic import make_batch
    torch.manual_seed(0)
    model = create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), list(CROP)).cuda()
    ts = HipTrainStep(model, B, CROP[0], CROP[1], lr=0.01, momentum=0.9, weight_decay=1e-4, operands="split")
    xs, t = make_batch(B, CROP[0], CROP[1], 1234)
    xs, t = xs.cuda(), t.cuda()
    step = timed(lambda: ts.step(xs, t), inner=5, warmup=5)
    line("fused step (config 2: resnet18_latefusion b=%d %dx%d, split)" % (B, CROP[0], CROP[1]), step, "  %.0f samples/s" % (B / step[0] * 1e6))
    for name, a in added.items():
        ratio = a / step[0]
        print("%-62s added / step = %.4f (%s the 0.1 condition)" % (name, ratio, "meets" if ratio < 0.1 else "MISSES"))


if __name__ == "__main__":
    main()

"""The radar_filtered sparsifier against the step it has to feed, one job on one MI355X: b=16 frames of 900x1600 with 130 radar and 3000
lidar points each, crop 450x800.  Per batch: filter_radar_points (the point filter, the index_map fill and scatter), the
index-map-and-filter launch behind validation and training staging, stage_val_batch / stage_train_batch with sparsifier radar against
radar_filtered, and the fused config-2 training step (b=16, 450x800) in the same job.  Every line is the median of REPS timed groups
with the fastest and slowest group next to it.  The condition checked: what radar_filtered adds to a staged training batch
(filter_radar_points + stage_train_batch(radar_filtered) - stage_train_batch(radar)) stays below a tenth of the step.
The CPU lines run on one core of whatever host runs the tool: the numpy restatement tests/radar_filter_ref.py (one stable argsort), and
with --reference PATH the reference checkout's own filter_radar_points_gt (two full sorts of the distance matrix and a Python loop).
    python tools/bench_radar_filter.py [--no-step] [--cpu-only] [--reference PATH]"""
import ctypes as C
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")

B, H0, W0, CROP, NR, NL = 16, 900, 1600, (450, 800), 130, 3000
REPS = 15


def points(rng):
    """The fixture generator's mix: lidar uniform in the frame, radar near a lidar point (consistent or random depth) or anywhere."""
    lxy = rng.uniform(0, 1, (B, NL, 2)) * np.array([W0, H0])
    ldep = rng.uniform(2, 100, (B, NL))
    kind, near = rng.randint(0, 3, (B, NR)), rng.randint(0, NL, (B, NR))
    at = np.take_along_axis(lxy, near[..., None].repeat(2, -1), 1)
    rxy = np.where((kind < 2)[..., None], at + rng.normal(0, 1.5, (B, NR, 2)), rng.uniform(0, 1, (B, NR, 2)) * np.array([W0, H0]))
    rdep = np.where(kind == 0, np.take_along_axis(ldep, near, 1) + rng.uniform(-2, 2, (B, NR)), rng.uniform(2, 100, (B, NR)))
    return np.clip(rxy, 0.0, np.array([W0, H0]) - 1e-3), np.clip(rdep, 1.0, 125.0), lxy, ldep


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


def cpu_timed(fn, reps=7):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), min(out), max(out)


def line(name, t, extra=""):
    print("%-58s %10.1f us  [%.1f .. %.1f]%s" % (name, t[0], t[1], t[2], extra), flush=True)


def cpu_lines(rxy, rdep, lxy, ldep):
    import radar_filter_ref as F
    torch.set_num_threads(1)
    line("numpy restatement filter_points, one frame, one core", cpu_timed(lambda: F.filter_points(rxy[0], rdep[0], lxy[0], ldep[0])))
    if "--reference" in sys.argv:
        sys.path.insert(0, sys.argv[sys.argv.index("--reference") + 1])
        np.int = int
        for name in ("matplotlib", "matplotlib.pyplot", "dataset.nuscenes_dataset", "config", "config.config_nuscenes"):      # not needed by the filter
            m = types.ModuleType(name)
            m.Nuscenes_dataset = m.config_nuscenes = None
            sys.modules.setdefault(name, m)
        from dataset.radar_preprocessing import filter_radar_points_gt
        third = lambda xy: np.concatenate((xy.T, np.ones((1, xy.shape[0]))), 0)      # noqa: E731
        got = filter_radar_points_gt(third(rxy[0]), rdep[0], third(lxy[0]), ldep[0])["valid_labels"][:, 0]
        assert np.array_equal(got, F.filter_points(rxy[0], rdep[0], lxy[0], ldep[0])[0])
        line("reference filter_radar_points_gt, one frame, one core", cpu_timed(lambda: filter_radar_points_gt(third(rxy[0]), rdep[0], third(lxy[0]), ldep[0])))


def main():
    rng = np.random.RandomState(11)
    rxy, rdep, lxy, ldep = points(rng)
    print("radar_filtered: b=%d, %dx%d frames, %d radar / %d lidar points per frame, crop %dx%d; median of %d groups [fastest .. slowest]"
          % (B, H0, W0, NR, NL, CROP[0], CROP[1], REPS))
    if "--cpu-only" in sys.argv:
        return cpu_lines(rxy, rdep, lxy, ldep)
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    from radar_depth_amd.dataset import (center_crop_params, draw_train_params, filter_radar_points, prepare_train_params, stage_train_batch,
                                         stage_val_batch)
    dev = [torch.from_numpy(a).cuda() for a in (rxy, rdep, lxy, ldep)]
    nr, nl = [NR] * B, [NL] * B
    img = torch.randint(0, 256, (B, H0, W0, 3), dtype=torch.uint8, device="cuda")
    lid = torch.randint(0, 20000, (B, H0, W0), dtype=torch.int16, device="cuda")
    f = filter_radar_points(*dev, nr, nl, (H0, W0))
    rad = torch.zeros(B, H0, W0, dtype=torch.int16, device="cuda")                   # the radar map the points make
    bi = torch.arange(B, device="cuda").view(B, 1).expand(B, NR)
    rad[bi, dev[0][..., 1].long(), dev[0][..., 0].long()] = (dev[1] * 256).round().to(torch.int16)
    labels = f.valid_labels.cpu().numpy()
    print("labels 0 / 1 / 2 over the batch: %s" % np.bincount(labels.reshape(-1), minlength=3).tolist())
    p = draw_train_params(B, CROP, rng=np.random.RandomState(0))
    prep = prepare_train_params(p, H0, W0, CROP)
    L = lib()
    i0, j0, th, tw = center_crop_params(H0, W0, CROP)
    inputs = torch.zeros(B, 4, th, tw, device="cuda")
    imap_out = torch.empty(B, 1, th, tw, dtype=torch.int32, device="cuda")
    nrp, base = C.c_void_p(f.n_radar.ctypes.data), prep.tables.data_ptr()

    def launch_val():
        check(L.rd_stage_index_filter_val(ptr(f.index_map), ptr(f.valid_mask), nrp, B, NR, H0, W0, i0, j0, th, tw, 1, ptr(inputs), ptr(imap_out),
                                          current_stream()), "rd_stage_index_filter_val")

    def launch_train():
        check(L.rd_stage_index_filter_train(ptr(f.index_map), ptr(f.valid_mask), nrp, B, NR, H0, W0, th, tw, C.c_void_p(prep.records.ctypes.data),
                                            C.c_void_p(base + 4 * prep.offsets[0]), C.c_void_p(base + 4 * prep.offsets[1]), 1, ptr(inputs),
                                            ptr(imap_out), current_stream()), "rd_stage_index_filter_train")

    rows = {}
    for name, fn in (("filter_radar_points (filter + index_map fill + scatter)", lambda: filter_radar_points(*dev, nr, nl, (H0, W0))),
                     ("rd_stage_index_filter_val launch", launch_val),
                     ("rd_stage_index_filter_train launch", launch_train),
                     ("stage_val_batch radar", lambda: stage_val_batch(img, lid, rad, CROP, 80.0)),
                     ("stage_val_batch radar_filtered", lambda: stage_val_batch(img, lid, rad, CROP, 80.0, "radar_filtered", f)),
                     ("stage_train_batch radar", lambda: stage_train_batch(img, lid, rad, prep, CROP, 80.0)),
                     ("stage_train_batch radar_filtered", lambda: stage_train_batch(img, lid, rad, prep, CROP, 80.0, "rgbd", "radar_filtered", f))):
        rows[name] = timed(fn)
        line(name, rows[name])
    added = rows["filter_radar_points (filter + index_map fill + scatter)"][0] + rows["stage_train_batch radar_filtered"][0] - rows["stage_train_batch radar"][0]
    print("radar_filtered adds %.1f us to a staged training batch (%.1f us per frame)" % (added, added / B))
    cpu_lines(rxy, rdep, lxy, ldep)
    if "--no-step" in sys.argv:
        return
    from radar_depth_amd.main import HipTrainStep, create_model
    from radar_depth_amd.synthetic import make_batch
    torch.manual_seed(0)
    model = create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), list(CROP)).cuda()
    ts = HipTrainStep(model, B, CROP[0], CROP[1], lr=0.01, momentum=0.9, weight_decay=1e-4, operands="split")
    x, t = make_batch(B, CROP[0], CROP[1], 1234)
    x, t = x.cuda(), t.cuda()
    step = timed(lambda: ts.step(x, t), inner=5, warmup=5)
    line("fused step (config 2: resnet18_latefusion b=%d %dx%d, split)" % (B, CROP[0], CROP[1]), step, "  %.0f samples/s" % (B / step[0] * 1e6))
    ratio = added / step[0]
    print("radar_filtered added / step = %.4f (%s the 0.1 condition)" % (ratio, "meets" if ratio < 0.1 else "MISSES"))


if __name__ == "__main__":
    main()

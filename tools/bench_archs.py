#!/usr/bin/env python3
"""Fused training step (HipTrainStep, split plan, stream launches) at b=16, 450x800 for the early-fusion ResNet in its three
modalities and for resnet18_latefusion, with the upproj and the deconv2 decoder, in one process on one GPU: one JSON line per
(arch, modality, decoder) (samples/s, ms/step).

    python tools/bench_archs.py [--steps 20] [--warmup 5] [--batch 16] [--archs resnet18:rgb,resnet18:rgbd,resnet18:d,resnet18_latefusion:rgbd]
                                [--decoders upproj,deconv2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radar_depth_amd.main import HipTrainStep  # noqa: E402
from radar_depth_amd.model.models import ResNet, ResNet_latefusion  # noqa: E402
from radar_depth_amd.model.models import _close_plan  # noqa: E402
from radar_depth_amd.synthetic import make_batch, procedural_fill_  # noqa: E402

SLICES = {"rgb": (0, 3), "rgbd": (0, 4), "d": (3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=450)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--archs", default="resnet18:rgb,resnet18:rgbd,resnet18:d,resnet18_latefusion:rgbd")
    ap.add_argument("--decoders", default="upproj,deconv2")
    a = ap.parse_args()
    b, h, w = a.batch, a.height, a.width
    x4, t = make_batch(b, h, w, 1234)
    t = t.cuda()
    for dec in a.decoders.split(","):
        for spec in a.archs.split(","):
            arch, modality = spec.split(":")
            lo, hi = SLICES[modality]
            x = x4[:, lo:hi].contiguous().cuda()
            torch.manual_seed(0)
            if arch == "resnet18_latefusion":
                m = ResNet_latefusion(18, dec, [h, w], hi - lo, False)
            else:
                m = ResNet(int(arch[6:]), dec, [h, w], hi - lo, False)
            procedural_fill_(m)
            m = m.cuda().train()
            ts = HipTrainStep(m, b, h, w, use_graph=False, operands="split")
            for _ in range(a.warmup):
                ts.step(x, t)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                loss, _ = ts.step(x, t)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            print(json.dumps({"arch": arch, "modality": modality, "decoder": dec, "batch": b, "height": h, "width": w, "steps": a.steps,
                              "ms_per_step": round(ms, 3), "samples_per_s": round(b * 1e3 / ms, 1), "loss": round(float(loss.item()), 5)}),
                  flush=True)
            plans = list(ts.plans)
            ts.close()
            for pl in plans:
                _close_plan(pl)
            del ts, m, plans, x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Fused resnet18_latefusion training step (HipTrainStep, split plan, stream launches) at b=16, 450x800 for each of the four decoders,
in one process on one GPU: one JSON line per decoder (samples/s, ms/step).  The decoders' forward work from the shapes, in GMAC per
sample: upproj 3.34, upconv 1.23, deconv3 0.44, deconv2 0.20.

    python tools/bench_decoders.py [--steps 20] [--warmup 5] [--batch 16] [--decoders upproj,upconv,deconv3,deconv2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radar_depth_amd.main import HipTrainStep  # noqa: E402
from radar_depth_amd.model.models import ResNet_latefusion  # noqa: E402
from radar_depth_amd.model.models import _close_plan  # noqa: E402
from radar_depth_amd.synthetic import make_batch, procedural_fill_  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=450)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--decoders", default="upproj,upconv,deconv3,deconv2")
    a = ap.parse_args()
    b, h, w = a.batch, a.height, a.width
    x, t = make_batch(b, h, w, 1234)
    x, t = x.cuda(), t.cuda()
    for dec in a.decoders.split(","):
        torch.manual_seed(0)
        m = ResNet_latefusion(18, dec, [h, w], 4, False)
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
        print(json.dumps({"decoder": dec, "batch": b, "height": h, "width": w, "steps": a.steps, "ms_per_step": round(ms, 3),
                          "samples_per_s": round(b * 1e3 / ms, 1), "loss": round(float(loss.item()), 5)}), flush=True)
        plans = list(ts.plans)
        ts.close()
        for pl in plans:
            _close_plan(pl)
        del ts, m, plans
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

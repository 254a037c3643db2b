#!/usr/bin/env python3
"""Golden vectors for the on-device meters from the REAL reference (evaluation/metrics.py imports only torch, math, numpy):
three sequences of Result.evaluate / AverageMeter.update on the CPU.  Authoring container only:
    python tests/golden/make_golden_meter.py

  1. four training "steps" at [3,1,37,53], weights 3, 3, 2, 3: every step's Result and the AverageMeter.average() after each;
  2. five frames of [1,1,37,53] evaluated one at a time (weight 1) into three meters chosen by a per-frame bitmask; frame 3 has a
     single valid pixel: the three averages;
  3. a frame without a valid pixel: its Result (NaN in all ten).

Values are multiples of 2^-6 (the file stays small); no valid pixel's ratio max(o/t, t/o) lies within 1e-4 (relative) of 1.25,
1.25^2 or 1.25^3, so the delta counts cannot flip between the CPU's and the GPU's division and the deltas are exact."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from evaluation.metrics import AverageMeter, Result  # noqa: E402

NAMES = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10", "delta1", "delta2", "delta3")
Q = 64.0
g = torch.Generator().manual_seed(1010)


def quant(x):
    return torch.clamp(torch.round(x * Q), min=1.0) / Q


def pair(frames, share):
    tgt = quant(torch.rand(frames, 1, 37, 53, generator=g) * 80 + 0.1)
    out = quant(tgt * (torch.rand(frames, 1, 37, 53, generator=g) * 1.9 + 0.4))
    tgt = torch.where(torch.rand(frames, 1, 37, 53, generator=g) < share, tgt, torch.zeros_like(tgt))
    for _ in range(8):                     # move ratios out of the bands around the three thresholds
        ratio = torch.max(out / tgt.clamp(min=1 / Q), tgt / out).double()
        near = torch.zeros_like(tgt, dtype=torch.bool)
        for k in (1, 2, 3):
            near |= ((ratio / 1.25 ** k - 1).abs() < 2e-4)
        out = torch.where(near & (tgt > 0), quant(out * 1.01 + 1 / Q), out)
    return out, tgt


def check_bands(out, tgt):
    v = tgt > 0
    o, t = out[v].double(), tgt[v].double()
    ratio = torch.max(o / t, t / o)
    for k in (1, 2, 3):
        assert not bool(((ratio / 1.25 ** k - 1).abs() < 1e-4).any()), "a ratio inside the band of 1.25^%d" % k


def vec(r):
    return np.array([getattr(r, n) for n in NAMES], dtype=np.float64)


# ---- 1. four steps
s_out, s_tgt = pair(12, 0.3)
s_out, s_tgt = s_out.view(4, 3, 1, 37, 53), s_tgt.view(4, 3, 1, 37, 53)
weights = [3, 3, 2, 3]
meter = AverageMeter()
step_results, step_averages = [], []
for k in range(4):
    check_bands(s_out[k], s_tgt[k])
    r = Result()
    r.evaluate(s_out[k], s_tgt[k])
    meter.update(r, 0.0, 0.0, weights[k])
    step_results.append(vec(r))
    step_averages.append(vec(meter.average()))

# ---- 2. five frames, three meters
f_out, f_tgt = pair(5, 0.3)
keep = torch.zeros_like(f_tgt[3], dtype=torch.bool)
keep[0, 17, 29] = True
f_tgt[3] = torch.where(keep, quant(torch.full_like(f_tgt[3], 23.4)), torch.zeros_like(f_tgt[3]))
f_out[3, 0, 17, 29] = 20.0
groups = [0b001, 0b011, 0b101, 0b111, 0b010]
meters = [AverageMeter() for _ in range(3)]
for k in range(5):
    check_bands(f_out[k], f_tgt[k])
    r = Result()
    r.evaluate(f_out[k:k + 1], f_tgt[k:k + 1])
    for b, m in enumerate(meters):
        if groups[k] >> b & 1:
            m.update(r, 0.0, 0.0, 1)
assert int((f_tgt[3] > 0).sum()) == 1
frame_averages = [vec(m.average()) for m in meters]

# ---- 3. no valid pixel
e_out, _ = pair(1, 0.3)
e_tgt = torch.zeros_like(e_out)
r = Result()
r.evaluate(e_out, e_tgt)
empty = vec(r)
assert np.isnan(empty).all()

path = os.path.join(HERE, "meter.npz")
np.savez_compressed(path, names=np.array(NAMES), step_out=s_out.numpy(), step_target=s_tgt.numpy(),
                    step_weights=np.array(weights, dtype=np.float64), step_results=np.stack(step_results),
                    step_averages=np.stack(step_averages), frame_out=f_out.numpy(), frame_target=f_tgt.numpy(),
                    frame_groups=np.array(groups, dtype=np.int32), frame_averages=np.stack(frame_averages),
                    empty_out=e_out.numpy(), empty_target=e_tgt.numpy(), empty_result=empty)
print("wrote meter.npz, %d bytes" % os.path.getsize(path), [round(v, 5) for v in step_averages[-1]])

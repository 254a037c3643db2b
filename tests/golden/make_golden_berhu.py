#!/usr/bin/env python3
"""Golden vectors for MaskedBerHuLoss from the REAL reference class (evaluation/criteria_new.py:57-81 imports only torch and numpy), on
torch CPU.  Authoring container only:
    python tests/golden/make_golden_berhu.py <reference checkout>

Per case: pred, target, thresh, the reference's loss and its autograd gradient of (3 * loss).backward().

  rand     2x1x33x47, about 40 % valid, predictions on both sides of the target; one INVALID pixel has a larger |t - p| than any valid one
  ladder   1x1x9x13, thresh 0.2, the maximum planted (t = 70, p = 20) so that delta = 10 exactly; three rungs of pixels at diff = 10 and
           its +-1 and +-2 float32 neighbours (ladder_pos, ladder_steps: flat positions and the step of each)
  ladder2  the same around a delta that float32 cannot hold (maximum 50.3 -> delta = 0.2 * float32(50.3))
  thresh1  thresh = 1: the pixel holding the maximum is in neither branch
  equal    every valid pixel equals the prediction: NaN loss, zero gradient
  tail     1x1x1x5, the maximum in the last element
  big      3x1x900x800 from a seed (tests/berhu_ref.big_planes): only the seed and the reference's loss are stored"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import berhu_ref  # noqa: E402

spec = importlib.util.spec_from_file_location("reference_criteria_new", os.path.join(sys.argv[1], "evaluation", "criteria_new.py"))
crit = importlib.util.module_from_spec(spec)
spec.loader.exec_module(crit)

F = np.float32
rng = np.random.default_rng(571)
out = {}


def scene(shape, share=0.4, spread=30.0):
    n = int(np.prod(shape))
    target = (rng.random(n, dtype=F) * F(80) + F(0.5)).astype(F)
    pred = (target + (rng.random(n, dtype=F) - F(0.5)) * F(spread)).astype(F)
    target[rng.random(n, dtype=F) >= F(share)] = 0
    return pred.reshape(shape), target.reshape(shape)


def reference(pred, target, thresh, grad=True):
    p = torch.from_numpy(pred).clone().requires_grad_(grad)
    loss = crit.MaskedBerHuLoss(thresh)(p, torch.from_numpy(target))
    if not grad:
        return F(loss.item()), None
    (3 * loss).backward()
    return F(loss.item()), p.grad.numpy().copy()


def store(name, pred, target, thresh):
    loss, grad = reference(pred, target, thresh)
    out.update({name + "_pred": pred, name + "_target": target, name + "_thresh": np.float64(thresh), name + "_loss": loss, name + "_grad": grad})
    return loss


def steps_of(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


def ladder(name, top_t, top_p):
    pred, target = scene((1, 1, 9, 13), share=0.5, spread=60.0)
    p, t = pred.reshape(-1), target.reshape(-1)
    keep = np.abs(t - p) < F(29)                                # nothing of the scene reaches the planted maximum
    t[~keep] = 0
    t[0], p[0] = F(top_t), F(top_p)
    big = np.abs(t[0] - p[0])
    delta = 0.2 * float(big)
    pos, steps = [], []
    at = 20
    for base_t in (None, F(1), F(3)):                          # three rungs: p = 0, t = d;  t = 1, p = 1 + d;  t = 3, p = 3 + d
        for k in (-2, -1, 0, 1, 2):
            d = steps_of(F(delta), k)
            if base_t is None:
                t[at], p[at] = d, F(0)
            else:
                t[at], p[at] = base_t, F(base_t + d)
            assert np.abs(t[at] - p[at]) == d, (name, base_t, k)   # the planted difference is exact
            pos.append(at)
            steps.append(k)
            at += 3
    assert np.abs(t - p)[t > 0].max() == big
    out[name + "_pos"], out[name + "_steps"], out[name + "_delta"] = np.array(pos, np.int64), np.array(steps, np.int64), np.float64(delta)
    store(name, pred, target, 0.2)
    return delta


# ---- rand
pred, target = scene((2, 1, 33, 47))
flat_t, flat_p = target.reshape(-1), pred.reshape(-1)
bad = int(np.flatnonzero(flat_t == 0)[100])
flat_p[bad] = F(500)
out["rand_outlier"] = np.int64(bad)
store("rand", pred, target, 0.2)

# ---- ladder, ladder2
assert ladder("ladder", 70, 20) == 10.0
d2 = ladder("ladder2", 70.3, 20)
assert float(F(d2)) != d2

# ---- thresh1
pred, target = scene((1, 1, 7, 11), share=0.6)
store("thresh1", pred, target, 1.0)

# ---- equal
pred, target = scene((1, 1, 5, 7), share=0.5)
pred = np.where(target > 0, target, pred).astype(F)
loss = store("equal", pred, target, 0.2)
assert np.isnan(loss) and not out["equal_grad"].any()

# ---- tail
store("tail", np.array([1, 2, 3, 4, 5], F).reshape(1, 1, 1, 5), np.array([1.5, 0, 2.25, 4.5, 14], F).reshape(1, 1, 1, 5), 0.2)

# ---- big
seed = 90210
pred, target = berhu_ref.big_planes(seed)
loss, _ = reference(pred, target, 0.2, grad=False)
out.update({"big_seed": np.int64(seed), "big_thresh": np.float64(0.2), "big_loss": loss,
            "big_check": np.array([pred.astype(np.float64).sum(), target.astype(np.float64).sum()])})

path = os.path.join(HERE, "berhu.npz")
np.savez_compressed(path, **out)
print("wrote berhu.npz, %d bytes" % os.path.getsize(path), {k: float(v) for k, v in out.items() if k.endswith("_loss")})

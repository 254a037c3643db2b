"""numpy restatement of MaskedBerHuLoss as this port defines it (include/radar_depth_hip.h, rd_masked_berhu_sums), written from that
definition: every step is a float32 operation rounded on its own, delta alone is a double.

    v = target > 0;  diff = |t - p|;  M = max over v of diff;  delta = thresh * (double)M
    thr = f32(-delta), d2 = f32(delta * delta), den = f32(2 * delta)
    in1 = (-diff > thr);  y = f32(f32(diff * diff) - d2);  in2 = (y > 0)
    term = f32((in1 ? diff : 0) + f32(f32((in2 ? y : -d2) + d2) / den))
    loss = (float64 sum of the terms) / count
    d loss / d pred = -sign(t - p) * k * ([in1] + [in2] * 2 diff / den),  k = coef / count

`mode` swaps in a shortcut a kernel writer might take, to show that the fixture tells them apart:
    "single_compare"  one test diff < f32(delta) chooses the branch (no pixel is in neither)
    "textbook"        (diff^2 + delta^2) / (2 delta) above the threshold
    "reciprocal"      multiplication by f32(1 / den) instead of the division"""
from types import SimpleNamespace

import numpy as np

F = np.float32
MODES = ("exact", "single_compare", "textbook", "reciprocal")


def berhu(pred, target, thresh, coef=1.0, mode="exact"):
    assert mode in MODES, mode
    p = np.ascontiguousarray(pred, dtype=F)
    t = np.ascontiguousarray(target, dtype=F)
    v = t > 0
    count = int(v.sum())
    diff = np.abs(t - p)
    big = F(diff[v].max()) if count else F(0)
    delta = float(thresh) * float(big)
    thr, d2, den = F(-delta), F(delta * delta), F(2.0 * delta)
    with np.errstate(all="ignore"):
        sq = diff * diff
        y = sq - d2
        in1 = v & (-diff > thr)
        in2 = v & (y > 0)
        if mode == "single_compare":
            in1 = v & (diff < F(delta))
            in2 = v & ~in1
        part1 = np.where(in1, diff, F(0))
        num = np.where(in2, y, -d2) + d2
        if mode == "textbook":
            num = np.where(in2, sq + d2, F(0))
        part2 = num * (F(1) / den) if mode == "reciprocal" else num / den
        term = np.where(v, part1 + part2, F(0))
        assert term.dtype == F and y.dtype == F
        total = float(term[v].astype(np.float64).sum())
        loss = total / count if count else float("nan")
        k = F(coef) / F(count)
        through2 = (k / den) * (F(2) * diff)
        a = np.where(in1, k, F(0)) + np.where(in2, through2, F(0))
        grad = np.where(v, -np.sign(t - p) * a, F(0)).astype(F)
        grad[grad == 0] = 0                                      # (-0 -> +0)
    return SimpleNamespace(loss=loss, total=total, count=count, max=big, delta=delta, term=term, in1=in1, in2=in2, grad=grad, valid=v)


def big_planes(seed, shape=(3, 1, 900, 800)):
    """The `big` case of tests/golden/berhu.npz, which stores only this seed and the reference's loss: more than 1024 * 256 * 8 elements,
    so the kernels' grid-stride loops go round more than once.  About 40 % of the pixels are valid, predictions lie on both sides."""
    rng = np.random.default_rng(int(seed))
    n = int(np.prod(shape))
    target = (rng.random(n, dtype=F) * F(80) + F(0.5)).astype(F)
    pred = (target + (rng.random(n, dtype=F) - F(0.5)) * F(30)).astype(F)
    target[rng.random(n, dtype=F) >= F(0.4)] = 0
    return pred.reshape(shape), target.reshape(shape)

#!/usr/bin/env python3
"""Golden vectors for the distance-interval metrics from the REAL reference (evaluation/metrics.py imports only torch, math, numpy):
Result_multidist.evaluate on CPU tensors.  Authoring container only; the reference checkout is named on the command line:
    python tests/golden/make_golden_multidist.py /path/to/reference

What runs in the reference and what does not.  Result_multidist.evaluate runs; every `<case>_metrics` [10 intervals][10] (Result.update's
order, NaN where an interval has no pixel) and `<case>_valid` (valid_label) below is its output.  AverageMeter_multidist.update and
Result_multidist.update cannot run there (a call without gpu_time / data_time, an iteration over a non-iterable, an attribute `log10`
that does not exist), so the REPAIRED averaging has no live reference: `seq_averages` / `seq_valid` are formed here from the
reference's own Result and AverageMeter classes, driven per interval the way the repair describes -- interval k of a result enters
AverageMeter k through update(res, 0, 0, n) when its valid_label is 1 and is passed over otherwise; an AverageMeter that never
received anything stands for the zero Result and valid_label 0.

Cases (frames are at most 64 x 96):
  rand      [2,1,64,96] as one tensor: targets over 0..110 m, zeros and a few negatives mixed in; every interval holds at least
            500 pixels, because the reference sums in float32 and its lg10 term cancels: the bar of 1e-5 against these values is
            to be met with threefold headroom by a float64 sum of the same terms (tests/test_multidist_host.py)
  ladder    every edge 10, 20, ..., 90 and 100 with its float32 predecessor and successor, the smallest positive float32, targets
            above 100, a zero and a negative
  sparse    a frame with several empty intervals;  single: every pixel in one interval;  empty: no valid pixel
  batch     three frames with different populated sets, each evaluated on its own (the per-frame path)
  tail5 / tail1   hw = 5 and hw = 1
  seq       the repaired averaging over sparse (n = 2), single (n = 1), empty (n = 3), the three batch frames (n = 1) and rand (n = 2)

Values are multiples of 2^-6 except on the ladder (the file stays small); no valid pixel's ratio max(o/t, t/o) lies within 1e-4
(relative) of 1.25, 1.25^2 or 1.25^3, so the delta counts cannot flip between the CPU's and the GPU's division."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
from evaluation.metrics import AverageMeter, Result, Result_multidist  # noqa: E402

NAMES = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10", "delta1", "delta2", "delta3")
Q = 64.0
g = torch.Generator().manual_seed(1610)
EDGES = [10., 20., 30., 40., 50., 60., 70., 80., 90., 100.]


def quant(x):
    return torch.clamp(torch.round(x * Q), min=1.0) / Q


def off_bands(out, tgt, requant=True):
    """Move predictions whose ratio sits in the bands around the three thresholds."""
    for _ in range(8):
        ratio = torch.max(out / tgt.clamp(min=1e-30), tgt / out).double()
        near = torch.zeros_like(tgt, dtype=torch.bool)
        for k in (1, 2, 3):
            near |= ((ratio / 1.25 ** k - 1).abs() < 2e-4)
        moved = out * 1.01 + 1 / Q
        out = torch.where(near & (tgt > 0), quant(moved) if requant else moved, out)
    v = tgt > 0
    o, t = out[v].double(), tgt[v].double()
    ratio = torch.max(o / t, t / o)
    for k in (1, 2, 3):
        assert not bool(((ratio / 1.25 ** k - 1).abs() < 1e-4).any()), "a ratio inside the band of 1.25^%d" % k
    return out


def pair(shape, lo, hi, share, negatives=0.0):
    tgt = quant(torch.rand(shape, generator=g) * (hi - lo) + lo)
    out = quant(tgt * (torch.rand(shape, generator=g) * 1.9 + 0.4))
    u = torch.rand(shape, generator=g)
    tgt = torch.where(u < share, tgt, torch.zeros_like(tgt))
    tgt = torch.where(u > 1 - negatives, -quant(torch.rand(shape, generator=g) * 50), tgt)
    return off_bands(out, tgt), tgt


def vec(r):
    return np.array([getattr(r, n) for n in NAMES], dtype=np.float64)


def evaluate(out, tgt):
    r = Result_multidist()              # made fresh per evaluation: valid_label is only ever cleared
    assert r.dist_interval == EDGES
    r.evaluate(out, tgt)
    m = np.stack([vec(res) for res in r.result_lst])
    valid = np.array(r.valid_label, dtype=np.int32)
    assert np.array_equal(np.isnan(m).all(axis=1), valid == 0) and not np.isnan(m[valid == 1]).any()
    return r, m, valid


def counts(tgt):
    t = tgt.flatten()
    lo = [0.] + EDGES[:-1]
    hi = EDGES[:-1] + [float("inf")]
    return [int(((t > 0) & (t >= a) & (t <= b)).sum()) for a, b in zip(lo, hi)]


store, results = {"names": np.array(NAMES), "edges": np.array(EDGES, dtype=np.float32)}, {}


def case(name, out, tgt):
    r, m, valid = evaluate(out, tgt)
    store[name + "_out"], store[name + "_target"] = out.numpy(), tgt.numpy()
    store[name + "_metrics"], store[name + "_valid"] = m, valid
    store[name + "_counts"] = np.array(counts(tgt), dtype=np.int64)
    results[name] = r
    return r


# ---- rand
r_out, r_tgt = pair((2, 1, 64, 96), 0.05, 110.0, 0.88, negatives=0.02)
assert min(counts(r_tgt)) >= 500, counts(r_tgt)
case("rand", r_out, r_tgt)

# ---- ladder
f32 = np.float32
vals = [np.nextafter(f32(0), f32(1)), f32(0), f32(-3.5), f32(105.25), f32(1000)]
for e in EDGES:
    vals += [np.nextafter(f32(e), f32(0)), f32(e), np.nextafter(f32(e), f32(np.inf))]
l_tgt = torch.from_numpy(np.array(vals, dtype=np.float32)).view(1, 1, 1, -1)
l_out = l_tgt.abs() * (torch.rand(l_tgt.shape, generator=g) * 0.5 + 0.7) + 0.25
l_out = off_bands(l_out, l_tgt, requant=False)
r = case("ladder", l_out, l_tgt)
assert store["ladder_counts"].tolist() == [3, 4, 4, 4, 4, 4, 4, 4, 4, 7], store["ladder_counts"]     # every inner edge twice

# ---- sparse / single / empty
s_out, s_tgt = pair((1, 1, 24, 40), 12.0, 38.0, 0.4)
far_out, far_tgt = pair((1, 1, 24, 40), 72.0, 79.0, 0.1)
s_tgt = torch.where(s_tgt > 0, s_tgt, far_tgt)
s_out = torch.where(s_tgt == far_tgt, far_out, s_out)
case("sparse", s_out, s_tgt)
assert (store["sparse_valid"] == 0).sum() >= 4
o_out, o_tgt = pair((1, 1, 24, 40), 41.0, 49.0, 0.6)
case("single", o_out, o_tgt)
assert store["single_valid"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
e_out, _ = pair((1, 1, 24, 40), 1.0, 80.0, 0.5)
case("empty", e_out, torch.zeros_like(e_out))
assert store["empty_valid"].sum() == 0

# ---- batch: three frames, different populated sets
b_parts = [pair((1, 1, 24, 40), 0.5, 33.0, 0.5), pair((1, 1, 24, 40), 55.0, 130.0, 0.5, negatives=0.05), pair((1, 1, 24, 40), 25.0, 65.0, 0.02)]
b_out, b_tgt = torch.cat([p[0] for p in b_parts]), torch.cat([p[1] for p in b_parts])
bm, bv, bc, b_results = [], [], [], []
for k in range(3):
    r, m, valid = evaluate(b_out[k:k + 1], b_tgt[k:k + 1])
    bm.append(m), bv.append(valid), bc.append(counts(b_tgt[k])), b_results.append(r)
assert len({tuple(v.tolist()) for v in bv}) == 3
store.update(batch_out=b_out.numpy(), batch_target=b_tgt.numpy(), batch_metrics=np.stack(bm), batch_valid=np.stack(bv),
             batch_counts=np.array(bc, dtype=np.int64))

# ---- tails
t_out, t_tgt = pair((1, 1, 1, 5), 5.0, 95.0, 0.8)
case("tail5", t_out, t_tgt)
case("tail1", t_out[..., :1], torch.full((1, 1, 1, 1), 47.5))

# ---- the repaired averaging, from the reference's Result / AverageMeter
seq = [(results["sparse"], 2), (results["single"], 1), (results["empty"], 3)] + [(r, 1) for r in b_results] + [(results["rand"], 2)]
meters = [AverageMeter() for _ in EDGES]
for r, n in seq:
    for k, res in enumerate(r.result_lst):
        if r.valid_label[k] != 0:
            meters[k].update(res, 0, 0, n)
avg, avg_valid = np.zeros((len(EDGES), 10)), np.zeros(len(EDGES), dtype=np.int32)
for k, m in enumerate(meters):
    if m.count > 0:
        avg[k], avg_valid[k] = vec(m.average()), 1
# ... and a Result_multidist.update as repaired: a copy of every field of every interval
store.update(seq_names=np.array(["sparse", "single", "empty", "batch0", "batch1", "batch2", "rand"]),
             seq_weights=np.array([n for _, n in seq], dtype=np.float64), seq_averages=avg, seq_valid=avg_valid,
             seq_counts=np.array([m.count for m in meters], dtype=np.float64))

path = os.path.join(HERE, "multidist.npz")
np.savez_compressed(path, **store)
print("wrote multidist.npz, %d bytes; rand counts %s" % (os.path.getsize(path), counts(r_tgt)))

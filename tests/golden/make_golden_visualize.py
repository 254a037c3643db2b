"""Golden vectors for the comparison rows (rd_render_rows; radar_depth_amd.utils.merge_into_row, merge_into_row_with_gt,
colored_depthmap), produced from the reference checkout.

Every row comes from the reference's OWN ``utils.merge_into_row``, ``utils.merge_into_row_with_gt`` and ``utils.colored_depthmap``
(utils.py:114-153) on CPU tensors, followed by the ``.astype('uint8')`` of its ``save_image``; matplotlib and Pillow are the real ones,
the packages this environment lacks get the same stand-ins as in make_golden_radar_filter.py.  The reference's divide warnings of the
degenerate frames are suppressed.  The 259 x 3 uint8 table (trunc(255 * viridis._lut[:, :3])) is stored in the fixture and asserted
equal to the one the package ships (``--write-table`` regenerates that file).

For every case the numpy-only restatement tests/visualize_ref.py is asserted to reproduce the reference bit for bit, and what the
tests rely on is asserted here:
  * rgbd1: a negative minimum in the prediction, the maximum in the lidar plane;
  * ladder: for every bin k = 1..255 the smallest float32 depth whose index is k and that depth's float32 predecessor (510 pixels of
    the prediction); a reciprocal-multiply variant and a float64 variant of the restatement each change at least 50 of them;
  * const: black depth panels;  batch: five frames whose ranges differ by orders of magnitude, channel slices of one [5,4,H,W] tensor,
    the reference called per frame;  edge: rgb 0, 1, k/255 and both float32 neighbours of every k/255;
  * cmap: a given range with pixels below it, above it and exactly on d_max; d_min == d_max gives under, over and bad.
    python tests/golden/make_golden_visualize.py [--write-table]"""
import collections
import collections.abc
import importlib
import importlib.abc
import importlib.machinery
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import visualize_ref as V  # noqa: E402


class _Empty(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        d = _Empty(self.__name__ + "." + name)
        setattr(self, name, d)
        return d

    def __call__(self, *a, **k):
        return _Empty("call")


class _MissingPackages(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    NAMES = ("h5py", "nuscenes", "pyquaternion", "cv2", "torchvision", "skimage", "ipdb", "attrdict", "accimage")

    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in self.NAMES:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return _Empty(spec.name)

    def exec_module(self, module):
        module.__path__ = []


sys.meta_path.insert(0, _MissingPackages())
collections.Iterable = collections.abc.Iterable
np.int = int
sys.path.insert(0, os.environ.get("RADAR_DEPTH_REFERENCE", "/root/reference"))
ref_utils = importlib.import_module("utils")
assert hasattr(ref_utils, "merge_into_row_with_gt") and ref_utils.cmap.name == "viridis"

H, W = 33, 47
LH, LW = 45, 80
LADDER_MAX = np.float32(119.93791)


def u8(a):
    with np.errstate(all="ignore"):
        return np.asarray(a).astype("uint8")                # save_image's cast


def make_table():
    cmap = ref_utils.cmap
    cmap(np.zeros(1))                                       # fills _lut
    lut = np.asarray(cmap._lut, np.float64)
    assert lut.shape == (259, 4)
    table = np.trunc(255 * lut[:, :3]).astype(np.uint8)
    assert np.array_equal(table[V.UNDER], table[0]) and np.array_equal(table[V.OVER], table[255]) and not table[V.BAD].any()
    return table


def ref_row(inputs, target, pred):
    """The reference on one frame, as main.py:662-677 calls it: inputs [1,3|4,h,w], target / pred [1,1,h,w] (CPU tensors)."""
    t = torch.from_numpy
    with np.errstate(all="ignore"):
        if inputs.shape[1] == 4:
            return u8(ref_utils.merge_into_row_with_gt(t(inputs[:, :3]), t(inputs[:, 3:]), t(target), t(pred)))
        return u8(ref_utils.merge_into_row(t(inputs), t(target), t(pred)))


def restated_row(inputs, target, pred, table, mode="exact"):
    planes = ([inputs[:, 3:4]] if inputs.shape[1] == 4 else []) + [target, pred]
    return V.merge_rows(inputs[:, :3], planes, table, mode)[0]


def sparse(rng, shape, density, lo, hi):
    return (rng.uniform(lo, hi, shape) * (rng.rand(*shape) < density)).astype(np.float32)


def frame(rng, h, w, channels, scale=1.0):
    inputs = rng.rand(1, channels, h, w).astype(np.float32)
    if channels == 4:
        inputs[:, 3] = sparse(rng, (1, h, w), 0.02, 2, 100) * np.float32(scale)
    target = sparse(rng, (1, 1, h, w), 0.3, 2, 118.5) * np.float32(scale)
    pred = (rng.uniform(-1.5, 90, (1, 1, h, w)) * scale).astype(np.float32)
    return inputs, target, pred


def ladder_depths(d_max):
    """For k = 1..255: the smallest float32 d >= 0 with index(d) == k under d_min = 0, and its float32 predecessor (index k - 1)."""
    index = lambda d: int(V.lut_index(np.float32(d), 0.0, d_max)[()])      # noqa: E731
    out = []
    for k in range(1, 256):
        lo, hi = np.float32(0).view(np.uint32).item(), np.float32(d_max).view(np.uint32).item()     # positive floats order like their bits
        while hi - lo > 1:                                 # index(lo) < k <= index(hi)
            mid = (lo + hi) // 2
            if index(np.uint32(mid).view(np.float32)) >= k:
                hi = mid
            else:
                lo = mid
        first, before = np.uint32(hi).view(np.float32), np.uint32(lo).view(np.float32)
        assert index(first) == k and index(before) == k - 1 and np.nextafter(first, np.float32(-np.inf)) == before
        out += [before, first]
    return np.array(out, np.float32)


def main():
    table = make_table()
    if "--write-table" in sys.argv:
        with open(V.TABLE_PATH, "w") as fh:
            fh.write('{"source": "trunc(255 * matplotlib.cm.viridis._lut[:, :3]); rows 0..255 the colours, 256 under, 257 over, 258 bad",\n "rgb": [\n')
            fh.write(",\n".join("  [%d, %d, %d]" % tuple(r) for r in table.tolist()))
            fh.write("\n ]}\n")
    assert np.array_equal(V.package_table(), table), "radar_depth_amd/viridis_lut.json is not this matplotlib's table: --write-table"
    rng = np.random.RandomState(20261019)
    out = {"table": table}

    def case(name, inputs, target, pred):
        rows = np.stack([ref_row(inputs[b:b + 1], target[b:b + 1], pred[b:b + 1]) for b in range(inputs.shape[0])])
        planes = ([inputs[:, 3:4]] if inputs.shape[1] == 4 else []) + [target, pred]
        assert rows.dtype == np.uint8 and rows.shape == (inputs.shape[0], inputs.shape[2], (len(planes) + 1) * inputs.shape[3], 3)
        assert np.array_equal(V.merge_rows(inputs[:, :3], planes, table), rows), "%s: restatement != reference" % name
        out[name + "_inputs"], out[name + "_target"], out[name + "_pred"] = inputs, target, pred
        out[name + "_rows"] = rows
        return rows

    # 1, 2: one rgbd and two rgb frames
    inputs, target, pred = frame(rng, H, W, 4)
    assert pred.min() < 0 and pred.min() < min(inputs[:, 3].min(), target.min()) and target.max() > max(pred.max(), inputs[:, 3].max())
    case("rgbd1", inputs, target, pred)
    case("rgb1", *frame(rng, H, W, 3))
    case("rgb2", *frame(rng, H, W, 3, scale=0.37))

    # 3: the ladder
    inputs, target, pred = frame(rng, LH, LW, 4)
    target = np.minimum(target, np.float32(100))
    target[0, 0, 7, 11] = LADDER_MAX
    pred = np.abs(pred)
    steps = ladder_depths(LADDER_MAX)
    pos = rng.permutation(LH * LW)[:steps.size].astype(np.int64)
    pred.reshape(-1)[pos] = steps
    lo, hi = V.frame_range([inputs[:, 3], target, pred])
    assert lo == 0 and hi == LADDER_MAX and steps.size == 510
    case("ladder", inputs, target, pred)
    exact = V.lut_index(steps, lo, hi - lo)
    assert np.array_equal(exact, np.repeat(np.arange(256), 2)[1:-1])
    changed = [int((V.lut_index(steps, lo, hi - lo, mode) != exact).sum()) for mode in ("reciprocal", "float64")]
    assert min(changed) >= 50, changed
    for mode in ("reciprocal", "float64"):                  # ... and the shortcuts show in the rendered row
        assert (restated_row(inputs, target, pred, table, mode) != out["ladder_rows"][0]).any(axis=-1).sum() >= 40, mode
    out["ladder_pos"], out["ladder_changed"] = pos, np.array(changed, np.int64)

    # 4: every plane one value
    inputs, target, pred = frame(rng, H, W, 4)
    inputs[:, 3], target[:], pred[:] = 7.5, 7.5, 7.5
    rows = case("const", inputs, target, pred)
    assert not rows[0, :, W:].any() and rows[0, :, :W].any()

    # 5: five frames of one tensor, ranges orders of magnitude apart
    parts = [frame(rng, H, W, 4, scale=s) for s in (1.0, 0.01, 1000.0, 17.0, 1e-4)]
    inputs, target, pred = (np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(3))
    case("batch", inputs, target, pred)

    # 6: rgb on the byte boundaries
    inputs, target, pred = frame(rng, H, W, 3)
    ks = (np.arange(1, 255, dtype=np.float32) / np.float32(255)).astype(np.float32)
    edge = np.concatenate([[np.float32(0), np.float32(1)], ks, np.nextafter(ks, np.float32(0)), np.nextafter(ks, np.float32(1))]).astype(np.float32)
    epos = rng.permutation(3 * H * W)[:edge.size]
    inputs.reshape(-1)[epos] = edge
    rows = case("edge", inputs, target, pred)
    got = rows[0, :, :W].transpose(2, 0, 1).reshape(-1)[epos]
    assert got[0] == 0 and got[1] == 255 and len(set(got.tolist())) == 256

    # 7: colored_depthmap
    depth = rng.uniform(0, 80, (H, W)).astype(np.float32)
    d_min, d_max = 10.0, 60.5
    depth[3, 5], depth[4, 6], depth[5, 7] = d_max, d_min, np.nextafter(np.float32(d_max), np.float32(0))
    assert (depth < d_min).sum() > 50 and (depth > d_max).sum() > 50
    flat = np.full((H, W), 7.5, np.float32)
    flat[:11], flat[22:] = 2.25, 9.0
    with np.errstate(all="ignore"):
        img = u8(ref_utils.colored_depthmap(depth, d_min, d_max))
        img_own = u8(ref_utils.colored_depthmap(depth))
        img_flat = u8(ref_utils.colored_depthmap(flat, 7.5, 7.5))
    assert np.array_equal(V.colored_depthmap(depth, table, d_min, d_max), img) and np.array_equal(V.colored_depthmap(depth, table), img_own)
    assert np.array_equal(V.colored_depthmap(flat, table, 7.5, 7.5), img_flat)
    assert np.array_equal(img[3, 5], table[255]) and np.array_equal(img[4, 6], table[0]) and np.array_equal(img[5, 7], table[255])
    assert np.array_equal(img_flat[0, 0], table[V.UNDER]) and np.array_equal(img_flat[32, 0], table[V.OVER]) and not img_flat[11:22].any()
    out.update(cmap_depth=depth, cmap_range=np.array([d_min, d_max]), cmap_img=img, cmap_img_own=img_own, cmap_flat=flat,
               cmap_flat_range=np.array([7.5, 7.5]), cmap_flat_img=img_flat)

    path = os.path.join(HERE, "visualize.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes; ladder: reciprocal changes %d, float64 %d of 510" % (path, os.path.getsize(path), changed[0], changed[1]))


if __name__ == "__main__":
    main()

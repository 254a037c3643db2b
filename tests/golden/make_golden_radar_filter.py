"""Golden vectors for the radar_filtered sparsifier (rd_radar_filter_points, rd_radar_index_map, rd_stage_index_filter_val / _train),
produced from the reference checkout.

Every vector comes from the reference's OWN ``nuscenes_dataset_torch.filter_radar_points`` (dataset/nuscenes_dataset_torch_new.py:557-584,
which calls ``filter_radar_points_gt``, dataset/radar_preprocessing.py:77-122), ``transform_val`` and ``transform_train`` with
``sparsifier="radar_filtered"``, called unbound on seeded synthetic frames and points with a namespace standing in for ``self``, exactly
as make_golden_staging_train.py calls ``transform_train``: the same stand-ins for the packages this environment lacks, ``np.int = int``
and the ``imresize`` restatement.

For every case the numpy-only restatement tests/radar_filter_ref.py is asserted to reproduce the reference bit for bit, and the
conditions the tests rely on are asserted here and recorded in the file: every decision of the filter is at least MARGIN (relative)
away from its threshold and a point's four smallest distances at least that far from each other (so neither the device's exp nor the
reference's unstable argsort can change anything); the labels 0, 1, 2 all occur; one case has two radar points in one pixel; in every
staged case the filter changes the radar channel inside the crop and the radar depth map is written from the points; one training case
has point 0 invalid and rotation fill inside the crop; max_depth clamps something.  A case that falls short is reseeded.
    python tests/golden/make_golden_radar_filter.py"""
import collections
import collections.abc
import importlib
import importlib.abc
import importlib.machinery
import os
import sys
import types
import warnings

import numpy as np

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import radar_filter_ref as F  # noqa: E402
import staging_train_ref as R  # noqa: E402

MARGIN = 1e-6


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
    NAMES = ("h5py", "nuscenes", "matplotlib", "pyquaternion", "cv2", "torchvision", "skimage", "ipdb", "attrdict", "accimage")

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
import scipy.misc as misc  # noqa: E402
from PIL import Image  # noqa: E402


def _bytescale(d):
    cmin, cmax = d.min(), d.max()
    cs = cmax - cmin
    if cs == 0:
        cs = 1
    sc = np.float32(255.0 / float(cs))
    return (((d - cmin) * sc).clip(0, 255) + np.float32(0.5)).astype(np.uint8)


def imresize(arr, size, interp="bilinear", mode=None):
    """scipy 1.2's scipy.misc.imresize on today's Pillow."""
    if mode == "F":
        im = Image.fromarray(arr.astype(np.float32), mode="F")
    else:
        im = Image.fromarray(_bytescale(arr), "RGB")
    if isinstance(size, float):
        size = tuple((np.array(im.size) * size).astype(int))
    else:
        size = (size[1], size[0])
    return np.array(im.resize(size, resample={"nearest": Image.NEAREST, "bilinear": Image.BILINEAR}[interp]))


misc.imresize = imresize
sys.path.insert(0, os.environ.get("RADAR_DEPTH_REFERENCE", "/root/reference"))
ref_dataset = importlib.import_module("dataset.nuscenes_dataset_torch_new")
DS = ref_dataset.nuscenes_dataset_torch


def _self(crop, max_depth, scale_range=(1.0, 1.5), rotation=5.0):
    return types.SimpleNamespace(transform_mode="sparse-to-dense", sparsifier="radar_filtered", modality="rgbd", max_depth=max_depth,
                                 t_cfg=types.SimpleNamespace(crop_size_train=tuple(crop), crop_size_val=tuple(crop),
                                                             scale_factor_train=list(scale_range), rotation_factor=rotation))


def reference_filter(radar_xy, radar_depth, lidar_xy, lidar_depth, frame_shape, image=None):
    """The reference's filter_radar_points on one frame: (the data dict it filled, valid_labels of filter_radar_points_gt)."""
    third = lambda xy: np.concatenate((xy.T, np.ones((1, xy.shape[0]))), 0)      # noqa: E731  (the reference's points are [3, N])
    data = {"image": np.zeros(tuple(frame_shape) + (0,), np.uint8) if image is None else image,
            "radar_points": third(radar_xy), "radar_depth_points": radar_depth.copy(),
            "lidar_points": third(lidar_xy), "lidar_depth_points": lidar_depth.copy()}
    data = DS.filter_radar_points(_self((1, 1), np.inf), data)
    gt = ref_dataset.filter_radar_points_gt(data["radar_points"], data["radar_depth_points"], data["lidar_points"], data["lidar_depth_points"])
    assert np.array_equal(gt["valid_mask"], data["valid_mask"])
    return data, gt["valid_labels"][:, 0].astype(np.uint8)


def points(rng, n_radar, n_lidar, frame_shape, invalid0=False, duplicate=False):
    """Lidar uniform in the frame, 2..100 m; radar a three-way mix: near a lidar point with a consistent depth, near one with a random
    depth, anywhere.  invalid0: point 0 sits on a lidar point 25 m or more behind it (label 0); duplicate: point 1 shares point 0's pixel."""
    H0, W0 = frame_shape
    lxy = rng.uniform(0, 1, (n_lidar, 2)) * np.array([W0, H0])
    ldep = rng.uniform(2, 100, n_lidar)
    kind, near = rng.randint(0, 3, n_radar), rng.randint(0, n_lidar, n_radar)
    rxy = np.where((kind < 2)[:, None], lxy[near] + rng.normal(0, 1.5, (n_radar, 2)), rng.uniform(0, 1, (n_radar, 2)) * np.array([W0, H0]))
    rdep = np.where(kind == 0, ldep[near] + rng.uniform(-2, 2, n_radar), rng.uniform(2, 100, n_radar))
    if invalid0:
        rxy[0], rdep[0] = lxy[0] + np.array([0.3, 0.2]), 125.0
    if duplicate:
        rxy[1] = np.floor(rxy[0]) + rng.uniform(0.1, 0.9, 2)
    rxy = np.clip(rxy, 0.0, np.array([W0, H0]) - 1e-3)
    return rxy, np.clip(rdep, 1.0, 125.0), lxy, ldep


def checked_points(rng, n_radar, n_lidar, frame_shape, accept=lambda labels: True, **kw):
    """points() redrawn until the margins hold (and ``accept`` likes the labels); the restatement against the reference."""
    for _ in range(200):
        rxy, rdep, lxy, ldep = points(rng, n_radar, n_lidar, frame_shape, **kw)
        labels, valid, topk, margin = F.filter_points(rxy, rdep, lxy, ldep, with_margin=True)
        if margin >= MARGIN and accept(labels):
            break
    else:
        raise AssertionError("no acceptable draw")
    data, ref_labels = reference_filter(rxy, rdep, lxy, ldep, frame_shape)
    assert np.array_equal(ref_labels, labels) and np.array_equal(data["valid_mask"], valid), "restatement != reference (filter)"
    imap = F.index_map(rxy, frame_shape)
    assert np.array_equal(data["index_map"], imap.astype(np.float64)), "restatement != reference (index_map)"
    return dict(rxy=rxy, rdep=rdep, lxy=lxy, ldep=ldep, labels=labels, valid=valid, topk=topk, margin=margin, imap=imap)


def frames(rng, B, H0, W0):
    img = rng.randint(0, 256, size=(B, H0, W0, 3)).astype(np.uint8)
    lidar = (rng.rand(B, H0, W0) * 120.0 * 256 * (rng.rand(B, H0, W0) < 0.3)).astype(np.int16)
    return img, lidar


def staged_case(rng, name, mode, shape, crop, md, counts, seeds=None, sr=(1.0, 1.5), rot=5.0, invalid0=False):
    """One staged batch: per frame, points -> the reference's filter_radar_points -> its transform_val / transform_train."""
    B, (H0, W0) = len(counts), shape
    img, lidar = frames(rng, B, H0, W0)
    th, tw = crop
    for _ in range(200):
        pts = [checked_points(rng, nr, nl, shape, invalid0=invalid0) for nr, nl in counts]
        radar = np.stack([F.radar_map_from_points(q["rxy"], q["rdep"], shape) for q in pts])
        imaps, valids = [q["imap"] for q in pts], [q["valid"] for q in pts]
        if mode == "val":
            p = None
            got = F.stage_val(img, lidar, radar, imaps, valids, crop, md)
            plain = F.stage_val(img, lidar, radar, imaps, valids, crop, md, filtered=False)
        else:
            ps = [R.draw_params(1, crop, sr, rot, rng=np.random.RandomState(s)) for s in seeds]
            p = {k: np.concatenate([q[k] for q in ps]) for k in ps[0]}
            got = F.stage_train(img, lidar, radar, p, imaps, valids, crop, md)
            plain = F.stage_train(img, lidar, radar, p, imaps, valids, crop, md, filtered=False)
        if all((got[0][b, 3] != plain[0][b, 3]).any() for b in range(B)):          # the filter has an effect in every frame's crop
            break
    else:
        raise AssertionError(name + ": the filter never has an effect")
    outs = []
    for b in range(B):
        q = pts[b]
        data, _ = reference_filter(q["rxy"], q["rdep"], q["lxy"], q["ldep"], shape, image=img[b])
        data["lidar_depth"], data["radar_depth"] = lidar[b] / 256., radar[b] / 256.
        if mode == "val":
            o = DS.transform_val(_self(crop, md), data)
        else:
            np.random.seed(seeds[b])
            o = DS.transform_train(_self(crop, md, sr, rot), data)
        im = o["index_map"].numpy()                # an int64 array until the reference's ToTensor ends in .float(): integers in float32
        assert tuple(im.shape) == (1, th, tw) and np.array_equal(im, im.astype(np.int32))
        assert np.array_equal(o["radar_depth_filtered"].numpy(), o["inputs"].numpy()[3:4])
        outs.append((o["inputs"].numpy(), o["labels"].numpy(), im.astype(np.int32)))
    want = [np.stack([o[k] for o in outs]) for k in range(3)]
    for k, what in enumerate(("inputs", "labels", "index_map")):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s: restatement != reference (%s)" % (name, what)
    for b in range(B):                                                              # the radar map agrees with the points
        q = pts[b]
        assert all(radar[b][imaps[b] == i].tolist() in ([], [int(round(q["rdep"][i] * 256))]) for i in range(len(q["rdep"])))
        assert ((radar[b] != 0) == (imaps[b] >= 0)).all()
    out = {"image": img, "lidar": lidar, "radar": radar, "crop": np.array(crop), "max_depth": np.array(md, np.float64),
           "n_radar": np.array([c[0] for c in counts]), "n_lidar": np.array([c[1] for c in counts]),
           "inputs": want[0], "labels": want[1], "index_map_out": want[2].astype(np.int32),
           "margin": np.array(min(q["margin"] for q in pts)),
           "filter_changes": np.array([(got[0][b, 3] != plain[0][b, 3]).sum() for b in range(B)])}
    unclamped = (F.stage_val(img, lidar, radar, imaps, valids, crop, np.inf, filtered=False) if mode == "val" else
                 F.stage_train(img, lidar, radar, p, imaps, valids, crop, np.inf, filtered=False))[0][:, 3]
    out["clamped"] = np.array(int((unclamped > md).sum()))
    for b, q in enumerate(pts):
        for k in ("rxy", "rdep", "lxy", "ldep", "labels", "valid", "topk", "imap"):
            out["f%d_%s" % (b, k)] = q[k]
    if p is not None:
        out["seeds"], out["draw"] = np.array(seeds), np.array([sr[0], sr[1], rot])
        for k, v in p.items():
            out["p_" + k] = v
        fill = []
        for b in range(B):                                                          # rotation fill inside the crop, point 0 invalid
            ok = R.rotate_indices(R.rotation_coeffs(float(p["angle"][b]), H0, W0), H0, W0)[2]
            s = float(p["scale"][b])
            okc = R.resize_nearest(ok, int(H0 * s), int(W0 * s))[int(p["h_start"][b]):int(p["h_start"][b]) + th, int(p["w_start"][b]):int(p["w_start"][b]) + tw]
            fill.append(int((~okc).sum()) if not pts[b]["valid"][0] else 0)
        out["fill_with_invalid0"] = np.array(fill)
    print(name, "ok: B=%d margin %.2e filter changes %s clamped %d" % (B, out["margin"], out["filter_changes"].tolist(), out["clamped"]))
    return {name + "_" + k: v for k, v in out.items()}


FILTER_CASES = [("f2x3", 2, 3, (24, 40), {}), ("f5x3", 5, 3, (48, 80), {}), ("f37x70", 37, 70, (48, 80), dict(duplicate=True)),
                ("f64x257", 64, 257, (48, 80), {}), ("f130x3000", 130, 3000, (900, 1600), {})]


def main():
    rng = np.random.RandomState(20261019)
    out, counts = {}, np.zeros(3, np.int64)
    for name, nr, nl, shape, kw in FILTER_CASES:
        accept = (lambda lb: (lb == 2).any()) if name == "f5x3" else (lambda lb: len(set(lb.tolist())) == 3) if nr >= 130 else (lambda lb: True)
        q = checked_points(rng, nr, nl, shape, accept, **kw)
        if kw.get("duplicate"):
            assert (q["rxy"][0].astype(np.int32) == q["rxy"][1].astype(np.int32)).all() and (q["imap"] == 0).sum() == 0 and (q["imap"] == 1).sum() == 1
        for k in ("rxy", "rdep", "lxy", "ldep", "labels", "valid", "topk"):
            out["%s_%s" % (name, k)] = q[k]
        ys, xs = np.nonzero(q["imap"] >= 0)                                         # the map itself, sparse: (row, column, index)
        out[name + "_imap_sparse"] = np.stack((ys, xs, q["imap"][ys, xs]), 1).astype(np.int32)
        out[name + "_shape"], out[name + "_margin"] = np.array(shape), np.array(q["margin"])
        counts += np.bincount(q["labels"], minlength=3)
        print(name, "ok: labels 0/1/2 = %s margin %.2e" % (np.bincount(q["labels"], minlength=3).tolist(), q["margin"]))
    assert (counts > 0).all(), counts
    out["label_counts"] = counts
    out.update(staged_case(rng, "val1", "val", (31, 45), (24, 40), 50.0, [(21, 60), (9, 40)]))
    out.update(staged_case(rng, "val2", "val", (24, 40), (24, 40), np.inf, [(12, 30)]))
    out.update(staged_case(rng, "tr1", "train", (48, 80), (40, 64), 60.0, [(40, 120), (25, 90), (33, 64)], seeds=[3, 4, 8]))
    out.update(staged_case(rng, "tr2", "train", (24, 40), (24, 40), np.inf, [(16, 50), (18, 45)], seeds=[21, 22], sr=(1.0, 1.0), rot=5.0,
                           invalid0=True))
    assert (out["tr2_fill_with_invalid0"] > 0).any(), "no rotation fill inside a crop whose point 0 is invalid"
    assert out["val1_clamped"] > 0 and out["tr1_clamped"] > 0, "max_depth clamps nothing"
    assert len(set(out["tr1_p_flip"].tolist()) | set(out["tr2_p_flip"].tolist())) == 2, "both flip values"
    assert min(float(v) for k, v in out.items() if k.endswith("_margin")) >= MARGIN
    path = os.path.join(HERE, "radar_filter.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

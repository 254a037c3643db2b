"""Golden vectors for training-input staging (rd_stage_frames_train), produced from the reference checkout.

The vectors come from the reference's OWN ``nuscenes_dataset_torch.transform_train`` (dataset/nuscenes_dataset_torch_new.py:237-412),
called unbound on seeded frames with a namespace standing in for ``self`` and ``np.random.seed`` set per frame, exactly as
make_golden_staging.py calls ``transform_val``.  The module is imported with empty stand-ins for the packages this environment lacks.
``scipy.misc.imresize`` left scipy in 1.3; the stand-in below restates scipy 1.2's on Pillow (``toimage`` -> ``bytescale`` for a float
RGB array, mode 'F' for a depth map, a float size scales ``im.size`` and truncates, ``Image.resize``).  Rotation, Pillow's two
resamplers and Pillow's ImageEnhance are the installed libraries' own code.

For every case the numpy-only restatement tests/staging_train_ref.py is asserted to reproduce the reference's output bit for bit, fed
with the parameters its ``draw_params`` replays from the same seed: that is what makes both the vectors and the restatement
trustworthy on a machine that has neither library.  Two cases force their parameters (scale 1, angle 0, unit jitter factors) by
scripting ``np.random.uniform`` for that call.
    python tests/golden/make_golden_staging_train.py"""
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
import staging_train_ref as R  # noqa: E402


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


def reference_transform_train(image, lidar_i16, radar_i16, crop, max_depth, modality, scale_range, rotation, seed=None, script=None):
    self = types.SimpleNamespace(transform_mode="sparse-to-dense", sparsifier="radar", modality=modality, max_depth=max_depth,
                                 t_cfg=types.SimpleNamespace(crop_size_train=tuple(crop), crop_size_val=tuple(crop),
                                                             scale_factor_train=list(scale_range), rotation_factor=rotation))
    data = {"image": image, "lidar_depth": lidar_i16 / 256., "radar_depth": radar_i16 / 256.}
    real = np.random.uniform
    if script is not None:
        it = iter(script)
        np.random.uniform = lambda lo, hi: next(it)
    else:
        np.random.seed(seed)
    try:
        out = ref_dataset.nuscenes_dataset_torch.transform_train(self, data)
    finally:
        np.random.uniform = real
    return out["inputs"].numpy(), out["labels"].numpy()


def frames(rng, B, H0, W0, lo=0, hi=256):
    img = rng.randint(lo, hi, size=(B, H0, W0, 3)).astype(np.uint8)
    lidar = (rng.rand(B, H0, W0) * 120.0 * 256 * (rng.rand(B, H0, W0) < 0.3)).astype(np.int16)
    radar = (rng.rand(B, H0, W0) * 120.0 * 256 * (rng.rand(B, H0, W0) < 0.2)).astype(np.int16)
    return img, lidar, radar


IDENTITY = dict(scale=[1.0], angle=[0.0], flip=[False], h_start=[0], w_start=[0], factors=[[1.0, 1.0, 1.0]])


def main():
    rng = np.random.RandomState(20261018)
    cases, out = {}, {}
    # six jitter orders and both flip values: seeds picked by replaying the draws
    first = {}                                   # (order, flip) -> first seed that draws it
    for seed in range(400):
        p = R.draw_params(1, (24, 40), rng=np.random.RandomState(seed))
        first.setdefault((tuple(int(v) for v in p["order"][0]), bool(p["flip"][0])), seed)
    orders = sorted({k[0] for k in first})
    assert len(orders) == 6
    seeds = [first[(o, i % 2 == 0)] for i, o in enumerate(orders)]
    cases["six"] = dict(fr=frames(rng, 6, 24, 40), crop=(24, 40), md=80.0, seeds=seeds, sr=(1.0, 1.5), rot=5.0)
    cases["rag1"] = dict(fr=frames(rng, 2, 19, 33), crop=(16, 28), md=np.inf, seeds=[11, 12], sr=(1.0, 1.5), rot=5.0)
    cases["rag2"] = dict(fr=frames(rng, 2, 31, 45), crop=(24, 40), md=50.0, seeds=[21, 22], sr=(1.0, 1.5), rot=5.0)
    cases["range"] = dict(fr=frames(rng, 1, 24, 40, 30, 201), crop=(24, 40), md=np.inf, seeds=[31], sr=(1.0, 1.5), rot=0.0)
    const = frames(rng, 1, 24, 40)
    const[0][:] = 77
    cases["const"] = dict(fr=const, crop=(24, 40), md=np.inf, seeds=[41], sr=(1.0, 1.5), rot=0.0)
    cases["ident"] = dict(fr=frames(rng, 1, 24, 40), crop=(24, 40), md=60.0, forced=True)
    z = np.zeros((1, 16, 16), np.int16)
    cases["bytes"] = dict(fr=(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3), z, z), crop=(16, 16), md=np.inf, forced=True)
    for name, c in cases.items():
        img, lidar, radar = c["fr"]
        B, crop, md = img.shape[0], c["crop"], c["md"]
        if c.get("forced"):
            p = {k: np.array(v) for k, v in IDENTITY.items()}
            p["order"] = np.array([[0, 1, 2]])
            real_shuffle = np.random.shuffle
            np.random.shuffle = lambda x: None
            try:
                outs = [reference_transform_train(img[0], lidar[0], radar[0], crop, md, "rgbd", (1.0, 1.0), 0.0,
                                                  script=[1.0, 0.0, 0.75, 0.0, 0.0, 1.0, 1.0, 1.0])]
            finally:
                np.random.shuffle = real_shuffle
        else:
            ps = [R.draw_params(1, crop, c["sr"], c["rot"], rng=np.random.RandomState(s)) for s in c["seeds"]]
            p = {k: np.concatenate([q[k] for q in ps]) for k in ps[0]}
            outs = [reference_transform_train(img[b], lidar[b], radar[b], crop, md, "rgbd", c["sr"], c["rot"], seed=c["seeds"][b]) for b in range(B)]
            rgb_only = reference_transform_train(img[0], lidar[0], radar[0], crop, md, "rgb", c["sr"], c["rot"], seed=c["seeds"][0])
            assert np.array_equal(rgb_only[0], outs[0][0][:3]) and np.array_equal(rgb_only[1], outs[0][1])
            out[name + "_seeds"] = np.array(c["seeds"])
            out[name + "_draw"] = np.array([c["sr"][0], c["sr"][1], c["rot"]])
        want_in, want_lb = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
        got_in, got_lb = R.transform_train_batch(img, lidar, radar, p, crop, md)          # the restatement, bit for bit
        assert got_in.dtype == want_in.dtype == np.float32 and got_in.shape == want_in.shape, name
        assert np.array_equal(got_in, want_in) and np.array_equal(got_lb, want_lb), (name, int((got_in != want_in).sum()), int((got_lb != want_lb).sum()))
        if np.isfinite(md):
            assert (R.transform_train_batch(img, lidar, radar, p, crop)[0][:, 3] > md).any(), name + ": max_depth masks nothing"
        out[name + "_image"], out[name + "_lidar"], out[name + "_radar"] = img, lidar, radar
        out[name + "_crop"], out[name + "_max_depth"] = np.array(crop), np.array(md, dtype=np.float64)
        for k, v in p.items():
            out[name + "_p_" + k] = v
        out[name + "_inputs"], out[name + "_labels"] = want_in, want_lb
        print(name, "ok: B=%d scale %s angle %s flip %s order %s" % (B, np.round(p["scale"], 3), np.round(p["angle"], 2), p["flip"].astype(int), p["order"].tolist()))
    six = out["six_p_order"]
    assert len({tuple(r) for r in six.tolist()}) == 6 and len(set(out["six_p_flip"].tolist())) == 2
    path = os.path.join(HERE, "staging_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

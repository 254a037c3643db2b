"""Golden vectors for the lidar sparsifiers (rd_lidar_radar_sparsify, rd_uniform_sparsify), produced from the reference checkout.

Every vector comes from the reference's OWN ``LidarRadarSampling.dense_to_sparse`` / ``UniformSampling.dense_to_sparse``
(dataset/dense_to_sparse.py) through its ``get_sparse_depth`` (dataset/nuscenes_dataset_torch_new.py:200-216), and the staged cases from
its ``transform_val`` / ``transform_train`` with ``sparsifier="lidar_radar"`` / ``"uniform"``, called unbound on seeded synthetic frames
with a namespace standing in for ``self``.  The reference is imported the way make_golden_radar_filter.py imports it (that module is
imported for its stand-ins).

lidar_radar: the reference's argsort of float distances is not stable, so its output is defined only where no radar pixel has its
second and third nearest lidar pixels at the same distance.  Every radar pixel of a fixture frame is redrawn until that holds (a staged
frame: the whole frame), ``n_tied`` is stored per frame and is 0 everywhere, and the numpy restatement tests/lidar_sparsifier_ref.py
(stable sort on (d^2, index)) is asserted to reproduce the reference bit for bit on every case.
uniform: the draws are stored.  For the plain cases they are handed to the reference's code in place of its ``np.random.uniform`` call
(one of them is set exactly to ``prob``); for the staged cases they are what numpy's seeded global generator gives the reference, and the
recipe that reproduces them is recorded: ``RandomState(seed).uniform(0, 1, (1, th, tw))`` (validation), ``draw_params(1, rng=rs)``
followed by ``rs.uniform(0, 1, (1, ch, cw))`` per frame (training: the reference worker's order).
    python tests/golden/make_golden_lidar_sparsifiers.py"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_radar_filter as M  # noqa: E402  (the reference's import with the stand-ins for the packages it lacks)

import lidar_sparsifier_ref as S  # noqa: E402
import staging_train_ref as R  # noqa: E402

DS = M.DS
ref_d2s = importlib.import_module("dataset.dense_to_sparse")


def _self(sparsifier, func, crop, scale_range=(1.0, 1.5), rotation=5.0):
    ns = M._self(crop, func.max_depth, scale_range, rotation)
    ns.sparsifier, ns.sparsifier_func = sparsifier, func
    ns.get_sparse_depth = types.MethodType(DS.get_sparse_depth, ns)
    return ns


def reference_lidar_radar(lidar, radar):
    """The reference on one frame ([h,w] float32 arrays): (mask of dense_to_sparse, sparse depth of get_sparse_depth)."""
    func = ref_d2s.LidarRadarSampling(100, 80.0)                                   # both arguments are unused by the reference
    lt, rt = torch.from_numpy(lidar.copy())[None], torch.from_numpy(radar.copy())[None]
    mask = func.dense_to_sparse(lt, rt)
    sparse = _self("lidar_radar", func, (1, 1)).get_sparse_depth(lt, rt)
    return np.asarray(mask).astype(bool), sparse.numpy()[0]


class _Draws:
    """np.random.uniform replaced by the stored draws for the duration of one reference call."""

    def __init__(self, draws):
        self.draws, self.calls = draws, 0

    def __enter__(self):
        self.saved = np.random.uniform
        np.random.uniform = self
        return self

    def __exit__(self, *a):
        np.random.uniform = self.saved

    def __call__(self, lo, hi, shape):
        assert (lo, hi) == (0, 1) and tuple(shape) == self.draws.shape
        self.calls += 1
        return self.draws


def reference_uniform(depth, num_samples, max_depth, draws):
    """The reference on one frame (depth [1,h,w] float32, draws [1,h,w] float64): (mask, sparse depth)."""
    func = ref_d2s.UniformSampling(num_samples, max_depth)
    dt = torch.from_numpy(depth.copy())
    with _Draws(draws):
        mask = func.dense_to_sparse(dt)
    with _Draws(draws):
        sparse = _self("uniform", func, (1, 1)).get_sparse_depth(dt)
    return np.asarray(mask).astype(bool), sparse.numpy()


# ------------------------------------------------------------------------------------------------ lidar_radar frames
def tie_free_pixel(rng, lidar, taken, near=None, reach=4, accept=lambda y, x: True):
    """A pixel for a radar return whose second and third nearest lidar pixels are not equidistant (anywhere, or within ``reach`` of ``near``)."""
    h, w = lidar.shape
    for _ in range(2000):
        if near is None:
            y, x = int(rng.randint(0, h)), int(rng.randint(0, w))
        else:
            y, x = int(near[0] + rng.randint(-reach, reach + 1)), int(near[1] + rng.randint(-reach, reach + 1))
        if not (0 <= y < h and 0 <= x < w) or (y, x) in taken or not accept(y, x):
            continue
        one = np.zeros_like(lidar)
        one[y, x] = 1.0
        if S.n_tied(lidar, one) == 0:
            taken.add((y, x))
            return y, x
    raise AssertionError("no tie-free pixel")


def lidar_map(rng, shape, n, corners=False):
    h, w = shape
    lidar = np.zeros(shape, np.float32)
    flat = rng.choice(np.arange(1, h * w - 1), n - (2 if corners else 0), replace=False) if n else np.zeros(0, np.int64)
    lidar.reshape(-1)[flat] = rng.uniform(2, 120, len(flat)).astype(np.float32)
    if corners:
        lidar[0, 0], lidar[h - 1, w - 1] = np.float32(17.25), np.float32(93.5)
    assert (lidar > 0).sum() == n
    return lidar


def lr_frame(rng, shape, n_lidar, n_radar, special=False):
    """One frame.  special: lidar pixels in both corners with a radar return next to each, a radar return on a lidar pixel, two radar
    returns that choose one lidar pixel, radar values above any max_depth."""
    lidar = lidar_map(rng, shape, n_lidar, corners=special)
    h, w = shape
    radar, taken = np.zeros(shape, np.float32), set()
    pix = []
    if special:
        def chooses(cy, cx):
            def accept(y, x):
                one = np.zeros_like(lidar)
                one[y, x] = 1.0
                return S.lidar_radar_mask(lidar, one)[cy, cx]
            return accept
        pix.append(tie_free_pixel(rng, lidar, taken, near=(0, 0), accept=chooses(0, 0)))
        pix.append(tie_free_pixel(rng, lidar, taken, near=(h - 1, w - 1), accept=chooses(h - 1, w - 1)))
        pix.append(tie_free_pixel(rng, lidar, taken, accept=lambda y, x: lidar[y, x] > 0))            # distance 0
        first = tie_free_pixel(rng, lidar, taken)
        one = np.zeros_like(lidar)
        one[first] = 1.0
        chosen = S.lidar_radar_mask(lidar, one)

        def shares(y, x):
            two = np.zeros_like(lidar)
            two[y, x] = 1.0
            return (S.lidar_radar_mask(lidar, two) & chosen).any()
        pix += [first, tie_free_pixel(rng, lidar, taken, near=first, accept=shares)]
    while len(pix) < n_radar:
        pix.append(tie_free_pixel(rng, lidar, taken))
    for k, (y, x) in enumerate(pix[:n_radar]):
        radar[y, x] = np.float32(300.0 + k) if special and k % 3 == 0 else np.float32(rng.uniform(2, 100))
    return lidar, radar


def lr_case(name, lidar, radar):
    tied = S.n_tied(lidar, radar)
    assert tied == 0, (name, tied)
    mask, sparse = reference_lidar_radar(lidar, radar)
    want = S.lidar_radar_sparse(lidar, radar)
    assert sparse.dtype == np.float32 and np.array_equal(sparse, want), name + ": restatement != reference (sparse depth)"
    assert np.array_equal(mask, S.lidar_radar_mask(lidar, radar)), name + ": restatement != reference (mask)"
    print("%-10s %dx%d: %3d lidar %2d radar -> %3d chosen" % ((name,) + lidar.shape + ((lidar > 0).sum(), (radar > 0).sum(), mask.sum())))
    return {name + "_lidar": lidar, name + "_radar": radar, name + "_sparse": sparse, name + "_n_tied": np.array(tied)}


# ------------------------------------------------------------------------------------------------ uniform frames
def uniform_case(rng, name, shape, num_samples, max_depth, density=0.3, edge=False):
    h, w = shape
    depth = (rng.uniform(1, 120, (1, h, w)) * (rng.rand(1, h, w) < density)).astype(np.float32)
    draws = rng.uniform(0, 1, (1, h, w))
    extra = {}
    if edge:
        at, above = np.float32(max_depth), np.nextafter(np.float32(max_depth), np.float32(np.inf))
        assert float(at) > max_depth, "the fp32 rounding of max_depth must lie above it for the case to mean anything"
        depth[0, 3, 5], depth[0, 4, 6] = at, above
        draws[0, 3, 5] = draws[0, 4, 6] = 0.0                                      # kept if and only if they count as candidates
        keep = (depth > 0) & (depth <= np.float32(max_depth))
        prob = float(num_samples) / int(keep.sum())
        ys, xs = np.nonzero(keep[0])
        (y0, x0), (y1, x1) = [(int(ys[k]), int(xs[k])) for k in (len(ys) // 3, 2 * len(ys) // 3)]
        draws[0, y0, x0], draws[0, y1, x1] = prob, np.nextafter(prob, 0.0)         # a draw equal to prob is not kept, the one below is
        extra = {name + "_at": np.array([3, 5]), name + "_above": np.array([4, 6]), name + "_equal": np.array([y0, x0]),
                 name + "_below": np.array([y1, x1]), name + "_prob": np.array(prob)}
    mask, sparse = reference_uniform(depth, num_samples, max_depth, draws)
    want = S.uniform_sparse(depth, num_samples, max_depth, draws)
    assert sparse.dtype == np.float32 and np.array_equal(sparse, want), name + ": restatement != reference (sparse depth)"
    assert np.array_equal(mask, S.uniform_mask(depth, num_samples, max_depth, draws)), name + ": restatement != reference (mask)"
    if edge:
        assert sparse[0, 3, 5] == at and sparse[0, 4, 6] == 0 and sparse[0, y0, x0] == 0 and sparse[0, y1, x1] == depth[0, y1, x1]
    print("%-10s ns=%d md=%s: %d candidates -> %d kept" % (name, num_samples, max_depth, (depth > 0).sum(), mask.sum()))
    out = {name + "_depth": depth, name + "_draws": draws, name + "_sparse": sparse, name + "_num_samples": np.array(num_samples),
           name + "_max_depth": np.array(max_depth, np.float64)}
    out.update(extra)
    return out


# ------------------------------------------------------------------------------------------------ staged cases
def sparse_frames(rng, B, H0, W0, n_lidar, n_radar):
    img = rng.randint(0, 256, size=(B, H0, W0, 3)).astype(np.uint8)
    lidar, radar = np.zeros((B, H0, W0), np.int16), np.zeros((B, H0, W0), np.int16)
    for b in range(B):
        lidar[b].reshape(-1)[rng.choice(H0 * W0, n_lidar, replace=False)] = rng.randint(2 * 256, 120 * 256, n_lidar)
        radar[b].reshape(-1)[rng.choice(H0 * W0, n_radar, replace=False)] = rng.randint(2 * 256, 120 * 256, n_radar)
    return img, lidar, radar


def staged_case(rng, name, mode, sparsifier, shape, crop, seeds, num_samples=0, max_depth=np.inf, sr=(1.0, 1.5), rot=5.0, n_lidar=150, n_radar=14):
    """One staged batch, frame by frame: a frame (and, for lidar_radar in training, its seed) is redrawn until it has no tie and the
    sparsifier changes the plane."""
    H0, W0 = shape
    th, tw = crop
    func = (ref_d2s.LidarRadarSampling if sparsifier == "lidar_radar" else ref_d2s.UniformSampling)(num_samples, max_depth)
    seeds, frames, params, draws, outs, tied = list(seeds), [], [], [], [], []
    for b in range(len(seeds)):
        for attempt in range(400):
            img, lidar, radar = sparse_frames(rng, 1, H0, W0, n_lidar, n_radar)
            rs = np.random.RandomState(seeds[b])
            p = R.draw_params(1, crop, sr, rot, rng=rs) if mode == "train" else None
            u = rs.uniform(0, 1, (1, th, tw)) if sparsifier == "uniform" else None               # the recorded recipe
            got = S.staged(mode, img, lidar, radar, p, crop, sparsifier, num_samples, max_depth, None if u is None else u[None])
            t = S.n_tied(got[1][0, 0], got[2][0, 0]) if sparsifier == "lidar_radar" else 0
            if t == 0 and (got[0][0, 3] != got[2][0, 0]).any() and (got[0][0, 3] != 0).any():
                break
            if mode == "train":
                seeds[b] += 1000
        else:
            raise AssertionError(name + ": no acceptable frame")
        data = {"image": img[0], "lidar_depth": lidar[0] / 256., "radar_depth": radar[0] / 256.}
        np.random.seed(seeds[b])
        o = (DS.transform_val if mode == "val" else DS.transform_train)(_self(sparsifier, func, crop, sr, rot), data)
        ref_in, ref_lb = o["inputs"].numpy(), o["labels"].numpy()
        assert np.array_equal(ref_in, got[0][0]) and np.array_equal(ref_lb, got[1][0]), name + ": restatement != reference"
        assert np.array_equal(o["radar_depth"].numpy(), got[2][0]), name + ": the radar map the sparsifier saw"
        frames.append((img[0], lidar[0], radar[0]))
        params.append(p)
        draws.append(u)
        outs.append((ref_in, ref_lb, got[2][0]))
        tied.append(t)
    out = {"image": np.stack([f[0] for f in frames]), "lidar": np.stack([f[1] for f in frames]), "radar": np.stack([f[2] for f in frames]),
           "crop": np.array(crop), "inputs": np.stack([o[0] for o in outs]), "labels": np.stack([o[1] for o in outs]),
           "plane_before": np.stack([o[2] for o in outs]), "n_tied": np.array(tied), "seeds": np.array(seeds),
           "num_samples": np.array(num_samples), "max_depth": np.array(max_depth, np.float64), "draw": np.array([sr[0], sr[1], rot])}
    if mode == "train":
        for k in params[0]:
            out["p_" + k] = np.concatenate([q[k] for q in params])
    if sparsifier == "uniform":
        out["draws"] = np.stack(draws)
    print("%-10s %s %s: B=%d, pixels in the plane %s" % (name, mode, sparsifier, len(seeds), [(o[0][3] != 0).sum() for o in outs]))
    return {name + "_" + k: v for k, v in out.items()}


LR_COUNTS = [("lr_l0", 0), ("lr_l1", 1), ("lr_l2", 2), ("lr_l63", 63), ("lr_l64", 64), ("lr_l65", 65)]


def main():
    rng = np.random.RandomState(20261019)
    out, names = {}, []
    for name, n in LR_COUNTS:                                                                     # 33 x 47
        out.update(lr_case(name, *lr_frame(rng, (33, 47), n, 12)))
        names.append(name)
    lidar, _ = lr_frame(rng, (33, 47), 120, 0)
    out.update(lr_case("lr_norad", lidar, np.zeros((33, 47), np.float32)))
    out.update(lr_case("lr_special", *lr_frame(rng, (33, 47), 120, 12, special=True)))
    out.update(lr_case("lr_l300", *lr_frame(rng, (45, 80), 300, 16)))                             # 45 x 80
    out.update(lr_case("lr_special2", *lr_frame(rng, (45, 80), 290, 14, special=True)))
    names += ["lr_norad", "lr_special", "lr_l300", "lr_special2"]
    out["lr_names"] = np.array(names)

    unames = []
    for name, ns, md, kw in (("un_empty", 100, np.inf, dict(density=0.0)), ("un_ns0", 0, np.inf, {}), ("un_all", 10 ** 6, 80.0, {}),
                             ("un_inf", 100, np.inf, {}), ("un_md", 150, 79.9, dict(edge=True)), ("un_big", 400, 60.0, dict(density=0.6))):
        out.update(uniform_case(rng, name, (45, 80) if name == "un_big" else (33, 47), ns, md, **kw))
        unames.append(name)
    out["un_names"] = np.array(unames)

    out.update(staged_case(rng, "val_lr", "val", "lidar_radar", (48, 80), (40, 64), [1, 2]))
    out.update(staged_case(rng, "tr_lr", "train", "lidar_radar", (48, 80), (40, 64), [3, 4]))
    out.update(staged_case(rng, "val_un", "val", "uniform", (31, 45), (24, 40), [5, 6], num_samples=30, max_depth=60.0))
    out.update(staged_case(rng, "tr_un", "train", "uniform", (48, 80), (40, 64), [7, 8], num_samples=50, max_depth=np.inf))
    out["staged_names"] = np.array(["val_lr", "tr_lr", "val_un", "tr_un"])
    assert all(int(np.sum(v)) == 0 for k, v in out.items() if k.endswith("_n_tied"))
    path = os.path.join(HERE, "lidar_sparsifiers.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Training-input staging (rd_stage_frames_train / dataset.stage_train_batch): the reference's transform_train on the GPU.

tests/golden/staging_train.npz holds frames, seeds, drawn parameters and the outputs of the reference's own transform_train
(tests/golden/make_golden_staging_train.py, which also asserts that tests/staging_train_ref.py -- the numpy-only restatement used
here -- reproduces every one of them bit for bit).  Everything is integer / table / correctly rounded arithmetic, so every comparison
is np.array_equal."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import staging_train_ref as R  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "staging_train.npz"))
CASES = ["six", "rag1", "rag2", "range", "const", "ident", "bytes"]
PKEYS = ("scale", "angle", "flip", "h_start", "w_start", "factors", "order")


def _case(name):
    p = {k: G["%s_p_%s" % (name, k)] for k in PKEYS}
    return (G[name + "_image"], G[name + "_lidar"], G[name + "_radar"], p, tuple(int(v) for v in G[name + "_crop"]),
            float(G[name + "_max_depth"]), G[name + "_inputs"], G[name + "_labels"])


def _frames(seed, B, H0, W0):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(B, H0, W0, 3)).astype(np.uint8)
    lidar = (rng.rand(B, H0, W0) * 100 * 256 * (rng.rand(B, H0, W0) < 0.3)).astype(np.int16)
    radar = (rng.rand(B, H0, W0) * 100 * 256 * (rng.rand(B, H0, W0) < 0.2)).astype(np.int16)
    return img, lidar, radar


@functools.lru_cache(maxsize=None)
def _random_case(B, H0, W0, crop, md):
    """Seeded frames, B different parameter sets and the restatement's outputs; computed once and shared."""
    from radar_depth_amd.dataset import draw_train_params
    img, lidar, radar = _frames(B * 1000 + H0, B, H0, W0)
    p = draw_train_params(B, crop, rng=np.random.RandomState(B + W0))
    want = R.transform_train_batch(img, lidar, radar, p, crop, md)
    for a in (img, lidar, radar) + want:
        a.setflags(write=False)
    return img, lidar, radar, p, want


def _gpu(*arrays):
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


# ------------------------------------------------------------------------------------------------ host
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_vectors(name):
    img, lidar, radar, p, crop, md, want_in, want_lb = _case(name)
    got_in, got_lb = R.transform_train_batch(img, lidar, radar, p, crop, md)
    assert got_in.dtype == np.float32 and got_lb.dtype == np.float32
    assert np.array_equal(got_in, want_in) and np.array_equal(got_lb, want_lb)
    rgb_in, rgb_lb = R.transform_train_batch(img, lidar, None, p, crop, md, "rgb")
    assert np.array_equal(rgb_in, want_in[:, :3]) and np.array_equal(rgb_lb, want_lb)


def test_golden_cases_cover_what_they_claim():
    assert len({tuple(r) for r in G["six_p_order"].tolist()}) == 6 and set(G["six_p_flip"].tolist()) == {False, True}
    assert G["range_image"].min() >= 30 and G["range_image"].max() <= 200 and float(G["range_p_angle"][0]) == 0.0
    assert G["const_image"].min() == G["const_image"].max()
    assert float(G["ident_p_scale"][0]) == 1.0 and np.array_equal(G["ident_p_factors"], np.ones((1, 3)))
    assert sorted(set(G["bytes_image"].reshape(-1).tolist())) == list(range(256))
    assert np.array_equal(np.sort(G["bytes_inputs"][0, 0].reshape(-1)), (np.arange(256) / 255.).astype(np.float32))
    for name in ("six", "rag2", "ident"):       # a finite max_depth that does mask radar points
        img, lidar, radar, p, crop, md, want_in, _ = _case(name)
        unclamped = R.transform_train_batch(img, lidar, radar, p, crop)[0][:, 3]
        assert np.isfinite(md) and (unclamped > md).any() and want_in[:, 3].max() <= md


@pytest.mark.parametrize("name", ["six", "rag1", "rag2", "range", "const"])
def test_draw_train_params_reproduces_the_reference_draws(name):
    from radar_depth_amd.dataset import draw_train_params
    lo, hi, rot = (float(v) for v in G[name + "_draw"])
    crop = tuple(int(v) for v in G[name + "_crop"])
    for i, seed in enumerate(G[name + "_seeds"]):
        p = draw_train_params(1, crop, (lo, hi), rot, rng=np.random.RandomState(int(seed)))
        for k in PKEYS:
            assert np.array_equal(p[k][0], G["%s_p_%s" % (name, k)][i]), (name, i, k)
    # the default generator is numpy's global one, as in the reference
    np.random.seed(int(G[name + "_seeds"][0]))
    p = draw_train_params(1, crop, (lo, hi), rot)
    assert all(np.array_equal(p[k][0], G["%s_p_%s" % (name, k)][0]) for k in PKEYS)


def test_host_tables_match_the_restatement():
    from radar_depth_amd.dataset import staging as S
    for a in np.random.RandomState(3).uniform(-5, 5, 200).tolist() + [0.0, 5.0, -5.0, 45.0, 90.0, -135.0, 400.0]:
        assert S.cos_sin_degrees(a) == (R.cosdg(a), R.sindg(a))
        assert S.rotation_coefficients(a, 450, 800) == R.rotation_coeffs(a, 450, 800)
    for n_in, n_out in [(450, 450), (450, 451), (450, 674), (800, 1199), (19, 20), (24, 36), (7, 21)]:
        xmin, k = R.bilinear_coeffs(n_in, n_out)
        t = S.bilinear_table(n_in, n_out)
        assert t.dtype == np.int32 and np.array_equal(t[:, 0], xmin) and np.array_equal(t[:, 1:3], k[:, :2]) and not k[:, 2:].any()
        assert np.array_equal(S.nearest_table(n_in, n_out), R.nearest_table(n_in, n_out))
    # the batched crop-window tables are slices of the per-frame ones
    H0, W0, crop = 57, 83, (40, 64)
    p = S.draw_train_params(9, crop, rng=np.random.RandomState(4))
    near_y, near_x, bil_y, bil_x = S.train_tables(p, H0, W0, crop)
    for i in range(9):
        oh, ow, hs, ws = int(H0 * p["scale"][i]), int(W0 * p["scale"][i]), int(p["h_start"][i]), int(p["w_start"][i])
        assert np.array_equal(near_y[i], R.nearest_table(H0, oh)[hs:hs + crop[0]]) and np.array_equal(near_x[i], R.nearest_table(W0, ow)[ws:ws + crop[1]])
        for tab, (xmin, k), st in ((bil_y[i], R.bilinear_coeffs(H0, oh), hs), (bil_x[i], R.bilinear_coeffs(W0, ow), ws)):
            assert np.array_equal(tab[:, 0], xmin[st:st + len(tab)]) and np.array_equal(tab[:, 1:3], k[st:st + len(tab), :2])
    recs = S.train_frame_records(p, H0, W0)
    assert recs.dtype.itemsize == 96 and all(tuple(recs["rot"][i]) == R.rotation_coeffs(p["angle"][i], H0, W0) for i in range(9))


def test_restatement_pieces_match_the_live_libraries():
    """Where Pillow and scipy import: rotation, both resamplers and the three enhancers against the installed code."""
    ndi = pytest.importorskip("scipy.ndimage")
    special = pytest.importorskip("scipy.special")
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    rng = np.random.RandomState(5)
    for a in rng.uniform(-5, 5, 300).tolist() + [0.0, 45.0, -90.0, 123.4]:
        assert (R.cosdg(a), R.sindg(a)) == (special.cosdg(a), special.sindg(a))
    for H, W, ang in [(24, 40, 3.3), (19, 33, -4.9), (90, 160, 2.17), (225, 400, -0.31)]:
        a = (rng.rand(H, W) * 255 + 1).astype(np.float32)
        assert np.array_equal(R.rotate0(a, R.rotation_coeffs(ang, H, W)), ndi.rotate(a, ang, reshape=False, prefilter=False, order=0))
    for H, W, s in [(24, 40, 1.37), (19, 33, 1.0), (17, 23, 1.4999), (24, 40, 1.013), (90, 160, 1.2345)]:
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        ow, oh = int(W * s), int(H * s)
        assert np.array_equal(R.resize_bilinear_u8(img, oh, ow), np.array(Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR)))
        d = rng.rand(H, W).astype(np.float32)
        assert np.array_equal(R.resize_nearest(d, oh, ow), np.array(Image.fromarray(d, "F").resize((ow, oh), Image.NEAREST)))
    img = rng.randint(0, 256, (24, 40, 3)).astype(np.uint8)
    pil = Image.fromarray(img)
    for f in (0.8123, 1.1877, 1.0, 0.93, 1.2):
        for which, enh in enumerate((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)):
            assert np.array_equal(R.enhance(img, which, f), np.array(enh(pil).enhance(f))), (which, f)


@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_new_symbols_are_exported(L):
    assert hasattr(L, "rd_stage_frames_train") and hasattr(L, "rd_stage_train_workspace_bytes")
    assert L.rd_stage_train_workspace_bytes(16, 450, 800, 450, 800) >= 16 * 450 * 800 * 4
    assert L.rd_stage_train_workspace_bytes(1, 8, 8, 9, 8) < 0 and b"crop" in L.rd_last_error()


def test_abi_rejects_bad_arguments_without_gpu(L):
    """Every rejection happens before anything reaches the GPU: the pointers below are host dummies that are never followed."""
    from radar_depth_amd.dataset.staging import train_frame_records
    buf = C.create_string_buffer(256)
    dummy = C.c_void_p((C.addressof(buf) + 15) & ~15)

    def good():
        return dict(scale=np.array([1.25]), angle=np.array([2.0]), flip=np.array([True]), h_start=np.array([3]), w_start=np.array([5]),
                    factors=np.array([[0.9, 1.1, 1.0]]), order=np.array([[2, 0, 1]]))

    def call(p, H0=24, W0=40, ch=24, cw=40, null=None, modality=0):
        ptrs = {k: dummy for k in ("rgb", "lidar", "radar", "near_y", "near_x", "bil_y", "bil_x", "work", "inputs", "labels")}
        records = train_frame_records(p, H0, W0)
        recs = C.c_void_p(records.ctypes.data)
        if null == "frames":
            recs = None
        elif null:
            ptrs[null] = None
        rc = L.rd_stage_frames_train(ptrs["rgb"], ptrs["lidar"], ptrs["radar"], 1, H0, W0, ch, cw, recs, ptrs["near_y"], ptrs["near_x"],
                                     ptrs["bil_y"], ptrs["bil_x"], ptrs["work"], C.c_float(80.0), modality, ptrs["inputs"], ptrs["labels"], None)
        return rc, L.rd_last_error()

    for null in ("rgb", "lidar", "radar", "frames", "near_y", "near_x", "bil_y", "bil_x", "work", "inputs", "labels"):
        rc, err = call(good(), null=null)
        assert rc < 0 and b"null" in err, null
    rc, err = call(good(), H0=23)
    assert rc < 0 and b"does not fit" in err
    rc, err = call(good(), W0=39)
    assert rc < 0 and b"does not fit" in err
    for key, value in (("h_start", 7), ("w_start", 11), ("h_start", -1)):     # int(24*1.25) = 30, int(40*1.25) = 50
        p = good()
        p[key][0] = value
        rc, err = call(p)
        assert rc < 0 and b"outside the resized" in err, (key, value)
    p = good()
    p["scale"][0] = 0.999
    rc, err = call(p)
    assert rc < 0 and b"scale" in err
    for order in ([0, 0, 2], [0, 1, 3], [1, 2, -1]):
        p = good()
        p["order"][0] = order
        rc, err = call(p)
        assert rc < 0 and b"permutation" in err, order
    rc, err = call(good(), modality=2)
    assert rc < 0 and b"modality" in err


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("modality", ["rgbd", "rgb"])
@pytest.mark.parametrize("name", CASES)
def test_hip_train_staging_matches_golden(name, modality):
    from radar_depth_amd.dataset import stage_train_batch
    img, lidar, radar, p, crop, md, want_in, want_lb = _case(name)
    gi, gl, gr = _gpu(img, lidar, None if modality == "rgb" else radar)
    x, y = stage_train_batch(gi, gl, gr, p, crop, md if np.isfinite(md) else -1.0, modality)
    x, y = x.cpu().numpy(), y.cpu().numpy()
    print("%s/%s: %d input and %d label elements differ" % (name, modality, (x != want_in[:, :x.shape[1]]).sum(), (y != want_lb).sum()))
    assert x.shape == (img.shape[0], 4 if modality == "rgbd" else 3) + crop and y.shape == (img.shape[0], 1) + crop
    assert np.array_equal(x, want_in[:, :x.shape[1]]) and np.array_equal(y, want_lb)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H0,W0,crop,md", [(16, 90, 160, (90, 160), 80.0),        # 16 different parameter sets
                                             (2, 455, 803, (450, 800), 80.0),       # the training geometry, frames larger than the crop
                                             (18, 19, 33, (16, 28), -1.0)])         # more frames than one launch chain takes, ragged rows
def test_hip_train_staging_vs_restatement(B, H0, W0, crop, md):
    from radar_depth_amd.dataset import stage_train_batch
    img, lidar, radar, p, (want_x, want_y) = _random_case(B, H0, W0, crop, md if md >= 0 else np.inf)
    x, y = stage_train_batch(*_gpu(img, lidar, radar), p, crop, md)
    x, y = x.cpu().numpy(), y.cpu().numpy()
    print("B=%d %dx%d: %d input and %d label elements differ" % (B, H0, W0, (x != want_x).sum(), (y != want_y).sum()))
    assert np.array_equal(x, want_x) and np.array_equal(y, want_y)
    if md >= 0:
        assert x[:, 3].max() <= md


@pytest.mark.gpu
def test_hip_train_staging_is_deterministic():
    from radar_depth_amd.dataset import prepare_train_params, stage_train_batch
    img, lidar, radar, p, _ = _random_case(16, 90, 160, (90, 160), 80.0)
    t = _gpu(img, lidar, radar)
    x1, y1 = stage_train_batch(*t, p, (90, 160), 80.0)
    x2, y2 = stage_train_batch(*t, p, (90, 160), 80.0)
    assert torch.equal(x1, x2) and torch.equal(y1, y2)
    x3, y3 = stage_train_batch(*t, prepare_train_params(p, 90, 160, (90, 160)), (90, 160), 80.0)      # tables built ahead of the call
    assert torch.equal(x1, x3) and torch.equal(y1, y3)


@pytest.mark.gpu
def test_hip_train_staging_identity_equals_val_staging():
    """scale 1, angle 0, no flip, unit factors, the crop window at CenterCrop's corner: the depth planes are stage_val_batch's; with
    0 and 255 both present the byte scaling is the identity and so are the RGB planes."""
    from radar_depth_amd.dataset import center_crop_params, stage_train_batch, stage_val_batch
    B, H0, W0, crop = 3, 31, 45, (24, 40)
    img, lidar, radar = _frames(7, B, H0, W0)
    img[:, 0, 0, 0], img[:, 0, 0, 1] = 0, 255
    i0, j0, _, _ = center_crop_params(H0, W0, crop)
    p = dict(scale=np.ones(B), angle=np.zeros(B), flip=np.zeros(B, bool), h_start=np.full(B, i0), w_start=np.full(B, j0),
             factors=np.ones((B, 3)), order=np.tile(np.array([2, 1, 0]), (B, 1)))
    t = _gpu(img, lidar, radar)
    x, y = stage_train_batch(*t, p, crop, 50.0)
    vx, vy = stage_val_batch(*t, crop, 50.0)
    assert torch.equal(x[:, 3], vx[:, 3]) and torch.equal(y, vy)
    assert torch.equal(x[:, :3], vx[:, :3])


@pytest.mark.gpu
def test_hip_train_staging_rejects_bad_crop():
    from radar_depth_amd._lib import RadarDepthHipError
    from radar_depth_amd.dataset import draw_train_params, stage_train_batch
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8).cuda()
    z = torch.zeros(1, 8, 8, dtype=torch.int16).cuda()
    with pytest.raises(RadarDepthHipError, match="does not fit"):
        stage_train_batch(img, z, z, draw_train_params(1, (9, 8), rng=np.random.RandomState(0)), (9, 8))
    p = draw_train_params(1, (8, 8), rng=np.random.RandomState(0))
    p["h_start"][0] = 5                                        # int(8 * 1.27) = 10 rows: 5 + 8 > 10
    with pytest.raises(RadarDepthHipError, match="outside the resized"):
        stage_train_batch(img, z, z, p, (8, 8))

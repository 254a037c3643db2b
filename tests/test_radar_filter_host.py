"""The radar_filtered sparsifier without a GPU: the numpy restatement (tests/radar_filter_ref.py) against the vectors of the reference's
own filter_radar_points / transform_val / transform_train (tests/golden/radar_filter.npz, tests/golden/make_golden_radar_filter.py),
the tie rule, every argument check of the C ABI (nothing is launched), and the Python surface."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radar_filter_ref as F  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "radar_filter.npz"))
FILTER_CASES = ["f2x3", "f5x3", "f37x70", "f64x257", "f130x3000"]
STAGED = [("val1", "val"), ("val2", "val"), ("tr1", "train"), ("tr2", "train")]
PKEYS = ("scale", "angle", "flip", "h_start", "w_start", "factors", "order")
MARGIN = 1e-6

# four lidar points at distance 3 from the radar point and one at 5 from it, a second radar point with two equal pairs
TIE = dict(rxy=np.array([[10.0, 10.0], [20.0, 14.0]]), rdep=np.array([30.0, 90.0]),
           lxy=np.array([[10.0, 13.0], [13.0, 10.0], [7.0, 10.0], [10.0, 7.0], [13.0, 14.0], [20.0, 10.0], [24.0, 14.0], [16.0, 14.0], [20.0, 18.0]]),
           ldep=np.array([31.0, 5.0, 5.0, 30.0, 12.0, 88.0, 20.0, 91.0, 89.0]))


def sparse_map(name):
    out = np.full(tuple(int(v) for v in G[name + "_shape"]), -1, np.int32)
    s = G[name + "_imap_sparse"]
    out[s[:, 0], s[:, 1]] = s[:, 2]
    return out


def staged(name):
    B = len(G[name + "_n_radar"])
    pts = [{k: G["%s_f%d_%s" % (name, b, k)] for k in ("rxy", "rdep", "lxy", "ldep", "labels", "valid", "topk", "imap")} for b in range(B)]
    p = {k: G["%s_p_%s" % (name, k)] for k in PKEYS} if name + "_p_scale" in G.files else None
    return (G[name + "_image"], G[name + "_lidar"], G[name + "_radar"], pts, p, tuple(int(v) for v in G[name + "_crop"]),
            float(G[name + "_max_depth"]), G[name + "_inputs"], G[name + "_labels"], G[name + "_index_map_out"])


# ------------------------------------------------------------------------------------------------ restatement and fixture
@pytest.mark.parametrize("name", FILTER_CASES)
def test_restatement_filter_matches_reference_vectors(name):
    labels, valid, topk, margin = F.filter_points(G[name + "_rxy"], G[name + "_rdep"], G[name + "_lxy"], G[name + "_ldep"], with_margin=True)
    assert np.array_equal(labels, G[name + "_labels"]) and np.array_equal(valid, G[name + "_valid"]) and np.array_equal(topk, G[name + "_topk"])
    assert labels.dtype == np.uint8 and topk.dtype == np.int32 and np.array_equal(valid, labels > 0)
    assert margin == float(G[name + "_margin"]) >= MARGIN
    assert np.array_equal(F.index_map(G[name + "_rxy"], tuple(G[name + "_shape"])), sparse_map(name))


@pytest.mark.parametrize("name,mode", STAGED)
def test_restatement_staging_matches_reference_vectors(name, mode):
    img, lidar, radar, pts, p, crop, md, want_in, want_lb, want_im = staged(name)
    imaps, valids = [q["imap"] for q in pts], [q["valid"] for q in pts]
    for q in pts:
        assert np.array_equal(F.filter_points(q["rxy"], q["rdep"], q["lxy"], q["ldep"])[1], q["valid"])
        assert np.array_equal(F.index_map(q["rxy"], img.shape[1:3]), q["imap"])
    got = F.stage_val(img, lidar, radar, imaps, valids, crop, md) if mode == "val" else F.stage_train(img, lidar, radar, p, imaps, valids, crop, md)
    assert np.array_equal(got[0], want_in) and np.array_equal(got[1], want_lb) and np.array_equal(got[2], want_im)
    assert got[0].dtype == np.float32 and got[2].dtype == np.int32


def test_golden_cases_cover_what_they_claim():
    assert (G["label_counts"] > 0).all()                                                   # labels 0, 1, 2 all occur
    assert np.array_equal(G["label_counts"], sum(np.bincount(G[n + "_labels"], minlength=3) for n in FILTER_CASES))
    assert len(set(G["f130x3000_labels"].tolist())) == 3 and (G["f5x3_labels"] == 2).any()
    rxy = G["f37x70_rxy"]                                                                  # two radar points in one pixel: the later stays
    assert (rxy[0].astype(np.int32) == rxy[1].astype(np.int32)).all() and sparse_map("f37x70")[int(rxy[0, 1]), int(rxy[0, 0])] == 1
    for name, mode in STAGED:
        img, lidar, radar, pts, p, crop, md, want_in, _, want_im = staged(name)
        imaps, valids = [q["imap"] for q in pts], [q["valid"] for q in pts]
        plain = (F.stage_val(img, lidar, radar, imaps, valids, crop, md, filtered=False) if mode == "val" else
                 F.stage_train(img, lidar, radar, p, imaps, valids, crop, md, filtered=False))[0]
        assert all((plain[b, 3] != want_in[b, 3]).any() for b in range(len(pts))), name    # the filter has an effect inside every crop
        assert float(G[name + "_margin"]) >= MARGIN
        for b, q in enumerate(pts):                                                        # the radar map is written from the points
            assert np.array_equal(radar[b], F.radar_map_from_points(q["rxy"], q["rdep"], radar[b].shape))
    assert G["val1_clamped"] > 0 and G["tr1_clamped"] > 0 and np.isfinite(float(G["tr1_max_depth"]))
    assert (G["tr2_fill_with_invalid0"] > 0).any() and not G["tr2_f0_valid"][0]              # rotation fill (index 0) with point 0 invalid
    assert (G["tr2_index_map_out"] == 0).sum() >= G["tr2_fill_with_invalid0"].sum()


def test_equal_distances_go_to_the_lower_index():
    """Checked against the restatement only: the reference's argsort is not stable.  Point 0 has four lidar points at distance 3; with
    indices (0, 1, 2) = (31 m, 5 m, 5 m) one of three passes the depth test (label 0), with index 3 (30 m) in place of 2 two would."""
    labels, valid, topk = F.filter_points(TIE["rxy"], TIE["rdep"], TIE["lxy"], TIE["ldep"])
    assert topk.tolist() == [[0, 1, 2], [5, 6, 7]] and labels.tolist() == [0, 1] and valid.tolist() == [False, True]
    perm = np.array([3, 2, 1, 0, 4, 8, 7, 6, 5])                                           # the rule is about indices, not about points
    labels_p, _, topk_p = F.filter_points(TIE["rxy"], TIE["rdep"], TIE["lxy"][perm], TIE["ldep"][perm])
    assert topk_p.tolist() == [[0, 1, 2], [5, 6, 7]] and labels_p.tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_new_symbols_are_exported(L):
    for name in ("rd_radar_filter_points", "rd_radar_index_map", "rd_stage_index_filter_val", "rd_stage_index_filter_train"):
        assert hasattr(L, name), name


def test_abi_rejects_bad_arguments_without_gpu(L):
    """Every rejection happens before anything reaches the GPU (the pointers are host dummies that are never followed), each with a code
    of its own."""
    from radar_depth_amd import _lib as E
    from radar_depth_amd.dataset.staging import train_frame_records
    buf = C.create_string_buffer(256)
    d = C.c_void_p((C.addressof(buf) + 15) & ~15)
    thr = np.zeros(4)
    host = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    i32 = lambda *v: np.array(v, np.int32)          # noqa: E731

    def filt(nr=i32(5, 0), nl=i32(7, 0), B=2, Rmax=8, Lmax=16, null=None):
        a = [d, d, d, d, host(nr), host(nl), B, Rmax, Lmax, host(thr), d, d, d, None]
        if null is not None:
            a[null] = None
        return L.rd_radar_filter_points(*a), L.rd_last_error()

    for k in (0, 1, 2, 3, 4, 5, 9, 10, 11, 12):
        rc, err = filt(null=k)
        assert rc == E.RD_ERADAR_NULL and b"null" in err, k
    for kw in (dict(B=0), dict(B=65537), dict(Rmax=0), dict(Rmax=(1 << 20) + 1), dict(Lmax=0), dict(Lmax=(1 << 24) + 1)):
        rc, err = filt(**kw)
        assert rc == E.RD_ERADAR_RANGE and b"Rmax" in err, kw
    assert filt(nr=i32(9, 0))[0] == E.RD_ERADAR_NRADAR and filt(nr=i32(5, -1))[0] == E.RD_ERADAR_NRADAR
    assert filt(nl=i32(17, 0))[0] == E.RD_ERADAR_NLIDAR and filt(nl=i32(7, -1))[0] == E.RD_ERADAR_NLIDAR
    rc, err = filt(nl=i32(2, 0))
    assert rc == E.RD_ERADAR_FEWLIDAR and b"three neighbours" in err
    assert filt(nr=i32(1, 1), nl=i32(3, 0))[0] == E.RD_ERADAR_FEWLIDAR                      # the second frame

    def imap(nr=i32(5), B=1, Rmax=8, H0=24, W0=40, null=None):
        a = [d, host(nr), B, Rmax, H0, W0, d, None]
        if null is not None:
            a[null] = None
        return L.rd_radar_index_map(*a)

    assert [imap(null=k) for k in (0, 1, 6)] == [E.RD_ERADAR_NULL] * 3
    assert [imap(B=0), imap(Rmax=0), imap(H0=0), imap(W0=0), imap(H0=1 << 15, W0=1 << 15)] == [E.RD_ERADAR_RANGE] * 5
    assert imap(nr=i32(9)) == E.RD_ERADAR_NRADAR

    def val(nr=i32(5), B=1, Rmax=8, H0=24, W0=40, i0=2, j0=4, H=20, W=32, apply=1, null=None):
        a = [d, d, host(nr), B, Rmax, H0, W0, i0, j0, H, W, apply, d, d, None]
        if null is not None:
            a[null] = None
        return L.rd_stage_index_filter_val(*a)

    assert [val(null=k) for k in (0, 1, 2, 12, 13)] == [E.RD_ERADAR_NULL] * 5
    assert [val(B=0), val(Rmax=0), val(H0=0)] == [E.RD_ERADAR_RANGE] * 3
    assert val(nr=i32(9)) == E.RD_ERADAR_NRADAR
    assert [val(i0=5), val(j0=9), val(i0=-1), val(H=0), val(W=41, j0=0)] == [E.RD_ERADAR_CROP] * 5
    assert b"does not fit" in L.rd_last_error()

    def params():
        return dict(scale=np.array([1.25]), angle=np.array([2.0]), flip=np.array([True]), h_start=np.array([3]), w_start=np.array([5]),
                    factors=np.array([[0.9, 1.1, 1.0]]), order=np.array([[2, 0, 1]]))

    def train(p=None, nr=i32(5), B=1, Rmax=8, H0=24, W0=40, ch=24, cw=40, apply=1, null=None):
        recs = train_frame_records(p or params(), H0, W0)
        a = [d, d, host(nr), B, Rmax, H0, W0, ch, cw, host(recs), d, d, apply, d, d, None]
        if null is not None:
            a[null] = None
        return L.rd_stage_index_filter_train(*a)

    assert [train(null=k) for k in (0, 1, 2, 9, 10, 11, 13, 14)] == [E.RD_ERADAR_NULL] * 8
    assert [train(B=0), train(Rmax=0), train(W0=0)] == [E.RD_ERADAR_RANGE] * 3
    assert train(nr=i32(9)) == E.RD_ERADAR_NRADAR
    assert [train(H0=23), train(W0=39)] == [E.RD_ERADAR_CROP] * 2
    for key, value in (("h_start", 7), ("w_start", 11), ("h_start", -1), ("scale", 0.999)):     # int(24*1.25) = 30, int(40*1.25) = 50
        p = params()
        p[key][0] = value
        assert train(p) == E.RD_ERADAR_CROP, (key, value)
    codes = {E.RD_ERADAR_NULL, E.RD_ERADAR_RANGE, E.RD_ERADAR_NRADAR, E.RD_ERADAR_NLIDAR, E.RD_ERADAR_FEWLIDAR, E.RD_ERADAR_CROP}
    assert len(codes) == 6 and all(c < 0 for c in codes) and not codes & {-1, -2}


# ------------------------------------------------------------------------------------------------ Python surface
def test_sparsifier_errors():
    from radar_depth_amd.dataset import stage_train_batch, stage_val_batch
    for call in (lambda **kw: stage_val_batch(None, None, None, **kw), lambda **kw: stage_train_batch(None, None, None, None, **kw)):
        with pytest.raises(ValueError, match=r"^\[Error\] Invalid sparsifier\.$"):
            call(sparsifier="lidar")
        for name in ("uniform", "lidar_radar"):
            with pytest.raises(NotImplementedError, match="scope"):
                call(sparsifier=name)
        with pytest.raises(NotImplementedError, match="with_mask"):
            call(sparsifier="radar_filtered2")
        with pytest.raises(ValueError, match="needs radar_filter"):
            call(sparsifier="radar_filtered")
        with pytest.raises(ValueError, match="extras=True needs radar_filter"):
            call(extras=True)
        with pytest.raises(ValueError, match="a RadarFilter"):
            call(sparsifier="radar_filtered", radar_filter=object())
    with pytest.raises(ValueError, match="modality 'rgb'"):
        stage_train_batch(None, None, None, None, modality="rgb", sparsifier="radar_filtered", radar_filter=object())


def test_default_signatures_are_unchanged():
    from radar_depth_amd import dataset
    from radar_depth_amd.dataset import staging
    val, train = inspect.signature(staging.stage_val_batch).parameters, inspect.signature(staging.stage_train_batch).parameters
    inf = float("inf")
    assert [(k, v.default) for k, v in val.items()] == [
        ("image_u8", inspect.Parameter.empty), ("lidar_i16", inspect.Parameter.empty), ("radar_i16", inspect.Parameter.empty),
        ("crop_size", (450, 800)), ("max_depth", inf), ("sparsifier", "radar"), ("radar_filter", None), ("extras", False)]
    assert [(k, v.default) for k, v in train.items()] == [
        ("image_u8", inspect.Parameter.empty), ("lidar_i16", inspect.Parameter.empty), ("radar_i16", inspect.Parameter.empty),
        ("params", inspect.Parameter.empty), ("crop_size", (450, 800)), ("max_depth", inf), ("modality", "rgbd"), ("sparsifier", "radar"),
        ("radar_filter", None), ("extras", False)]
    assert list(inspect.signature(staging.filter_radar_points).parameters) == [
        "radar_points", "radar_depth_points", "lidar_points", "lidar_depth_points", "n_radar", "n_lidar", "frame_shape"]
    assert dataset.filter_radar_points is staging.filter_radar_points and dataset.RadarFilter is staging.RadarFilter
    # the return arity: two values unless extras is asked for
    x, y = object(), object()
    assert staging._with_extras(x, y, None, False) == (x, y)
    assert np.allclose(staging._FILTER_THRESHOLDS, [np.log(4 / 14), np.log(14), np.log(16 / 5), np.log(5)], rtol=0, atol=0)

"""The comparison rows without a GPU: the numpy restatement (tests/visualize_ref.py) against the vectors of the reference's own utils
functions (tests/golden/visualize.npz), what that fixture claims to cover, the shipped colour table, the RD_EVIS_* argument checks of
rd_render_rows (nothing is launched: the pointers are host dummies that are never followed), and the Python surface of
radar_depth_amd.utils."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visualize_ref as V  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "visualize.npz"))
CASES = ("rgbd1", "rgb1", "rgb2", "ladder", "const", "batch", "edge")


def planes_of(name):
    inputs, target, pred = G[name + "_inputs"], G[name + "_target"], G[name + "_pred"]
    return inputs[:, :3], ([inputs[:, 3:4]] if inputs.shape[1] == 4 else []) + [target, pred]


# ------------------------------------------------------------------------------------------------ restatement and fixture
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_rows(name):
    rgb, planes = planes_of(name)
    want = G[name + "_rows"]
    assert want.dtype == np.uint8 and want.shape == (rgb.shape[0], rgb.shape[2], (1 + len(planes)) * rgb.shape[3], 3)
    assert np.array_equal(V.merge_rows(rgb, planes, G["table"]), want)


def test_restatement_matches_reference_colored_depthmap():
    t = G["table"]
    assert np.array_equal(V.colored_depthmap(G["cmap_depth"], t, *G["cmap_range"]), G["cmap_img"])
    assert np.array_equal(V.colored_depthmap(G["cmap_depth"], t), G["cmap_img_own"])
    assert np.array_equal(V.colored_depthmap(G["cmap_flat"], t, *G["cmap_flat_range"]), G["cmap_flat_img"])


def test_fixture_covers_what_it_claims():
    t = G["table"]
    # shapes: odd sizes whose panels and canvas rows start on odd bytes, and one multiple of four
    assert G["rgbd1_inputs"].shape == (1, 4, 33, 47) and G["rgb1_inputs"].shape == (1, 3, 33, 47) and G["ladder_inputs"].shape == (1, 4, 45, 80)
    assert (3 * 47) % 4 != 0 and (3 * 3 * 47) % 4 != 0                         # panel 1 of any row, and row 1 of a k = 3 canvas
    # rgbd1: a negative minimum in the prediction, the maximum in another plane
    _, (radar, lidar, pred) = planes_of("rgbd1")
    lo, hi = V.frame_range([radar, lidar, pred])
    assert lo < 0 and pred.min() == lo and lidar.max() == hi and pred.max() < hi and radar.min() == 0
    # ladder: 510 boundary depths; the two shortcuts change at least 50 of them each (161 and 121 when the fixture was made)
    _, planes = planes_of("ladder")
    lo, hi = V.frame_range(planes)
    steps = planes[2].reshape(-1)[G["ladder_pos"]]
    exact = V.lut_index(steps, lo, hi - lo)
    assert steps.size == 510 and lo == 0 and np.array_equal(exact, np.repeat(np.arange(256), 2)[1:-1])
    assert np.array_equal(np.nextafter(steps[1::2], np.float32(-np.inf)), steps[0::2])
    changed = [int((V.lut_index(steps, lo, hi - lo, mode) != exact).sum()) for mode in ("reciprocal", "float64")]
    assert changed == G["ladder_changed"].tolist() and min(changed) >= 50
    rgb, _ = planes_of("ladder")
    for mode in ("reciprocal", "float64"):
        assert not np.array_equal(V.merge_rows(rgb, planes, t, mode), G["ladder_rows"])
    # const: black depth panels next to a live rgb panel
    assert not G["const_rows"][0, :, 47:].any() and G["const_rows"][0, :, :47].any()
    # batch: five frames of one tensor, ranges orders of magnitude apart
    _, planes = planes_of("batch")
    spans = [float(np.subtract(*V.frame_range([p[b] for p in planes])[::-1])) for b in range(5)]
    assert G["batch_inputs"].shape == (5, 4, 33, 47) and max(spans) / min(spans) > 1e6
    # edge: every byte value from the rgb panel, 0 and 1 included
    vals = G["edge_inputs"].reshape(-1)
    k = np.arange(1, 255, dtype=np.float32) / np.float32(255)
    for probe in (np.float32([0, 1]), k, np.nextafter(k, np.float32(0)), np.nextafter(k, np.float32(1))):
        assert np.isin(probe, vals).all()
    # cmap: below, above and exactly on d_max; d_min == d_max gives under / bad / over
    d, (d_min, d_max) = G["cmap_depth"], G["cmap_range"]
    assert (d < d_min).any() and (d > d_max).any() and (d == np.float32(d_max)).any()
    assert np.array_equal(G["cmap_img"][d == np.float32(d_max)][0], t[255]) and np.array_equal(G["cmap_img"][d > d_max][0], t[V.OVER])
    flat = G["cmap_flat_img"]
    assert np.array_equal(flat[0, 0], t[V.UNDER]) and np.array_equal(flat[-1, 0], t[V.OVER]) and not flat[11:22].any()


def test_index_branches():
    idx = V.lut_index(np.float32([-1, -0.0, 0, 0.49, 0.5, 99.99, 100, 100.5, np.inf, np.nan]), 0.0, 100.0)
    assert idx.tolist() == [V.UNDER, 0, 0, 1, 1, 255, 255, V.OVER, V.OVER, V.BAD]
    assert V.lut_index(np.float32([1, 2, 3]), 2.0, 0.0).tolist() == [V.UNDER, V.BAD, V.OVER]
    lo, denom = V.given_range(0.1, 0.7)
    assert lo == np.float32(0.1) and denom == np.float32(0.7 - 0.1) and denom != np.float32(0.7) - np.float32(0.1)


# ------------------------------------------------------------------------------------------------ the table
def test_shipped_table_is_the_fixture_table():
    from radar_depth_amd import utils
    t = utils.viridis_table()
    assert t.dtype == np.uint8 and t.shape == (259, 3) and np.array_equal(t, G["table"]) and np.array_equal(t, V.package_table())
    assert np.array_equal(t[256], t[0]) and np.array_equal(t[257], t[255]) and not t[258].any()
    assert t[0].tolist() == [68, 1, 84] and t[255].tolist() == [253, 231, 36]


def test_table_is_matplotlibs_viridis():
    cm = pytest.importorskip("matplotlib.cm")
    cmap = cm.viridis
    cmap(np.zeros(1))
    assert np.array_equal(np.trunc(255 * np.asarray(cmap._lut)[:, :3]).astype(np.uint8), G["table"])


def test_import_needs_neither_matplotlib_nor_pillow():
    import subprocess
    code = ("import sys; sys.modules['matplotlib'] = None; sys.modules['PIL'] = None; "
            "from radar_depth_amd import utils; assert utils.viridis_table().shape == (259, 3)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_new_symbols_are_exported(L):
    assert hasattr(L, "rd_render_rows") and hasattr(L, "rd_render_workspace_bytes")
    assert L.rd_render_workspace_bytes(1) >= 8 and L.rd_render_workspace_bytes(16) >= 128
    assert L.rd_render_workspace_bytes(0) < 0 and L.rd_render_workspace_bytes(65536) < 0


def test_abi_rejects_bad_arguments_without_gpu(L):
    """Every rejection happens before anything reaches the GPU, each with a code of its own."""
    from radar_depth_amd import _lib as E
    big = C.create_string_buffer(1 << 16)
    base = (C.addressof(big) + 15) & ~15
    at = lambda byte: C.c_void_p(base + byte)               # noqa: E731
    H, W, n = 3, 5, 15

    def call(rgb=0, rs=4 * n, planes=(4 * 3 * n, 4 * 3 * n + 4 * 2 * 4 * n), ps=None, count=None, B=2, H=H, W=W, rng=None, work=30000, table=31000,
             out=32000, fs=None, pitch=None, null_planes=False, null_strides=False):
        k = len(planes) + (rgb is not None)
        count = len(planes) if count is None else count
        ptrs = (C.c_void_p * 3)(*[None if p is None else base + p for p in planes])
        strides = (C.c_int64 * 3)(*(ps or [4 * n] * len(planes)))
        pitch = 3 * k * W if pitch is None else pitch
        fs = H * pitch if fs is None else fs
        r = None if rng is None else (C.c_double * 2)(*rng)
        opt = lambda v: None if v is None else at(v)        # noqa: E731
        return L.rd_render_rows(opt(rgb), rs, None if null_planes else ptrs, None if null_strides else strides, count, B, H, W, r, opt(work),
                                opt(table), opt(out), fs, pitch, None)

    assert [call(null_planes=True), call(null_strides=True), call(table=None), call(out=None), call(work=None), call(planes=(4 * 3 * n, None))] == \
        [E.RD_EVIS_NULL] * 6 and b"null" in L.rd_last_error()
    assert [call(B=0), call(B=65536), call(H=0), call(W=0), call(W=-2), call(H=65536), call(H=40000, W=40000)] == [E.RD_EVIS_RANGE] * 7
    assert [call(count=0), call(count=4), call(count=-1)] == [E.RD_EVIS_PLANES] * 3 and b"depth planes" in L.rd_last_error()
    assert [call(ps=[n - 1, 4 * n]), call(ps=[4 * n, 0]), call(rs=3 * n - 1)] == [E.RD_EVIS_STRIDE] * 3 and b"rgb" in L.rd_last_error()
    assert [call(pitch=3 * 3 * W - 1), call(pitch=50, fs=H * 50 - 1), call(rgb=None, pitch=3 * 2 * W - 1)] == [E.RD_EVIS_PITCH] * 3
    assert [call(rng=(float("nan"), 1.0)), call(rng=(0.0, float("nan")))] == [E.RD_EVIS_NAN] * 2 and b"NaN" in L.rd_last_error()
    # out against what is read: rgb occupies bytes 0 .. (4n + 3n) * 4, the two planes [180, 180 + (4n + n) * 4) and [660, ...)
    assert [call(out=0), call(out=4 * 7 * n - 1), call(out=4 * 3 * n + 4 * 5 * n - 1), call(out=660 - 2 * H * 45 + 1), call(out=700)] == \
        [E.RD_EVIS_OVERLAP] * 5
    assert call(rgb=None, out=0, planes=(60,), ps=[n]) == E.RD_EVIS_OVERLAP and b"depth plane 0" in L.rd_last_error()
    codes = [E.RD_EVIS_NULL, E.RD_EVIS_RANGE, E.RD_EVIS_PLANES, E.RD_EVIS_STRIDE, E.RD_EVIS_PITCH, E.RD_EVIS_NAN, E.RD_EVIS_OVERLAP]
    assert codes == list(range(E.RD_ESPARSE_OVERLAP - 1, E.RD_ESPARSE_OVERLAP - 8, -1))          # the numbering goes on after RD_ESPARSE_OVERLAP
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "radar_depth_hip.h")).read()
    for name in ("NULL", "RANGE", "PLANES", "STRIDE", "PITCH", "NAN", "OVERLAP"):
        assert "#define RD_EVIS_%s (%d)" % (name, getattr(E, "RD_EVIS_" + name)) in hdr


# ------------------------------------------------------------------------------------------------ Python surface
def test_signatures_are_the_references():
    from radar_depth_amd import utils
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]        # noqa: E731
    empty = inspect.Parameter.empty
    assert sig(utils.colored_depthmap) == [("depth", empty), ("d_min", None), ("d_max", None)]
    assert sig(utils.merge_into_row) == [("input", empty), ("depth_target", empty), ("depth_pred", empty), ("out", None)]
    assert sig(utils.merge_into_row_with_gt) == [("input", empty), ("depth_input", empty), ("depth_target", empty), ("depth_pred", empty), ("out", None)]
    assert sig(utils.add_row) == [("img_merge", empty), ("row", empty)]
    assert sig(utils.save_image) == [("img_merge", empty), ("filename", empty)]
    assert sig(utils.adjust_learning_rate_new) == sig(utils.adjust_learning_rate) == [("optimizer", empty), ("epoch", empty), ("lr_init", empty)]
    assert [k for k, _ in sig(utils.ComparisonImage.__init__)][1:5] == ["rows", "height", "width", "panels"]
    with pytest.raises(ValueError, match="together"):
        utils.colored_depthmap(torch.zeros(2, 2), d_min=1.0)


def test_adjust_learning_rate_new():
    from radar_depth_amd import utils
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], 0.5)

    class Step:                                              # the part of HipTrainStep the schedules use
        def set_lr(self, lr):
            self.lr = lr
    step = Step()
    for epoch, want in ((0, 0.01), (6, 0.01), (7, 0.1 * 0.01), (15, 0.1 * 0.01), (16, 0.01 * 0.01)):
        assert utils.adjust_learning_rate_new(opt, epoch, 0.01) == want and opt.param_groups[0]["lr"] == want
        assert utils.adjust_learning_rate_new(step, epoch, 0.01) == want and step.lr == want


def test_add_row_and_save_image_on_numpy(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from radar_depth_amd import utils
    a, b = G["rgb1_rows"][0], G["rgb2_rows"][0]
    both = utils.add_row(a, b)
    assert isinstance(both, np.ndarray) and np.array_equal(both, np.vstack([a, b]))
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    assert torch.equal(utils.add_row(ta, tb), torch.from_numpy(both))
    path = str(tmp_path / "comparison.png")
    utils.save_image(both.astype(np.float64), path)          # the reference hands float64 over
    assert np.array_equal(np.array(Image.open(path)), both)
    utils.save_image(torch.from_numpy(both), path)
    assert np.array_equal(np.array(Image.open(path)), both)

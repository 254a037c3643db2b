"""GPU checks of the KITTI devkit evaluation (csrc/kitti_eval.hip behind radar_depth_amd/evaluation/kitti.py) against the fixture that
the devkit's own functions produced (tests/golden/kitti_eval.npz) and against the numpy restatement tests/kitti_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
NO_LOG, WITH_LOG = [0, 1, 2, 3, 7, 8], [4, 5, 6]            # the sums without a logarithm and the three with one


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "kitti_eval.npz")))


@pytest.fixture(scope="module")
def kitti():
    from radar_depth_amd.evaluation import kitti as mod
    return mod


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cases(G, kind):
    return sorted(k[len(kind) + 1:-3] for k in G if k.startswith(kind + "_") and k.endswith("_in" if kind == "interp" else "_gt"))


def holed(rng, shape, keep=0.3):
    """Depth planes with holes, a NaN, zeros and empty rows."""
    d = rng.uniform(0.5, 90, shape).astype(np.float32)
    d[rng.uniform(size=shape) > keep] = -1
    flat = d.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = np.nan
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = 0.0
    if shape[-2] > 3:
        d[..., rng.integers(0, shape[-2]), :] = -1
        d[..., 0, :] = -1
    return d


def assert_errors_close(got, want):
    """Counts exact; 1e-12 relative for the sums without a logarithm, 1e-9 for the three with one; NaN and inf where the restatement
    has them."""
    assert np.array_equal(got[..., 9], want[..., 9])
    for cols, tol in ((NO_LOG, 1e-12), (WITH_LOG, 1e-9)):
        g, w = got[..., cols], want[..., cols]
        fin = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), fin), (g, w)
        assert np.array_equal(g[~fin], w[~fin], equal_nan=True), (g, w)
        assert np.all(np.abs(g[fin] - w[fin]) <= tol * np.abs(w[fin])), (g, w, tol)


def test_fixture_cases_bit_for_bit(G, kitti):
    for n in cases(G, "interp"):
        d = dev(G["interp_%s_in" % n])
        out = kitti.interpolate_background(d)
        assert np.array_equal(bits(out.cpu().numpy()), bits(G["interp_%s_out" % n])), n
        assert np.array_equal(bits(d.cpu().numpy()), bits(G["interp_%s_in" % n])), n
        assert kitti.interpolate_background(d, out=d) is d
        assert np.array_equal(bits(d.cpu().numpy()), bits(G["interp_%s_out" % n])), n + " in place"
    for n in cases(G, "img"):
        img = kitti.error_image(dev(G["img_%s_gt" % n]), dev(G["img_%s_pred" % n]))
        assert img.dtype == torch.uint8 and np.array_equal(img.cpu().numpy(), G["img_%s_rgb" % n]), n


def test_fixture_errors_within_the_accumulation_bound(G, kitti):
    for n in cases(G, "err"):
        gt, pred, ref = G["err_%s_gt" % n], G["err_%s_pred" % n], G["err_%s_errors" % n].astype(np.float64)
        got = kitti.depth_errors(dev(gt), dev(pred)).cpu().numpy()
        assert got.shape == (1, 10) and got.dtype == np.float64
        s = K.error_sums(gt, pred)
        nv = s[9]
        base = 2.0 * nv * EPS
        k = (s[5] / nv) / (s[5] / nv - (s[6] / nv) ** 2)
        bound = np.array([base, base / 2, base, base / 2, base, base / 2, base / 2 * k, base, base])
        gap = np.abs(got[0, :9] - ref) / np.abs(ref)
        print(n, " ".join("%.2e" % g for g in gap))
        assert got[0, 9] == nv and np.all(gap <= bound), (n, gap, bound)
        assert_errors_close(got[0], K.errors(gt, pred))


@pytest.mark.parametrize("h", [1, 2, 3, 7])
def test_small_shapes_against_the_restatement(kitti, h):
    rng = np.random.default_rng(100 + h)
    table = kitti.log_colormap()
    for w in (1, 2, 63, 64, 65, 130):
        B = 3
        full = rng.uniform(0.5, 90, (B, 4, h, w)).astype(np.float32)
        full[:, 3] = holed(rng, (B, h, w), keep=0.3 if w > 2 else 0.6)
        gt = holed(rng, (B, 1, h, w), keep=0.5)
        want = np.stack([K.interpolate(full[b, 3]) for b in range(B)])
        t = dev(full)
        view = t[:, 3:4]                                     # frames 4*h*w apart
        # out of place into the middle of a canaried buffer
        pad = 37
        buf = torch.full((B * h * w + 2 * pad,), -777.0, dtype=torch.float32, device="cuda")
        out = buf[pad:pad + B * h * w].view(B, 1, h, w)
        assert kitti.interpolate_background(view, out=out) is out
        got = buf.cpu().numpy()
        assert np.all(got[:pad] == -777) and np.all(got[-pad:] == -777)
        assert np.array_equal(bits(got[pad:-pad].reshape(B, h, w)), bits(want)), (h, w)
        assert np.array_equal(bits(t.cpu().numpy()), bits(full))
        # errors and the image read the view and the filled planes
        g = dev(gt)
        for zi in (False, True):
            e = kitti.depth_errors(g, out, zero_invalid=zi).cpu().numpy()
            assert_errors_close(e, np.stack([K.errors(gt[b, 0], want[b], zi) for b in range(B)]))
            want_img = np.stack([K.error_image(gt[b, 0], want[b], table, zi) for b in range(B)])
            for a in range(4):                               # every byte alignment of the image base, a pitch and a frame stride
                pitch, fs = 3 * w + 5, h * (3 * w + 5) + 7
                raw = torch.full((64 + a + B * fs + 64,), 0xAB, dtype=torch.uint8, device="cuda")
                img = raw[64 + a:].as_strided((B, h, w, 3), (fs, pitch, 3, 1))
                assert img.data_ptr() % 4 == (raw.data_ptr() + a) % 4
                assert kitti.error_image(g, out, zero_invalid=zi, out=img) is img
                r = raw.cpu().numpy()
                assert np.array_equal(r[64 + a:].copy()[:B * fs].reshape(B, fs)[:, :h * pitch].reshape(B, h, pitch)[:, :, :3 * w]
                                      .reshape(B, h, w, 3), want_img), (h, w, zi, a)
                mask = np.ones(r.shape, dtype=bool)
                idx = (64 + a + np.arange(B)[:, None, None] * fs + np.arange(h)[None, :, None] * pitch + np.arange(3 * w)[None, None, :])
                mask[idx.reshape(-1)] = False
                assert np.all(r[mask] == 0xAB), (h, w, zi, a)
        # in place on the slice: the other channels are the canaries
        assert kitti.interpolate_background(view, out=view) is view
        got = t.cpu().numpy()
        assert np.array_equal(bits(got[:, 3]), bits(want)) and np.array_equal(bits(got[:, :3]), bits(full[:, :3])), (h, w)


def test_errors_edge_cases_and_reproducibility(kitti):
    rng = np.random.default_rng(7)
    gt = holed(rng, (4, 1, 33, 70), keep=0.4)
    gt[2] = -1                                               # a frame without a valid pixel
    gt[3, 0, 5, 5] = 0.0
    pred = (np.abs(rng.uniform(0.5, 90, gt.shape)) * np.exp(rng.normal(0, 0.2, gt.shape))).astype(np.float32)
    g, p = dev(gt), dev(pred)
    for zi in (False, True):
        e = kitti.depth_errors(g, p, zero_invalid=zi)
        assert torch.equal(e.view(torch.int64), kitti.depth_errors(g, p, zero_invalid=zi).view(torch.int64))
        e = e.cpu().numpy()
        assert np.isnan(e[2, :9]).all() and e[2, 9] == 0
        with np.errstate(all="ignore"):
            want = np.stack([K.errors(gt[b, 0], pred[b, 0], zi) for b in range(4)])
        assert_errors_close(e, want)
        if not zi:                                           # gt == 0.0 is valid there: 1/0 and log 0 poison the frame, as in the devkit
            assert not np.isfinite(e[3, 2]) and not np.isfinite(e[3, 4])


def test_decode_encode_every_uint16(kitti):
    v = np.arange(65536, dtype=np.uint16).reshape(1, 1, 256, 256)
    d = kitti.decode_depth(dev(v))
    assert d.dtype == torch.float32 and np.array_equal(bits(d.cpu().numpy()), bits(K.decode(v)))
    assert np.array_equal(kitti.encode_depth(d).cpu().numpy(), v)
    odd = np.array([[-1, np.nan, 0.0, 0.001, 1 / 256, 255.99, 255.99609375, 256.0, 1e6, np.inf, -0.0]], dtype=np.float32)
    assert np.array_equal(kitti.encode_depth(dev(odd)).cpu().numpy(), K.encode(odd))
    assert list(kitti.encode_depth(dev(odd)).cpu().numpy()[0, 5:10]) == [65533, 65535, 65535, 65535, 65535]      # saturation


def test_meter_five_updates_of_three_frames(kitti):
    rng = np.random.default_rng(11)
    shape = (3, 1, 21, 67)
    batches = []
    for i in range(5):
        gt = holed(rng, shape, keep=0.5)
        gt[np.isnan(gt) | (gt == 0)] = -1
        pred = (np.abs(gt) * (1.0 + 0.05 * i) * np.exp(rng.normal(0, 0.2, shape))).astype(np.float32)
        pred[rng.uniform(size=shape) < 0.3] = -1            # holes for the devkit's fill
        pred[:, :, 10, 3] = 5.0                              # (no row stays empty)
        batches.append((gt, pred))
    runs = []
    for _ in range(2):
        meter = kitti.KittiDepthMeter()
        for gt, pred in batches:
            meter.update(dev(pred), dev(gt))
        runs.append(meter.state.clone())
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))
    rows = np.array([K.errors(gt[b, 0], K.interpolate(pred[b, 0])) for gt, pred in batches for b in range(3)])
    mean, mn, mx = K.stats(rows)
    got = meter.stats()
    assert meter.frames() == 15 and list(got) == list(K.METRICS)
    for i, n in enumerate(K.METRICS):
        tol = 1e-9 if i in WITH_LOG else 1e-12
        for a, b in zip(got[n], (mean[i], mn[i], mx[i])):
            assert abs(a - b) <= tol * abs(b), (n, a, b)
    meter.reset()
    assert meter.frames() == 0 and meter.state.cpu().numpy().tolist() == [[0.0, 1.0, 0.0, 0.0]] * 9
    # this project's targets: 0 is "no measurement", the prediction is dense and is scored as it is
    gt, pred = batches[0]
    tgt = np.where(gt >= 0, gt, 0).astype(np.float32)
    dense = np.abs(pred) + 1
    e = meter.update(dev(dense), dev(tgt), zero_invalid=True, interpolate=False).cpu().numpy()
    assert_errors_close(e, np.stack([K.errors(tgt[b, 0], dense[b, 0], True) for b in range(3)]))


@pytest.mark.parametrize("shape", [(1, 352, 1216), (2, 450, 800)])
def test_full_size_frames(kitti, shape):
    rng = np.random.default_rng(shape[1])
    B, h, w = shape
    pred = holed(rng, (B, 1, h, w), keep=0.05)
    pred[:, :, :40] = -1
    gt = rng.uniform(0.5, 90, (B, 1, h, w)).astype(np.float32)
    gt[rng.uniform(size=gt.shape) > 0.05] = -1
    p, g = dev(pred), dev(gt)
    filled = kitti.interpolate_background(p)
    want = np.stack([K.interpolate(pred[b, 0]) for b in range(B)])
    assert np.array_equal(bits(filled.cpu().numpy()[:, 0]), bits(want))
    safe = np.where(want > 0, want, 1).astype(np.float32)    # (a 0.0 or an unfilled pixel would poison the sums)
    e = kitti.depth_errors(g, dev(safe[:, None])).cpu().numpy()
    assert_errors_close(e, np.stack([K.errors(gt[b, 0], safe[b]) for b in range(B)]))
    img = kitti.error_image(g, filled).cpu().numpy()
    assert np.array_equal(img, np.stack([K.error_image(gt[b, 0], want[b], kitti.log_colormap()) for b in range(B)]))


def test_evaluate_dirs(kitti, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    gt_dir, pred_dir = tmp_path / "gt", tmp_path / "pred"
    gt_dir.mkdir()
    pred_dir.mkdir()
    frames = []
    for i, (h, w) in enumerate(((20, 70), (20, 70), (12, 65), (12, 65))):
        gt = (rng.uniform(1, 80, (h, w)) * 256).astype(np.uint16)
        gt[rng.uniform(size=(h, w)) < 0.6] = 0
        pred = np.clip(gt.astype(np.float64) * np.exp(rng.normal(0, 0.2, (h, w))), 300, 65000).astype(np.uint16)
        pred[gt == 0] = (rng.uniform(1, 80, (h, w)) * 256).astype(np.uint16)[gt == 0]
        pred[rng.uniform(size=(h, w)) < 0.4] = 0
        pred[h // 2, w // 2] = 2560
        Image.fromarray(gt).save(str(gt_dir / ("%04d.png" % i)))
        Image.fromarray(pred).save(str(pred_dir / ("f%04d.png" % i)))
        frames.append((gt, pred))
    assert kitti.evaluate_dirs(str(gt_dir), str(pred_dir)) is True
    rows = []
    for i, (gt, pred) in enumerate(frames):
        g, p = K.decode(gt), K.interpolate(K.decode(pred))
        e = K.errors(g, p)
        rows.append(e)
        assert open(str(pred_dir / "errors_out" / ("%04d.txt" % i))).read() == "".join("%f " % v for v in e[:9])
        img = np.asarray(Image.open(str(pred_dir / "errors_img" / ("%04d.png" % i))))
        assert np.array_equal(img, K.error_image(g, p, kitti.log_colormap()))
    assert open(str(pred_dir / "stats_depth.txt")).read() == K.format_stats(*K.stats(np.array(rows)))
    # a count mismatch, and a ground truth that is not a 16-bit grey PNG
    Image.fromarray(frames[0][0]).save(str(gt_dir / "9999.png"))
    assert kitti.evaluate_dirs(str(gt_dir), str(pred_dir)) is False
    os.remove(str(gt_dir / "9999.png"))
    Image.fromarray((frames[0][0] >> 8).astype(np.uint8)).save(str(gt_dir / "0000.png"))
    assert kitti.evaluate_dirs(str(gt_dir), str(pred_dir)) is False

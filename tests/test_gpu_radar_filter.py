"""The radar_filtered sparsifier on the GPU (csrc/radar_filter.hip through dataset.filter_radar_points / stage_val_batch /
stage_train_batch) against the vectors of the reference's own code (tests/golden/radar_filter.npz) and, for the cases the reference cannot
run, against the numpy restatement the generator pinned to it (tests/radar_filter_ref.py).  Everything is integer work or a decision the
fixture keeps at least 1e-6 away from its threshold, so every comparison is np.array_equal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radar_filter_ref as F  # noqa: E402
from test_radar_filter_host import FILTER_CASES, G, STAGED, TIE, sparse_map, staged  # noqa: E402

pytestmark = pytest.mark.gpu
G_VAL = np.load(os.path.join(os.path.dirname(__file__), "golden", "staging.npz"))
G_TRAIN = np.load(os.path.join(os.path.dirname(__file__), "golden", "staging_train.npz"))
PKEYS = ("scale", "angle", "flip", "h_start", "w_start", "factors", "order")


def pad_batch(points, fill=np.nan, rmax=None, lmax=None):
    """points: per frame (rxy, rdep, lxy, ldep) -> padded float64 arrays, the padding filled with ``fill``, and the counts."""
    nr, nl = [len(q[1]) for q in points], [len(q[3]) for q in points]
    B, Rmax, Lmax = len(points), rmax or max(max(nr), 1), lmax or max(max(nl), 1)
    rxy, rdep = np.full((B, Rmax, 2), fill), np.full((B, Rmax), fill)
    lxy, ldep = np.full((B, Lmax, 2), fill), np.full((B, Lmax), fill)
    for b, q in enumerate(points):
        rxy[b, :nr[b]], rdep[b, :nr[b]], lxy[b, :nl[b]], ldep[b, :nl[b]] = q
    return rxy, rdep, lxy, ldep, nr, nl


def run_filter(points, frame_shape, **kw):
    from radar_depth_amd.dataset import filter_radar_points
    rxy, rdep, lxy, ldep, nr, nl = pad_batch(points, **kw)
    f = filter_radar_points(*(torch.from_numpy(a).cuda() for a in (rxy, rdep, lxy, ldep)), nr, nl, frame_shape)
    return f, nr


def case_points(name):
    return tuple(G["%s_%s" % (name, k)] for k in ("rxy", "rdep", "lxy", "ldep"))


def staged_filter(pts, frame_shape):
    return run_filter([(q["rxy"], q["rdep"], q["lxy"], q["ldep"]) for q in pts], frame_shape)[0]


def gpu(*arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]


@pytest.mark.parametrize("name", FILTER_CASES)
def test_filter_matches_reference_vectors(name):
    shape = tuple(int(v) for v in G[name + "_shape"])
    f, _ = run_filter([case_points(name)], shape)
    labels, valid, topk = f.valid_labels.cpu().numpy()[0], f.valid_mask.cpu().numpy()[0], f.topk.cpu().numpy()[0]
    print("%s: %d labels, %d neighbours differ" % (name, (labels != G[name + "_labels"]).sum(), (topk != G[name + "_topk"]).sum()))
    assert f.valid_labels.dtype == torch.uint8 and f.valid_mask.dtype == torch.bool and f.topk.dtype == torch.int32 and f.index_map.dtype == torch.int32
    assert np.array_equal(labels, G[name + "_labels"]) and np.array_equal(valid, G[name + "_valid"]) and np.array_equal(topk, G[name + "_topk"])
    assert np.array_equal(f.index_map.cpu().numpy()[0], sparse_map(name))        # f37x70: two points in one pixel, the later one stays


def test_ragged_nan_padded_batch():
    """The five cases as one batch, padded with NaN to Rmax x Lmax: the padding is never read, the tail rows hold 0 / 0 / -1."""
    f, nr = run_filter([case_points(n) for n in FILTER_CASES], (900, 1600))
    labels, valid, topk, imap = f.valid_labels.cpu().numpy(), f.valid_mask.cpu().numpy(), f.topk.cpu().numpy(), f.index_map.cpu().numpy()
    assert labels.shape == (5, 130) and topk.shape == (5, 130, 3) and imap.shape == (5, 900, 1600)
    for b, name in enumerate(FILTER_CASES):
        n = nr[b]
        assert np.array_equal(labels[b, :n], G[name + "_labels"]) and np.array_equal(valid[b, :n], G[name + "_valid"]), name
        assert np.array_equal(topk[b, :n], G[name + "_topk"]), name
        assert not labels[b, n:].any() and not valid[b, n:].any() and (topk[b, n:] == -1).all(), name
        want = np.full((900, 1600), -1, np.int32)
        small = sparse_map(name)
        want[:small.shape[0], :small.shape[1]] = small
        assert np.array_equal(imap[b], want), name


def test_no_point_and_one_point():
    """n_radar 0 (with no lidar point either) and 1: the reference's np.squeeze breaks at one point; the restatement is the rule."""
    rxy, rdep, lxy, ldep = case_points("f37x70")
    one = (rxy[4:5], rdep[4:5], lxy, ldep)
    empty = (rxy[:0], rdep[:0], lxy[:0], ldep[:0])
    f, nr = run_filter([empty, one, (rxy[:0], rdep[:0], lxy, ldep)], (48, 80), rmax=3)
    want = F.filter_batch(*pad_batch([empty, one, empty], rmax=3)[:4], nr, [0, len(ldep), 0])
    assert np.array_equal(f.valid_labels.cpu().numpy(), want[0]) and np.array_equal(f.valid_mask.cpu().numpy(), want[1])
    assert np.array_equal(f.topk.cpu().numpy(), want[2]) and want[2][1, 0].min() >= 0
    imap = f.index_map.cpu().numpy()
    assert (imap[0] == -1).all() and (imap[2] == -1).all() and np.array_equal(imap[1], F.index_map(one[0], (48, 80))) and (imap[1] == 0).sum() == 1


def test_equal_distances_go_to_the_lower_index():
    f, _ = run_filter([(TIE["rxy"], TIE["rdep"], TIE["lxy"], TIE["ldep"])], (24, 40))
    want = F.filter_points(TIE["rxy"], TIE["rdep"], TIE["lxy"], TIE["ldep"])
    assert f.topk.cpu().numpy()[0].tolist() == [[0, 1, 2], [5, 6, 7]] == want[2].tolist()
    assert np.array_equal(f.valid_labels.cpu().numpy()[0], want[0]) and want[0].tolist() == [0, 1]


def test_index_map_skips_points_outside_the_frame():
    rxy, rdep, lxy, ldep = case_points("f37x70")
    H0, W0 = 48, 80
    out = np.array([[-3.2, 5.0], [W0 + 0.5, 5.0], [5.0, -1.0], [5.0, float(H0)], [np.nan, 3.0]])
    rxy2, rdep2 = np.concatenate((rxy, out)), np.concatenate((rdep, np.full(len(out), 10.0)))
    f, _ = run_filter([(rxy2, rdep2, lxy, ldep)], (H0, W0))
    imap = f.index_map.cpu().numpy()[0]
    assert np.array_equal(imap, sparse_map("f37x70")) and imap.max() == len(rdep) - 1           # the appended points left no trace
    assert np.array_equal(f.valid_labels.cpu().numpy()[0, :len(rdep)], G["f37x70_labels"])
    edge = np.array([[-0.5, 2.2], [W0 - 0.01, H0 - 0.01], [0.0, -0.99]])                        # truncation toward zero keeps these
    f, _ = run_filter([(edge, np.full(3, 10.0), lxy, ldep)], (H0, W0))
    imap = f.index_map.cpu().numpy()[0]
    assert np.array_equal(imap, F.index_map(edge, (H0, W0))) and imap[2, 0] == 0 and imap[H0 - 1, W0 - 1] == 1 and imap[0, 0] == 2


@pytest.mark.parametrize("name,mode", STAGED)
def test_staging_radar_filtered_matches_the_reference(name, mode):
    from radar_depth_amd.dataset import stage_train_batch, stage_val_batch
    img, lidar, radar, pts, p, crop, md, want_in, want_lb, want_im = staged(name)
    f = staged_filter(pts, img.shape[1:3])
    md = md if np.isfinite(md) else -1.0
    if mode == "val":
        x, y, extra = stage_val_batch(*gpu(img, lidar, radar), crop, md, sparsifier="radar_filtered", radar_filter=f, extras=True)
    else:
        x, y, extra = stage_train_batch(*gpu(img, lidar, radar), p, crop, md, sparsifier="radar_filtered", radar_filter=f, extras=True)
    im = extra["index_map"]
    assert im.dtype == torch.int32 and tuple(im.shape) == (len(pts), 1) + crop
    assert extra["radar_depth_filtered"].data_ptr() == x[:, 3:4].data_ptr()
    x, y, im = x.cpu().numpy(), y.cpu().numpy(), im.cpu().numpy()
    print("%s: %d input, %d label, %d index_map elements differ" % (name, (x != want_in).sum(), (y != want_lb).sum(), (im != want_im).sum()))
    assert np.array_equal(x, want_in) and np.array_equal(y, want_lb) and np.array_equal(im, want_im)
    for b, q in enumerate(pts):
        assert np.array_equal(f.valid_mask.cpu().numpy()[b, :len(q["valid"])], q["valid"])


def test_sparsifier_radar_still_matches_the_staging_fixtures():
    """The defaults, and sparsifier "radar" with a radar_filter and extras, leave inputs and labels as the existing fixtures have them."""
    from radar_depth_amd.dataset import stage_train_batch, stage_val_batch
    rng = np.random.RandomState(5)
    for name in ("a", "b", "c"):
        img, lidar, radar = (G_VAL[name + k] for k in ("_image", "_lidar", "_radar"))
        crop, md = tuple(int(v) for v in G_VAL[name + "_crop"]), float(G_VAL[name + "_max_depth"])
        B, H0, W0 = lidar.shape
        pts = [(rng.uniform(0, 1, (9, 2)) * [W0, H0], rng.uniform(2, 100, 9), rng.uniform(0, 1, (20, 2)) * [W0, H0], rng.uniform(2, 100, 20))] * B
        f, _ = run_filter(pts, (H0, W0))
        t = gpu(img, lidar, radar)
        got = stage_val_batch(*t, crop, md if np.isfinite(md) else -1.0)
        assert len(got) == 2 and np.array_equal(got[0].cpu().numpy(), G_VAL[name + "_inputs"]) and np.array_equal(got[1].cpu().numpy(), G_VAL[name + "_labels"])
        x, y, extra = stage_val_batch(*t, crop, md if np.isfinite(md) else -1.0, sparsifier="radar", radar_filter=f, extras=True)
        assert np.array_equal(x.cpu().numpy(), G_VAL[name + "_inputs"]) and np.array_equal(y.cpu().numpy(), G_VAL[name + "_labels"])
        want_im = np.stack([F.index_map_val(F.index_map(pts[b][0], (H0, W0)), crop) for b in range(B)])
        assert np.array_equal(extra["index_map"].cpu().numpy(), want_im)
    for name in ("six", "rag1"):
        img, lidar, radar = (G_TRAIN[name + k] for k in ("_image", "_lidar", "_radar"))
        p = {k: G_TRAIN["%s_p_%s" % (name, k)] for k in PKEYS}
        crop, md = tuple(int(v) for v in G_TRAIN[name + "_crop"]), float(G_TRAIN[name + "_max_depth"])
        B, H0, W0 = lidar.shape
        pts = [(rng.uniform(0, 1, (9, 2)) * [W0, H0], rng.uniform(2, 100, 9), rng.uniform(0, 1, (20, 2)) * [W0, H0], rng.uniform(2, 100, 20))] * B
        f, _ = run_filter(pts, (H0, W0))
        t = gpu(img, lidar, radar)
        got = stage_train_batch(*t, p, crop, md if np.isfinite(md) else -1.0)
        assert len(got) == 2 and np.array_equal(got[0].cpu().numpy(), G_TRAIN[name + "_inputs"]) and np.array_equal(got[1].cpu().numpy(), G_TRAIN[name + "_labels"])
        x, y, extra = stage_train_batch(*t, p, crop, md if np.isfinite(md) else -1.0, sparsifier="radar", radar_filter=f, extras=True)
        assert np.array_equal(x.cpu().numpy(), G_TRAIN[name + "_inputs"]) and np.array_equal(y.cpu().numpy(), G_TRAIN[name + "_labels"])
        imap = F.index_map(pts[0][0], (H0, W0))
        assert np.array_equal(extra["index_map"].cpu().numpy(), np.stack([F.index_map_train(imap, p, b, crop) for b in range(B)]))
        # modality rgb: three channels, no radar channel to filter, index_map all the same
        x3, _, extra3 = stage_train_batch(t[0], t[1], None, p, crop, -1.0, "rgb", radar_filter=f, extras=True)
        assert x3.shape[1] == 3 and extra3["radar_depth_filtered"] is None and torch.equal(extra3["index_map"], extra["index_map"])


@pytest.mark.parametrize("name,mode", [("val1", "val"), ("tr1", "train")])
def test_with_mask(name, mode):
    """A caller's mask in place of valid_mask (the reference's radar_filtered2): all true is sparsifier radar, all false zeroes every pixel
    whose index names a point of the frame."""
    from radar_depth_amd.dataset import stage_train_batch, stage_val_batch
    img, lidar, radar, pts, p, crop, md, want_in, _, want_im = staged(name)
    f = staged_filter(pts, img.shape[1:3])
    t = gpu(img, lidar, radar)
    call = (lambda **kw: stage_val_batch(*t, crop, md, **kw)) if mode == "val" else (lambda **kw: stage_train_batch(*t, p, crop, md, **kw))
    plain = call()[0]
    keep = call(sparsifier="radar_filtered", radar_filter=f.with_mask(torch.ones_like(f.valid_mask)))[0]
    assert torch.equal(keep, plain)
    none, _, extra = call(sparsifier="radar_filtered", radar_filter=f.with_mask(torch.zeros_like(f.valid_mask, dtype=torch.uint8)), extras=True)
    n = torch.tensor(np.asarray(f.n_radar)).cuda().view(-1, 1, 1, 1)
    indexed = (extra["index_map"] >= 0) & (extra["index_map"] < n)
    assert indexed.any() and (plain[:, 3:4][indexed] != 0).any()
    assert torch.equal(none[:, 3:4], torch.where(indexed, torch.zeros_like(plain[:, 3:4]), plain[:, 3:4])) and torch.equal(none[:, :3], plain[:, :3])
    assert np.array_equal(extra["index_map"].cpu().numpy(), want_im) and f.valid_mask.dtype == torch.bool            # f itself is untouched


def test_side_stream_without_synchronisation():
    """Filter and staging queued back to back on a side stream; the only synchronisation is the one before the comparison."""
    from radar_depth_amd.dataset import stage_train_batch
    img, lidar, radar, pts, p, crop, md, want_in, want_lb, want_im = staged("tr1")
    rxy, rdep, lxy, ldep, nr, nl = pad_batch([(q["rxy"], q["rdep"], q["lxy"], q["ldep"]) for q in pts])
    from radar_depth_amd.dataset import filter_radar_points, prepare_train_params
    side = torch.cuda.Stream()
    host = [torch.from_numpy(np.array(a)).pin_memory() for a in (img, lidar, radar, rxy, rdep, lxy, ldep)]
    with torch.cuda.stream(side):
        dev = [h.to("cuda", non_blocking=True) for h in host]
        prep = prepare_train_params(p, img.shape[1], img.shape[2], crop)
        f = filter_radar_points(*dev[3:], nr, nl, img.shape[1:3])
        x, y, extra = stage_train_batch(*dev[:3], prep, crop, md, sparsifier="radar_filtered", radar_filter=f, extras=True)
    side.synchronize()
    assert np.array_equal(x.cpu().numpy(), want_in) and np.array_equal(y.cpu().numpy(), want_lb)
    assert np.array_equal(extra["index_map"].cpu().numpy(), want_im)

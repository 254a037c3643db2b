"""numpy-only restatement of the reference's radar_filtered sparsifier: ``filter_radar_points_gt`` (dataset/radar_preprocessing.py:77-122)
with the tie rule written out (distance, then the lower lidar index; the reference's argsort is not stable), the index_map scatter of
``nuscenes_dataset_torch.filter_radar_points`` (dataset/nuscenes_dataset_torch_new.py:557-584) and what ``transform_val`` /
``transform_train`` do with index_map and valid_mask (:323-348, :462-486).  tests/golden/make_golden_radar_filter.py asserts that this
file reproduces the reference's own code bit for bit on every golden case, so that the GPU tests can build further cases from it alone.
The geometry comes from staging_train_ref.py; nothing is shared with radar_depth_amd/dataset/staging.py on purpose."""
import numpy as np

import staging_train_ref as R

K = 3


def dist_thresh(depth):
    """sid_dist_thresh: alpha 14, beta 4, K 100."""
    return np.exp(((depth * np.log(4 / 14)) / 100) + np.log(14))


def depth_thresh(depth):
    """sid_depth_thresh: alpha 5, beta 16, K 100."""
    return np.exp(((depth * np.log(16 / 5)) / 100) + np.log(5))


def filter_points(radar_xy, radar_depth, lidar_xy, lidar_depth, with_margin=False):
    """One frame.  radar_xy [R,2], radar_depth [R], lidar_xy [L,2], lidar_depth [L] float64, L >= 3.
    Returns (labels uint8 [R], valid bool [R], topk int32 [R,3]); with_margin adds the smallest relative distance of any decision from
    its threshold and of any two of a point's four smallest distances from each other."""
    radar_xy, lidar_xy = np.asarray(radar_xy, np.float64)[:, :2], np.asarray(lidar_xy, np.float64)[:, :2]
    radar_depth, lidar_depth = np.asarray(radar_depth, np.float64), np.asarray(lidar_depth, np.float64)
    n, m = radar_xy.shape[0], lidar_xy.shape[0]
    assert n == 0 or m >= K, "three neighbours are needed"
    labels, topk = np.zeros(n, np.uint8), np.full((n, K), -1, np.int32)
    margin = np.inf
    if n:
        diff = radar_xy[:, None, :] - lidar_xy[None, :, :]
        dist = np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1])
        order = np.argsort(dist, axis=-1, kind="stable")                 # equal distances: the lower index first
        topk = order[:, :K].astype(np.int32)
        d = np.take_along_axis(dist, order[:, :K], axis=-1)
        dep = lidar_depth[topk]
        thr = dist_thresh(dep)
        count = (d <= thr).sum(axis=-1)                                  # over all three neighbours, not a prefix
        dd = radar_depth[:, None] - dep                                  # signed
        dthr = depth_thresh(dep)
        for i in range(n):
            c = int(count[i])
            passed = int((dd[i, :c] < dthr[i, :c]).sum())                # the FIRST c neighbours
            labels[i] = 2 if c == 0 else (1 if passed >= np.ceil(c / 2) else 0)
            if with_margin:
                margin = min(margin, float((np.abs(d[i] - thr[i]) / thr[i]).min()))
                if c:
                    margin = min(margin, float((np.abs(dd[i, :c] - dthr[i, :c]) / dthr[i, :c]).min()))
        if with_margin:
            four = np.take_along_axis(dist, order[:, :K + 1], axis=-1)
            gaps = np.diff(four, axis=-1) / np.maximum(four[:, 1:], np.finfo(np.float64).tiny)
            margin = min(margin, float(gaps.min()))
    out = (labels, labels > 0, topk)
    return out + (margin,) if with_margin else out


def filter_batch(radar_xy, radar_depth, lidar_xy, lidar_depth, n_radar, n_lidar):
    """Padded batch: [B,Rmax,2], [B,Rmax], [B,Lmax,2], [B,Lmax] and the counts.  Rows at or beyond n_radar[b]: label 0, valid False,
    topk -1."""
    B, Rmax = radar_depth.shape
    labels, valid, topk = np.zeros((B, Rmax), np.uint8), np.zeros((B, Rmax), bool), np.full((B, Rmax, K), -1, np.int32)
    for b in range(B):
        nr, nl = int(n_radar[b]), int(n_lidar[b])
        labels[b, :nr], valid[b, :nr], topk[b, :nr] = filter_points(radar_xy[b, :nr], radar_depth[b, :nr], lidar_xy[b, :nl], lidar_depth[b, :nl])
    return labels, valid, topk


def index_map(radar_xy, frame_shape):
    """int32 [H0,W0]: -1, then point i at (int(y), int(x)) in ascending i (the last one stays); a point outside the frame is skipped."""
    H0, W0 = frame_shape
    out = np.full((H0, W0), -1, np.int32)
    xy = np.asarray(radar_xy, np.float64)
    for i in range(xy.shape[0]):
        x, y = xy[i, 0], xy[i, 1]
        if x > -1.0 and x < W0 and y > -1.0 and y < H0:                  # truncation toward zero; False for NaN
            out[int(y), int(x)] = i
    return out


def index_map_val(imap, crop_size):
    H0, W0 = imap.shape
    th, tw = crop_size
    i0, j0 = int(round((H0 - th) / 2.)), int(round((W0 - tw) / 2.))
    return imap[i0:i0 + th, j0:j0 + tw][None].copy()


def index_map_train(imap, p, i, crop_size):
    """index_map of frame i through transform_depth: rotation (order 0, cval 0) -> NEAREST resize -> crop -> flip.  [1,ch,cw]."""
    ch, cw = crop_size
    H0, W0 = imap.shape
    s = float(p["scale"][i])
    rot = R.rotate0(imap.astype(np.int64), R.rotation_coeffs(float(p["angle"][i]), H0, W0))
    a = R.resize_nearest(rot, int(H0 * s), int(W0 * s))
    hs, ws = int(p["h_start"][i]), int(p["w_start"][i])
    a = a[hs:hs + ch, ws:ws + cw]
    return (a[:, ::-1] if bool(p["flip"][i]) else a)[None].astype(np.int32)


def apply_filter(radar_channel, imap_t, valid):
    """radar_channel [ch,cw] float32 (already clamped: zeroing commutes with the clamp), imap_t [1,ch,cw], valid bool [n]."""
    invalid = np.where(~np.asarray(valid, bool))[0]
    out = radar_channel.copy()
    out[np.isin(imap_t[0], invalid)] = 0
    return out


def radar_map_from_points(radar_xy, radar_depth, frame_shape):
    """The int16 radar depth map (metres * 256) a frame's points make: the later point keeps a shared pixel, like index_map."""
    H0, W0 = frame_shape
    out = np.zeros((H0, W0), np.int16)
    for i in range(len(radar_depth)):
        out[int(radar_xy[i, 1]), int(radar_xy[i, 0])] = int(round(float(radar_depth[i]) * 256))
    return out


def stage_val(image, lidar_i16, radar_i16, imaps, valids, crop_size, max_depth=np.inf, filtered=True):
    """transform_val of a batch with sparsifier radar_filtered (or radar): (inputs [B,4,th,tw], labels [B,1,th,tw], index_map [B,1,th,tw])."""
    B, H0, W0 = lidar_i16.shape
    th, tw = crop_size
    i0, j0 = int(round((H0 - th) / 2.)), int(round((W0 - tw) / 2.))
    win = (slice(None), slice(i0, i0 + th), slice(j0, j0 + tw))
    rgb = (image[win].astype(np.float32) / 255.).astype(np.float32).transpose(0, 3, 1, 2)
    radar = (radar_i16[win] / 256.).astype(np.float32)
    radar[radar > np.float32(max_depth)] = 0
    labels = (lidar_i16[win] / 256.).astype(np.float32)[:, None]
    im = np.stack([index_map_val(imaps[b], crop_size) for b in range(B)])
    if filtered:
        radar = np.stack([apply_filter(radar[b], im[b], valids[b]) for b in range(B)])
    return np.concatenate((rgb, radar[:, None]), 1), labels, im


def stage_train(image, lidar_i16, radar_i16, p, imaps, valids, crop_size, max_depth=np.inf, filtered=True):
    """transform_train of a batch with sparsifier radar_filtered (or radar)."""
    inputs, labels = R.transform_train_batch(image, lidar_i16, radar_i16, p, crop_size, max_depth)
    B = image.shape[0]
    im = np.stack([index_map_train(imaps[b], p, b, crop_size) for b in range(B)])
    if filtered:
        for b in range(B):
            inputs[b, 3] = apply_filter(inputs[b, 3], im[b], valids[b])
    return inputs, labels, im

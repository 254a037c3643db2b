"""Input staging from the exported frames on the GPU.

Mirrors the deterministic part of the reference's DataLoader worker -- ``nuscenes_dataset_torch.get_data``'s depth decompression
(dataset/nuscenes_dataset_torch_new.py:191-195) and ``transform_val`` for ``modality="rgbd", sparsifier="radar"``
(same file :415-455, :503-512) -- for a whole batch in one kernel launch (``rd_stage_frames``): the uint8 / int16 arrays of the
.h5 frames go to the device as they are (7 bytes per pixel instead of 20) and come out as the network's ``inputs`` [B,4,H,W] and
``labels`` [B,1,H,W].  Decoding the .h5 container itself needs h5py, which this environment does not have; the boundary is
therefore the decoded arrays (``np.array(f[key])``, :186-188).  There is no CPU fallback.

The second half of the file is the training input: ``transform_train`` (same file :237-412) with its random rotation, scale, crop,
flip and colour jitter, bit-identical for the same draws (``draw_train_params``, ``stage_train_batch``; ``rd_stage_frames_train``).

Between the two sits the ``radar_filtered`` sparsifier: ``filter_radar_points`` restates what the reference's ``__getitem__`` does to
every frame (same file :557-584 and ``filter_radar_points_gt``, dataset/radar_preprocessing.py:77-122) for a padded batch of radar and
lidar points -- per-point labels, ``valid_mask``, the dense ``index_map`` -- and both staging calls take its result
(``sparsifier="radar_filtered", radar_filter=..., extras=...``): ``index_map`` follows the depth maps through the transform and the radar
returns the filter rejected are zeroed, equal to the reference's output for the same frames, points and draws
(``rd_radar_filter_points``, ``rd_radar_index_map``, ``rd_stage_index_filter_val`` / ``_train``).  ``uniform`` and ``lidar_radar`` stay out
of the staging calls' scope: they work on the staged planes and live in dense_to_sparse.py (``uniform_sparse_depth``,
``lidar_radar_sparse_depth``)."""
import ctypes as C
import math

import numpy as np
import torch

from .._lib import RdStageTrainFrame, check, current_stream, lib, ptr


def center_crop_params(h, w, size):
    """(i, j, th, tw) exactly as ``CenterCrop.get_params`` computes them (dataset/transforms.py:347-365; Python's round)."""
    th, tw = size
    return int(round((h - th) / 2.)), int(round((w - tw) / 2.)), th, tw


# ------------------------------------------------------------------------------------------------ the radar_filtered sparsifier
# The reference's __getitem__ runs filter_radar_points on every frame (:557-584, :638): it scatters the radar points into a dense
# index_map, labels every radar point against the lidar ground truth (filter_radar_points_gt, dataset/radar_preprocessing.py:77-122)
# and keeps valid_mask; transform_val / transform_train carry index_map through the depth maps' transform and, for
# sparsifier="radar_filtered", zero the radar pixels whose index names a rejected point.  Here: filter_radar_points for a padded batch
# of point sets (rd_radar_filter_points, rd_radar_index_map), then one launch behind rd_stage_frames / rd_stage_frames_train
# (rd_stage_index_filter_val / _train).  Quirks kept: the distance count is over all three neighbours while the depth test looks at
# the first ``count`` of them; the depth difference is signed; where the training rotation samples outside the frame index_map is 0
# (scipy's cval), which names point 0.  Differences: index_map is int32 (the reference: an int64 array that its ToTensor hands out as
# float32); a point whose truncated pixel lies
# outside the frame is skipped (the reference wraps a negative index around and raises IndexError beyond the frame); one radar point
# is labelled like any other count (the reference's np.squeeze breaks there).
_FILTER_THRESHOLDS = np.array([np.log(4 / 14), np.log(14), np.log(16 / 5), np.log(5)], dtype=np.float64)      # sid_dist_thresh, sid_depth_thresh


def _counts(n, B, what):
    a = np.ascontiguousarray(np.asarray(n.cpu() if torch.is_tensor(n) else n).reshape(-1), dtype=np.int32)
    if a.shape[0] != B:
        raise ValueError("%s: %d counts for %d frames" % (what, a.shape[0], B))
    return a


class RadarFilter:
    """What ``filter_radar_points`` keeps of a batch: index_map int32 [B,H0,W0] (-1 where no point falls), valid_mask bool [B,Rmax],
    valid_labels uint8 [B,Rmax] (0 invalid, 1 valid, 2 unknown: no lidar point near), topk int32 [B,Rmax,3] (the neighbours by
    distance, then index) on the GPU, and the host counts n_radar [B].  Rows at or beyond n_radar[b] hold 0 / False / -1."""

    def __init__(self, index_map, valid_mask, valid_labels, topk, n_radar):
        self.index_map, self.valid_mask, self.valid_labels, self.topk, self.n_radar = index_map, valid_mask, valid_labels, topk, n_radar

    def __iter__(self):
        return iter((self.index_map, self.valid_mask, self.valid_labels, self.topk, self.n_radar))

    def with_mask(self, mask):
        """The same frames with a caller's per-point mask [B,Rmax] (truthy = keep) in place of valid_mask: the reference's
        ``radar_filtered2`` (``pred_labels``) is nothing else."""
        assert torch.is_tensor(mask) and mask.is_cuda and tuple(mask.shape) == tuple(self.valid_mask.shape), "mask: [B,Rmax] on the GPU"
        return RadarFilter(self.index_map, mask.to(torch.bool).contiguous(), self.valid_labels, self.topk, self.n_radar)


def filter_radar_points(radar_points, radar_depth_points, lidar_points, lidar_depth_points, n_radar, n_lidar, frame_shape):
    """The reference's per-frame ``filter_radar_points`` for a batch.  radar_points [B,Rmax,2] (x, y in pixels; a third column is
    ignored), radar_depth_points [B,Rmax], lidar_points [B,Lmax,2 or 3], lidar_depth_points [B,Lmax]: padded GPU tensors, cast to
    float64 if they are not; n_radar / n_lidar: the B host counts; frame_shape (H0, W0).  The padding is never read.  Returns a
    ``RadarFilter``.  Everything is queued on the current stream; nothing synchronises with the host."""
    pts = []
    for t, what in ((radar_points, "radar_points"), (lidar_points, "lidar_points")):
        assert torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.shape[-1] in (2, 3), what + ": [B,N,2] or [B,N,3] on the GPU"
        pts.append(t[..., :2].to(torch.float64).contiguous())
    rxy, lxy = pts
    B, Rmax, Lmax = rxy.shape[0], rxy.shape[1], lxy.shape[1]
    assert lxy.shape[0] == B, "lidar_points: another batch size"
    deps = []
    for t, n, what in ((radar_depth_points, Rmax, "radar_depth_points"), (lidar_depth_points, Lmax, "lidar_depth_points")):
        assert torch.is_tensor(t) and t.is_cuda and tuple(t.shape) == (B, n), what + ": [B,N] on the GPU, padded like its points"
        deps.append(t.to(torch.float64).contiguous())
    rdep, ldep = deps
    nr, nl = _counts(n_radar, B, "n_radar"), _counts(n_lidar, B, "n_lidar")
    H0, W0 = (int(v) for v in frame_shape)
    dev = rxy.device
    labels = torch.empty(B, Rmax, dtype=torch.uint8, device=dev)
    valid = torch.empty(B, Rmax, dtype=torch.uint8, device=dev)
    topk = torch.empty(B, Rmax, 3, dtype=torch.int32, device=dev)
    index_map = torch.empty(B, H0, W0, dtype=torch.int32, device=dev)
    L, host = lib(), lambda a: C.c_void_p(a.ctypes.data)
    check(L.rd_radar_filter_points(ptr(rxy), ptr(rdep), ptr(lxy), ptr(ldep), host(nr), host(nl), B, Rmax, Lmax, host(_FILTER_THRESHOLDS),
                                   ptr(labels), ptr(valid), ptr(topk), current_stream()), "rd_radar_filter_points")
    check(L.rd_radar_index_map(ptr(rxy), host(nr), B, Rmax, H0, W0, ptr(index_map), current_stream()), "rd_radar_index_map")
    return RadarFilter(index_map, valid.view(torch.bool), labels, topk, nr)


def _check_sparsifier(sparsifier, modality, radar_filter, extras):
    """Whether the radar channel is to be filtered; raises what the reference raises for what it cannot feed either."""
    if sparsifier in ("uniform", "lidar_radar"):
        raise NotImplementedError("sparsifier %r is out of the staging's scope (staged are radar and radar_filtered): stage with "
                                  "sparsifier='radar' and max_depth=inf, then call radar_depth_amd.dataset.uniform_sparse_depth / "
                                  "lidar_radar_sparse_depth with out=inputs[:, 3:4]" % sparsifier)
    if sparsifier == "radar_filtered2":
        raise NotImplementedError("[Error] The filtering method using point classifier is not supported in the released code.  Pass the "
                                  "classifier's per-point mask as radar_filter.with_mask(mask) with sparsifier='radar_filtered'.")
    if sparsifier not in ("radar", "radar_filtered"):
        raise ValueError("[Error] Invalid sparsifier.")
    if sparsifier == "radar_filtered":
        if modality == "rgb":
            raise ValueError("sparsifier 'radar_filtered' needs modality 'rgbd': modality 'rgb' has no radar channel to filter")
        if radar_filter is None:
            raise ValueError("sparsifier 'radar_filtered' needs radar_filter=filter_radar_points(...)")
    if extras and radar_filter is None:
        raise ValueError("extras=True needs radar_filter=filter_radar_points(...): index_map comes from it")
    if radar_filter is not None and not isinstance(radar_filter, RadarFilter):
        raise ValueError("radar_filter: a RadarFilter (filter_radar_points)")
    return sparsifier == "radar_filtered"


def _filter_geometry(radar_filter, B, H0, W0, dev):
    f = radar_filter
    assert tuple(f.index_map.shape) == (B, H0, W0) and f.index_map.dtype == torch.int32 and f.index_map.device == dev, \
        "radar_filter was made for another batch or frame size"
    assert f.valid_mask.dtype == torch.bool and f.valid_mask.dim() == 2 and f.valid_mask.shape[0] == B and len(f.n_radar) == B
    return f.index_map.contiguous(), f.valid_mask.contiguous(), f.valid_mask.shape[1]


def _with_extras(inputs, labels, index_map, extras):
    """(inputs, labels), plus the reference's extra keys when asked for (radar_depth_filtered is a view of inputs' radar channel)."""
    if not extras:
        return inputs, labels
    return inputs, labels, {"index_map": index_map, "radar_depth_filtered": inputs[:, 3:4] if inputs.shape[1] == 4 else None}


def stage_val_batch(image_u8, lidar_i16, radar_i16, crop_size=(450, 800), max_depth=float("inf"), sparsifier="radar", radar_filter=None,
                    extras=False):
    """image_u8 [B,H0,W0,3] uint8, lidar_i16 / radar_i16 [B,H0,W0] int16 (metres * 256), all on the GPU.
    Returns (inputs [B,4,th,tw], labels [B,1,th,tw]) fp32, like ``output_dict["inputs"], output_dict["labels"]`` stacked over
    the batch.  max_depth < 0 means no clamp, as in main.py:71.
    sparsifier "radar_filtered" needs ``radar_filter`` (``filter_radar_points`` of the same frames): channel 3 of inputs is then the
    filtered, clamped radar depth.  extras=True (with a radar_filter, whatever the sparsifier: the reference emits index_map for all)
    adds a third value {"index_map": int32 [B,1,th,tw] (the reference: int64, float32 after its ToTensor), "radar_depth_filtered": view of
    inputs[:, 3:4]}."""
    apply = _check_sparsifier(sparsifier, "rgbd", radar_filter, extras)
    assert image_u8.is_cuda and image_u8.dtype == torch.uint8 and image_u8.dim() == 4 and image_u8.shape[-1] == 3, "image: uint8 [B,H,W,3] on the GPU"
    B, H0, W0, _ = image_u8.shape
    for t in (lidar_i16, radar_i16):
        assert t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (B, H0, W0), "depth maps: int16 [B,H,W] on the GPU"
    image_u8, lidar_i16, radar_i16 = image_u8.contiguous(), lidar_i16.contiguous(), radar_i16.contiguous()
    i0, j0, th, tw = center_crop_params(H0, W0, crop_size)
    md = float("inf") if max_depth < 0.0 else float(max_depth)
    inputs = torch.empty(B, 4, th, tw, dtype=torch.float32, device=image_u8.device)
    labels = torch.empty(B, 1, th, tw, dtype=torch.float32, device=image_u8.device)
    check(lib().rd_stage_frames(ptr(image_u8), ptr(lidar_i16), ptr(radar_i16), B, H0, W0, i0, j0, th, tw, md,
                                ptr(inputs), ptr(labels), current_stream()), "rd_stage_frames")
    index_map = None
    if apply or extras:
        src, valid, Rmax = _filter_geometry(radar_filter, B, H0, W0, image_u8.device)
        index_map = torch.empty(B, 1, th, tw, dtype=torch.int32, device=image_u8.device)
        check(lib().rd_stage_index_filter_val(ptr(src), ptr(valid), C.c_void_p(radar_filter.n_radar.ctypes.data), B, Rmax, H0, W0, i0, j0, th, tw,
                                              int(apply), ptr(inputs), ptr(index_map), current_stream()), "rd_stage_index_filter_val")
    return _with_extras(inputs, labels, index_map, extras)


# ------------------------------------------------------------------------------------------------ training input (transform_train)
# The reference's transform_train (dataset/nuscenes_dataset_torch_new.py:237-412) for transform_mode "sparse-to-dense", sparsifier
# "radar": random rotation, scale, crop, flip and colour jitter.  The host draws the parameters and builds the small per-frame tables
# that depend only on (frame size, scale); every pixel is computed on the GPU by rd_stage_frames_train (csrc/staging_train.hip).

_SINCOF = (1.58962301572218447952E-10, -2.50507477628503540135E-8, 2.75573136213856773549E-6, -1.98412698295895384658E-4,
           8.33333333332211858862E-3, -1.66666666666666307295E-1)
_COSCOF = (1.13678171382044553091E-11, -2.08758833757683644217E-9, 2.75573155429816611547E-7, -2.48015872936186303776E-5,
           1.38888888888806666760E-3, -4.16666666666666348141E-2, 4.99999999999999999798E-1)


def _polevl(x, coef):
    ans = coef[0]
    for c in coef[1:]:
        ans = ans * x + c
    return ans


def cos_sin_degrees(angle):
    """(scipy.special.cosdg(angle), scipy.special.sindg(angle)) -- the Cephes routines scipy.ndimage.rotate builds its matrix from
    -- without scipy, for a scalar or an array: reduction to an octant in degrees, then the sine or cosine polynomial on the
    remainder in radians.  Element-wise float64 numpy arithmetic rounds like the C code's doubles."""
    a = np.asarray(angle, dtype=np.float64)
    x = np.abs(a)
    y = np.floor(x / 45.0)
    j = (y - np.ldexp(np.floor(np.ldexp(y, -4)), 4)).astype(np.int64)
    odd = (j & 1) == 1
    j, y = (j + odd) & 7, y + odd
    upper = j > 3
    j = np.where(upper, j - 4, j)
    z = (x - y * 45.0) * 1.74532925199432957692E-2
    zz = z * z
    cos_poly, sin_poly = 1.0 - zz * _polevl(zz, _COSCOF), z + z * (zz * _polevl(zz, _SINCOF))
    mid = (j == 1) | (j == 2)
    c = np.where(upper != (j > 1), -1.0, 1.0) * np.where(mid, sin_poly, cos_poly)
    s = np.where(upper != (a < 0), -1.0, 1.0) * np.where(mid, cos_poly, sin_poly)
    return (float(c), float(s)) if a.ndim == 0 else (c, s)


def rotation_coefficients(angle, h, w):
    """(m00, m01, off0, m10, m11, off1) of ``scipy.ndimage.rotate(img, angle, reshape=False)``: the source coordinate of output
    pixel (y, x) is (y*m00 + x*m01 + off0, y*m10 + x*m11 + off1)."""
    c, s = cos_sin_degrees(float(angle))
    m = np.array([[c, s], [-s, c]])
    centre = (np.array([h, w]) - 1) / 2
    off = centre - m @ centre             # scipy's own expression: numpy's matmul may fuse the two products, so it is kept as is
    return c, s, float(off[0]), -s, c, float(off[1])


def _nearest_window(in_size, out, start, length):
    """Source index of output indices start[i] .. start[i]+length of Pillow's NEAREST resize in_size -> out[i], one row per frame:
    the coordinate starts at a/2 and grows by repeated addition of a = in/out in float64 (np.cumsum along a row is that sequential
    sum; floor((x + 0.5) * a) is not the same thing)."""
    a = in_size / out.astype(np.float64)
    steps = np.repeat(a[:, None], int(start.max()) + length, axis=1)
    steps[:, 0] = a * 0.5
    xo = np.take_along_axis(np.cumsum(steps, axis=1), start[:, None] + np.arange(length)[None, :], axis=1)
    return np.minimum(xo.astype(np.int64), in_size - 1).astype(np.int32)


def _bilinear_window(in_size, out, start, length):
    """[n, length, 4] int32 = (first source index, k0, k1, 0) for output indices start[i] .. start[i]+length: Pillow's BILINEAR
    coefficients for 8-bit data (Resample.c precompute_coeffs + normalize_coeffs_8bpc, 22 fraction bits) when out >= in: the
    filter's support is then one source pixel and no output has more than two taps.
    out[x] = clip((2^21 + in[i]*k0 + in[i+1]*k1) >> 22)."""
    assert (out >= in_size).all(), "bilinear table: enlarging only (scale >= 1)"
    scale = in_size / out.astype(np.float64)
    c = ((start[:, None] + np.arange(length)[None, :]) + 0.5) * scale[:, None]
    lo = np.maximum((c - 1.0 + 0.5).astype(np.int64), 0)
    hi = np.minimum((c + 1.0 + 0.5).astype(np.int64), in_size)
    assert int((hi - lo).max()) <= 2
    w0, w1 = np.abs(lo - c + 0.5), np.abs(1 + lo - c + 0.5)
    w0 = np.where(w0 < 1.0, 1.0 - w0, 0.0)
    w1 = np.where((w1 < 1.0) & (hi - lo > 1), 1.0 - w1, 0.0)
    ww = w0 + w1
    one = np.where(ww == 0.0, 1.0, ww)
    w0, w1 = np.where(ww != 0.0, w0 / one, w0), np.where(ww != 0.0, w1 / one, w1)
    k0, k1 = (0.5 + w0 * float(1 << 22)).astype(np.int64), (0.5 + w1 * float(1 << 22)).astype(np.int64)
    return np.stack((lo, k0, k1, np.zeros_like(lo)), axis=2).astype(np.int32)


def nearest_table(in_size, out_size):
    """The whole NEAREST table of one (in, out) pair, [out]."""
    return _nearest_window(in_size, np.array([out_size]), np.array([0]), out_size)[0]


def bilinear_table(in_size, out_size):
    """The whole BILINEAR table of one (in, out) pair, [out, 4]."""
    return _bilinear_window(in_size, np.array([out_size]), np.array([0]), out_size)[0]


def draw_train_params(n, crop_size=(450, 800), scale_range=(1.0, 1.5), rotation=5.0, jitter=(0.2, 0.2, 0.2), rng=None):
    """The random parameters of n frames, drawn in the reference's order (transform_train :247-249, :281-282, then
    ColorJitter.get_params, dataset/transforms.py:450-477) from ``rng`` -- a ``np.random.RandomState``, or the global ``np.random``
    the reference itself uses -- so that a worker seeded like the reference's augments identically.  Returns a dict of arrays:
    scale, angle (degrees), flip, h_start, w_start, factors [n,3] (brightness, contrast, saturation) and order [n,3] (the enhancer
    applied first, second, third).  The crop bounds come from the crop size, not from the frame size, as in the reference."""
    rng = np.random if rng is None else rng
    ch, cw = crop_size
    p = dict(scale=np.zeros(n), angle=np.zeros(n), flip=np.zeros(n, dtype=bool), h_start=np.zeros(n, dtype=np.int64),
             w_start=np.zeros(n, dtype=np.int64), factors=np.zeros((n, 3)), order=np.zeros((n, 3), dtype=np.int64))
    for i in range(n):
        s = rng.uniform(scale_range[0], scale_range[1])
        p["scale"][i] = s
        p["angle"][i] = rng.uniform(-rotation, rotation)
        p["flip"][i] = rng.uniform(0.0, 1.0) < 0.5
        p["h_start"][i] = round(rng.uniform(0, math.floor(ch * s) - ch))
        p["w_start"][i] = round(rng.uniform(0, math.floor(cw * s) - cw))
        p["factors"][i] = [rng.uniform(max(0, 1 - j), 1 + j) for j in jitter]
        order = [0, 1, 2]
        rng.shuffle(order)
        p["order"][i] = order
    return p


FRAME_DTYPE = np.dtype(RdStageTrainFrame)


def train_frame_records(params, h0, w0):
    """The ``RdStageTrainFrame`` records of ``params`` (draw_train_params' dict) for h0 x w0 frames, as a structured array."""
    n = len(params["scale"])
    recs = np.zeros(n, dtype=FRAME_DTYPE)
    c, s = cos_sin_degrees(np.asarray(params["angle"], dtype=np.float64).reshape(n))
    centre = (np.array([h0, w0]) - 1) / 2
    for i in range(n):                    # scipy's own expression per frame: numpy's matmul may fuse the two products
        off = centre - np.array([[c[i], s[i]], [-s[i], c[i]]]) @ centre
        recs["rot"][i] = (c[i], s[i], off[0], -s[i], c[i], off[1])
    recs["scale"] = params["scale"]
    recs["factor"] = np.asarray(params["factors"]).astype(np.float32)          # Image.blend takes a C float
    recs["order"] = params["order"]
    recs["h_start"], recs["w_start"], recs["flip"] = params["h_start"], params["w_start"], np.asarray(params["flip"]).astype(bool)
    return recs


def train_tables(params, h0, w0, crop_size):
    """(near_y [B,ch], near_x [B,cw], bil_y [B,ch,4], bil_x [B,cw,4]) int32: the resize tables of every frame's crop window, all
    frames at once.  A frame rd_stage_frames_train is going to reject (scale below 1, window outside the resized frame) gets the
    identity tables."""
    ch, cw = crop_size
    s = np.asarray(params["scale"], dtype=np.float64)
    oh, ow = (h0 * s).astype(np.int64), (w0 * s).astype(np.int64)         # imresize: (np.array(im.size) * scale).astype(int)
    hs, ws = np.asarray(params["h_start"]).astype(np.int64), np.asarray(params["w_start"]).astype(np.int64)
    bad = ~((s >= 1.0) & (s <= 64.0) & (hs >= 0) & (ws >= 0) & (hs + ch <= oh) & (ws + cw <= ow))
    oh, ow, hs, ws = np.where(bad, max(h0, ch), oh), np.where(bad, max(w0, cw), ow), np.where(bad, 0, hs), np.where(bad, 0, ws)
    return (_nearest_window(h0, oh, hs, ch), _nearest_window(w0, ow, ws, cw), _bilinear_window(h0, oh, hs, ch), _bilinear_window(w0, ow, ws, cw))


class PreparedTrainParams:
    """Host records and device tables of one batch's parameters (prepare_train_params): everything stage_train_batch needs from
    the host, so that a loader thread can build the next batch's while the GPU works."""

    def __init__(self, records, tables, offsets, frame_shape, crop_size):
        self.records, self.tables, self.offsets, self.frame_shape, self.crop_size = records, tables, offsets, frame_shape, crop_size


def prepare_train_params(params, h0, w0, crop_size=(450, 800), device="cuda"):
    """Frame records + resize tables of ``params`` for h0 x w0 frames; the tables go up in one asynchronous copy from pinned memory
    on the current stream (near_y | near_x | bil_y | bil_x, the bilinear tables on 16-byte boundaries)."""
    recs = train_frame_records(params, h0, w0)
    tabs = train_tables(params, h0, w0, crop_size)
    off, total = [], 0
    for t in tabs:
        off.append(total)
        total += (t.size + 3) // 4 * 4
    host = torch.empty(max(total, 4), dtype=torch.int32, pin_memory=True)
    view = host.numpy()
    for o, t in zip(off, tabs):
        view[o:o + t.size] = t.reshape(-1)
    return PreparedTrainParams(recs, host.to(device, non_blocking=True), off, (h0, w0), tuple(crop_size))


def stage_train_batch(image_u8, lidar_i16, radar_i16, params, crop_size=(450, 800), max_depth=float("inf"), modality="rgbd", sparsifier="radar",
                      radar_filter=None, extras=False):
    """The reference's ``transform_train`` for a whole batch on the GPU, bit-identical to it for the same draws.
    image_u8 [B,H0,W0,3] uint8, lidar_i16 / radar_i16 [B,H0,W0] int16 (metres * 256) on the GPU as for ``stage_val_batch``; ``params``
    from ``draw_train_params(B, crop_size, ...)``, or what ``prepare_train_params`` made of them ahead of time.  Returns
    (inputs [B,4,ch,cw], labels [B,1,ch,cw]) fp32; with modality "rgb" the radar argument may be None and inputs is [B,3,ch,cw].  max_depth < 0 means no clamp, as in main.py:71.  Everything is queued on
    the current stream; nothing synchronises with the host.
    sparsifier / radar_filter / extras as for ``stage_val_batch``: with "radar_filtered" (modality rgbd only) channel 3 is the filtered,
    clamped radar depth; index_map goes through the depth maps' rotation, NEAREST resize, crop and flip, with 0 (the rotation's cval, not
    -1) where the rotation samples outside the frame."""
    assert modality in ("rgbd", "rgb"), "modality: rgbd or rgb"
    apply = _check_sparsifier(sparsifier, modality, radar_filter, extras)
    assert image_u8.is_cuda and image_u8.dtype == torch.uint8 and image_u8.dim() == 4 and image_u8.shape[-1] == 3, "image: uint8 [B,H,W,3] on the GPU"
    B, H0, W0, _ = image_u8.shape
    depth = (lidar_i16,) if modality == "rgb" and radar_i16 is None else (lidar_i16, radar_i16)
    for t in depth:
        assert t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (B, H0, W0), "depth maps: int16 [B,H,W] on the GPU"
    image_u8, lidar_i16 = image_u8.contiguous(), lidar_i16.contiguous()
    radar_i16 = None if modality == "rgb" else radar_i16.contiguous()
    ch, cw = crop_size
    dev = image_u8.device
    md = float("inf") if max_depth < 0.0 else float(max_depth)
    prep = params if isinstance(params, PreparedTrainParams) else prepare_train_params(params, H0, W0, crop_size, dev)
    assert prep.frame_shape == (H0, W0) and prep.crop_size == (ch, cw) and len(prep.records) == B, "params were prepared for another geometry"
    cin = 3 if modality == "rgb" else 4
    inputs = torch.empty(B, cin, ch, cw, dtype=torch.float32, device=dev)
    labels = torch.empty(B, 1, ch, cw, dtype=torch.float32, device=dev)
    L = lib()
    # (a crop that does not fit gives a negative size here; rd_stage_frames_train then reports it)
    work = torch.empty(max(int(L.rd_stage_train_workspace_bytes(B, H0, W0, ch, cw)), 16), dtype=torch.uint8, device=dev)
    base = prep.tables.data_ptr()
    check(L.rd_stage_frames_train(ptr(image_u8), ptr(lidar_i16), ptr(radar_i16), B, H0, W0, ch, cw, C.c_void_p(prep.records.ctypes.data),
                                  *[C.c_void_p(base + 4 * o) for o in prep.offsets], ptr(work), md, 1 if modality == "rgb" else 0,
                                  ptr(inputs), ptr(labels), current_stream()), "rd_stage_frames_train")
    index_map = None
    if apply or extras:
        src, valid, Rmax = _filter_geometry(radar_filter, B, H0, W0, dev)
        index_map = torch.empty(B, 1, ch, cw, dtype=torch.int32, device=dev)
        check(L.rd_stage_index_filter_train(ptr(src), ptr(valid), C.c_void_p(radar_filter.n_radar.ctypes.data), B, Rmax, H0, W0, ch, cw,
                                            C.c_void_p(prep.records.ctypes.data), C.c_void_p(base + 4 * prep.offsets[0]),
                                            C.c_void_p(base + 4 * prep.offsets[1]), int(apply), ptr(inputs) if apply else None, ptr(index_map),
                                            current_stream()), "rd_stage_index_filter_train")
    return _with_extras(inputs, labels, index_map, extras)

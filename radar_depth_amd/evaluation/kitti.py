"""The KITTI depth devkit's evaluation on the GPU (csrc/kitti_eval.hip; the reference: misc/devkit/cpp).

A depth plane is float32; a pixel is valid when ``d >= 0`` and invalid pixels hold ``-1`` (NaN is invalid, ``0.0`` is valid), as in the
devkit's ``DepthImage``.  This project's targets hold ``0`` for "no measurement": every function that takes a ground truth has
``zero_invalid``; with it ``gt > 0`` is the validity test.

    decode_depth / encode_depth     readDepthMap / writeDepthMap (uint16 <-> float32, ``/ 256``)
    interpolate_background          interpolateBackground (the hole filling the devkit applies to a prediction before scoring it)
    depth_errors                    depthError: float64 [B,10] = the nine errors in the devkit's order, then the valid-pixel count
    error_image                     errorImage(D_gt, true): uint8 RGB
    KittiDepthMeter                 statMean / statMin / statMax over frames, kept on the device
    evaluate_dirs                   the devkit's ``eval`` over two directories of 16-bit PNGs

Nothing here synchronises with the host except ``KittiDepthMeter.stats`` (one readback) and ``evaluate_dirs`` (files).  There is no
fallback: without the HIP library every call raises.
"""
import ctypes
import json
import os

import numpy as np
import torch

from .._lib import check, current_stream, lib, ptr

METRICS = ("mae", "rmse", "inverse mae", "inverse rmse", "log mae", "log rmse", "scale invariant log", "abs relative",
           "squared relative")
_TABLE_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kitti_log_colormap.json")
_table = []


def log_colormap():
    """float32 [10,5] numpy array: lo, hi, R, G, B of the devkit's ten logarithmic error bins (lo <= n_err < hi)."""
    if not _table:
        with open(_TABLE_PATH) as fh:
            t = np.array(json.load(fh)["rows"], dtype=np.float32)
        assert t.shape == (10, 5), "kitti_log_colormap.json: ten rows of lo, hi, r, g, b"
        _table.append(t)
    return _table[0]


def _planes(t, dtype, what):
    """[H,W] or [B,1,H,W] of `dtype` on the GPU, every frame contiguous, any frame stride -> (tensor as [B,1,H,W], stride in elements,
    whether the batch axis was added)."""
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == dtype, "%s: a %s tensor on the GPU" % (what, dtype)
    squeeze = t.dim() == 2
    if squeeze:
        t = t.reshape((1, 1) + tuple(t.shape))
    assert t.dim() == 4 and t.shape[1] == 1 and t.numel() > 0, what + ": [H,W] or [B,1,H,W]"
    B, _, h, w = t.shape
    assert (w == 1 or t.stride(3) == 1) and (h == 1 or t.stride(2) == w), what + ": every frame must be contiguous"
    return t, (t.stride(0) if B > 1 else h * w), squeeze


def _workspace(B, h, w, dev):
    # (sizes the library rejects give a negative size here; the call that follows reports it)
    return torch.empty(max(int(lib().rd_kitti_workspace_bytes(B, h, w)), 16), dtype=torch.uint8, device=dev)


def decode_depth(u16):
    """uint16 [H,W] or [B,1,H,W] (a KITTI depth PNG's samples) -> float32 depth of the same shape: 0 -> -1, v -> v / 256."""
    t, stride, _ = _planes(u16, torch.uint16, "u16")
    out = torch.empty(tuple(t.shape), dtype=torch.float32, device=t.device)
    B, _, h, w = t.shape
    check(lib().rd_kitti_decode(ptr(t), stride, ptr(out), h * w, B, h, w, current_stream()), "rd_kitti_decode")
    return out.reshape(u16.shape)


def encode_depth(depth):
    """float32 depth -> uint16 of the same shape: valid d -> trunc(max(d * 256, 1)) (saturating at 65535), invalid -> 0."""
    t, stride, _ = _planes(depth, torch.float32, "depth")
    out = torch.empty(tuple(t.shape), dtype=torch.uint16, device=t.device)
    B, _, h, w = t.shape
    check(lib().rd_kitti_encode(ptr(t), stride, ptr(out), h * w, B, h, w, current_stream()), "rd_kitti_encode")
    return out.reshape(depth.shape)


def interpolate_background(depth, out=None):
    """The devkit's hole filling.  ``out``: a tensor like ``depth`` to fill (``depth`` itself fills in place); a new one otherwise."""
    t, stride, _ = _planes(depth, torch.float32, "depth")
    if out is None:
        out = torch.empty(tuple(depth.shape), dtype=torch.float32, device=depth.device)
    assert torch.is_tensor(out) and tuple(out.shape) == tuple(depth.shape) and out.device == depth.device, "out: like depth"
    o, ostride, _ = _planes(out, torch.float32, "out")
    B, _, h, w = t.shape
    ws = _workspace(B, h, w, t.device)
    check(lib().rd_kitti_interpolate(ptr(t), stride, ptr(o), ostride, B, h, w, ptr(ws), current_stream()), "rd_kitti_interpolate")
    return out


def _pair(gt, pred):
    g, gs, squeeze = _planes(gt, torch.float32, "gt")
    p, ps, _ = _planes(pred, torch.float32, "pred")
    assert tuple(g.shape) == tuple(p.shape) and g.device == p.device, "gt and pred: one shape, one device"
    return g, gs, p, ps, squeeze


def depth_errors(gt, pred, zero_invalid=False):
    """float64 [B,10] on the device: mae, rmse, inverse mae, inverse rmse, log mae, log rmse, scale invariant log, abs relative,
    squared relative, number of valid ground-truth pixels.  A frame without one gets nine NaNs and a count of 0."""
    g, gs, p, ps, _ = _pair(gt, pred)
    B, _, h, w = g.shape
    out = torch.empty((B, 10), dtype=torch.float64, device=g.device)
    ws = _workspace(B, h, w, g.device)
    check(lib().rd_kitti_errors(ptr(g), gs, ptr(p), ps, B, h, w, int(bool(zero_invalid)), ptr(ws), ptr(out), current_stream()),
          "rd_kitti_errors")
    return out


def error_image(gt, pred, zero_invalid=False, out=None):
    """The devkit's logarithmic error image: uint8 [B,H,W,3], or [H,W,3] for 2-D inputs.  ``out``: such a tensor to render into (rows
    may have any pitch and frames any stride; pixels are packed)."""
    g, gs, p, ps, squeeze = _pair(gt, pred)
    B, _, h, w = g.shape
    shape = (h, w, 3) if squeeze else (B, h, w, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=g.device)
    assert torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == g.device and tuple(out.shape) == shape, \
        "out: uint8 %s on the planes' device" % (shape,)
    o4 = out if out.dim() == 4 else out.unsqueeze(0)
    assert o4.stride(3) == 1 and o4.stride(2) == 3, "out: packed pixels (a row may have any pitch, a frame any stride)"
    pitch = o4.stride(1) if h > 1 else 3 * w
    frame_stride = o4.stride(0) if B > 1 else h * pitch
    table = log_colormap().ctypes.data_as(ctypes.c_void_p)
    check(lib().rd_kitti_error_image(ptr(g), gs, ptr(p), ps, B, h, w, int(bool(zero_invalid)), table, ptr(out), frame_stride, pitch,
                                     current_stream()), "rd_kitti_error_image")
    return out


def format_stats(stats):
    """The text of the devkit's stats_depth.txt for ``{name: (mean, min, max)}``."""
    return "".join("mean %s: %f \nmin  %s: %f \nmax  %s: %f \n" % (n, stats[n][0], n, stats[n][1], n, stats[n][2]) for n in METRICS)


class KittiDepthMeter(object):
    """statMean / statMin / statMax of the nine errors over frames, on the device: per metric a float64 sum, minimum, maximum and
    frame count.  As in the devkit the minimum starts at 1 and the maximum at 0, and a NaN error fails both comparisons but
    poisons the mean."""

    def __init__(self, device=None):
        self.device = torch.device("cuda" if device is None else device)
        self.state = None
        self.reset()

    def reset(self):
        if self.state is None:
            self.state = torch.empty((9, 4), dtype=torch.float64, device=self.device)
        self.state.zero_()
        self.state[:, 1].fill_(1.0)

    def update_errors(self, errors):
        """Fold float64 [B,10] rows as depth_errors returns them."""
        assert torch.is_tensor(errors) and errors.dtype == torch.float64 and errors.dim() == 2 and errors.shape[1] == 10 and \
            errors.is_contiguous() and errors.device == self.state.device, "errors: contiguous float64 [B,10] on the meter's device"
        check(lib().rd_kitti_stats_update(ptr(errors), errors.shape[0], ptr(self.state), current_stream()), "rd_kitti_stats_update")
        return errors

    def update(self, pred, gt, zero_invalid=False, interpolate=True):
        """Score a batch; returns its float64 [B,10] errors (on the device).  ``interpolate``: fill the prediction's holes first, as
        the devkit does (into a copy; ``pred`` is left alone)."""
        if interpolate:
            pred = interpolate_background(pred)
        return self.update_errors(depth_errors(gt, pred, zero_invalid))

    def stats(self):
        """{name: (mean, min, max)} for the devkit's nine names; one readback."""
        s = self.state.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            return {n: (float(s[i, 0] / s[i, 3]), float(s[i, 1]), float(s[i, 2])) for i, n in enumerate(METRICS)}

    def frames(self):
        return int(self.state[0, 3].item())

    def write_stats(self, path):
        with open(path, "w") as fh:
            fh.write(format_stats(self.stats()))


def evaluate_dirs(gt_dir, pred_dir, device=None, batch=16):
    """The devkit's ``eval``: score the ``*.png`` files of ``pred_dir`` against those of ``gt_dir``, paired by sorted (byte) order.
    Writes ``errors_out/<prefix>.txt`` and ``errors_img/<prefix>.png`` for the first twenty frames and ``stats_depth.txt`` into
    ``pred_dir``; returns True.  A count mismatch, no file at all, a ground truth that is not a 16-bit grey PNG, or a pair of
    different sizes returns False.  Frames of equal size are scored in batches."""
    from PIL import Image

    def pngs(d):
        return sorted((f for f in os.listdir(d) if os.path.splitext(f)[1] == ".png" and os.path.isfile(os.path.join(d, f))),
                      key=os.fsencode)

    def read(path, strict):
        try:
            with Image.open(path) as im:
                if strict and (im.format != "PNG" or im.mode not in ("I;16", "I;16B")):
                    return None
                a = np.asarray(im)
        except Exception:
            return None
        if a.ndim != 2:
            return None
        return np.ascontiguousarray(a.astype(np.uint16))

    names_gt, names_pred = pngs(gt_dir), pngs(pred_dir)
    if len(names_gt) != len(names_pred) or not names_gt:
        return False
    dev = torch.device("cuda" if device is None else device)
    meter = KittiDepthMeter(dev)
    os.makedirs(os.path.join(pred_dir, "errors_out"), exist_ok=True)
    os.makedirs(os.path.join(pred_dir, "errors_img"), exist_ok=True)
    rows, images = [], []                                   # detail of the first twenty frames, read back once at the end

    def flush(group):
        if not group:
            return
        g = decode_depth(torch.from_numpy(np.stack([x[1] for x in group])[:, None]).to(dev))
        p = decode_depth(torch.from_numpy(np.stack([x[2] for x in group])[:, None]).to(dev))
        interpolate_background(p, out=p)
        err = meter.update_errors(depth_errors(g, p))
        k = sum(1 for x in group if x[0] < 20)              # frames arrive in order: the detailed ones lead the group
        if k:
            rows.append(([names_gt[x[0]] for x in group[:k]], err[:k]))
            images.append(error_image(g[:k], p[:k]))

    group = []
    for i, (ng, npd) in enumerate(zip(names_gt, names_pred)):
        a, b = read(os.path.join(gt_dir, ng), True), read(os.path.join(pred_dir, npd), False)
        if a is None or b is None or a.shape != b.shape:
            return False
        if group and (group[0][1].shape != a.shape or len(group) >= batch):
            flush(group)
            group = []
        group.append((i, a, b))
    flush(group)
    for (names, err), img in zip(rows, images):
        err, img = err.cpu().numpy(), img.cpu().numpy()
        for j, name in enumerate(names):
            prefix = name[:name.rfind(".")]
            with open(os.path.join(pred_dir, "errors_out", prefix + ".txt"), "w") as fh:
                fh.write("".join("%f " % v for v in err[j, :9]))
            Image.fromarray(img[j], "RGB").save(os.path.join(pred_dir, "errors_img", prefix + ".png"))
    meter.write_stats(os.path.join(pred_dir, "stats_depth.txt"))
    return True

"""numpy-only restatement of the reference's ``transform_train`` (dataset/nuscenes_dataset_torch_new.py:237-412) for
``transform_mode="sparse-to-dense"``, ``sparsifier="radar"``, modality rgbd / rgb: what scipy.ndimage.rotate(order=0), scipy <= 1.2's
``imresize`` (byte scaling + Pillow BILINEAR on 8-bit / NEAREST on 'F' images) and Pillow's ImageEnhance compute, written out so that a
machine without scipy, Pillow or the reference can check the HIP path bit for bit.  tests/golden/make_golden_staging_train.py asserts
that this file reproduces the reference's own method on every golden case; tests/test_staging_train.py compares its pieces against the
live libraries where they import.  Nothing here is shared with radar_depth_amd/dataset/staging.py on purpose."""
import math

import numpy as np

PRECISION_BITS = 22          # Pillow Resample.c: 32 - 8 - 2

_SINCOF = (1.58962301572218447952E-10, -2.50507477628503540135E-8, 2.75573136213856773549E-6, -1.98412698295895384658E-4,
           8.33333333332211858862E-3, -1.66666666666666307295E-1)
_COSCOF = (1.13678171382044553091E-11, -2.08758833757683644217E-9, 2.75573155429816611547E-7, -2.48015872936186303776E-5,
           1.38888888888806666760E-3, -4.16666666666666348141E-2, 4.99999999999999999798E-1)
_PI180 = 1.74532925199432957692E-2


def _polevl(x, coef):
    ans = coef[0]
    for c in coef[1:]:
        ans = ans * x + c
    return ans


def _dg(x, want_cos):
    """cephes sindg / cosdg (what scipy.special.sindg / cosdg run): octant reduction in degrees, then a polynomial."""
    x = float(x)
    sign = 1
    if x < 0:
        x = -x
        if not want_cos:
            sign = -1
    y = math.floor(x / 45.0)
    z = math.floor(math.ldexp(y, -4))
    z = y - math.ldexp(z, 4)
    j = int(z)
    if j & 1:
        j += 1
        y += 1.0
    j &= 7
    if j > 3:
        sign = -sign
        j -= 4
    if want_cos and j > 1:
        sign = -sign
    z = (x - y * 45.0) * _PI180
    zz = z * z
    if (j == 1 or j == 2) != want_cos:
        r = 1.0 - zz * _polevl(zz, _COSCOF)
    else:
        r = z + z * (zz * _polevl(zz, _SINCOF))
    return -r if sign < 0 else r


def sindg(x):
    return _dg(x, False)


def cosdg(x):
    return _dg(x, True)


def draw_params(n, crop_size, scale_range=(1.0, 1.5), rotation=5.0, jitter=(0.2, 0.2, 0.2), rng=None):
    """The reference's draws for n frames, in its order (transform_train :247-249,:281-282; ColorJitter.get_params)."""
    rng = np.random if rng is None else rng
    ch, cw = crop_size
    p = dict(scale=np.zeros(n), angle=np.zeros(n), flip=np.zeros(n, bool), h_start=np.zeros(n, np.int64), w_start=np.zeros(n, np.int64),
             factors=np.zeros((n, 3)), order=np.zeros((n, 3), np.int64))
    for i in range(n):
        s = rng.uniform(scale_range[0], scale_range[1])
        p["scale"][i], p["angle"][i] = s, rng.uniform(-rotation, rotation)
        p["flip"][i] = rng.uniform(0.0, 1.0) < 0.5
        p["h_start"][i] = round(rng.uniform(0, math.floor(ch * s) - ch))
        p["w_start"][i] = round(rng.uniform(0, math.floor(cw * s) - cw))
        p["factors"][i] = [rng.uniform(max(0, 1 - j), 1 + j) for j in jitter]
        order = [0, 1, 2]
        rng.shuffle(order)
        p["order"][i] = order
    return p


def rotation_coeffs(angle, H0, W0):
    """(m00, m01, off0, m10, m11, off1) of scipy.ndimage.rotate(reshape=False): matrix [[c, s], [-s, c]], offset centre - M centre."""
    c, s = cosdg(angle), sindg(angle)
    m = np.array([[c, s], [-s, c]])
    centre = (np.array([H0, W0]) - 1) / 2
    off = centre - m @ centre             # literally scipy's expression (numpy's matmul may fuse the products: not restated by hand)
    return c, s, float(off[0]), -s, c, float(off[1])


def rotate_indices(rc, H0, W0, ys=None, xs=None):
    """Source indices and validity of the order-0 rotation for output rows ys / columns xs (default: the whole frame)."""
    m00, m01, off0, m10, m11, off1 = rc
    y = (np.arange(H0) if ys is None else np.asarray(ys)).astype(np.float64)[:, None]
    x = (np.arange(W0) if xs is None else np.asarray(xs)).astype(np.float64)[None, :]
    cy = (y * m00 + x * m01) + off0
    cx = (y * m10 + x * m11) + off1
    ok = (cy >= 0) & (cy <= H0 - 1) & (cx >= 0) & (cx <= W0 - 1)          # the bound is on the coordinate, not on the index
    iy = np.where(ok, np.floor(cy + 0.5), 0).astype(np.int64)
    ix = np.where(ok, np.floor(cx + 0.5), 0).astype(np.int64)
    return iy, ix, ok


def rotate0(a, rc):
    iy, ix, ok = rotate_indices(rc, a.shape[0], a.shape[1])
    out = a[iy, ix]
    out[~ok] = 0
    return out


def bytescale(d):
    """scipy <= 1.2 bytescale(low=0, high=255) of a float32 array."""
    d = d.astype(np.float32)
    cmin, cmax = d.min(), d.max()
    cs = cmax - cmin
    if cs == 0:
        cs = np.float32(1)
    sc = np.float32(255.0 / float(cs))
    return (np.clip((d - cmin) * sc, np.float32(0), np.float32(255)) + np.float32(0.5)).astype(np.uint8)


def bilinear_coeffs(in_size, out_size):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter: (xmin [out], k [out, ksize] int64, zero padded)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    c = (np.arange(out_size) + 0.5) * scale
    xmin = np.maximum((c - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((c + support + 0.5).astype(np.int64), in_size)
    t = np.arange(ksize)[None, :]
    w = np.abs((t + xmin[:, None] - c[:, None] + 0.5) * ss)
    w = np.where((w < 1.0) & (t < (xmax - xmin)[:, None]), 1.0 - w, 0.0)
    ww = np.zeros(out_size)
    for j in range(ksize):                      # the sequential sum of the C loop
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, (-0.5 + w * (1 << PRECISION_BITS)).astype(np.int64), (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64))
    return xmin, k


def _resample_axis1(img, out_size):
    xmin, k = bilinear_coeffs(img.shape[1], out_size)
    acc = np.full((img.shape[0], out_size) + img.shape[2:], 1 << (PRECISION_BITS - 1), np.int64)
    kx = k.reshape((1,) + k.shape + (1,) * (img.ndim - 2))
    for t in range(k.shape[1]):
        acc += img[:, np.minimum(xmin + t, img.shape[1] - 1)].astype(np.int64) * kx[:, :, t]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_bilinear_u8(img, oh, ow):
    """Pillow Image.resize((ow, oh), BILINEAR) of an 8-bit HWC image: horizontal pass, uint8 intermediate, vertical pass."""
    t = _resample_axis1(img, ow) if ow != img.shape[1] else img
    return np.swapaxes(_resample_axis1(np.swapaxes(t, 0, 1), oh), 0, 1) if oh != img.shape[0] else t


def nearest_table(in_size, out_size):
    """Pillow NEAREST (affine scale path): the source coordinate starts at a/2 and grows by repeated addition of a = in/out."""
    a = in_size / out_size
    steps = np.full(out_size, a)
    steps[0] = a * 0.5
    return np.cumsum(steps).astype(np.int64)


def resize_nearest(d, oh, ow):
    return d[nearest_table(d.shape[0], oh)][:, nearest_table(d.shape[1], ow)]


def luma(img):
    v = img.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, p, f):
    """Pillow Image.blend(d, p, f) on uint8 arrays: float32 arithmetic, product and sum rounded separately."""
    al = np.float32(f)
    d32 = d.astype(np.float32)
    t = d32 + al * (p.astype(np.float32) - d32)
    if 0 <= al <= 1:
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def enhance(img, which, f):
    """ImageEnhance.Brightness (0) / Contrast (1) / Color (2) .enhance(f) of a uint8 HWC image."""
    if which == 0:
        deg = np.zeros_like(img)
    elif which == 1:
        l = luma(img)
        deg = np.full_like(img, int(int(l.astype(np.int64).sum()) / l.size + 0.5))
    else:
        deg = np.repeat(luma(img)[..., None], 3, axis=2)
    return blend(deg, img, f)


def transform_train_frame(image, lidar_i16, radar_i16, p, i, crop_size, max_depth=np.inf, modality="rgbd"):
    """One frame with the parameters p[...][i]: (inputs [4 or 3, ch, cw], labels [1, ch, cw]) float32."""
    ch, cw = crop_size
    H0, W0 = image.shape[:2]
    s = float(p["scale"][i])
    rc = rotation_coeffs(float(p["angle"][i]), H0, W0)
    oh, ow = int(H0 * s), int(W0 * s)
    hs, ws = int(p["h_start"][i]), int(p["w_start"][i])
    flip = bool(p["flip"][i])

    def geom(a):
        a = a[hs:hs + ch, ws:ws + cw]
        return a[:, ::-1] if flip else a

    rgb = rotate0(image.astype(np.float32), rc)
    rgb = geom(resize_bilinear_u8(bytescale(rgb), oh, ow))
    for which in p["order"][i]:
        rgb = enhance(rgb, int(which), float(p["factors"][i][int(which)]))
    rgb = (rgb / 255.).astype(np.float32).transpose(2, 0, 1)

    def depth(d_i16):
        d = np.array(d_i16 / 256.).astype(np.float32)
        d /= np.float32(s)
        return geom(resize_nearest(rotate0(d, rc), oh, ow))[None]

    labels = np.ascontiguousarray(depth(lidar_i16))
    if modality == "rgb":
        return np.ascontiguousarray(rgb), labels
    radar = depth(radar_i16).copy()
    radar[radar > np.float32(max_depth)] = 0
    return np.concatenate((rgb, radar), 0), labels


def transform_train_batch(image, lidar_i16, radar_i16, p, crop_size, max_depth=np.inf, modality="rgbd"):
    outs = [transform_train_frame(image[b], lidar_i16[b], None if radar_i16 is None else radar_i16[b], p, b, crop_size, max_depth, modality)
            for b in range(image.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])

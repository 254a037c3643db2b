"""numpy restatement of the KITTI depth devkit's evaluation (the reference: misc/devkit/cpp), the arithmetic that
radar_depth_amd/csrc/kitti_eval.hip implements: per-pixel terms in the devkit's types, sums in float64.

Each function takes one frame ([H,W] float32).  The keyword switches select SHORTCUT VARIANTS that a careless implementation
might take; tests/test_kitti_eval_host.py checks that every one of them misses the fixture.
"""
import numpy as np

METRICS = ("mae", "rmse", "inverse mae", "inverse rmse", "log mae", "log rmse", "scale invariant log", "abs relative",
           "squared relative")


def is_valid(d, zero_invalid=False):
    with np.errstate(invalid="ignore"):
        return d > 0 if zero_invalid else d >= 0


def decode(u16):
    u16 = np.asarray(u16, dtype=np.uint16)
    return np.where(u16 == 0, np.float32(-1), (u16.astype(np.float32).astype(np.float64) / 256.0).astype(np.float32))


def encode(d):
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.maximum(d.astype(np.float64) * 256.0, 1.0)
        v = np.where(v >= 65535.0, 65535.0, v)
        return np.where(is_valid(d), np.nan_to_num(v, nan=0.0), 0.0).astype(np.uint16)


def interpolate(d, row_fill="min", fill_interior_rows=False, positive_only=False):
    """interpolateBackground.  Variants: row_fill="mean", fill_interior_rows=True, positive_only=True (d > 0 as validity)."""
    d = np.array(d, dtype=np.float32)
    h, w = d.shape
    valid = is_valid(d, positive_only)
    cols = np.arange(w)[None, :]
    li = np.maximum.accumulate(np.where(valid, cols, -1), axis=1)                    # nearest valid column at or left of x
    ri = np.minimum.accumulate(np.where(valid, cols, w)[:, ::-1], axis=1)[:, ::-1]   # ... at or right of x
    rows = np.arange(h)[:, None]
    L, R = d[rows, np.maximum(li, 0)], d[rows, np.minimum(ri, w - 1)]
    has_l, has_r = li >= 0, ri < w
    with np.errstate(invalid="ignore"):
        if row_fill == "mean":
            both = ((L.astype(np.float64) + R.astype(np.float64)) / 2).astype(np.float32)
        else:
            both = np.where(R < L, R, L)                                             # std::min(L, R)
    out = d.copy()
    hole = ~valid
    out[hole & has_l & has_r] = both[hole & has_l & has_r]
    out[hole & has_l & ~has_r] = L[hole & has_l & ~has_r]
    out[hole & ~has_l & has_r] = R[hole & ~has_l & has_r]
    row_ok = valid.any(axis=1)
    if row_ok.any():
        ys = np.nonzero(row_ok)[0]
        first, last = ys[0], ys[-1]
        out[:first] = out[first]
        out[last + 1:] = out[last]
        if fill_interior_rows:
            for y in range(first + 1, last):
                if not row_ok[y]:
                    out[y] = out[y - 1]
    return out


def error_sums(gt, pred, zero_invalid=False):
    """The eight sums, sum(ld) and the count, float64 [10], in the kernel's order."""
    gt, pred = np.asarray(gt, dtype=np.float32), np.asarray(pred, dtype=np.float32)
    m = is_valid(gt, zero_invalid)
    g, p = gt[m], pred[m]
    with np.errstate(all="ignore"):
        d = np.abs(g - p)
        d2 = d * d
        g64, p64 = g.astype(np.float64), p.astype(np.float64)
        di = np.abs(1.0 / g64 - 1.0 / p64).astype(np.float32)
        di2 = di * di
        ld = np.log(g64) - np.log(p64)
        dl = np.abs(ld).astype(np.float32)
        dl2 = dl * dl
        rel = d / g
        sq = d2 / (g * g)
        terms = [d, d2, di, di2, dl, dl2, ld, rel, sq]
        return np.array([np.sum(t, dtype=np.float64) for t in terms] + [float(g.size)], dtype=np.float64)


def errors_from_sums(s):
    with np.errstate(all="ignore"):
        s = np.asarray(s, dtype=np.float64)
        n = s[9]
        mean = s[6] / n
        return np.array([s[0] / n, np.sqrt(s[1] / n), s[2] / n, np.sqrt(s[3] / n), s[4] / n, np.sqrt(s[5] / n),
                         np.sqrt(s[5] / n - mean * mean), s[7] / n, s[8] / n, n], dtype=np.float64)


def errors(gt, pred, zero_invalid=False):
    """depthError: float64 [10] = the nine errors in the devkit's order, then the valid-pixel count (n == 0: NaN row, count 0)."""
    return errors_from_sums(error_sums(gt, pred, zero_invalid))


def n_err(gt, pred):
    gt, pred = np.asarray(gt, dtype=np.float32), np.asarray(pred, dtype=np.float32)
    with np.errstate(all="ignore"):
        d_err = np.abs(pred - gt).astype(np.float64)
        d_mag = np.abs(gt).astype(np.float64)
        a, b = d_err / 3.0, 20.0 * d_err / d_mag
        return np.where(b < a, b, a).astype(np.float32)                              # std::min(a, b) into a float


def error_image(gt, pred, table, zero_invalid=False, first_wins=False, bins_reversed=False):
    """errorImage(D_gt, true): uint8 [H,W,3].  table: [10,5] lo, hi, r, g, b.  Variants: first_wins (the first centre in raster order
    keeps a pixel), bins_reversed (lo < n_err <= hi)."""
    gt, pred = np.asarray(gt, dtype=np.float32), np.asarray(pred, dtype=np.float32)
    table = np.asarray(table, dtype=np.float32)
    h, w = gt.shape
    out = np.zeros((h, w, 3), dtype=np.uint8)
    if h < 3 or w < 3:
        return out
    ne = n_err(gt, pred)
    colour = np.zeros((h, w, 3), dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for lo, hi, r, g, b in table:
            hit = ((ne > lo) & (ne <= hi)) if bins_reversed else ((ne >= lo) & (ne < hi))
            colour[hit] = (int(r), int(g), int(b))
    centre = np.zeros((h, w), dtype=bool)
    centre[1:h - 1, 1:w - 1] = is_valid(gt, zero_invalid)[1:h - 1, 1:w - 1]
    # the centres that reach a pixel, in raster order of the CENTRE: (dv, du) is the centre's offset from the pixel
    order = [(dv, du) for dv in (-1, 0, 1) for du in (-1, 0, 1)]
    if first_wins:
        order = order[::-1]
    for dv, du in order:
        ys, xs = np.arange(h) + dv, np.arange(w) + du
        oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
        py, px = np.nonzero(oky)[0], np.nonzero(okx)[0]
        c = centre[np.ix_(ys[oky], xs[okx])]
        col = colour[np.ix_(ys[oky], xs[okx])]
        sub = out[np.ix_(py, px)]
        sub[c] = col[c]
        out[np.ix_(py, px)] = sub
    return out


def stats(rows):
    """statMean / statMin / statMax over rows [N,>=9] in float64: ([9] mean, [9] min, [9] max).  The minimum starts at 1, the maximum
    at 0; a NaN fails both comparisons."""
    rows = np.asarray(rows, dtype=np.float64)[:, :9]
    mean, mn, mx = np.zeros(9), np.ones(9), np.zeros(9)
    for r in rows:
        mean = mean + r
        with np.errstate(invalid="ignore"):
            mn = np.where(r < mn, r, mn)
            mx = np.where(r > mx, r, mx)
    with np.errstate(all="ignore"):
        return mean / float(len(rows)), mn, mx


def format_stats(mean, mn, mx):
    return "".join("mean %s: %f \nmin  %s: %f \nmax  %s: %f \n" % (n, mean[i], n, mn[i], n, mx[i]) for i, n in enumerate(METRICS))

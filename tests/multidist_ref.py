"""numpy restatement of the distance-interval metrics (evaluation/metrics.py:61-176 of the reference; here
radar_depth_amd/csrc/metrics_multidist.hip and evaluation.metrics.*_multidist): the interval rule, the ten float32 terms of a valid
pixel added in float64, Result's ten metrics, and the REPAIRED averaging (an interval a result has no pixel in is passed over; an
interval that never received anything averages to the zero Result with valid_label 0).  Shared by tests/test_multidist_host.py and
tests/test_gpu_multidist.py.

`closed` / `last_inf` exist only so that a test can show that the boundary ladder tells the reference's rule (both ends closed, the
last interval unbounded) from its two plausible misreadings."""
import numpy as np

NAMES = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10", "delta1", "delta2", "delta3")
DIST_INTERVAL = (10., 20., 30., 40., 50., 60., 70., 80., 90., 100.)
F = np.float32


def bounds(edges=DIST_INTERVAL, last_inf=True):
    e = np.asarray(edges, dtype=F)
    lo = np.concatenate([np.zeros(1, F), e[:-1]])
    hi = e.copy()
    if last_inf:
        hi[-1] = np.inf
    return lo, hi


def membership(target, edges=DIST_INTERVAL, closed=True, last_inf=True):
    """[n_intervals, N] bool: pixel in interval k  <=>  target > 0 and lo_k <= target <= hi_k, compared in float32."""
    t = np.asarray(target, dtype=F).ravel()
    lo, hi = bounds(edges, last_inf)
    upper = (t[None, :] <= hi[:, None]) if closed else (t[None, :] < hi[:, None])
    return (t[None, :] > 0) & (t[None, :] >= lo[:, None]) & upper


def terms(output, target):
    """[N, 10] float64 holding the float32 terms of rd_depth_metrics' sums (count, d^2, |d|, |log10 o - log10 t|, |d|/t, the three
    ratio tests, (1/o-1/t)^2, |1/o-1/t|); rows of invalid pixels hold garbage and are never selected."""
    o, t = np.asarray(output, dtype=F).ravel(), np.asarray(target, dtype=F).ravel()
    with np.errstate(all="ignore"):
        inv_ln10 = F(0.4342944819032518)
        ad = np.abs(o - t)
        r = np.maximum(o / t, t / o)
        idf = np.abs(F(1) / o - F(1) / t)
        cols = [np.ones_like(o), ad * ad, ad, np.abs(np.log(o) * inv_ln10 - np.log(t) * inv_ln10), ad / t,
                (r < F(1.25)).astype(F), (r < F(1.25) * F(1.25)).astype(F), (r < F(1.25) * F(1.25) * F(1.25)).astype(F), idf * idf, idf]
    assert all(c.dtype == F for c in cols)
    return np.stack(cols, axis=1).astype(np.float64)


def sums(output, target, edges=DIST_INTERVAL, closed=True, last_inf=True):
    """[n_intervals, 10] float64 sums; an interval without a pixel is a row of zeros."""
    tm = terms(output, target)
    mem = membership(target, edges, closed, last_inf)
    return np.stack([tm[m].sum(axis=0) if m.any() else np.zeros(10) for m in mem])


def metrics_from_sums(s):
    """([n, 10] metrics in Result.update's order, NaN where the count is 0; [n] valid_label)."""
    s = np.asarray(s, dtype=np.float64)
    c = s[:, 0]
    with np.errstate(all="ignore"):
        m = np.stack([np.sqrt(s[:, 8] / c), s[:, 9] / c, s[:, 1] / c, np.sqrt(s[:, 1] / c), s[:, 2] / c, s[:, 4] / c, s[:, 3] / c,
                      s[:, 5] / c, s[:, 6] / c, s[:, 7] / c], axis=1)
    m[c == 0] = np.nan
    return m, (c > 0).astype(np.int32)


def evaluate(output, target, edges=DIST_INTERVAL, **rule):
    return metrics_from_sums(sums(output, target, edges, **rule))


class Meter(object):
    """AverageMeter_multidist as repaired: per interval a weight sum, ten weighted metric sums and the number of updates."""

    def __init__(self, n_intervals=len(DIST_INTERVAL)):
        self.buf = np.zeros((n_intervals, 12), dtype=np.float64)

    def update(self, metrics, valid, n=1.0):
        for k in range(self.buf.shape[0]):
            if valid[k]:
                self.buf[k, 0] += n
                self.buf[k, 1:11] += n * np.asarray(metrics[k], dtype=np.float64)
                self.buf[k, 11] += 1

    def average(self):
        """([n, 10], [n] valid_label): zeros and 0 where the interval never received anything."""
        c = self.buf[:, 0]
        avg = np.zeros((self.buf.shape[0], 10))
        avg[c > 0] = self.buf[c > 0, 1:11] / c[c > 0, None]
        return avg, (c > 0).astype(np.int32)


def rel(got, want):
    """Worst relative error; NaN must meet NaN and an infinity the same infinity."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (got, want)
    ok = ~np.isnan(want) & ~inf
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)).max())

"""The lattice classes of tests/wgrad_lattice_cases.py on the two split stem kernels (7x7, stride 2, pad 3; the input is Cin separate
planes of an NCHW tensor), for tests/test_gpu_wgrad_lattice.py and tests/test_wgrad_lattice_host.py.

rd_stem_wgrad_split_t (csrc/stem_wgrad_split.hip, RD_SPLIT_TERMS; output tile 4 x 32):
    dW[(kh, kw, c)][co] = sum over (n, oh, ow) of in[n, c, 2 oh + kh - 3, 2 ow + kw - 3] dout[n, oh, ow, co]
    A   in dense integers in +-2^18, dout in {-1, 0, 1} at PER["A"] pixels per output channel
    B   in {-1, 0, 1} at PER["B"] pixels per plane, dout dense odd 19-bit integers
    C   in dense in +-2^9, dout odd 10-bit integers at PER["C"] pixels per channel
    D   dout one-hot per output channel (+-2^k), in = randn 2^randint(-20, 20): every element one product, the expected tensor a gather
    A bf16-storage dout is its own single piece: classes A and D only, their dout values (+-1, +-2^k) being bf16 numbers.
rd_stem_fwd_split (csrc/stem_split.hip, its own term list RD_SS_TERM; output tile 8 x 32):
    out[n, oh, ow, co] = sum over (kh, kw, c) of in[n, c, 2 oh + kh - 3, 2 ow + kw - 3] w[kh * 7 + kw][c][co]
    A-C as above with w_packed [49][Cin][Cout] as the second operand, at most PER non-zero rows of the 49 Cin per output channel;
    D   one-hot weights: the output is a stride-2 gather of in times 2^k;
    S   in and w in {-1, 0, 1}, 8 non-zero rows per column: |y| <= 8 and sum y^2 over a tile <= 2^14, so the BatchNorm partial sums
        are exact as well: summed over the tiles they must equal the integer sums of the stored output.
Every premise (sums of absolute values below 2^24 quanta, piece counts, at least half of the result non-zero) is asserted by
*_premise()."""
import collections
import functools

import numpy as np

from wgrad_lattice_cases import emulate, pieces, split  # noqa: F401  (emulate: for the tests)
from wino_cases import LATTICE
from wino_ref import KEPT

F, D = np.float32, np.float64
PER = {"A": 16, "B": 16, "C": 8, "S": 8}
CARRIED = dict(LATTICE, D=LATTICE["A"], S=((0, 0),))
PIECES = {"A": (3, 1), "B": (1, 3), "C": (2, 2), "D": (3, 1), "S": (1, 1)}

WgradCfg = collections.namedtuple("WgradCfg", "cin cout bf16")
# every plain instantiation of stem_wgrad_split_kernel: (K tiles, N tiles, bf16 dout) = (5, 2), (2, 1), (4, 1), (7, 2) "owned row tiles",
# (2, 2) with an fp32 dout; (5, 2), (2, 1), (4, 1) with a bf16 one
WGRAD_CONFIGS = [WgradCfg(3, 64, 0), WgradCfg(1, 16, 0), WgradCfg(2, 16, 0), WgradCfg(4, 64, 0), WgradCfg(1, 64, 0),
                 WgradCfg(3, 64, 1), WgradCfg(1, 16, 1), WgradCfg(2, 16, 1)]
# (N, H, W): Ho x Wo = 5 x 6 (narrower than a 4 x 32 output tile, one row past it), 4 x 32 (exactly one tile), 5 x 33 (one row and column past)
WGRAD_SHAPES = [(2, 9, 11), (1, 8, 64), (2, 9, 66)]
WGRAD_BIG = (3, 33, 130)                                 # Ho x Wo = 17 x 65: 45 tiles, 23 splits -- the two-stage slab reduction; 3 -> 64 fp32 only
FWD_CONFIGS = [(ci, co) for ci in (1, 2, 3) for co in (16, 32, 64)] + [(4, 64)]
FWD_SHAPES = [(2, 9, 11), (1, 16, 64), (2, 17, 66)]      # smaller than an 8 x 32 output tile, exactly one, one past it in both directions
FWD_CLASSES = ("A", "B", "C", "D", "S")


def wgrad_id(cfg):
    return "%dto%d-%s" % (cfg.cin, cfg.cout, "bf16" if cfg.bf16 else "fp32")


def fwd_id(cfg):
    return "%dto%d" % cfg


def wgrad_shapes(cfg):
    return WGRAD_SHAPES + ([WGRAD_BIG] if cfg == WGRAD_CONFIGS[0] else [])


def wgrad_classes(cfg):
    return ("A", "D") if cfg.bf16 else ("A", "B", "C", "D")


def wgrad_variants(cfg):
    """(class, log2 of the power of two the input is scaled by)."""
    return [(c, 0) for c in wgrad_classes(cfg)] + [(c, -40) for c in wgrad_classes(cfg) if c != "D"]


def out_size(v):
    return (v - 1) // 2 + 1


# ------------------------------------------------------------------------------------------------ float64 references
def patches(x):
    """x [N,C,H,W] -> [49][N,C,Ho,Wo] float64: in[n, c, 2 oh + kh - 3, 2 ow + kw - 3], zero outside the image."""
    n, c, h, w = x.shape
    ho, wo = out_size(h), out_size(w)
    p = np.zeros((n, c, 2 * ho + 6, 2 * wo + 6), D)
    p[:, :, 3:3 + h, 3:3 + w] = x
    return [p[:, :, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] for kh in range(7) for kw in range(7)]


def wgrad_ref(x, dout):
    """x [N,C,H,W], dout [N,Ho,Wo,Cout] -> float64 OIHW gradient [Cout,C,7,7]."""
    dd = np.asarray(dout, D)
    g = np.stack([np.einsum("nchw,nhwo->oc", p, dd) for p in patches(x)], 2)          # [Cout][C][49]
    return g.reshape(g.shape[0], g.shape[1], 7, 7)


def fwd_ref(x, w):
    """x [N,C,H,W], w [49][C][Cout] -> float64 NHWC output [N,Ho,Wo,Cout]."""
    ww = np.asarray(w, D)
    return sum(np.einsum("nchw,co->nhwo", p, ww[t]) for t, p in enumerate(patches(x)))


def wgrad_terms(x, dout):
    xp, yp = split(x), split(dout)
    return {(a, b): wgrad_ref(xp[a], yp[b]) for (a, b) in KEPT}


def fwd_terms(x, w):
    xp, wp = split(x), split(w)
    return {(a, b): fwd_ref(xp[a], wp[b]) for (a, b) in KEPT}


def _sparse_cols(rng, rows, cols, per, values):
    """[rows][cols] int64 with `per` non-zero rows per column."""
    a = np.zeros((rows, cols), np.int64)
    for q in range(cols):
        a[rng.choice(rows, per, replace=False), q] = values(per) * rng.choice([-1, 1], per)
    return a


def _wide_x(rng, shape):
    return (rng.standard_normal(shape) * 2.0 ** rng.integers(-20, 21, shape)).astype(F)


# ------------------------------------------------------------------------------------------------ the weight gradient
def wgrad_hot_pixels(shape):
    """Output pixels class D places hot pixels on: the corners and the four pixels around the first corner of a 4 x 32 tile."""
    n, h, w = shape
    ho, wo = out_size(h), out_size(w)
    rows = sorted({0, ho - 1} | {v for v in (3, 4) if v < ho})
    cols = sorted({0, wo - 1} | {v for v in (31, 32) if v < wo})
    return [(m, i, j) for m in sorted({0, n - 1}) for i in rows for j in cols]


def wgrad_integers(cfg, shape, cls):
    n, h, w = shape
    ho, wo = out_size(h), out_size(w)
    rng = np.random.default_rng([36, WGRAD_CONFIGS.index(cfg), n, h, w, "ABC".index(cls)])
    ones = lambda k: np.ones(k, np.int64)
    sparse_y = lambda per, values: _sparse_cols(rng, n * ho * wo, cfg.cout, per, values).reshape(n, ho, wo, cfg.cout)
    if cls == "A":
        return rng.integers(-2 ** 18, 2 ** 18 + 1, (n, cfg.cin, h, w)), sparse_y(PER["A"], ones)
    if cls == "B":
        x = _sparse_cols(rng, n * h * w, cfg.cin, PER["B"], ones).reshape(n, h, w, cfg.cin).transpose(0, 3, 1, 2)
        ys = (n, ho, wo, cfg.cout)
        return np.ascontiguousarray(x), (2 * rng.integers(2 ** 17, 2 ** 18, ys) + 1) * rng.choice([-1, 1], ys)
    return rng.integers(-2 ** 9, 2 ** 9 + 1, (n, cfg.cin, h, w)), sparse_y(PER["C"], lambda k: 2 * rng.integers(2 ** 8, 2 ** 9, k) + 1)


def wgrad_one_hot(cfg, shape):
    """-> (x, dout, (n, oh, ow, k, sign) per output channel); the listed hot pixels (shuffled) take every fourth channel, the others are drawn:
    a corner pixel leaves 33 of its 49 taps outside the image, and at least half of the gradient is to be non-zero."""
    n, h, w = shape
    ho, wo = out_size(h), out_size(w)
    rng = np.random.default_rng([37, WGRAD_CONFIGS.index(cfg), n, h, w])
    x = _wide_x(rng, (n, cfg.cin, h, w))
    dout = np.zeros((n, ho, wo, cfg.cout), F)
    hot, where = wgrad_hot_pixels(shape), []
    hot = [hot[i] for i in rng.permutation(len(hot))]
    for q in range(cfg.cout):
        m, i, j = hot[q // 4 % len(hot)] if q % 4 == 0 else (int(rng.integers(n)), int(rng.integers(ho)), int(rng.integers(wo)))
        k, s = q % 7 - 3, int(rng.choice([-1, 1]))
        dout[m, i, j, q] = s * 2.0 ** k
        where.append((m, i, j, k, s))
    return x, dout, where


def wgrad_gather(cfg, x, where):
    g = np.zeros((cfg.cout, cfg.cin, 7, 7), D)
    n, c, h, w = x.shape
    for q, (m, oh, ow, k, s) in enumerate(where):
        for kh in range(7):
            for kw in range(7):
                ih, iw = 2 * oh + kh - 3, 2 * ow + kw - 3
                if 0 <= ih < h and 0 <= iw < w:
                    g[q, :, kh, kw] = x[m, :, ih, iw].astype(D) * (s * 2.0 ** k)
    return g


@functools.lru_cache(maxsize=None)
def wgrad_data(cfg, shape, cls, e=0):
    """-> (x [N,Cin,H,W] float32, dout [N,Ho,Wo,Cout] float32 (bf16 numbers for a bf16 configuration), float64 OIHW gradient)."""
    if cls == "D":
        assert e == 0
        x, dout, _ = wgrad_one_hot(cfg, shape)
    else:
        xi, yi = wgrad_integers(cfg, shape, cls)
        x, dout = (xi * 2.0 ** e).astype(F), yi.astype(F)
        assert np.array_equal(x.astype(D), xi * 2.0 ** e) and np.array_equal(dout.astype(np.int64), yi)
    return x, dout, wgrad_ref(x, dout)


def wgrad_premise(cfg, shape, cls, e=0):
    x, dout, want = wgrad_data(cfg, shape, cls, e)
    worst = 0.0
    if cls == "D":
        assert np.array_equal(wgrad_gather(cfg, x, wgrad_one_hot(cfg, shape)[2]), want), "class D: the float64 gradient is the gather"
    else:
        xi, yi = wgrad_integers(cfg, shape, cls)
        worst = float(wgrad_ref(np.abs(xi), np.abs(yi)).max())
        assert worst < 2 ** 24, (cfg, shape, cls, worst)
        assert np.array_equal(wgrad_ref(xi, yi) * 2.0 ** e, want)
    assert (pieces(x), pieces(dout)) == PIECES[cls], (cfg, shape, cls, pieces(x), pieces(dout))
    if cfg.bf16:
        assert pieces(dout) == 1, "a bf16 dout holds bf16 numbers"
    nz = float((want != 0).mean())
    assert nz >= 0.5, (cfg, shape, cls, nz)
    return dict(worst_log2=float(np.log2(worst)) if worst else 0.0, nonzero=nz)


# ------------------------------------------------------------------------------------------------ the forward
def fwd_integers(cfg, shape, cls):
    cin, cout = cfg
    n, h, w = shape
    rng = np.random.default_rng([38, cin, cout, n, h, w, FWD_CLASSES.index(cls)])
    xs, rows = (n, cin, h, w), 49 * cin
    per = min(PER[cls], rows)
    ones = lambda k: np.ones(k, np.int64)
    if cls == "A":
        x, wt = rng.integers(-2 ** 18, 2 ** 18 + 1, xs), _sparse_cols(rng, rows, cout, per, ones)
    elif cls == "B":
        x, wt = rng.integers(-1, 2, xs), _sparse_cols(rng, rows, cout, per, lambda k: 2 * rng.integers(2 ** 17, 2 ** 18, k) + 1)
    elif cls == "C":
        x, wt = rng.integers(-2 ** 9, 2 ** 9 + 1, xs), _sparse_cols(rng, rows, cout, per, lambda k: 2 * rng.integers(2 ** 8, 2 ** 9, k) + 1)
    else:
        x, wt = rng.integers(-1, 2, xs), _sparse_cols(rng, rows, cout, per, ones)
    return x, wt.reshape(49, cin, cout)


def fwd_one_hot(cfg, shape):
    """-> (x, w, (tap, c, k, sign) per output channel): the rows walk through all 49 Cin (tap, plane) pairs as far as Cout reaches."""
    cin, cout = cfg
    n, h, w = shape
    rng = np.random.default_rng([39, cin, cout, n, h, w])
    x = _wide_x(rng, (n, cin, h, w))
    wt = np.zeros((49 * cin, cout), F)
    rows = rng.permutation(49 * cin)
    where = []
    for q in range(cout):
        r, k, s = int(rows[q % len(rows)]), q % 7 - 3, int(rng.choice([-1, 1]))
        wt[r, q] = s * 2.0 ** k
        where.append((r // cin, r % cin, k, s))
    return x, wt.reshape(49, cin, cout), where


def fwd_gather(x, where):
    p = patches(x)
    return np.stack([p[t][:, c] * (s * 2.0 ** k) for (t, c, k, s) in where], 3)


@functools.lru_cache(maxsize=None)
def fwd_data(cfg, shape, cls):
    """-> (x [N,Cin,H,W] float32, w_packed [49][Cin][Cout] float32, float64 NHWC output)."""
    if cls == "D":
        x, w, _ = fwd_one_hot(cfg, shape)
    else:
        xi, wi = fwd_integers(cfg, shape, cls)
        x, w = xi.astype(F), wi.astype(F)
        assert np.array_equal(x.astype(np.int64), xi) and np.array_equal(w.astype(np.int64), wi)
    return x, w, fwd_ref(x, w)


def fwd_premise(cfg, shape, cls):
    x, w, want = fwd_data(cfg, shape, cls)
    worst = 0.0
    if cls == "D":
        assert np.array_equal(fwd_gather(x, fwd_one_hot(cfg, shape)[2]), want), "class D: the float64 output is the gather"
    else:
        xi, wi = fwd_integers(cfg, shape, cls)
        worst = float(fwd_ref(np.abs(xi), np.abs(wi)).max())
        assert worst < 2 ** 24, (cfg, shape, cls, worst)
    if cls == "S":
        assert np.abs(want).max() <= 8 and (want * want).sum((0, 1, 2)).max() <= 2 ** 14 * int(np.prod(stat_tiles(shape)))
        assert (want * want).reshape(-1, want.shape[3]).sum(0).max() < 2 ** 24
    assert (pieces(x), pieces(w)) == PIECES[cls], (cfg, shape, cls, pieces(x), pieces(w))
    nz = float((want != 0).mean())
    assert nz >= 0.5, (cfg, shape, cls, nz)
    return dict(worst_log2=float(np.log2(worst)) if worst else 0.0, nonzero=nz)


def stat_tiles(shape):
    n, h, w = shape
    return n, -(-out_size(h) // 8), -(-out_size(w) // 32)

"""Cases of tests/test_gpu_wgrad_lattice.py and tests/test_wgrad_lattice_host.py: the split weight-gradient kernels
(csrc/wgrad_split.hip: wgrad_split_kernel, 3x3 / 2x3 / 3x2 / 2x2 tap rectangles x wide 2x32 or tall 4x16 pixel tiles x staged or
pre-split) on inputs where the stored gradient IS the float64 gradient, so that no tolerance is involved.

    dW[tap][ci][co] = sum over output pixels p of x[p + tap][ci] dy[p][co]

The reduction index is the pixel, so the sparsity that keeps every partial sum below 2^24 quanta goes on the pixel axis:
    A   x dense integers in +-2^18 (three bf16 pieces), dy in {-1, 0, 1} with PER["A"] non-zero pixels per output channel (one piece)
    B   x in {-1, 0, 1} with PER["B"] non-zero pixels per input channel, dy dense odd 19-bit integers of either sign
    C   x dense in +-2^9, dy odd 10-bit integers at PER["C"] pixels per channel (two pieces each: the cross term a1 b1)
    D   "one product per element": dy one-hot per output channel (one pixel, +-2^k, k in -3..3), x dense randn 2^randint(-20, 20) with
        full 24-bit significands.  dW[tap][ci][co] is then the single product x[p + tap][ci] 2^k (or zero outside the image), the three
        non-zero terms a2 b0, a1 b0, a0 b0 add up to it exactly in fp32 in either order: the expected tensor is a pure gather.  Hot
        pixels sit on the first and last row and column and on both sides of a pixel-tile boundary.  (UpProj: one hot pixel per output
        channel and PHASE -- a tap belongs to one phase, so an element is still one product.)
A-C also run with x scaled by 2^-40 (e = -40).  premise() asserts in int64: sums of absolute values below 2^24 quanta, the piece counts
of the class (pack_ref.split3), at least half of the gradient non-zero.  LATTICE (tests/wino_cases.py) says which kept terms carry
which class, with x as the first operand and dy as the second; D is carried by A's terms."""
import collections
import functools

import numpy as np
import torch

import pack_ref as PK
from desc_emulator import run_wgrad
from wino_cases import LATTICE
from wino_ref import KEPT

F, D = np.float32, np.float64
PER = {"A": 16, "B": 16, "C": 8}
CLASSES = ("A", "B", "C", "D")
CARRIED = dict(LATTICE, D=LATTICE["A"])
PIECES = {"A": (3, 1), "B": (1, 3), "C": (2, 2), "D": (3, 1)}
# (class, log2 of the power of two x is scaled by)
VARIANTS = [("A", 0), ("B", 0), ("C", 0), ("D", 0), ("A", -40), ("B", -40), ("C", -40)]

Case = collections.namedtuple("Case", "id kind n h w cin cout tall splits tiles_per_split tiles pre")


def _case(kind, n, h, w, cin, cout, tall, splits, tps, tiles, pre=True):
    return Case("%s_%dx%dx%d_%dto%d" % (kind, n, h, w, cin, cout), kind, n, h, w, cin, cout, tall, splits, tps, tiles, pre)


# The plan figures are rd_wgrad_split_plan_info's on a 256-CU device (tests/test_wgrad_lattice_host.py asserts them: a planner change must
# not hollow the cases out): pixel tile tall 4 x 16 or wide 2 x 32, splits, tiles per split, pixel tiles.
CASES = [
    _case("conv", 2, 7, 10, 64, 64, 1, 1, 4, 4),              # ragged in both directions
    _case("conv", 1, 2, 32, 64, 64, 0, 1, 1, 1),              # exactly one tile
    _case("conv", 1, 2, 33, 64, 64, 0, 1, 2, 2),              # one column past a tile
    _case("conv", 2, 6, 31, 64, 64, 0, 2, 3, 6),              # one column short
    _case("conv", 3, 5, 33, 72, 96, 1, 5, 4, 18, pre=False),  # partial 64-blocks on both sides (the pre-split form needs multiples of 16)
    _case("conv", 4, 23, 40, 64, 64, 1, 18, 4, 72),           # more than 16 splits: the two-stage slab reduction (J = 16)
    _case("conv", 9, 2, 32, 64, 64, 0, 3, 3, 9),              # tiles that are whole images
    _case("upproj", 2, 5, 3, 64, 64, 1, 1, 4, 4),             # all four tap rectangles, tiny
    _case("upproj", 1, 2, 32, 64, 64, 0, 1, 1, 1),            # the four rectangles on the wide tile
    _case("upproj", 3, 7, 10, 96, 96, 1, 2, 3, 6),            # partial block, two splits
]
BY_ID = {c.id: c for c in CASES}
WINDOW_CASES = (CASES[0].id, CASES[7].id)       # run once more on channel windows of wider NaN-filled buffers (staged entry point)
WINDOW_EXTRA, WINDOW_OFF = 8, 4                 # ldi = Cin + 8, ldo = Cout + 8, first channel 4: 16-byte alignment holds


def desc(case, window=False):
    from radar_depth_amd import convdesc as cd
    ldi, ldo = (case.cin + WINDOW_EXTRA, case.cout + WINDOW_EXTRA) if window else (case.cin, case.cout)
    if case.kind == "upproj":
        return cd.upproj_fwd(case.n, case.h, case.w, case.cin, case.cout, ldi=ldi, ldo=ldo)
    return cd.conv_fwd(case.n, case.h, case.w, case.cin, case.cout, 3, 1, 1, ldi=ldi, ldo=ldo)


def kernel_shape(case):
    return (5, 5) if case.kind == "upproj" else (3, 3)


def tile_shape(case):
    """(rows, columns) of the pixel tile on the logical grid (= the x grid)."""
    return (4, 16) if case.tall else (2, 32)


def oihw(case, dw):
    """[slabs][Cin][Cout] -> [Cout][Cin][KH][KW]."""
    kh, kw = kernel_shape(case)
    return np.ascontiguousarray(np.asarray(dw).transpose(2, 1, 0).reshape(case.cout, case.cin, kh, kw))


def gradient(case, x, dy, d=None):
    """float64 OIHW gradient of desc_emulator.run_wgrad."""
    kh, kw = kernel_shape(case)
    dw = run_wgrad(d or desc(case), torch.from_numpy(np.asarray(x, D)), torch.from_numpy(np.asarray(dy, D)), kh * kw)
    return oihw(case, dw.numpy())


def _sparse(rng, shape, per, values):
    """[N,H,W,C] int64, `per` non-zero pixels per channel; values(n) draws the magnitudes."""
    n, h, w, c = shape
    a = np.zeros((n * h * w, c), np.int64)
    for q in range(c):
        a[rng.choice(n * h * w, per, replace=False), q] = values(per) * rng.choice([-1, 1], per)
    return a.reshape(shape)


def hot_pixels(case):
    """Logical pixels (n, row, column) class D must place hot pixels on: the corners, and the four pixels around the first tile corner
    in either direction where the grid reaches it."""
    r, tw = tile_shape(case)
    rows = sorted({0, case.h - 1} | {v for v in (r - 1, r) if v < case.h})
    cols = sorted({0, case.w - 1} | {v for v in (tw - 1, tw) if v < case.w})
    return [(n, i, j) for n in sorted({0, case.n - 1}) for i in rows for j in cols]


def integers(case, cls):
    """Classes A-C -> (x [N,Hi,Wi,Cin], dy [N,Ho,Wo,Cout]) in int64."""
    d = desc(case)
    rng = np.random.default_rng([34, CASES.index(case), "ABC".index(cls)])
    xs, ys = (d.N, d.Hi, d.Wi, d.Cin), (d.N, d.Ho, d.Wo, d.Cout)
    if cls == "A":
        return rng.integers(-2 ** 18, 2 ** 18 + 1, xs), _sparse(rng, ys, PER["A"], lambda n: np.ones(n, np.int64))
    if cls == "B":
        return _sparse(rng, xs, PER["B"], lambda n: np.ones(n, np.int64)), (2 * rng.integers(2 ** 17, 2 ** 18, ys) + 1) * rng.choice([-1, 1], ys)
    return rng.integers(-2 ** 9, 2 ** 9 + 1, xs), _sparse(rng, ys, PER["C"], lambda n: 2 * rng.integers(2 ** 8, 2 ** 9, n) + 1)


def one_hot(case):
    """Class D -> (x float32, dy float32, [(co, n, oh, ow, k, sign)]): one hot pixel per output channel and phase.  A tap belongs to
    one phase, so every element of the gradient is still one product (the UpProj's four phases would otherwise leave at least 16 of
    its 25 taps zero)."""
    d = desc(case)
    rng = np.random.default_rng([35, CASES.index(case)])
    x = (rng.standard_normal((d.N, d.Hi, d.Wi, d.Cin)) * 2.0 ** rng.integers(-20, 21, (d.N, d.Hi, d.Wi, d.Cin))).astype(F)
    dy = np.zeros((d.N, d.Ho, d.Wo, d.Cout), F)
    hot, where = hot_pixels(case), []
    for q in range(d.Cout):
        for i in range(d.n_phases):
            at = q * d.n_phases + i
            n, r, c = hot[at] if at < len(hot) else (int(rng.integers(d.N)), int(rng.integers(case.h)), int(rng.integers(case.w)))
            oh, ow = d.out_stride * r + d.phase[i].out_off_h, d.out_stride * c + d.phase[i].out_off_w
            k, s = int(rng.integers(-3, 4)), int(rng.choice([-1, 1]))
            dy[n, oh, ow, q] = s * 2.0 ** k
            where.append((q, n, oh, ow, k, s))
    return x, dy, where


def gather(case, x, where):
    """Class D's expected gradient without a sum: dW[tap][ci][co] = x[p + tap][ci] (+-2^k) for the hot pixel p of co in the tap's phase,
    zero outside the image."""
    d = desc(case)
    kh, kw = kernel_shape(case)
    dw = np.zeros((kh * kw, case.cin, case.cout), D)
    for (q, n, oh, ow, k, s) in where:
        for i in range(d.n_phases):
            ph = d.phase[i]
            if (oh - ph.out_off_h) % d.out_stride or (ow - ph.out_off_w) % d.out_stride:
                continue
            lh, lw = (oh - ph.out_off_h) // d.out_stride, (ow - ph.out_off_w) // d.out_stride
            for t in range(ph.n_taps):
                ih, iw = lh + ph.dh[t], lw + ph.dw[t]
                if 0 <= ih < d.Hi and 0 <= iw < d.Wi:
                    assert not dw[ph.widx[t], :, q].any()
                    dw[ph.widx[t], :, q] = x[n, ih, iw].astype(D) * (s * 2.0 ** k)
    return oihw(case, dw)


def pieces(a):
    """How many of the three bf16 pieces of a float32 array are not all zero."""
    p = PK.split3(np.ascontiguousarray(a, F))
    return 1 + int((p[1] << 1).any()) + int((p[2] << 1).any())


def split(a):
    """The three pieces as float32 arrays of a's shape."""
    return [PK.bf16_to_f32(p).reshape(a.shape) for p in PK.split3(np.ascontiguousarray(a, F))]


@functools.lru_cache(maxsize=None)
def data(case_id, cls, e=0):
    """-> (x float32, dy float32, float64 OIHW gradient).  Computed once, shared, never modified."""
    case = BY_ID[case_id]
    if cls == "D":
        assert e == 0
        x, dy, _ = one_hot(case)
    else:
        xi, yi = integers(case, cls)
        x, dy = (xi * 2.0 ** e).astype(F), yi.astype(F)
        assert np.array_equal(x.astype(D), xi * 2.0 ** e) and np.array_equal(dy.astype(np.int64), yi)
    return x, dy, gradient(case, x, dy)


def premise(case, cls, e=0):
    """The premises of a case and class, asserted -> the figures."""
    x, dy, want = data(case.id, cls, e)
    if cls == "D":
        _, _, where = one_hot(case)
        assert np.array_equal(gather(case, x, where), want), "class D: the float64 gradient is the gather"
        worst = 0.0
    else:
        xi, yi = integers(case, cls)
        worst = float(gradient(case, np.abs(xi), np.abs(yi)).max())
        assert worst < 2 ** 24, (case.id, cls, worst)
        assert np.array_equal(gradient(case, xi, yi) * 2.0 ** e, want)
    assert (pieces(x), pieces(dy)) == PIECES[cls], (case.id, cls, pieces(x), pieces(dy))
    nz = float((want != 0).mean())
    assert nz >= 0.5, (case.id, cls, nz)
    return dict(worst_log2=float(np.log2(worst)) if worst else 0.0, nonzero=nz)


def terms(case, x, dy):
    """{(a, b): the piece product x_a dy_b summed exactly over the pixels (float64 OIHW)} for the six kept terms."""
    xp, yp = split(x), split(dy)
    return {(a, b): gradient(case, xp[a], yp[b]) for (a, b) in KEPT}


def emulate(tm, drop=None):
    """The kept piece products, summed exactly; drop: one of them left out."""
    return sum(v for k, v in tm.items() if k != drop)


# ------------------------------------------------------------------------------------------------ indexing shortcuts
SHORTCUTS = ("taps_transposed", "halo_column_off_by_one", "last_tile_of_a_row_skipped", "split_counted_twice", "upproj_phase_offsets_swapped")


def tile_mask(case, keep):
    """[N, lh, lw] bool: the logical pixels whose tile (index (n tiles_h + th) tiles_w + tw, the kernel's order) satisfies keep(tile, tw,
    tiles_w)."""
    r, tw = tile_shape(case)
    th_n, tw_n = -(-case.h // r), -(-case.w // tw)
    assert case.n * th_n * tw_n == case.tiles
    m = np.zeros((case.n, case.h, case.w), bool)
    for n in range(case.n):
        for i in range(case.h):
            for j in range(case.w):
                m[n, i, j] = keep((n * th_n + i // r) * tw_n + j // tw, j // tw, tw_n)
    return m


def _masked_dy(case, dy, m):
    """dy with the output pixels of the logical pixels outside m zeroed."""
    os_ = 2 if case.kind == "upproj" else 1
    return dy * np.repeat(np.repeat(m, os_, 1), os_, 2)[..., None]


def shortcut(case, x, dy, mode):
    """What a kernel that took the indexing shortcut would store (float64 OIHW); None where the shortcut does not apply to the case."""
    if mode == "taps_transposed":
        return np.ascontiguousarray(gradient(case, x, dy).transpose(0, 1, 3, 2))
    if mode == "halo_column_off_by_one":
        xs = np.zeros_like(x)
        xs[:, :, 1:] = x[:, :, :-1]
        return gradient(case, xs, dy)
    if mode == "last_tile_of_a_row_skipped":
        return gradient(case, x, _masked_dy(case, dy, tile_mask(case, lambda t, tw, n: tw != n - 1)))
    if mode == "split_counted_twice":
        first = tile_mask(case, lambda t, tw, n: t < case.tiles_per_split)
        return gradient(case, x, dy) + gradient(case, x, _masked_dy(case, dy, first))
    if mode == "upproj_phase_offsets_swapped":
        if case.kind != "upproj":
            return None
        from radar_depth_amd._lib import RdConvDesc
        d = RdConvDesc.from_buffer_copy(desc(case))
        for i in range(d.n_phases):
            d.phase[i].out_off_h, d.phase[i].out_off_w = d.phase[i].out_off_w, d.phase[i].out_off_h
        return gradient(case, x, dy, d)
    raise ValueError(mode)

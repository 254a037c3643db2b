"""Cases of tests/test_gpu_bf16_lattice.py and tests/test_bf16_lattice_host.py: the bf16-operand matrix-core kernels (csrc/gconv_bf16.hip,
csrc/gconv_bf16p.hip, csrc/wgrad_bf16.hip, csrc/stem_bf16.hip) on inputs where the stored result IS the exact result, so that every
comparison is an equality of bit patterns.  A product of two bf16 numbers is exact in fp32 and, on integer operands, every partial sum
below 2^24 is exact in any order: an fp32 output must be the integer result, a bf16 output RNE_bf16(integer result), ties included.

First operand a = the activation (weight gradient: x), second operand b = the weights (weight gradient: dy):
    P   a and b dense non-zero integers in +-[1, 15]: every product matters (also with a, bias and addend scaled by 2^-40)
    R   a dense in +-127, b non-zero in +-[1, 127] at PER["R"] places per output channel: |y| <= 16 * 127^2 needs rounding to 8 bits
        (bf16-stored outputs only; expected RNE_bf16(y))
    D   a = randn 2^randint(-20, 20) with full significands and PLANTED bit patterns, b one-hot +-2^k: the output is a gather of
        RNE_bf16(a) (+-2^k) -- the conversion on load of the fp32-tensor forms (weight gradient: dy one-hot at hot pixels)
    S   a in {-1, 0, 1}, b in {-1, 0, 1} at PER["S"] places: |y| <= 8, sums and sums of squares per statistics tile exact
    T   a dense in +-127, b in +-[1, 3] at PER["T"] places: |y| <= 1524 needs rounding on store, the per-tile SUM is exact and must be
        the sum of the unrounded integers (bf16 storage; the squares column is not asserted)
The epilogue (fp32 integer bias, integer addend, ReLU on the first act_cols channels, a row stride that defeats the 4-channel stores) runs
on P and R.  *_premise() assert every premise in int64; *_shortcut() restate each operation with one named fault (CONV_SHORTCUTS,
WGRAD_SHORTCUTS; CARRIER names the class that catches it).

Run as a script, this file runs every rd_gconv_bf16[_t] / persistent-kernel job under the tile choice of THIS process (the tile-forcing
knobs are read once per process) and writes one record per launch:
    python tests/bf16_lattice_cases.py OUT.json"""
import collections
import ctypes as C
import functools
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import stem_lattice_cases as SL  # noqa: E402
from desc_emulator import run_desc, run_wgrad  # noqa: E402

F, D = np.float32, np.float64
BF16, RELU = 1, 1            # RD_DTYPE_BF16, RD_ACT_RELU
PER = {"R": 16, "S": 8, "T": 4}
CANARY, CANARY_VALUE = 4096, -1234.5
# fp32 bit patterns class D plants into a: low half 0x8000 under an even and an odd upper half (ties: down / up to even), 0x7fff
# (just below the tie), 0x8001 (just above), and a tie that rounds up into the next binade (0x3f7f8000 -> 1.0)
PLANTED = (0x40408000, 0x40418000, 0x40407fff, 0x40408001, 0x3f7f8000)


# ------------------------------------------------------------------------------------------------ bf16 rounding, restated on the bits
def bf16_bits(a, mode="rne"):
    """fp32-representable values -> the uint16 pattern of their bf16 rounding.  rne: nearest, ties to even (the documented store and
    load conversion); trunc / half_away: the two named faults."""
    a = np.asarray(a)
    a32 = np.ascontiguousarray(a, F)
    assert np.array_equal(a32.astype(D), np.asarray(a, D), equal_nan=True), "the value to be rounded is an fp32 number"
    u = a32.view(np.uint32).astype(np.uint64)
    if mode == "rne":
        u = u + 0x7fff + ((u >> 16) & 1)
    elif mode == "half_away":
        u = u + 0x8000
    else:
        assert mode == "trunc"
    return (u >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(F)


def rne(a, mode="rne"):
    """float64 values of the bf16 rounding of a."""
    return bf16_value(bf16_bits(a, mode)).astype(D)


def is_bf16(a):
    a32 = np.ascontiguousarray(a, F)
    return bool(np.array_equal(a32.astype(D), np.asarray(a, D)) and not (a32.view(np.uint32) & 0xffff).any())


def ties(y):
    """(ties of y that RNE rounds down to even, ties it rounds up to even)."""
    u = np.ascontiguousarray(y, F).view(np.uint32)
    tie = (u & 0xffff) == 0x8000
    return int((tie & ((u >> 16) & 1 == 0)).sum()), int((tie & ((u >> 16) & 1 == 1)).sum())


# ------------------------------------------------------------------------------------------------ descriptor arithmetic in numpy
def gather(d, p, t, x, mode="exact", shift=0):
    """x [N,Hi,Wi,C] -> [N,lh,lw,C] of x[n, r IS + dh, c IS + dw + shift], zero outside the image.  row_wrap: the column test is missing
    (a column past the edge reads the neighbouring row); next_image: the row test is missing (a row past the edge reads the next image)."""
    N, Hi, Wi, Cc = x.shape
    ih, iw = np.meshgrid(np.arange(p.lh) * d.in_stride + p.dh[t], np.arange(p.lw) * d.in_stride + p.dw[t] + shift, indexing="ij")
    flat = ih * Wi + iw
    if mode == "exact":
        ok = (ih >= 0) & (ih < Hi) & (iw >= 0) & (iw < Wi)
    elif mode == "row_wrap":
        ok = (flat >= 0) & (flat < Hi * Wi)
    else:
        assert mode == "next_image"
        ok = (iw >= 0) & (iw < Wi)
    idx = np.arange(N)[:, None, None] * Hi * Wi + flat[None]
    ok = ok[None] & (idx >= 0) & (idx < N * Hi * Wi)
    return x.reshape(N * Hi * Wi, Cc)[np.clip(idx, 0, N * Hi * Wi - 1)] * ok[..., None]


def emulate_conv(d, x, w, mode="exact", keep=None, swap=False):
    """run_desc in numpy float64 -> [N,Ho,Wo,Cout], NaN where no phase writes.  keep(phase, tap) -> False drops a tap; swap: the phases'
    output offsets exchanged (rows for columns)."""
    x, w = np.asarray(x, D), np.asarray(w, D)
    out = np.full((d.N, d.Ho, d.Wo, d.Cout), np.nan, D)
    for i in range(d.n_phases):
        p = d.phase[i]
        acc = np.zeros((d.N, p.lh, p.lw, d.Cout), D)
        for t in range(p.n_taps):
            if keep is None or keep(i, t):
                acc += gather(d, p, t, x, mode) @ w[p.widx[t]]
        oh, ow = (p.out_off_w, p.out_off_h) if swap else (p.out_off_h, p.out_off_w)
        out[:, oh::d.out_stride, ow::d.out_stride][:, :p.lh, :p.lw] = acc
    return out


def emulate_wgrad(d, x, dy, S, mode="exact", shift=None, pixels=None, swap=False):
    """run_wgrad in numpy float64 -> [S][Cin][Cout].  shift(phase, tap) -> columns a tap's read is displaced by; pixels [N,lh,lw] bool:
    the logical pixels that are reduced over."""
    x, dy = np.asarray(x, D), np.asarray(dy, D)
    dw = np.zeros((S, d.Cin, d.Cout), D)
    for i in range(d.n_phases):
        p = d.phase[i]
        oh, ow = (p.out_off_w, p.out_off_h) if swap else (p.out_off_h, p.out_off_w)
        g = dy[:, oh::d.out_stride, ow::d.out_stride][:, :p.lh, :p.lw]
        if pixels is not None:
            g = g * pixels[..., None]
        for t in range(p.n_taps):
            dw[p.widx[t]] += np.einsum("nhwi,nhwo->io", gather(d, p, t, x, mode, shift(i, t) if shift else 0), g)
    return dw


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, D))


def _nz(rng, shape, hi):
    return rng.integers(1, hi + 1, shape) * rng.choice([-1, 1], shape)


def _sparse_cols(rng, rows, cols, per, values):
    """[rows][cols] int64 with `per` non-zero rows per column (tests/wgrad_lattice_cases.py's _sparse, on the reduction axis)."""
    a = np.zeros((rows, cols), np.int64)
    for q in range(cols):
        a[rng.choice(rows, min(per, rows), replace=False), q] = values(min(per, rows)) * rng.choice([-1, 1], min(per, rows))
    return a


def wide(rng, shape):
    """Class D's a -> (float32 values with a quarter of them PLANTED patterns of either sign, the pattern's index + 1 or 0)."""
    x = (rng.standard_normal(shape) * 2.0 ** rng.integers(-20, 21, shape)).astype(F)
    flat, tag = x.reshape(-1), np.zeros(x.size, np.int64)
    idx = rng.permutation(x.size)[:x.size // 4]
    j = np.arange(idx.size)
    flat.view(np.uint32)[idx] = np.array(PLANTED, np.uint32)[j % 5] | ((j // 5 % 2).astype(np.uint32) << 31)
    tag[idx] = 1 + j % 5
    return x, tag.reshape(shape)


def _first(got, want, bad):
    return [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]


# ================================================================================================ the convolutions
# kind -> (descriptor, weight slabs).  2x7x10, 64 -> 64 unless the kind says otherwise.
def _kinds():
    from radar_depth_amd import convdesc as cd
    return {
        "3x3": (lambda: cd.conv_fwd(2, 7, 10, 64, 64, 3, 1, 1), 9),
        "upproj_fwd": (lambda: cd.upproj_fwd(2, 7, 10, 64, 64), 25),                    # phases of 9 / 6 / 6 / 4 taps
        "dgrad_s2": (lambda: cd.conv_dgrad(2, 7, 10, 64, 64, 3, 2, 1)[0], 9),           # phases of 1 / 2 / 2 / 4 taps
        "dgrad_1x1_s2": (lambda: cd.conv_dgrad(2, 7, 10, 64, 64, 1, 2, 0)[0], 1),       # one phase: three pixels of four stay untouched
        "upproj_dgrad": (lambda: cd.upproj_dgrad(2, 7, 10, 64, 64), 25),                # one phase of 25 taps, input stride 2
        "3x3_partial": (lambda: cd.conv_fwd(2, 13, 35, 96, 96, 3, 1, 1), 9),            # CKP 32, partial channel tiles
        "1x1": (lambda: cd.conv_fwd(2, 7, 10, 64, 64, 1, 1, 0), 1),
        "3x3_320": (lambda: cd.conv_fwd(2, 7, 10, 320, 64, 3, 1, 1), 9),                # the pipelined chunk loop on the NT 1 tiles (nine taps)
        "1x1_320": (lambda: cd.conv_fwd(2, 7, 10, 320, 64, 1, 1, 0), 1),                # the pipelined chunk loop on every tile (one tap)
        "3x3_48": (lambda: cd.conv_fwd(2, 7, 10, 48, 64, 3, 1, 1), 9),                  # CKP 16, three chunks
        "3x3_16": (lambda: cd.conv_fwd(2, 7, 10, 16, 32, 3, 1, 1), 9),                  # CKP 16, one chunk
        # the persistent kernel (rd_gconv_bf16p_plan_all(1), bf16 tensors)
        "p_3x3": (lambda: cd.conv_fwd(2, 7, 10, 64, 64, 3, 1, 1), 9),
        "p_dgrad": (lambda: cd.conv_dgrad(2, 7, 10, 64, 64, 3, 1, 1)[0], 9),
        "p_upproj": (lambda: cd.upproj_fwd(2, 7, 10, 64, 32), 25),                      # NT 1
        "p_ragged": (lambda: cd.conv_fwd(2, 13, 35, 64, 96, 3, 1, 1), 9),               # NT 1, ragged in both directions
        "p_wide": (lambda: cd.conv_fwd(1, 5, 61, 32, 64, 3, 1, 1), 9),                  # wider than 32 - halo: several tile columns
        # maps tall enough that the planner's TH x TW tile of gconv_bf16_kernel fills every wave and every M-block of each forced (MT, NT)
        # (fills(): asserted from the plan query), still ragged in both directions
        "3x3_tall": (lambda: cd.conv_fwd(1, 189, 12, 64, 64, 3, 1, 1), 9),
        "upproj_tall": (lambda: cd.upproj_fwd(1, 189, 12, 64, 64), 25),
        "1x1_320_tall": (lambda: cd.conv_fwd(1, 189, 12, 320, 64, 1, 1, 0), 1),         # pipelined and filled on every tile but (3, 2)
        "1x1_320_wide": (lambda: cd.conv_fwd(1, 189, 64, 320, 64, 1, 1, 0), 1),         # (3, 2) pipelined: 16 x 22 pixels, 11 of its 12 M-blocks
    }


SMALL_KINDS = ("3x3", "upproj_fwd", "dgrad_s2", "dgrad_1x1_s2", "upproj_dgrad", "3x3_partial", "1x1", "3x3_320", "1x1_320", "3x3_48", "3x3_16")
TALL_KINDS = ("3x3_tall", "upproj_tall", "1x1_320_tall")
GCONV_KINDS = SMALL_KINDS + TALL_KINDS + ("1x1_320_wide",)
BF16P_KINDS = ("p_3x3", "p_dgrad", "p_upproj", "p_ragged", "p_wide")
ALL_KINDS = SMALL_KINDS + BF16P_KINDS + TALL_KINDS + ("1x1_320_wide",)          # (a kind's index here seeds its data)
CONV_CLASSES = ("P", "R", "D", "S", "T")
# epilogue -> (bias, addend, ReLU columns as a function of Cout, extra row stride of the output)
EPILOGUES = {"none": (0, 0, lambda co: 0, 0),
             "vec": (1, 1, lambda co: co // 2, 0),              # act_cols a multiple of 4: the 4-channel epilogue
             "scalar": (1, 1, lambda co: co // 2 - 2, 0),       # act_cols not a multiple of 4: the element-wise epilogue
             "ldo": (1, 0, lambda co: co // 2, 2),              # ldo = Cout + 2 defeats vec4; the two spare columns stay NaN
             "add": (0, 1, lambda co: 0, 0)}                    # the residual addend of an input gradient
KIND_EPILOGUES = {"3x3": ("none", "vec", "scalar", "ldo"), "upproj_fwd": ("none", "vec"), "dgrad_s2": ("none", "add"), "upproj_dgrad": ("none", "add"),
                  "3x3_partial": ("none", "scalar"), "3x3_tall": ("none", "vec", "add"), "upproj_tall": ("none", "vec"), "1x1_320_tall": ("none", "vec"),
                  "p_3x3": ("none", "vec", "scalar", "ldo"), "p_dgrad": ("none", "add"), "p_upproj": ("none", "vec")}
BF16P_GRIDS = (0, 1, 3)      # RD_GCONV_BF16P_GRID: the launch's own grid, one workgroup, three


def conv_desc(kind, ldo_extra=0):
    make, S = _kinds()[kind]
    d = make()
    d.ldo = d.Cout + ldo_extra
    return d, S


def fills(plan):
    """Whether the TH x TW tile of a gconv_bf16_kernel plan puts valid pixels into every 32-slot M-block of every wave: slots are filled
    row-major, block (wave MT + mt) 32 belongs to wave `wave`, so the last block starts at slot 32 (4 MT - 1).  All blocks before it are
    then FULL M-tiles: the 4-channel epilogue (vec4 and all 32 rows valid) runs on them."""
    return plan[3] * plan[4] > 32 * (4 * plan[0] - 1)


def d_sets(rows, cout):
    """Class D runs once per one-hot weight set "D", "D1", ...: ceil(rows / Cout) sets give every (slab, input channel) row a weight."""
    return -(-rows // cout)


def d_classes(n):
    return ["D" + (str(v) if v else "") for v in range(n)]


def conv_jobs(kind):
    """(class, log2 scale of a, bf16 tensors, epilogue) of a kind.  D runs on fp32 tensors only (the conversion on load), once per weight
    set; R and T on bf16 tensors only (the rounding on store); the persistent kernel takes bf16 tensors only."""
    if kind == "1x1_320_wide":         # (twelve thousand pixels of 320 channels: the products and the statistics only)
        return [(c, 0, io16, "none") for io16 in (0, 1) for c in "PS"]
    epis = KIND_EPILOGUES.get(kind, ("none",))
    jobs = []
    for io16 in ((1,) if kind in BF16P_KINDS else (0, 1)):
        for ep in epis:
            jobs += [("P", 0, io16, ep), ("P", -40, io16, ep)] + ([("R", 0, io16, ep)] if io16 else [])
        jobs += [("S", 0, io16, "none")] + ([("T", 0, io16, "none")] if io16 else [(c, 0, io16, "none") for c in conv_d_classes(kind)])
    return jobs


def conv_d_classes(kind):
    """Every weight set on the small maps (the staging path does not depend on the map), the first one on the tall ones."""
    d, S = conv_desc(kind)
    return d_classes(1 if kind in TALL_KINDS else d_sets(S * d.Cin, d.Cout))


def conv_integers(kind, cls):
    """Classes P, R, S, T -> (a [N,Hi,Wi,Cin], b [S,Cin,Cout], bias [Cout], addend [N,Ho,Wo,Cout]) in int64."""
    d, S = conv_desc(kind)
    rng = np.random.default_rng([41, ALL_KINDS.index(kind), CONV_CLASSES.index(cls)])
    xs, rows = (d.N, d.Hi, d.Wi, d.Cin), S * d.Cin
    if cls == "P":
        a, b = _nz(rng, xs, 15), _nz(rng, (rows, d.Cout), 15)
    elif cls == "R":
        a, b = rng.integers(-127, 128, xs), _sparse_cols(rng, rows, d.Cout, PER["R"], lambda n: rng.integers(1, 128, n))
    elif cls == "S":
        a, b = rng.integers(-1, 2, xs), _sparse_cols(rng, rows, d.Cout, PER["S"], lambda n: np.ones(n, np.int64))
    else:
        assert cls == "T"
        a, b = rng.integers(-127, 128, xs), _sparse_cols(rng, rows, d.Cout, PER["T"], lambda n: rng.integers(1, 4, n))
    return a, b.reshape(S, d.Cin, d.Cout), rng.integers(-100, 101, d.Cout), rng.integers(-127, 128, (d.N, d.Ho, d.Wo, d.Cout))


def conv_one_hot(kind, v=0):
    """Class D, weight set v -> (a float32, its planted tags, b float32 [S,Cin,Cout]): one weight +-2^k per output channel; channel q of
    set v takes row v Cout + q of a permutation of all (slab, input channel) pairs, so the sets together give every row a weight."""
    d, S = conv_desc(kind)
    rng = np.random.default_rng([42, ALL_KINDS.index(kind)])
    a, tag = wide(rng, (d.N, d.Hi, d.Wi, d.Cin))
    rows = rng.permutation(S * d.Cin)
    b = np.zeros((S * d.Cin, d.Cout), F)
    for q in range(d.Cout):
        b[rows[(v * d.Cout + q) % rows.size], q] = float(rng.choice([-1, 1])) * 2.0 ** (q % 7 - 3)
    return a, tag, b.reshape(S, d.Cin, d.Cout)


def epilogue(d, y, bias, addend, act_cols):
    """y (float64, NaN where unwritten) -> act_{co < act_cols}(y + bias + addend); every step exact on the lattice."""
    y = y.copy()
    if bias is not None:
        y += bias
    if addend is not None:
        y += addend
    y[..., :act_cols] = np.where(y[..., :act_cols] < 0, 0.0, y[..., :act_cols])
    return y + 0.0


@functools.lru_cache(maxsize=None)
def conv_data(kind, cls, e=0, ep="none"):
    """-> dict(a, b float32; bias, addend float32 or None; act_cols; y: the float64 result of the convolution alone; want: after the
    epilogue -- the fp32 accumulator's value, NaN where no phase writes).  Computed once, shared, never modified."""
    use_b, use_a, cols, _ = EPILOGUES[ep]
    d, S = conv_desc(kind)
    q = 2.0 ** e
    if cls[0] == "D":
        assert e == 0 and ep == "none"
        a, _, b = conv_one_hot(kind, int(cls[1:] or 0))
        y = run_desc(d, _t64(rne(a)), _t64(b)).numpy()
        bias = addend = None
    else:
        ai, bi, ci, di = conv_integers(kind, cls)
        a, b = (ai * q).astype(F), bi.astype(F)
        bias, addend = ((ci * q).astype(F) if use_b else None), ((di * q).astype(F) if use_a else None)
        y = run_desc(d, _t64(a), _t64(b)).numpy()
    act_cols = cols(d.Cout)
    return dict(a=a, b=b, bias=bias, addend=addend, act_cols=act_cols, y=y, want=epilogue(d, y, bias, addend, act_cols))


def stat_rows(d, v, TH, TW):
    """The [tiles][2][Cout] partial sums of v (float64 [N,Ho,Wo,Cout]) in the kernels' row order: image, phase, TH x TW tiles of the
    phase's logical grid, row-major."""
    rows = []
    for n in range(d.N):
        for i in range(d.n_phases):
            p = d.phase[i]
            g = v[n, p.out_off_h::d.out_stride, p.out_off_w::d.out_stride][:p.lh, :p.lw]
            for r0 in range(0, p.lh, TH):
                for c0 in range(0, p.lw, TW):
                    t = g[r0:r0 + TH, c0:c0 + TW].reshape(-1, d.Cout)
                    rows.append(np.stack([t.sum(0), (t * t).sum(0)]))
    return np.stack(rows)


MAX_STAT_TILE = 384          # pixels of the largest statistics tile any plan of the two kernels can use: 4 waves x MT 3 x 32


def conv_premise(kind, cls, e=0, ep="none"):
    """The premises of a (kind, class, scale, epilogue), asserted in int64 -> the figures."""
    d, S = conv_desc(kind)
    dd = conv_data(kind, cls, e, ep)
    fig = {}
    if cls[0] == "D":
        a, tag, b = conv_one_hot(kind, int(cls[1:] or 0))
        assert is_bf16(b) and not is_bf16(a)
        if cls == "D" and kind not in TALL_KINDS:
            used = sum((conv_one_hot(kind, v)[2] != 0).any(2) for v in range(len(conv_d_classes(kind))))
            assert used.all(), "the weight sets together give every (slab, input channel) row a weight"
        terms = emulate_conv(d, np.ones(a.shape), b != 0)
        assert np.nanmax(terms) == 1, "class D: one product per element at the most, so the output is a gather"
        for k in range(1, len(PLANTED) + 1):
            assert np.nansum(emulate_conv(d, tag == k, b != 0)) > 0, "planted pattern %d does not reach the output" % k
        return dict(gathered=float(np.nanmean(terms)))
    ai, bi, ci, di = conv_integers(kind, cls)
    use_b, use_a, cols, _ = EPILOGUES[ep]
    assert is_bf16(dd["a"]) and is_bf16(dd["b"]) and (dd["addend"] is None or is_bf16(dd["addend"])), "operands are bf16 numbers"
    worst = np.nanmax(emulate_conv(d, np.abs(ai), np.abs(bi))) + (np.abs(ci).max() if use_b else 0) + (np.abs(di).max() if use_a else 0)
    assert worst < 2 ** 24, (kind, cls, worst)
    yi = emulate_conv(d, ai, bi)
    assert np.array_equal(yi * 2.0 ** e, dd["y"], equal_nan=True), "the float64 reference is the integer result"
    fig["worst_log2"] = float(np.log2(worst))
    if cls == "P":
        assert (ai != 0).all() and (bi != 0).all() and np.abs(ai).max() <= 15 and np.abs(bi).max() <= 15
    if cls == "R":
        assert np.abs(ai).max() <= 127 and np.abs(bi).max() <= 127 and ((bi != 0).reshape(-1, d.Cout).sum(0) == min(PER["R"], S * d.Cin)).all()
        w = dd["want"][~np.isnan(dd["want"])]
        fig["ties"] = ties(w)
        assert min(fig["ties"]) > 0, (kind, ep, fig["ties"])
        assert (bf16_bits(w) != bf16_bits(w, "trunc")).any() and (bf16_bits(w) != bf16_bits(w, "half_away")).any()
    if cls in "ST":
        bound = {"S": 8, "T": 3 * 127 * PER["T"]}[cls]
        assert np.nanmax(np.abs(yi)) <= bound
        assert MAX_STAT_TILE * bound < 2 ** 24 and (cls == "T" or MAX_STAT_TILE * bound * bound < 2 ** 24), "exact partial sums on the largest tile"
    if cls == "T":
        w = np.nan_to_num(dd["want"])
        assert (stat_rows(d, w, 4, 8)[:, 0] != stat_rows(d, rne(w), 4, 8)[:, 0]).any(), "sums of the rounded outputs differ"
    return fig


# ------------------------------------------------------------------------------------------------ named faults
CONV_SHORTCUTS = ("truncating_store", "round_half_away", "truncating_load", "stats_from_rounded_outputs", "dropped_tap", "dropped_k_step",
                  "last_partial_channel_block_dropped", "row_wrap", "next_image", "upproj_phases_swapped")
WGRAD_SHORTCUTS = ("truncating_load", "dropped_tap", "dropped_k_step", "last_partial_channel_block_dropped", "row_wrap", "next_image",
                   "upproj_phases_swapped", "horizontal_tap_shifted", "dropped_split")
# which class carries which fault (the README lists the same table)
CARRIER = {"truncating_store": "R", "round_half_away": "R", "truncating_load": "D", "stats_from_rounded_outputs": "T", "dropped_tap": "P",
           "dropped_k_step": "P", "last_partial_channel_block_dropped": "P", "row_wrap": "P", "next_image": "P", "upproj_phases_swapped": "P",
           "horizontal_tap_shifted": "P", "dropped_split": "P"}


def reads_outside(d, mode):
    """Whether a tap of d reads a column outside the image (row_wrap) or a row outside it next to another image (next_image)."""
    for i in range(d.n_phases):
        p = d.phase[i]
        for t in range(p.n_taps):
            if mode == "row_wrap" and (p.dw[t] < 0 or (p.lw - 1) * d.in_stride + p.dw[t] >= d.Wi):
                return True
            if mode == "next_image" and d.N > 1 and (p.dh[t] < 0 or (p.lh - 1) * d.in_stride + p.dh[t] >= d.Hi):
                return True
    return False


def conv_shortcut(kind, mode):
    """-> (expected, what a kernel with the fault would leave) on the class that carries the fault: uint16 patterns for the stores,
    [tiles][Cout] sums for the statistics, float64 outputs otherwise; None where the fault does not apply to the kind."""
    d, S = conv_desc(kind)
    cls = CARRIER[mode]
    if mode in ("truncating_store", "round_half_away"):
        w = np.nan_to_num(conv_data(kind, "R")["want"])
        return bf16_bits(w), bf16_bits(w, "trunc" if mode == "truncating_store" else "half_away")
    if mode == "stats_from_rounded_outputs":
        w = np.nan_to_num(conv_data(kind, "T")["want"])
        return stat_rows(d, w, 4, 8)[:, 0], stat_rows(d, rne(w), 4, 8)[:, 0]
    dd = conv_data(kind, cls)
    a, b, want = dd["a"].astype(D), dd["b"].astype(D), dd["y"]
    if mode == "truncating_load":
        return want, emulate_conv(d, rne(dd["a"], "trunc"), b)
    if mode == "dropped_tap":          # the last tap of the last phase
        return want, emulate_conv(d, a, b, keep=lambda i, t: (i, t) != (d.n_phases - 1, d.phase[d.n_phases - 1].n_taps - 1))
    if mode == "dropped_k_step":       # input channels 16..31 of the first tap's slab (the first 16 where there are no more)
        b2 = b.copy()
        lo = 16 if d.Cin >= 32 else 0
        b2[d.phase[0].widx[0], lo:lo + 16] = 0
        return want, emulate_conv(d, a, b2)
    if mode == "last_partial_channel_block_dropped":
        if d.Cin % 64 == 0 or d.Cin < 64:
            return None
        b2 = b.copy()
        b2[:, d.Cin // 64 * 64:] = 0
        return want, emulate_conv(d, a, b2)
    if mode in ("row_wrap", "next_image"):
        if not reads_outside(d, mode):
            return None
        return want, emulate_conv(d, a, b, mode)
    assert mode == "upproj_phases_swapped"
    if d.n_phases != 4 or len({(d.phase[i].lh, d.phase[i].lw) for i in range(4)}) != 1:
        return None                    # (the UpProj forward: four phases on one logical grid)
    return want, emulate_conv(d, a, b, swap=True)


# ================================================================================================ the weight gradient
WCase = collections.namedtuple("WCase", "id kind n h w cin cout")


def _w(kind, n, h, w, cin, cout):
    return WCase("%s_%dx%dx%d_%dto%d" % (kind, n, h, w, cin, cout), kind, n, h, w, cin, cout)


# pixel tile 4 x 32 on the logical grid.  FULL: conv3 (all nine taps in its one pass); NK = 4 / (tile pairs of a channel block): 1 with
# both sides >= 64, 2 with one side below, 4 with both below.
WGRAD_CASES = [
    _w("conv3", 2, 7, 10, 64, 64),            # ragged in both directions
    _w("conv3", 1, 4, 32, 64, 64),            # exactly one tile
    _w("conv3", 1, 4, 33, 64, 32),            # one column past a tile; NK 2
    _w("conv3", 2, 6, 31, 32, 48),            # one column short (odd width: the pixel-pair packing, the byte-aligned tap shifts); NK 4
    _w("conv3", 4, 23, 40, 64, 64),           # many tiles: several pixel splits
    _w("conv3", 2, 7, 10, 80, 96),            # partial 64-channel blocks on both sides
    _w("conv3", 2, 7, 10, 16, 16),            # NK 4, one 16-channel group a side
    _w("upproj", 2, 7, 10, 64, 64),           # four passes of 9 / 6 / 6 / 4 taps; the two branch weights as column ranges
    _w("upproj", 1, 4, 33, 32, 32),           # NK 4
    _w("conv3s2", 2, 13, 21, 64, 32),         # four input-parity passes of 4 / 2 / 2 / 1 taps, odd sizes; NK 2
    _w("conv1", 2, 7, 10, 32, 48),            # one tap; NK 4
    _w("conv1", 2, 7, 10, 64, 64),            # one tap; NK 1
]
WGRAD_BY_ID = {c.id: c for c in WGRAD_CASES}
WGRAD_WINDOW_CASES = (WGRAD_CASES[0].id, WGRAD_CASES[7].id)      # once more on channel windows of wider NaN-filled buffers
WINDOW_EXTRA, WINDOW_OFF = 8, 8               # ldi = Cin + 8, ldo = Cout + 8, first channel 8: bf16 bases stay 16-byte aligned
WGRAD_REFUSED = ("conv3", 2, 7, 10, 72, 96)   # channel counts must be multiples of 16: rd_wgrad_bf16_supported says no


def wgrad_desc(case, window=False):
    from radar_depth_amd import convdesc as cd
    ldi, ldo = (case.cin + WINDOW_EXTRA, case.cout + WINDOW_EXTRA) if window else (case.cin, case.cout)
    if case.kind == "upproj":
        return cd.upproj_fwd(case.n, case.h, case.w, case.cin, case.cout, ldi=ldi, ldo=ldo)
    k, s = {"conv3": (3, 1), "conv3s2": (3, 2), "conv1": (1, 1)}[case.kind]
    return cd.conv_fwd(case.n, case.h, case.w, case.cin, case.cout, k, s, k // 2, ldi=ldi, ldo=ldo)


def kernel_shape(case):
    return {"upproj": (5, 5), "conv1": (1, 1)}.get(case.kind, (3, 3))


def oihw(case, dw):
    kh, kw = kernel_shape(case)
    return np.ascontiguousarray(np.asarray(dw).transpose(2, 1, 0).reshape(case.cout, case.cin, kh, kw))


def wgrad_jobs(case):
    """(class, log2 scale of x, bf16 tensors)."""
    return [("P", 0, 0), ("P", -40, 0), ("D", 0, 0), ("P", 0, 1), ("P", -40, 1)]


def hot_pixels(d):
    """Logical pixels class D places hot pixels on: the corners and the four pixels around the first corner of a 4 x 32 tile."""
    lh, lw = d.phase[0].lh, d.phase[0].lw
    rows = sorted({0, lh - 1} | {v for v in (3, 4) if v < lh})
    cols = sorted({0, lw - 1} | {v for v in (31, 32) if v < lw})
    return [(n, i, j) for n in sorted({0, d.N - 1}) for i in rows for j in cols]


def wgrad_integers(case):
    d = wgrad_desc(case)
    rng = np.random.default_rng([43, WGRAD_CASES.index(case)])
    return _nz(rng, (d.N, d.Hi, d.Wi, d.Cin), 15), _nz(rng, (d.N, d.Ho, d.Wo, d.Cout), 15)


def wgrad_one_hot(case):
    """Class D -> (x float32, its planted tags, dy float32): one hot pixel +-2^k per output channel and phase, so that every element of the
    gradient is one product (a tap belongs to one phase)."""
    d = wgrad_desc(case)
    rng = np.random.default_rng([44, WGRAD_CASES.index(case)])
    x, tag = wide(rng, (d.N, d.Hi, d.Wi, d.Cin))
    dy = np.zeros((d.N, d.Ho, d.Wo, d.Cout), F)
    hot = hot_pixels(d)
    for q in range(d.Cout):
        for i in range(d.n_phases):
            at = q * d.n_phases + i
            n, r, c = hot[at] if at < len(hot) else (int(rng.integers(d.N)), int(rng.integers(d.phase[0].lh)), int(rng.integers(d.phase[0].lw)))
            dy[n, d.out_stride * r + d.phase[i].out_off_h, d.out_stride * c + d.phase[i].out_off_w, q] = float(rng.choice([-1, 1])) * 2.0 ** (q % 7 - 3)
    return x, tag, dy


@functools.lru_cache(maxsize=None)
def wgrad_data(case_id, cls, e=0):
    """-> (x float32, dy float32, float64 OIHW gradient)."""
    case = WGRAD_BY_ID[case_id]
    d = wgrad_desc(case)
    kh, kw = kernel_shape(case)
    if cls == "D":
        assert e == 0
        x, _, dy = wgrad_one_hot(case)
        return x, dy, oihw(case, run_wgrad(d, _t64(rne(x)), _t64(dy), kh * kw).numpy())
    xi, yi = wgrad_integers(case)
    x, dy = (xi * 2.0 ** e).astype(F), yi.astype(F)
    return x, dy, oihw(case, run_wgrad(d, _t64(x), _t64(dy), kh * kw).numpy())


def wgrad_premise(case, cls, e=0):
    d = wgrad_desc(case)
    kh, kw = kernel_shape(case)
    x, dy, want = wgrad_data(case.id, cls, e)
    if cls == "D":
        _, tag, _ = wgrad_one_hot(case)
        assert is_bf16(dy) and not is_bf16(x)
        assert emulate_wgrad(d, np.ones(x.shape), dy != 0, kh * kw).max() == 1, "class D: one product per element at the most"
        for k in range(1, len(PLANTED) + 1):
            assert emulate_wgrad(d, tag == k, dy != 0, kh * kw).sum() > 0, "planted pattern %d does not reach the gradient" % k
        assert set(hot_pixels(d)) <= {(n, r // d.out_stride, c // d.out_stride) for n, r, c, _ in np.argwhere(dy != 0)}
        return dict(nonzero=float((want != 0).mean()))
    xi, yi = wgrad_integers(case)
    assert is_bf16(x) and is_bf16(dy) and (xi != 0).all() and (yi != 0).all() and np.abs(xi).max() <= 15 and np.abs(yi).max() <= 15
    worst = emulate_wgrad(d, np.abs(xi), np.abs(yi), kh * kw).max()
    assert worst < 2 ** 24, (case.id, worst)
    assert np.array_equal(oihw(case, emulate_wgrad(d, xi, yi, kh * kw)) * 2.0 ** e, want), "the float64 reference is the integer result"
    return dict(worst_log2=float(np.log2(worst)), nonzero=float((want != 0).mean()))


def wgrad_plan(d):
    from radar_depth_amd._lib import lib
    info = (C.c_int32 * 7)()
    assert lib().rd_wgrad_bf16_plan_info(C.byref(d), info) == 0
    return [int(v) for v in info]


def wgrad_inst(d, S, plan, io16):
    """(FULL, NK, IO16) of wgrad_bf16_kernel from the plan query: the slabs are disjoint over the passes and each is produced once, so all
    nine taps are present in every pass exactly when slabs = 9 x passes."""
    return (int(S == 9 * plan[6]), 4 // (plan[0] * plan[1]), int(io16))


def wgrad_shortcut(case, mode):
    d = wgrad_desc(case)
    kh, kw = kernel_shape(case)
    S = kh * kw
    x, dy, want = wgrad_data(case.id, CARRIER[mode])
    xd, yd = x.astype(D), dy.astype(D)
    taps = [(i, t) for i in range(d.n_phases) for t in range(d.phase[i].n_taps)]
    if mode == "truncating_load":
        return want, oihw(case, emulate_wgrad(d, rne(x, "trunc"), yd, S))
    if mode == "dropped_tap":
        g = emulate_wgrad(d, xd, yd, S)
        g[d.phase[d.n_phases - 1].widx[d.phase[d.n_phases - 1].n_taps - 1]] = 0
        return want, oihw(case, g)
    if mode == "dropped_k_step":       # eight consecutive pixels of one tile row: one lane's share of a 16-pixel MFMA step
        m = np.ones((d.N, d.phase[0].lh, d.phase[0].lw), bool)
        m[0, 0, :8] = False
        return want, oihw(case, emulate_wgrad(d, xd, yd, S, pixels=m))
    if mode == "last_partial_channel_block_dropped":
        if case.cin % 64 == 0 or case.cin < 64:
            return None
        x2 = xd.copy()
        x2[..., case.cin // 64 * 64:] = 0
        return want, oihw(case, emulate_wgrad(d, x2, yd, S))
    if mode in ("row_wrap", "next_image"):
        if not reads_outside(d, mode):
            return None
        return want, oihw(case, emulate_wgrad(d, xd, yd, S, mode))
    if mode == "upproj_phases_swapped":
        return (want, oihw(case, emulate_wgrad(d, xd, yd, S, swap=True))) if case.kind == "upproj" else None
    if mode == "horizontal_tap_shifted":      # the taps that read one column to the right read two
        right = max(d.phase[i].dw[t] for i, t in taps)
        if right <= 0:
            return None
        return want, oihw(case, emulate_wgrad(d, xd, yd, S, shift=lambda i, t: int(d.phase[i].dw[t] == right)))
    assert mode == "dropped_split"            # the last pixel split of the plan: tiles of 4 x 32 logical pixels, image-major
    plan = wgrad_plan(d)
    lh, lw = d.phase[0].lh, d.phase[0].lw
    th, tw = -(-lh // 4), -(-lw // 32)
    total = d.N * th * tw
    tps = -(-total // min(-(-256 // (plan[2] * plan[6])), total))          # the planner's rule: 256 workgroups over blocks x passes
    assert -(-total // tps) == plan[3], (case.id, plan, tps)
    n, r, c = np.meshgrid(np.arange(d.N), np.arange(lh), np.arange(lw), indexing="ij")
    tile = (n * th + r // 4) * tw + c // 32
    return want, oihw(case, emulate_wgrad(d, xd, yd, S, pixels=tile < (plan[3] - 1) * tps))


# ================================================================================================ the stem
STEM_CONFIGS = [(ci, co) for ci in (1, 2, 3) for co in (16, 32, 64)]
STEM_SHAPES = SL.FWD_SHAPES                    # 2x9x11, 1x16x64, 2x17x66: smaller than an 8 x 32 output tile, exactly one, one past it
STEM_CLASSES = ("P", "R", "D", "S", "T")


def stem_jobs(cfg):
    """(class, bf16 output).  The fp32 planes and weights are converted on load, so D applies to both output types."""
    ds = d_classes(d_sets(49 * cfg[0], cfg[1]))
    return [("P", 0), ("S", 0)] + [(c, 0) for c in ds] + [("P", 1), ("S", 1)] + [(c, 1) for c in ds] + [("R", 1), ("T", 1)]


def stem_integers(cfg, shape, cls):
    cin, cout = cfg
    n, h, w = shape
    if cls == "S":
        return SL.fwd_integers(cfg, shape, "S")
    rng = np.random.default_rng([45, cin, cout, n, h, w, STEM_CLASSES.index(cls)])
    xs, rows = (n, cin, h, w), 49 * cin
    if cls == "P":
        x, wt = _nz(rng, xs, 15), _nz(rng, (rows, cout), 15)
    elif cls == "R":
        x, wt = rng.integers(-127, 128, xs), _sparse_cols(rng, rows, cout, PER["R"], lambda k: rng.integers(1, 128, k))
    else:
        assert cls == "T"
        x, wt = rng.integers(-127, 128, xs), _sparse_cols(rng, rows, cout, PER["T"], lambda k: rng.integers(1, 4, k))
    return x, wt.reshape(49, cin, cout)


def stem_one_hot(cfg, shape, v=0):
    """Class D, weight set v (see conv_one_hot)."""
    cin, cout = cfg
    n, h, w = shape
    rng = np.random.default_rng([46, cin, cout, n, h, w])
    x, tag = wide(rng, (n, cin, h, w))
    rows = rng.permutation(49 * cin)
    wt = np.zeros((49 * cin, cout), F)
    for q in range(cout):
        wt[rows[(v * cout + q) % rows.size], q] = float(rng.choice([-1, 1])) * 2.0 ** (q % 7 - 3)
    return x, tag, wt.reshape(49, cin, cout)


@functools.lru_cache(maxsize=None)
def stem_data(cfg, shape, cls):
    """-> (x [N,Cin,H,W] float32, w_packed [49][Cin][Cout] float32, float64 NHWC output)."""
    if cls[0] == "D":
        x, _, w = stem_one_hot(cfg, shape, int(cls[1:] or 0))
        return x, w, SL.fwd_ref(rne(x), w) + 0.0
    xi, wi = stem_integers(cfg, shape, cls)
    x, w = xi.astype(F), wi.astype(F)
    return x, w, SL.fwd_ref(x, w) + 0.0


def stem_stat_rows(shape, v):
    """[tiles][2][Cout] sums of v [N,Ho,Wo,Cout] over the 8 x 32 output tiles, image-major."""
    n, th, tw = SL.stat_tiles(shape)
    rows = []
    for m in range(n):
        for i in range(th):
            for j in range(tw):
                t = v[m, 8 * i:8 * i + 8, 32 * j:32 * j + 32].reshape(-1, v.shape[3])
                rows.append(np.stack([t.sum(0), (t * t).sum(0)]))
    return np.stack(rows)


def stem_premise(cfg, shape, cls):
    x, w, want = stem_data(cfg, shape, cls)
    if cls[0] == "D":
        _, tag, _ = stem_one_hot(cfg, shape, int(cls[1:] or 0))
        assert is_bf16(w) and not is_bf16(x)
        if cls == "D":
            used = sum((stem_one_hot(cfg, shape, v)[2] != 0).any(2) for v in range(d_sets(49 * cfg[0], cfg[1])))
            assert used.all(), "the weight sets together give every (tap, plane) row a weight"
        assert SL.fwd_ref(np.ones(x.shape), w != 0).max() == 1, "class D: one product per element at the most"
        for k in range(1, len(PLANTED) + 1):
            assert SL.fwd_ref(tag == k, w != 0).sum() > 0, "planted pattern %d does not reach the output" % k
        return {}
    xi, wi = stem_integers(cfg, shape, cls)
    assert is_bf16(x) and is_bf16(w)
    worst = SL.fwd_ref(np.abs(xi), np.abs(wi)).max()
    assert worst < 2 ** 24
    fig = dict(worst_log2=float(np.log2(worst)))
    if cls == "R":
        fig["ties"] = ties(want)
        assert min(fig["ties"]) > 0, (cfg, shape, fig["ties"])
    if cls in "ST":
        bound = {"S": 8, "T": 3 * 127 * PER["T"]}[cls]
        assert np.abs(want).max() <= bound and 256 * bound < 2 ** 24 and (cls == "T" or 256 * bound * bound < 2 ** 24)
    if cls == "T":
        assert (stem_stat_rows(shape, want)[:, 0] != stem_stat_rows(shape, rne(want))[:, 0]).any()
    return fig


def stem_walk_shape(n_cu):
    """The tile-walk case: Cout 64 keeps two workgroups per CU, 32 x 128 inputs are four 8 x 32 output tiles per image -> the smallest N
    with more than 2 n_cu tiles."""
    return (2 * n_cu // 4 + 1, 32, 128)


# ================================================================================================ on the device
def _env():
    from radar_depth_amd._lib import check, current_stream, lib
    return lib(), check, current_stream()


def _vp(t, elems=0):
    return C.c_void_p(None if t is None else t.data_ptr() + elems * t.element_size())


def _nan_buffer(n, dtype):
    """n NaN elements (bf16: the pattern 0x7fc0) and a canary block behind them."""
    buf = torch.full((n + CANARY,), float("nan"), dtype=dtype, device="cuda")
    buf[n:] = CANARY_VALUE
    return buf


def _bits_t(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _tail_ok(buf, n):
    return bool((_bits_t(buf[n:]) == _bits_t(torch.full((1,), CANARY_VALUE, dtype=buf.dtype))[0].item()).all())


def _dev(a, io16):
    t = torch.from_numpy(np.ascontiguousarray(a, F))
    if io16:
        assert is_bf16(a)
        t = t.to(torch.bfloat16)
    return t.cuda()


def _stored(buf, n, io16):
    """The first n elements -> (float64 values, the patterns that are compared: uint16 for bf16 tensors, uint32 for fp32 ones)."""
    if io16:
        b = buf[:n].view(torch.int16).cpu().numpy().view(np.uint16)
        return bf16_value(b).astype(D), b
    v = buf[:n].cpu().numpy()
    return v.astype(D), v.view(np.uint32)


def _expected(want, io16):
    """float64 expectation -> (values, patterns) as stored: RNE_bf16 for bf16 tensors; NaN where nothing is written."""
    nan = np.isnan(want)
    w = np.where(nan, 0.0, want)
    if io16:
        b = bf16_bits(w)
        b[nan] = 0x7fc0
        return np.where(nan, np.nan, bf16_value(b).astype(D)), b
    v = np.where(nan, np.nan, w).astype(F)
    assert np.array_equal(v.astype(D), want, equal_nan=True)
    return v.astype(D), v.view(np.uint32)


def conv_plan(d, io16):
    """rd_gconv_bf16_plan_info_t's eight figures (no device needed): MT, NT, pipelined * 1000 + CKP (+ 2000: the persistent kernel), TH, TW,
    patch pixels, LDS bytes, workgroups."""
    from radar_depth_amd._lib import check, lib
    info = (C.c_int32 * 8)()
    check(lib().rd_gconv_bf16_plan_info_t(BF16 if io16 else 0, C.byref(d), info), "rd_gconv_bf16_plan_info_t")
    return [int(v) for v in info]


def run_conv(kind, cls, e, io16, ep, grid=0):
    """One launch of rd_gconv_bf16 (fp32 tensors) / rd_gconv_bf16_t (bf16 tensors) under poisoned LDS into NaN-filled buffers -> record.
    Kinds of BF16P_KINDS run under rd_gconv_bf16p_plan_all(1) with RD_GCONV_BF16P_GRID = grid (0: unset); the caller holds both."""
    from radar_depth_amd import ops
    L, check, st = _env()
    use_b, use_a, cols, ldo_extra = EPILOGUES[ep]
    d, S = conv_desc(kind, ldo_extra)
    dd = conv_data(kind, cls, e, ep)
    persistent = kind in BF16P_KINDS
    plan = conv_plan(d, io16)
    assert (plan[2] >= 2000) == persistent, (kind, plan)
    dt = torch.bfloat16 if io16 else torch.float32
    x = _dev(dd["a"], io16)
    wp = ops.pack_weights_bf16(torch.from_numpy(np.ascontiguousarray(dd["b"].transpose(2, 1, 0)[..., None])).cuda())      # [Cout][Cin][slabs][1]
    bias = None if dd["bias"] is None else torch.from_numpy(dd["bias"]).cuda()
    add = None if dd["addend"] is None else _dev(dd["addend"], io16)
    keep = [(t, t.clone()) for t in (x, wp, bias, add) if t is not None]
    n_out = d.N * d.Ho * d.Wo * d.ldo
    out = _nan_buffer(n_out, dt)
    stat = None
    if cls in "ST":
        tiles = int(L.rd_gconv_bf16_stat_tiles_t(BF16 if io16 else 0, C.byref(d)))
        assert tiles > 0
        stat = _nan_buffer(tiles * 2 * d.Cout, torch.float32)
    check(L.rd_debug_poison_lds(st), "rd_debug_poison_lds")
    args = (C.byref(d), _vp(x), _vp(wp), _vp(out), _vp(bias), RELU if dd["act_cols"] else 0, dd["act_cols"], _vp(add), d.Cout if add is not None else 0,
            _vp(stat), st)
    if io16:
        check(L.rd_gconv_bf16_t(BF16, *args), "rd_gconv_bf16_t")
    else:
        check(L.rd_gconv_bf16(*args), "rd_gconv_bf16")
    torch.cuda.synchronize()
    assert _tail_ok(out, n_out) and (stat is None or _tail_ok(stat, stat.numel() - CANARY)), "wrote behind the output or the partial sums"
    for t, t0 in keep:
        assert torch.equal(_bits_t(t), _bits_t(t0)), "an operand changed"
    shape = (d.N, d.Ho, d.Wo, d.ldo)
    gv, gb = (v.reshape(shape) for v in _stored(out, n_out, io16))
    assert np.isnan(gv[..., d.Cout:]).all(), "a channel outside the output window was written"
    gv, gb = gv[..., :d.Cout], gb[..., :d.Cout]
    wv, wb = _expected(dd["want"], io16)
    assert np.array_equal(np.isnan(gv), np.isnan(wv)), "exactly the phases' pixels are written"
    bad = np.argwhere((gb != wb) & ~np.isnan(wv))
    n_stat = None
    if stat is not None:
        rows = stat[:tiles * 2 * d.Cout].view(tiles, 2, d.Cout).cpu().numpy().astype(D)
        assert np.isfinite(rows).all(), "a statistics row was not written"
        want_rows = stat_rows(d, np.nan_to_num(dd["want"]), plan[3], plan[4])          # of the fp32 accumulators, not of the stored tensor
        assert want_rows.shape == rows.shape, (want_rows.shape, rows.shape)
        n_stat = int((rows[:, 0] != want_rows[:, 0]).sum()) + (int((rows[:, 1] != want_rows[:, 1]).sum()) if cls == "S" else 0)
    rec = dict(kernel="gconv_bf16p" if persistent else "gconv_bf16", kind=kind, cls=cls, e=e, io16=io16, ep=ep, grid=grid, plan=plan,
               inst=[plan[0], plan[1]] + ([] if persistent else [plan[2] // 1000, io16]), ckp=plan[2] % 1000, n_bad=len(bad), n_bad_stat=n_stat,
               first=_first(gv, wv, bad))
    return rec


def _what(r):
    return r.get("kind") or r.get("case") or "%dto%d" % tuple(r["cfg"])


def show(r):
    """One launch in full."""
    print("BF16-LATTICE %-11s %-28s inst %-14s class %s 2^%-3d %s %-6s%s%s plan %s differing elements: %d, statistics: %s, accumulated: %s %s" % (
        r["kernel"], _what(r), tuple(r["inst"]), r["cls"], r.get("e", 0), "bf16" if r["io16"] else "fp32", r.get("ep", ""),
        (" grid %d" % r["grid"]) if r.get("grid") else "", (" " + "x".join(map(str, r["shape"]))) if "shape" in r else "", r.get("plan", "-"),
        r["n_bad"], "-" if r.get("n_bad_stat") is None else r["n_bad_stat"], "-" if r.get("n_bad_acc") is None else r["n_bad_acc"], r["first"]))


def summarize(records, label=""):
    """The record of a set of launches: one line per (kernel, case, instantiation and plan from the plan query, tensor type, grid cap) with
    the launches per class, the epilogues, and the differing elements / statistics sums / accumulated elements summed over them, then every
    launch that differs in full (kernel, instantiation, class, differing elements, the first of them)."""
    groups = {}
    for r in records:
        if "seconds" in r:
            print("BF16-LATTICE %-8s all launches of the process: %.1f s" % (label, r["seconds"]))
            continue
        groups.setdefault((r["kernel"], _what(r), tuple(r["inst"]), r["io16"], r.get("grid", 0), tuple(r.get("plan", ()))), []).append(r)
    for (kernel, what, inst, io16, grid, plan), rs in groups.items():
        per = collections.Counter(r["cls"][0] + ("*2^%d" % r["e"] if r.get("e") else "") for r in rs)          # (D: over its weight sets)
        eps = sorted({r["ep"] for r in rs if r.get("ep")})
        tot = lambda k: sum(r.get(k) or 0 for r in rs)
        print("BF16-LATTICE %-8s %-11s %-28s inst %-13s %s%s plan %s launches %s%s differing elements: %d, statistics: %d, accumulated: %d" % (
            label, kernel, what, inst, "bf16" if io16 else "fp32", (" grid %d" % grid) if grid else "", list(plan) or "-",
            " ".join("%s:%d" % kv for kv in sorted(per.items())), (" epilogues " + ",".join(eps)) if eps else "", tot("n_bad"), tot("n_bad_stat"),
            tot("n_bad_acc")))
        for r in rs:
            if r["n_bad"] or r.get("n_bad_stat") or r.get("n_bad_acc"):
                show(r)


def run_conv_all():
    """Every job of GCONV_KINDS under the plan of this process, then every job of BF16P_KINDS on the persistent kernel under each grid cap
    -> one record per launch; the last record carries the seconds the whole run took."""
    L, _, _ = _env()
    t0 = time.perf_counter()
    records = []
    saved = os.environ.pop("RD_GCONV_BF16P_GRID", None)
    try:
        for kind in GCONV_KINDS:
            for job in conv_jobs(kind):
                records.append(run_conv(kind, *job))
        prev = L.rd_gconv_bf16p_plan_all(1)          # (set before any buffer is sized, restored after the last launch)
        try:
            for grid in BF16P_GRIDS:
                if grid:
                    os.environ["RD_GCONV_BF16P_GRID"] = str(grid)          # read at every launch
                for kind in BF16P_KINDS:
                    for job in conv_jobs(kind):
                        records.append(run_conv(kind, *job, grid=grid))
        finally:
            L.rd_gconv_bf16p_plan_all(1 if prev == 1 else 0)
    finally:
        os.environ.pop("RD_GCONV_BF16P_GRID", None)
        if saved is not None:
            os.environ["RD_GCONV_BF16P_GRID"] = saved
    records.append({"seconds": time.perf_counter() - t0})
    return records


@functools.lru_cache(maxsize=None)
def run_wgrad_case(case_id, cls, e, io16, window=False):
    """rd_wgrad_bf16 / rd_wgrad_bf16_t + rd_wgrad_bf16_reduce -> record."""
    L, check, st = _env()
    case = WGRAD_BY_ID[case_id]
    d = wgrad_desc(case, window)
    kh, kw = kernel_shape(case)
    x, dy, want = wgrad_data(case_id, cls, e)
    off = WINDOW_OFF if window else 0
    dt = torch.bfloat16 if io16 else torch.float32
    assert not io16 or (is_bf16(x) and is_bf16(dy))

    def widen(a, ld):
        buf = torch.full(a.shape[:3] + (ld,), float("nan"), dtype=dt)
        buf[..., off:off + a.shape[3]] = torch.from_numpy(a).to(dt)
        return buf.cuda()
    xb, yb = widen(x, d.ldi), widen(dy, d.ldo)
    x0, y0 = xb.clone(), yb.clone()
    assert L.rd_wgrad_bf16_supported(C.byref(d)) == 1
    plan = wgrad_plan(d)
    assert plan == wgrad_plan(wgrad_desc(case)), "the plan does not depend on the channel strides"
    nws = int(L.rd_wgrad_bf16_workspace_floats(C.byref(d)))
    assert nws > 0
    ws = _nan_buffer(nws, torch.float32)
    nel = case.cout * case.cin * kh * kw
    gbuf = torch.full((2 * CANARY + nel,), CANARY_VALUE, device="cuda")
    grad = gbuf[CANARY:CANARY + nel].view(case.cout, case.cin, kh, kw)
    grad.fill_(float("nan"))
    xp, yp = _vp(xb, off), _vp(yb, off)
    assert xp.value % 16 == 0 and yp.value % 16 == 0
    check(L.rd_debug_poison_lds(st), "rd_debug_poison_lds")
    if io16:
        check(L.rd_wgrad_bf16_t(BF16, C.byref(d), xp, yp, _vp(ws), st), "rd_wgrad_bf16_t")
    else:
        check(L.rd_wgrad_bf16(C.byref(d), xp, yp, _vp(ws), st), "rd_wgrad_bf16")
    # (UpProj: the two branch tensors are column ranges [co_off, co_off + O) of one slab set)
    ranges = [(0, case.cout // 2), (case.cout // 2, case.cout // 2)] if case.kind == "upproj" else [(0, case.cout)]

    def reduce(g, lo, n, accumulate):
        check(L.rd_wgrad_bf16_reduce(C.byref(d), _vp(ws), _vp(g[lo:lo + n]), n, case.cin, kh, kw, lo, accumulate, st), "rd_wgrad_bf16_reduce")
    for lo, n in ranges:
        reduce(grad, lo, n, 0)
    acc = None
    if case.kind == "upproj" and cls == "P":
        # once more with accumulate = 1 onto an integer-lattice gradient: G0 + dW is still exact
        q = 2.0 ** e
        assert np.abs(want).max() / q + 2 ** 10 < 2 ** 24
        g0 = torch.randint(-2 ** 10, 2 ** 10 + 1, grad.shape, generator=torch.Generator().manual_seed(5)).double() * q
        acc = g0.float().cuda()
        for lo, n in ranges:
            reduce(acc, lo, n, 1)
    torch.cuda.synchronize()
    assert _tail_ok(ws, nws), "wrote behind the %d workspace floats" % nws
    assert bool((gbuf[:CANARY] == CANARY_VALUE).all()) and bool((gbuf[CANARY + nel:] == CANARY_VALUE).all()), "wrote outside the gradient"
    assert torch.equal(_bits_t(xb), _bits_t(x0)) and torch.equal(_bits_t(yb), _bits_t(y0)), "an operand buffer changed"
    got = grad.cpu().numpy()
    assert not np.isnan(got).any(), "the NaN-filled gradient is not fully overwritten"
    wv, wb = _expected(want, 0)
    bad = np.argwhere(got.view(np.uint32) != wb)
    n_acc = None if acc is None else int((acc.cpu().numpy().astype(D) != g0.numpy() + want).sum())
    rec = dict(kernel="wgrad_bf16", case=case_id + ("/window" if window else ""), cls=cls, e=e, io16=io16, plan=plan,
               inst=wgrad_inst(d, kh * kw, plan, io16), n_bad=len(bad), n_bad_acc=n_acc, first=_first(got.astype(D), wv, bad))
    return rec


@functools.lru_cache(maxsize=None)
def run_stem(cfg, shape, cls, io16):
    """rd_stem_fwd_bf16 (fp32 output) / rd_stem_fwd_bf16_t (bf16 output) on strided planes of a wider NaN-filled NCHW tensor -> record."""
    L, check, st = _env()
    cin, cout = cfg
    n, h, w = shape
    x, wt, want = stem_data(cfg, shape, cls)
    xw = torch.full((n, cin + 1, h, w), float("nan"))
    xw[:, 1:] = torch.from_numpy(x)
    xw, wg = xw.cuda(), torch.from_numpy(wt).cuda()
    x0, w0 = xw.clone(), wg.clone()
    planes = (C.c_void_p * 3)(*[xw.data_ptr() + 4 * h * w * (1 + c) if c < cin else None for c in range(3)])
    strides = (C.c_int64 * 3)(*[(cin + 1) * h * w if c < cin else 0 for c in range(3)])
    ho, wo = SL.out_size(h), SL.out_size(w)
    tiles = int(L.rd_stem_stat_tiles(n, h, w))
    assert tiles == int(np.prod(SL.stat_tiles(shape)))
    nel = n * ho * wo * cout
    out = _nan_buffer(nel, torch.bfloat16 if io16 else torch.float32)
    stat = _nan_buffer(tiles * 2 * cout, torch.float32)
    check(L.rd_debug_poison_lds(st), "rd_debug_poison_lds")
    if io16:
        check(L.rd_stem_fwd_bf16_t(BF16, planes, strides, cin, n, h, w, _vp(wg), cout, _vp(out), _vp(stat), st), "rd_stem_fwd_bf16_t")
    else:
        check(L.rd_stem_fwd_bf16(planes, strides, cin, n, h, w, _vp(wg), cout, _vp(out), _vp(stat), st), "rd_stem_fwd_bf16")
    torch.cuda.synchronize()
    assert _tail_ok(out, nel) and _tail_ok(stat, tiles * 2 * cout), "wrote behind the output or the partial sums"
    assert torch.equal(_bits_t(xw), _bits_t(x0)) and torch.equal(_bits_t(wg), _bits_t(w0)), "an operand changed"
    gv, gb = (v.reshape(n, ho, wo, cout) for v in _stored(out, nel, io16))
    rows = stat[:tiles * 2 * cout].view(tiles, 2, cout).cpu().numpy().astype(D)
    assert not np.isnan(gv).any() and np.isfinite(rows).all(), "the output and every partial-sum row are written"
    wv, wb = _expected(want, io16)
    bad = np.argwhere(gb != wb)
    n_stat = None
    if cls in "ST":
        want_rows = stem_stat_rows(shape, want)
        n_stat = int((rows[:, 0] != want_rows[:, 0]).sum()) + (int((rows[:, 1] != want_rows[:, 1]).sum()) if cls == "S" else 0)
    rec = dict(kernel="stem_bf16", cfg=cfg, shape=shape, cls=cls, io16=io16, inst=(2 if cout > 32 else 1,), tiles=tiles, n_bad=len(bad), n_bad_stat=n_stat,
               first=_first(gv, wv, bad))
    return rec


def forced_plans():
    """kind -> rd_gconv_bf16_plan_info_t on fp32 tensors under the tile choice of THIS process (no device needed)."""
    return {k: conv_plan(conv_desc(k)[0], 0) for k in GCONV_KINDS}


def check_fill(plans, tile=None):
    """What the tall kinds are there for, from the plan query: on every tile the planner's TH x TW fills every wave and M-block, the tall
    320-channel 1x1 is pipelined as well, except on (3, 2), whose pipelined loop takes 16 patch rows at the most: there the wide map is
    pipelined with 16 x 22 pixels = 11 of the 12 M-blocks, the most any map was found to give."""
    for k in TALL_KINDS:
        assert fills(plans[k]) and (tile is None or tuple(plans[k][:2]) == tile), (k, plans[k])
    mt_nt = tuple(plans["1x1_320_tall"][:2])
    if mt_nt == (3, 2):
        w = plans["1x1_320_wide"]
        assert w[2] // 1000 == 1 and w[3] * w[4] >= 32 * (4 * w[0] - 1), w
    else:
        assert plans["1x1_320_tall"][2] // 1000 == 1, plans["1x1_320_tall"]


if __name__ == "__main__":
    with open(sys.argv[-1], "w") as fh:
        json.dump(forced_plans() if sys.argv[1] == "--plans" else run_conv_all(), fh)

"""numpy restatement of the packed operands every matrix kernel of this library reads, written from include/radar_depth_hip.h
(rd_pack_weights, rd_pack_weights_bf16, rd_pack_weights_batched, rd_wino_pack[_batched], rd_bn_eval_coeffs[_batched]) and the layout
comments of csrc/layout.hip / csrc/wino_split.hip -- not from the kernels' index arithmetic.  No torch.

    logical operand   L[slab][row][col] of an OIHW tensor w[o][i][slab]
                      forward    : row = i            (R = I rows),          col = co_off + o
                      transposed : row = co_off + o   (R = rows_total rows), col = i
                      value = w[o][i][slab] (* scale[o], or * scale[i] with scale_col: ONE float32 multiply, before any rounding)
    physical index    quad 0  (slab R + row) ldc + col                                      fp32, plain (the 7x7 stems)
                      quad 1  ((slab R/4 + row/4) ldc + col) 4 + row%4                      fp32, rows interleaved by four
                      quad 2  ((slab R/8 + row/8) ldc + col) 8 + row%8                      bf16, rows interleaved by eight
                      quad 3  piece p of the quad 2 layout at p T R ldc + (quad 2 index)    three bf16 piece planes
    bf16              round to nearest, ties to even, on the bits
    three pieces      p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), every subtraction in float32; p0 + p1 + p2 == x exactly
                      for 2^-60 <= |x| <= 2^60 (and +-0): no piece is subnormal there, so the definition has no special cases
    Winograd operand  U = G g G^T in float64 -- columns first, t = G g, then rows, every half-sum 0.5 * (a +- b + c) --, rounded ONCE
                      to float32: x.  p0 = the float64 U rounded once to bf16 (equal to bf16(x) unless x is an exact bf16 tie: then the
                      neighbour U lay nearer to, not the even one), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1); p0 + p1 + p2 == x.
                      Laid out [cot][chunk][pos 16][piece 3][k half 2][co 64][8 reduction channels];
                      flip = 1: reduction channel = o, output channel = i, taps rotated by 180 degrees
    eval coefficients scale = gamma / sqrt(rv + eps), shift = beta - rm scale (here in float64: the yardstick, not the bits)

`mode` swaps in ONE shortcut a kernel could plausibly take, to show that the fixtures tell it apart from the contract (MODES)."""
import ctypes as C

import numpy as np

F = np.float32
MODES = ("exact",
         "truncate",                # bf16 by dropping the low 16 bits
         "half_up",                 # bf16 ties away from zero
         "two_pieces",              # p2 = 0
         "scale_after_round",       # the fold applied to the value already rounded to bf16
         "scale_by_row_when_col",   # scale_col ignored: scale[o] where scale[i] is meant (index taken modulo the scale's length)
         "wino_round_twice",        # G g rounded to float32 before the second product
         "wino_flip_no_rotation",   # flip = 1 transposes the channels but leaves the taps where they are
         "wino_p0_from_float",      # p0 = bf16(fp32(U)), the plain three-piece split of the rounded value: differs from the operand's
                                    # p0 (the double rounded once to bf16) where fp32(U) is an exact bf16 tie and the double is not
         "quad4_for_bf16")          # the by-four interleave used for a bf16 operand
RANGE_LOG2 = 60                    # |x| in [2^-60, 2^60]: the range the piece definition is stated (and tested) for
WINO_CHUNK_ELEMS = 16 * 3 * 2 * 64 * 8          # bf16 elements of one [pos][piece][k half][co][8] block: 16 reduction x 64 output channels


# ------------------------------------------------------------------------------------------------ bit-level conversions
def _f32(x):
    return np.ascontiguousarray(x, dtype=F)


def bf16_rne(x32, mode="exact"):
    """float32 -> bf16 bits (uint16), round to nearest even on the bits (finite values)."""
    b = _f32(x32).view(np.uint32).astype(np.uint64)
    if mode == "truncate":
        r = b
    elif mode == "half_up":
        r = b + 0x8000
    else:
        r = b + 0x7fff + ((b >> 16) & 1)
    return (r >> 16).astype(np.uint16)


def bf16_to_f32(u16):
    return (np.asarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(F)


def split3(x32, mode="exact"):
    """-> (p0, p1, p2) bf16 bits of the three pieces of a float32 array."""
    x = _f32(x32)
    p0 = bf16_rne(x, mode)
    r1 = x - bf16_to_f32(p0)
    p1 = bf16_rne(r1, mode)
    r2 = r1 - bf16_to_f32(p1)
    assert r1.dtype == F and r2.dtype == F
    p2 = np.zeros_like(p0) if mode == "two_pieces" else bf16_rne(r2, mode)
    return p0, p1, p2


def rounding_ladder():
    """The float32 values at which a bf16 rounding can go wrong, built deterministically: for several exponents inside
    [2^-60, 2^60] and both signs -- the exact ties (low half 0x8000) over an even and an odd kept mantissa, their float32 neighbours on
    either side, a tie whose carry runs through the kept mantissa into the exponent, a mantissa of all ones -- and +-0."""
    out = []
    for e in (-RANGE_LOG2, -20, -3, 0, 1, 7, RANGE_LOG2 - 1):
        for sign in (0, 1):
            head = (sign << 31) | ((e + 127) << 23)
            for kept in (0x00, 0x01, 0x2a, 0x55, 0x7e, 0x7f):          # even, odd, ..., 0x7f: the carry reaches the exponent
                for low in (0x7fff, 0x8000, 0x8001):
                    out.append(head | (kept << 16) | low)
            out.append(head | 0x7fffff)
            out.append(head)
    out += [0x00000000, 0x80000000]
    v = np.array(out, dtype=np.uint32).view(F)
    a = np.abs(v[v != 0])
    assert a.min() >= F(2.0) ** -RANGE_LOG2 and a.max() <= F(2.0) ** RANGE_LOG2
    return v


# ------------------------------------------------------------------------------------------------ physical index maps
def phys_index(quad, T, R, ldc, slab, row, col, mode="exact"):
    """Element index of L[slab][row][col] inside ONE plane of T * R * ldc elements (quad 3: add piece * T * R * ldc)."""
    slab, row, col = (np.asarray(a, dtype=np.int64) for a in (slab, row, col))
    if quad == 0:
        return (slab * R + row) * ldc + col
    k = 4 if (quad == 1 or mode == "quad4_for_bf16") else 8
    assert R % k == 0, "the reduction rows come in groups of %d" % k
    return ((slab * (R // k) + row // k) * ldc + col) * k + row % k


def plane_elems(T, R, ldc):
    return T * R * ldc


def logical(w, O, I, T, off, transpose, scale=None, scale_col=0, mode="exact"):
    """-> (slab, row, col, value) of every element an OIHW tensor contributes, value folded in float32."""
    w = _f32(w).reshape(O, I, T)
    o, i, t = np.meshgrid(np.arange(O), np.arange(I), np.arange(T), indexing="ij")
    v = w
    if scale is not None:
        s = _f32(scale)
        by_col = bool(scale_col) and mode != "scale_by_row_when_col"
        f = s[i % len(s)] if by_col else s[o % len(s)]
        assert (len(s) == (I if scale_col else O))
        v = bf16_to_f32(bf16_rne(w)) * f if mode == "scale_after_round" else w * f
        assert v.dtype == F
    if transpose:
        return t.ravel(), (off + o).ravel(), i.ravel(), v.ravel()
    return t.ravel(), i.ravel(), (off + o).ravel(), v.ravel()


def pack_into(dst, w, O, I, T, ldc, off, rows_total, transpose, quad, scale=None, scale_col=0, base=0, mode="exact"):
    """Write what ONE pack job owns into dst (1-D: uint32 bit patterns for quad 0 / 1, uint16 for quad 2 / 3), the operand starting
    at element `base`; everything else is left alone.  -> the indices written."""
    R = rows_total if transpose else I
    slab, row, col, v = logical(w, O, I, T, off, transpose, scale, scale_col, mode)
    assert row.max() < R and col.max() < ldc and off >= 0, "the job leaves its operand"
    idx = base + phys_index(quad, T, R, ldc, slab, row, col, mode)
    if quad in (0, 1):
        assert dst.dtype == np.uint32
        dst[idx] = v.view(np.uint32)
        return idx
    assert dst.dtype == np.uint16
    if quad == 2:
        dst[idx] = bf16_rne(v, mode)
        return idx
    plane = plane_elems(T, R, ldc)
    for p, piece in enumerate(split3(v, mode)):
        dst[idx + p * plane] = piece
    return np.concatenate([idx, idx + plane, idx + 2 * plane])


# ------------------------------------------------------------------------------------------------ Winograd F(2x2, 3x3)
def wino_gggt(g, mode="exact"):
    """G g G^T of [..., 3, 3] float64 filters -> [..., 4, 4] float64, in the order the source states: columns first (t = G g), then
    rows; G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]."""
    g = np.asarray(g, dtype=np.float64)
    t = np.stack([g[..., 0, :], 0.5 * (g[..., 0, :] + g[..., 1, :] + g[..., 2, :]), 0.5 * (g[..., 0, :] - g[..., 1, :] + g[..., 2, :]),
                  g[..., 2, :]], axis=-2)                                                   # [..., 4, 3]
    if mode == "wino_round_twice":
        t = t.astype(F).astype(np.float64)
    return np.stack([t[..., 0], 0.5 * (t[..., 0] + t[..., 1] + t[..., 2]), 0.5 * (t[..., 0] - t[..., 1] + t[..., 2]), t[..., 2]], axis=-1)


def wino_packed_elems(O, I, flip):
    R, Q = (O, I) if flip else (I, O)
    return ((Q + 63) // 64) * (R // 16) * WINO_CHUNK_ELEMS


def wino_u(w, flip=0, mode="exact"):
    """The packed Winograd operand (uint16 bf16 bits) of an OIHW [O][I][3][3] tensor."""
    w = _f32(w)
    O, I = w.shape[:2]
    g = w.reshape(O, I, 3, 3)
    if flip:
        g = g.transpose(1, 0, 2, 3)                          # [output channel = i][reduction channel = o]
        if mode != "wino_flip_no_rotation":
            g = g[:, :, ::-1, ::-1]
    Q, R = g.shape[:2]
    assert R % 16 == 0 and Q % 64 == 0
    u64 = wino_gggt(g.astype(np.float64), mode).reshape(Q, R, 16)                   # pos = 4 * row + column
    u = u64.astype(F)                                                               # rounded once
    pieces = np.stack(split3(u, mode))                                              # [piece][q][r][pos]
    if mode not in ("wino_p0_from_float", "truncate", "half_up", "two_pieces"):
        b = np.ascontiguousarray(u64).view(np.uint64)
        direct = (((b + ((1 << 44) - 1) + ((b >> 45) & 1)) >> 45) << 45).view(np.float64).astype(F)      # nearest even at 8 significant bits
        p0 = (direct.view(np.uint32) >> 16).astype(np.uint16)
        r1 = u - bf16_to_f32(p0)
        p1 = bf16_rne(r1)
        pieces = np.stack([p0, p1, bf16_rne(r1 - bf16_to_f32(p1))])
    n_cot, n_chunk = Q // 64, R // 16
    x = pieces.reshape(3, n_cot, 64, n_chunk, 2, 8, 16)                             # [piece][cot][co][chunk][k half][k][pos]
    return np.ascontiguousarray(x.transpose(1, 3, 6, 0, 4, 2, 5)).reshape(-1)      # [cot][chunk][pos][piece][k half][co][k]


# ------------------------------------------------------------------------------------------------ eval-mode BatchNorm coefficients
def eval_coeffs(gamma, beta, rm, rv, eps):
    g, b, m, v = (np.asarray(a, dtype=F).astype(np.float64) for a in (gamma, beta, rm, rv))
    scale = g / np.sqrt(v + float(F(eps)))
    return scale, b - m * scale


def coeff_bars(scale64, shift64, rm):
    """The derived bars: add, sqrt, divide, multiply are four roundings of at most one ulp each (2.5 for a division the compiler need not
    round correctly) -> 8 * 2^-24 |scale|; shift = beta - (rm gamma) r, contracted or not -> 2^-24 (|shift| + 10 |rm scale|)."""
    u = 2.0 ** -24
    return 8 * u * np.abs(scale64), u * (np.abs(shift64) + 10 * np.abs(np.asarray(rm, dtype=np.float64) * scale64))


# ------------------------------------------------------------------------------------------------ the device job records (documented ABI)
class PackJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("scale", C.c_void_p), ("O", C.c_int32), ("I", C.c_int32), ("T", C.c_int32),
                ("ldc", C.c_int32), ("off", C.c_int32), ("rows_total", C.c_int32), ("transpose", C.c_int32), ("first_block", C.c_int32),
                ("quad", C.c_int32), ("scale_col", C.c_int32)]


class WinoJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("u", C.c_void_p), ("O", C.c_int32), ("I", C.c_int32), ("flip", C.c_int32), ("first_block", C.c_int32)]


class EvalCoefJob(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("C", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(PackJob) == 64 and C.sizeof(WinoJob) == 32 and C.sizeof(EvalCoefJob) == 56


def pack_blocks(O, I, T, chunk):
    """Blocks a pack job owns: ceil(O I T / rd_pack_chunk())."""
    return -(-(O * I * T) // chunk)


def block_table(counts):
    """-> (first_block of every job, block_job[b]) for jobs that take counts[k] consecutive blocks each."""
    first, table, nb = [], [], 0
    for k, n in enumerate(counts):
        first.append(nb)
        table += [k] * n
        nb += n
    return first, np.array(table, dtype=np.int32)


def records(structs):
    """ctypes records -> the bytes to upload (uint8 array)."""
    arr = (type(structs[0]) * len(structs))(*structs)
    return np.frombuffer(bytes(arr), dtype=np.uint8).copy()

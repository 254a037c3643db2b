"""float64 reference of rd_wino_conv3x3 / rd_wino_conv3x3_bnbwd (csrc/wino_split.hip), written from the operation and from
include/radar_depth_hip.h, not from the kernel's index arithmetic: a plain 3x3 / stride 1 / pad 1 convolution of an NHWC tensor
(forward: OIHW weights; input gradient: the transposed convolution of dy, i.e. the same sum over channel-transposed, 180-degree rotated
taps), the optional addend, the BatchNorm partial sums of the stored values and, for the _bnbwd form, sum g and sum g (x - mean) with
g = dx * act'(scale x + shift), ReLU or LeakyReLU(0.2).  No torch.

Beside it: the magnitude S of a result in the Winograd domain (what the per-element bar of tests/wino_cases.py is a multiple of) and
emulate(), the documented arithmetic -- B^T d B in float32, three bf16 pieces, U = G g G^T as rd_wino_pack lays it down, the six kept
piece products, A^T m A -- with every sum after the pieces taken exactly, and any of the six terms removable.

`mode` swaps in ONE shortcut a kernel could plausibly take (MODES); tests/test_wino_host.py shows that each leaves a bar or an exact
check on a committed case."""
import numpy as np

import pack_ref as PK

F, D = np.float32, np.float64
U = 2.0 ** -24
SLOPE = 0.2
ACT_RELU, ACT_LEAKY = 1, 2
MODES = ("exact",
         "taps_not_rotated",              # flip: channels transposed, taps left where they are
         "channels_not_transposed",       # flip: taps rotated, g[q][r] = w[q][r] (shows where O == I)
         "row_wrap",                      # a patch pixel left / right of the image = the flat neighbour: the end / start of the next row
         "next_image",                    # a patch row above / below the image = the previous / next image's last / first row
         "masked_counted",                # the masked last tile row / column (odd H / W) counted in the statistics
         "stats_unrounded",               # the statistics of the float64 values, not of the stored float32 ones
         "addend_at_out_stride",          # the addend read with the output's channel stride
         "bn_x_at_out_stride",            # bn_x read with the output's channel stride
         "no_mean",                       # slot 1 = sum g x
         "relu_for_leaky")                # act' = 0 on the negative side where 0.2 was asked
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], D)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], D)
# the piece products RD_SPLIT_TERMS keeps: (piece of the transformed patch, piece of U); a1 b2, a2 b1, a2 b2 are dropped
KEPT = ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (1, 1))


def eff_weights(w, flip, mode="exact"):
    """g[q][r][a][b] with out[n, y, x, q] = sum_{a, b, r} in[n, y + a - 1, x + b - 1, r] g[q][r][a][b], float64."""
    g = np.asarray(w, D)
    if not flip:
        return g
    if mode != "channels_not_transposed":
        g = g.transpose(1, 0, 2, 3)
    return g if mode == "taps_not_rotated" else g[:, :, ::-1, ::-1]


def _padded(x, mode):
    N, H, W, C = x.shape
    p = np.zeros((N, H + 2, W + 2, C), D)
    p[:, 1:H + 1, 1:W + 1] = x
    if mode == "row_wrap":
        p[:, 2:H + 1, 0] = x[:, :H - 1, W - 1]
        p[:, 1:H, W + 1] = x[:, 1:, 0]
    if mode == "next_image":
        p[:-1, H + 1, 1:W + 1] = x[1:, 0]
        p[1:, 0, 1:W + 1] = x[:-1, H - 1]
    return p


def conv(x, w, flip=False, mode="exact"):
    """x [N,H,W,R] -> (out [N,H,W,Q], sum |x||g|) float64."""
    x = np.asarray(x, D)
    N, H, W, _ = x.shape
    g = eff_weights(w, flip, mode)
    p, pa = _padded(x, mode), _padded(np.abs(x), "exact")
    out, mag = 0.0, 0.0
    for a in range(3):
        for b in range(3):
            out = out + p[:, a:a + H, b:b + W] @ g[:, :, a, b].T
            mag = mag + pa[:, a:a + H, b:b + W] @ np.abs(g[:, :, a, b]).T
    return out, mag


def conv_masked_extent(x, w, flip=False):
    """The convolution on the extent the tiles cover, [N, 2 ceil(H/2), 2 ceil(W/2), Q]: what a kernel holds for the masked last tile
    row / column (the image continued by zeros)."""
    N, H, W, C = x.shape
    xe = np.zeros((N, H + H % 2, W + W % 2, C), D)
    xe[:, :H, :W] = x
    return conv(xe, w, flip)[0]


def wino_magnitude(x, w, flip=False):
    """S [N,H,W,Q] = sum_{i,j} |A^T[r,i]| |A^T[s,j]| sum_r |U_ij| (|B^T| |d| |B|)_ij: the magnitude of a result in the Winograd domain
    (U = G g G^T rounded to float32, as the kernel reads it).  The transform's cancellation is the kernel's to pay for."""
    x = np.abs(np.asarray(x, D))
    N, H, W, C = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    ua = np.abs(PK.wino_gggt(eff_weights(w, flip)).astype(F).astype(D))                  # [Q][R][4][4]
    p = np.zeros((N, 2 * th + 2, 2 * tw + 2, C), D)
    p[:, 1:H + 1, 1:W + 1] = x
    d = np.stack([np.stack([p[:, a:a + 2 * th:2, b:b + 2 * tw:2] for b in range(4)], 3) for a in range(4)], 3)      # [N][th][tw][a][b][C]
    v = np.einsum("ia,ntxabc,jb->ntxijc", np.abs(BT), d, np.abs(BT), optimize=True)
    m = np.einsum("ntxijc,qcij->ntxijq", v, ua, optimize=True)
    s = np.einsum("ri,ntxijq,sj->ntrxsq", np.abs(AT), m, np.abs(AT), optimize=True)
    return s.reshape(N, 2 * th, 2 * tw, -1)[:, :H, :W]


def window(buf, rows, C, ld, c0):
    """Channels [c0, c0 + C) of `rows` pixels of a flat buffer read with channel stride ld (NaN where the read leaves the buffer)."""
    buf = np.asarray(buf).reshape(-1)
    idx = (np.arange(rows)[:, None] * ld + c0 + np.arange(C)[None]).reshape(-1)
    out = np.full(idx.size, np.nan, D)
    ok = idx < buf.size
    out[ok] = buf[idx[ok]]
    return out.reshape(rows, C)


def act_slope(z, act, mode="exact"):
    neg = 0.0 if (act == ACT_RELU or mode == "relu_for_leaky") else SLOPE
    return np.where(np.asarray(z, D) > 0, 1.0, neg)


def stats(y):
    """y [..., Q] float64 -> (sum, sum of squares, sum |y|) per channel."""
    y = np.asarray(y, D).reshape(-1, y.shape[-1])
    return y.sum(0), (y * y).sum(0), np.abs(y).sum(0)


def bn_terms(dx, bn_x, mean, scale, shift, act, mode="exact"):
    """-> (sum g, sum g (x - mean), sum |g|, sum |g| |x - mean|) per channel, g = dx * act'(scale x + shift), float64."""
    dx, x = np.asarray(dx, D).reshape(-1, dx.shape[-1]), np.asarray(bn_x, D).reshape(-1, dx.shape[-1])
    m, s, t = (np.asarray(a, D) for a in (mean, scale, shift))
    g = dx * act_slope(s * x + t, act, mode)
    xm = x if mode == "no_mean" else x - m
    return g.sum(0), (g * xm).sum(0), np.abs(g).sum(0), np.abs(g * xm).sum(0)


# ------------------------------------------------------------------------------------------------ the documented arithmetic
def u_pieces(w, flip=False):
    """The three bf16 pieces of U as rd_wino_pack lays them down (pack_ref.wino_u), as float64 [piece][q][r][pos]."""
    O, I = np.asarray(w).shape[:2]
    R, Q = (O, I) if flip else (I, O)
    packed = PK.wino_u(w, flip).reshape(Q // 64, R // 16, 16, 3, 2, 64, 8)            # [cot][chunk][pos][piece][k half][co][k]
    return PK.bf16_to_f32(packed.transpose(3, 0, 5, 1, 4, 6, 2).reshape(3, Q, R, 16)).astype(D)


def v_pieces(x):
    """B^T d B of every tile in float32 (rows first, then columns: one rounding each), split into three bf16 pieces:
    float64 [piece][N][th][tw][pos][C]."""
    x = np.asarray(x, F)
    N, H, W, C = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    p = np.zeros((N, 2 * th + 2, 2 * tw + 2, C), F)
    p[:, 1:H + 1, 1:W + 1] = x
    r = [[p[:, a:a + 2 * th:2, b:b + 2 * tw:2] for b in range(4)] for a in range(4)]
    t = [[r[0][c] - r[2][c], r[1][c] + r[2][c], r[2][c] - r[1][c], r[1][c] - r[3][c]] for c in range(4)]            # t[c][i]
    v = np.stack([np.stack([t[0][i] - t[2][i], t[1][i] + t[2][i], t[2][i] - t[1][i], t[1][i] - t[3][i]], 3) for i in range(4)], 3)
    assert v.dtype == F and v.shape == (N, th, tw, 4, 4, C)
    v = v.reshape(N, th, tw, 16, C)
    return np.stack([PK.bf16_to_f32(b).astype(D).reshape(v.shape) for b in PK.split3(v)]), v


def emulate(x, w, flip=False, drop=None):
    """The kernel's arithmetic with exact sums behind the pieces: [N,H,W,Q] float64.  drop = one of KEPT: that product is left out."""
    N, H, W, _ = np.asarray(x).shape
    vp, _ = v_pieces(x)
    up = u_pieces(w, flip)
    m = 0.0
    for (a, b) in KEPT:
        if (a, b) != drop:
            m = m + np.einsum("ntxpc,qcp->ntxpq", vp[a], up[b], optimize=True)
    m = m.reshape(m.shape[:3] + (4, 4, -1))
    y = np.einsum("ri,ntxijq,sj->ntrxsq", AT, m, AT, optimize=True)
    return y.reshape(N, m.shape[1] * 2, m.shape[2] * 2, -1)[:, :H, :W]

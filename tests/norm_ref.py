"""Training-mode BatchNorm + activation + residual joins and the stem's fused BN / activation / max-pool, restated in numpy float64
from include/radar_depth_hip.h ("BatchNorm2d (training mode) + activation + residual join": conventions, tile geometry).  Every
function takes what the C entry point takes -- flat buffers with strides and channel offsets -- and returns float64.

tests/test_norm_host.py proves the restatement against torch float64 autograd and ATen's max_pool2d; tests/test_gpu_norm_fp64.py
holds the fp32 kernels of csrc/norm_act.hip to it.  `mode` selects one named shortcut (MODES): what a subtly wrong kernel would
compute.  The case list of tests/norm_cases.py has to notice every one of them."""
import numpy as np

D = np.float64
U = 2.0 ** -24                    # unit roundoff of fp32
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
SLOPE = 0.2                       # (the kernels multiply by 0.2f: the GPU tests pass float(np.float32(0.2)))

MODES = ("c0_ignored", "ld_as_C", "last_tile_dropped", "tiles_from_768_dropped", "biased_running_var", "momentum_term_dropped",
         "count_minus_1_at_1", "nbt_not_incremented", "var_not_clamped", "mean_not_subtracted", "which_swapped", "relu_grad_1_at_0",
         "leaky_grad_1_at_0", "last_max_wins", "window_clipped", "K_dropped", "neighbour_column")


# ------------------------------------------------------------------------------------------------ tile geometry (header)
def cdiv(a, b):
    return -(-a // b)


def row_lanes(C):
    return max(1, 256 // (C // 4))


def rows_per_block(M):
    return max(64, cdiv(M, 2048))


def bwd_rows_per_block(M, C):
    return max(min(64, 4 * row_lanes(C)), cdiv(M, 2048))


def stats_tiles(M):
    return cdiv(M, rows_per_block(M))


def bwd_tiles(M, C):
    return cdiv(M, bwd_rows_per_block(M, C))


def chain(M, C, bwd):
    """Longest fp32 summation chain of one partial sum: the rows one thread adds, the RL lane sums added through LDS, one for the
    product."""
    rpb, RL = min(M, bwd_rows_per_block(M, C) if bwd else rows_per_block(M)), row_lanes(C)
    return cdiv(rpb, RL) + RL + 1


def pool_chain(N, H, W, C, tiles):
    """The same for the pool backward's sums: a thread adds the four positions of each 2 x 2 block it owns, one block per grid trip."""
    items = N * cdiv(H, 2) * cdiv(W, 2) * (C // 4)
    return 4 * cdiv(items, tiles * 256) + row_lanes(C) + 1


def window(buf, rows, ld, c0, C):
    """Channels [c0, c0 + C) of a flat buffer of `rows` rows with stride ld (a view)."""
    return np.asarray(buf).reshape(-1)[:rows * ld].reshape(rows, ld)[:, c0:c0 + C]


# ------------------------------------------------------------------------------------------------ finalize
def tile_sums(part, n_tiles, slots, ld, c0, C, mode="exact"):
    """Sum over the tiles of part [n_tiles][slots][ld], channels [c0, c0 + C), in float64 -> [slots][C]."""
    if mode == "ld_as_C":
        ld = C
    if mode == "c0_ignored":
        c0 = 0
    flat = np.asarray(part, dtype=D).reshape(-1)
    t, s, c = np.meshgrid(np.arange(n_tiles), np.arange(slots), c0 + np.arange(C), indexing="ij")
    at = (t * slots + s) * ld + c          # (a shortcut's wrong stride may point anywhere: past the end reads as NaN)
    p = np.where(at < flat.size, flat[np.minimum(at, flat.size - 1)], np.nan)
    if mode == "last_tile_dropped":
        p = p[:n_tiles - 1]
    if mode == "tiles_from_768_dropped":
        p = p[:768]
    return p.sum(0)


def finalize(part, n_tiles, ld, c0, C, count, gamma, beta, eps, momentum, rm, rv, nbt, mode="exact"):
    """rd_bn_finalize.  rm / rv / nbt: the running statistics before the call, or None (NULL).  -> dict of mean, invstd, scale,
    shift, rm, rv, nbt (after the call) and shift_terms = |beta| + |mean * gamma * invstd| for the bar on shift."""
    s, q = tile_sums(part, n_tiles, 2, ld, c0, C, mode)
    g, b, count = np.asarray(gamma, D), np.asarray(beta, D), float(count)
    with np.errstate(all="ignore"):
        m = s / count
        var = q / count - m * m
        if mode != "var_not_clamped":
            var = np.maximum(var, 0.0)
        r = 1.0 / np.sqrt(var + eps)
        out = dict(mean=m, invstd=r, scale=g * r, shift=b - m * g * r, shift_terms=np.abs(b) + np.abs(m * g * r), rm=None, rv=None, nbt=None)
        if rm is not None:
            bessel = count > 1.0 or mode == "count_minus_1_at_1"
            unbiased = var if (mode == "biased_running_var" or not bessel) else var * count / (count - 1.0)
            keep = 0.0 if mode == "momentum_term_dropped" else 1.0 - momentum
            out["rm"] = keep * np.asarray(rm, D) + momentum * m
            out["rv"] = keep * np.asarray(rv, D) + momentum * unbiased
    if nbt is not None:
        out["nbt"] = int(nbt) + (0 if mode == "nbt_not_incremented" else 1)
    return out


def stats_sums(x):
    """rd_bn_stats, summed over the tiles: (sum x, sum x^2) and the sums of the absolute terms (the bars), per channel."""
    x = np.asarray(x, D)
    return np.stack([x.sum(0), (x * x).sum(0)]), np.stack([np.abs(x).sum(0), (x * x).sum(0)])


# ------------------------------------------------------------------------------------------------ activation
def act_fwd(z, act, slope=SLOPE):
    if act == ACT_RELU:
        return np.where(z > 0, z, 0.0)          # (-0.0 and every z <= 0 give +0.0)
    if act == ACT_LEAKY:
        return np.where(z > 0, z, slope * z)
    return z


def act_grad(out, act, slope=SLOPE, mode="exact"):
    """Derivative on the activation's output (or pre-activation: same sign).  At exactly 0 (either sign): ReLU 0, LeakyReLU slope."""
    if act == ACT_RELU:
        return np.where((out >= 0) if mode == "relu_grad_1_at_0" else (out > 0), 1.0, 0.0)
    if act == ACT_LEAKY:
        return np.where((out >= 0) if mode == "leaky_grad_1_at_0" else (out > 0), 1.0, slope)
    return np.ones_like(out)


def pre_act(x1, s1, t1, x2=None, s2=None, t2=None, fp32=False):
    """z = s1*x1 + t1 [+ (s2*x2 + t2 | x2)] and the sum of its absolute addends.  fp32: each affine part is rounded to fp32 before
    the sum, and so is the sum, as the kernels' fmaf / add do -- what decides a recomputed SIGN must see the same cancellations."""
    rnd = (lambda a: a.astype(np.float32).astype(D)) if fp32 else (lambda a: a)
    x1 = np.asarray(x1, D)
    z, terms = rnd(s1 * x1 + t1), np.abs(s1 * x1) + np.abs(t1)
    if x2 is not None:
        x2 = np.asarray(x2, D)
        if s2 is not None:
            z, terms = rnd(z + rnd(s2 * x2 + t2)), terms + np.abs(s2 * x2) + np.abs(t2)
        else:
            z, terms = rnd(z + x2), terms + np.abs(x2)
    return z, terms


def bn_act(x1, s1, t1, x2, s2, t2, act, slope=SLOPE):
    """rd_bn_act in its three residual forms (x2 None: none; s2 None: identity; else bn) -> (y, sum of absolute addends)."""
    z, terms = pre_act(x1, s1, t1, x2, s2, t2)
    return act_fwd(z, act, slope), terms


# ------------------------------------------------------------------------------------------------ backward
def bwd_g(dy, sign_src, act, slope=SLOPE, mode="exact"):
    """g = dy * act'(.): sign_src is y (rd_bn_bwd_reduce) or the recomputed pre-activation (the _x / _x2 forms, the pool backward)."""
    return np.asarray(dy, D) * act_grad(sign_src, act, slope, mode)


def bwd_sums(g, x1=None, m1=None, x2=None, m2=None, mode="exact"):
    """The three backward sums (g, g*(x1 - m1), g*(x2 - m2)) over the rows and the sums of their absolute terms -> [3][C] each."""
    g = np.asarray(g, D)
    s, a = np.zeros((3, g.shape[-1])), np.zeros((3, g.shape[-1]))
    s[0], a[0] = g.sum(0), np.abs(g).sum(0)
    for k, (x, m) in ((1, (x1, m1)), (2, (x2, m2))):
        if x is not None:
            t = g * (np.asarray(x, D) - (0.0 if mode == "mean_not_subtracted" else m))
            s[k], a[k] = t.sum(0), np.abs(t).sum(0)
    return s, a


def bwd_coeffs(part, n_tiles, C, which, count, gamma, invstd, mode="exact"):
    """bn_bwd_coeffs_kernel on red_partial [n_tiles][3][C] -> dgamma, dbeta, A, B, K (header: dx = A*g + B*(x - mean) + K)."""
    sums = tile_sums(part, n_tiles, 3, C, 0, C, mode)
    s0, sw = sums[0], sums[(3 - which) if mode == "which_swapped" else which]
    r, gm, count = np.asarray(invstd, D), np.asarray(gamma, D), float(count)
    A = gm * r
    return dict(dgamma=r * sw, dbeta=s0, A=A, B=-gm * r * r * r * sw / count, K=-A * s0 / count)


def bwd_dx(g, x, mean, A, B, K, mode="exact"):
    """dx = A*g + B*(x - mean) + K and the sum of the absolute addends."""
    g, x = np.asarray(g, D), np.asarray(x, D)
    if mode == "K_dropped":
        K = np.zeros_like(K)
    return A * g + B * (x - mean) + K, np.abs(A * g) + np.abs(B * (x - mean)) + np.abs(K)


# ------------------------------------------------------------------------------------------------ max-pool 3x3 / 2 / 1
def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def _taps(H, W, mode="exact"):
    """(kh, kw, output rows, output columns, input rows, input columns) of every window position that lies inside the image."""
    Ho, Wo = pool_out(H), pool_out(W)
    He, We = (H - 1, W - 1) if mode == "window_clipped" else (H, W)
    for kh in range(3):
        for kw in range(3):
            oh = np.array([o for o in range(Ho) if 0 <= 2 * o - 1 + kh < He], dtype=np.int64)
            ow = np.array([o for o in range(Wo) if 0 <= 2 * o - 1 + kw < We], dtype=np.int64)
            if oh.size and ow.size:
                yield kh, kw, oh, ow, 2 * oh - 1 + kh, 2 * ow - 1 + kw


def pool_fwd(z, mode="exact"):
    """z [N,H,W,C] (after the activation) -> (y [N,Ho,Wo,C], idx uint8 = kh*3+kw).  Positions outside the image are skipped; among
    equal maxima the FIRST in (kh, kw) order wins (a later one replaces the best only if it is strictly greater)."""
    z = np.asarray(z, D)
    N, H, W, C = z.shape
    Ho, Wo = pool_out(H), pool_out(W)
    best, idx, have = np.zeros((N, Ho, Wo, C)), np.zeros((N, Ho, Wo, C), np.uint8), np.zeros((N, Ho, Wo, C), bool)
    for kh, kw, oh, ow, ih, iw in _taps(H, W, mode):
        o = np.ix_(range(N), oh, ow, range(C))
        cand = z[np.ix_(range(N), ih, iw, range(C))]
        take = ~have[o] | ((cand >= best[o]) if mode == "last_max_wins" else (cand > best[o]))
        best[o] = np.where(take, cand, best[o])
        idx[o] = np.where(take, kh * 3 + kw, idx[o])
        have[o] = True
    return best, idx


def pool_pick(a, idx):
    """a [N,H,W,C] at the position each window's argmax code names -> [N,Ho,Wo,C]."""
    a = np.asarray(a, D)
    N, H, W, C = a.shape
    out = np.full(idx.shape, np.nan)
    for kh, kw, oh, ow, ih, iw in _taps(H, W):
        o = np.ix_(range(N), oh, ow, range(C))
        out[o] = np.where(idx[o] == kh * 3 + kw, a[np.ix_(range(N), ih, iw, range(C))], out[o])
    return out


def pool_gather(dy, idx, H, W):
    """Sum of dy over the windows whose argmax is (h, w) -> ([N,H,W,C], the sum of the absolute contributions)."""
    dy = np.asarray(dy, D)
    N, _, _, C = dy.shape
    s, a = np.zeros((N, H, W, C)), np.zeros((N, H, W, C))
    for kh, kw, oh, ow, ih, iw in _taps(H, W):
        o, i = np.ix_(range(N), oh, ow, range(C)), np.ix_(range(N), ih, iw, range(C))
        d = np.where(idx[o] == kh * 3 + kw, dy[o], 0.0)
        s[i] += d
        a[i] += np.abs(d)
    return s, a


def pool_bwd(dy, idx, z, act, slope=SLOPE, mode="exact"):
    """rd_bnact_maxpool_bwd: g = act'(z) * gather, z = scale*x + shift at the full resolution -> (g, absolute contributions)."""
    s, a = pool_gather(dy, idx, z.shape[1], z.shape[2])
    k = act_grad(z, act, slope, mode)
    return s * k, a * k

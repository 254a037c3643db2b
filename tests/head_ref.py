"""The network head (csrc/head.hip) in numpy: the float64 reference of the 3x3 C=16 -> 1 convolution (forward, input gradient, weight
gradient) and of the bilinear align_corners=True resize (forward, backward) with the sums of absolute addends the bars are made of,
and an fp32 restatement of every kernel -- operation for operation, fmas emulated through float64 -- that takes a named shortcut
(MODES).  tests/head_cases.py holds the cases and the bars, tests/test_head_host.py shows that every shortcut leaves them.

Layouts: x, dx [N,H,W,C] (NHWC), w, dw [C,3,3] (OIHW with O == 1), d, dd [N,H,W], bilinear maps [N,H,W]."""
import numpy as np

import norm_bf16_cases as B

F, D = np.float32, np.float64
U = 2.0 ** -24
C = 16
PL = 64          # pixel lanes of a weight-gradient block (256 threads / 4 channel quads)
MODES = ("taps_transposed", "dgrad_unflipped", "wgrad_sign", "no_col_mask", "no_image_mask", "ld_as_C", "c0_ignored", "truncate", "half_up",
         "slab_dropped", "align_false", "i1_unclamped", "lx_swapped", "window_short")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ float64 reference: convolution
def _pad(a):
    a = np.asarray(a, D)
    return np.pad(a, [(0, 0), (1, 1), (1, 1)] + [(0, 0)] * (a.ndim - 3))


def conv_fwd(x, w):
    """d[n,h,w] = sum_{kh,kw,c} x[n,h+kh-1,w+kw-1,c] w[c,kh,kw] -> (d, the sum of the absolute addends)."""
    N, H, W, _ = x.shape
    xp, w = _pad(x), np.asarray(w, D)
    s, a = np.zeros((N, H, W)), np.zeros((N, H, W))
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + H, kw:kw + W]
            s += v @ w[:, kh, kw]
            a += np.abs(v) @ np.abs(w[:, kh, kw])
    return s, a


def conv_dgrad(dd, w):
    """dx[n,h,w,c] = sum_{kh,kw} dd[n,h-kh+1,w-kw+1] w[c,kh,kw] -> (dx, the sum of the absolute addends)."""
    N, H, W = dd.shape
    dp, w = _pad(dd), np.asarray(w, D)
    s, a = np.zeros((N, H, W, C)), np.zeros((N, H, W, C))
    for kh in range(3):
        for kw in range(3):
            g = dp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W, None]
            s += g * w[:, kh, kw]
            a += np.abs(g) * np.abs(w[:, kh, kw])
    return s, a


def conv_wgrad(x, dd):
    """dw[c,kh,kw] = sum_{n,h,w} x[n,h+kh-1,w+kw-1,c] dd[n,h,w] -> (dw, the sum of the absolute addends)."""
    N, H, W, _ = x.shape
    xp, dd = _pad(x), np.asarray(dd, D)
    s, a = np.zeros((C, 3, 3)), np.zeros((C, 3, 3))
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + H, kw:kw + W]
            s[:, kh, kw] = np.einsum("nhwc,nhw->c", v, dd)
            a[:, kh, kw] = np.einsum("nhwc,nhw->c", np.abs(v), np.abs(dd))
    return s, a


# ------------------------------------------------------------------------------------------------ the weight gradient's launch geometry
def wgrad_blocks(pixels, cap):
    """head_wgrad_blocks: cdiv(pixels, 512), at most cap (four blocks per CU)."""
    return max(1, min(cdiv(pixels, 512), cap))


def wgrad_regime(blocks, cap):
    return "one" if blocks == 1 else "direct" if blocks <= 16 else "cap" if blocks >= cap else "two_stage"


def wgrad_chain(pixels, blocks):
    """Roundings a term of dw[c][tap] can pass through, as head.hip and launch_slab_reduce are written:
      the lane's fmas            ceil(pix_per_block / 64), pix_per_block = cdiv(pixels, blocks)
      the serial LDS sum         63 additions (the first lane's value is added to 0: exact)
      the slab reduction         up to 16 slabs one serial sum over the slabs themselves: blocks - 1; above, every 16th slab into one of 16
                                 partial sums (cdiv(blocks, 16) - 1), then those 16 serially (15)."""
    depth = blocks - 1 if blocks <= 16 else cdiv(blocks, 16) - 1 + 15
    return cdiv(cdiv(pixels, blocks), PL) + (PL - 1) + depth


# ------------------------------------------------------------------------------------------------ float64 reference: bilinear
def coords(n_in, n_out):
    """Exact align_corners=True source coordinate of every output index."""
    return np.arange(n_out, dtype=D) * (n_in - 1) / (n_out - 1) if n_out > 1 else np.zeros(n_out)


def hat(n_in, n_out):
    """-> A [n_out, n_in], the hat-function weights max(0, 1 - |s(o) - i|), and B: delta(o) = 2u s(o) wherever |s(o) - i| < 1 + delta(o).
    The kernel's coordinate lies within delta of s(o) (one rounding of the scale, at most one of the product or of the fused
    product-minus-integer) and the hat function is 1-Lipschitz: |weight_kernel - A| <= B element-wise, before the weight's own roundings."""
    s = coords(n_in, n_out)[:, None]
    dist = np.abs(s - np.arange(n_in, dtype=D)[None])
    delta = 2 * U * s
    return np.maximum(0.0, 1.0 - dist), np.where(dist < 1 + delta, delta, 0.0) * np.ones_like(dist)


def bilinear_fwd(d, Ho, Wo):
    """-> (want [N,Ho,Wo], bar): 6u (Ay |d| Ax^T) -- 1 - lx, 1 - ly, two products and two additions per term -- plus the coordinate terms."""
    d = np.asarray(d, D)
    (Ay, By), (Ax, Bx) = hat(d.shape[1], Ho), hat(d.shape[2], Wo)
    a = np.abs(d)
    return Ay @ d @ Ax.T, 6 * U * (Ay @ a @ Ax.T) + By @ a @ Ax.T + Ay @ a @ Bx.T + By @ a @ Bx.T


def bilinear_bwd(dout, Hs, Ws):
    """-> (want [N,Hs,Ws], bar): the transpose, with (K + 4) u in place of 6u, K = the output pixels with a non-zero weight on the
    source pixel (the fmas of its gather; 1 - l, the sum of two weights on a clamped edge, the product of the two weights: 4)."""
    dout = np.asarray(dout, D)
    (Ay, By), (Ax, Bx) = hat(Hs, dout.shape[1]), hat(Ws, dout.shape[2])
    K = np.count_nonzero(Ay, axis=0)[:, None] * np.count_nonzero(Ax, axis=0)[None]
    a = np.abs(dout)
    return Ay.T @ dout @ Ax, (K + 4) * U * (Ay.T @ a @ Ax) + By.T @ a @ Ax + Ay.T @ a @ Bx + By.T @ a @ Bx


def bilinear_bwd_paths(Hs, Ws, Ho, Wo):
    """bilinear_bwd_kernel's candidate window per source pixel, restated in fp32 -> "fast" (every pixel takes the separable 8 x 8 form),
    "generic" (none does) or "mix"."""
    def span(n_in, n_out):
        sc = F(n_in - 1) / F(n_out - 1) if n_out > 1 else F(0)
        if sc == 0:
            return np.full(n_in, n_out - 1)
        inv, i = F(1) / sc, np.arange(n_in)
        lo = np.floor((i - 1).astype(F) * inv).astype(np.int64) - 1
        hi = np.ceil((i + 1).astype(F) * inv).astype(np.int64) + 1
        return np.minimum(hi, n_out - 1) - np.maximum(lo, 0)
    fast = (span(Hs, Ho)[:, None] < 8) & (span(Ws, Wo)[None] < 8)
    return "fast" if fast.all() else "mix" if fast.any() else "generic"


# ------------------------------------------------------------------------------------------------ fp32 restatement: what a kernel reads
def fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64; the sum is rounded to 53 bits before the 24 (double rounding: rare,
    half an ulp of the 53-bit sum)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(F)


def load(a, ld, c0, mode="exact"):
    """[N,H,W,C] as a kernel with the named shortcut reads it from its channel window (ld, c0) of the NaN-filled buffer."""
    a = np.asarray(a, F)
    return B._load(a.reshape(-1, a.shape[-1]), ld, c0, mode).reshape(a.shape)


def store(a, ld, c0, mode="exact"):
    """What the window (ld, c0) of the NaN-filled buffer holds after a kernel with the named shortcut stored [N,H,W,C] there."""
    a = np.asarray(a, F)
    rows = a.reshape(-1, a.shape[-1])
    if mode not in ("ld_as_C", "c0_ignored"):
        return a
    n, Cc = rows.shape
    buf = np.full(n * ld, np.nan, F)
    at = np.arange(n)[:, None] * (Cc if mode == "ld_as_C" else ld) + (c0 if mode == "ld_as_C" else 0) + np.arange(Cc)[None]
    buf[at] = rows
    return buf.reshape(n, ld)[:, c0:c0 + Cc].reshape(a.shape)


def neigh(a, dh, dw, mode="exact"):
    """a[n, h + dh, w + dw] for every pixel, 0 outside the image.  no_col_mask: only the row is checked (a column outside the image is the
    neighbouring row's first or last pixel in memory); no_image_mask: only the column (a row outside is the neighbouring image's); what
    lies before the first and behind the last image reads as 0."""
    a = np.asarray(a)
    N, H, W = a.shape[:3]
    n, h, w = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    ih, iw = h + dh, w + dw
    row_ok, col_ok = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
    ok = row_ok if mode == "no_col_mask" else col_ok if mode == "no_image_mask" else row_ok & col_ok
    idx = (n * H + ih) * W + iw
    ok = ok & (idx >= 0) & (idx < N * H * W)
    flat = a.reshape(N * H * W, -1)
    v = np.where(ok.reshape(-1, 1), flat[np.clip(idx, 0, N * H * W - 1).reshape(-1)], 0)
    return v.reshape(a.shape).astype(a.dtype)


def _tap(w, kh, kw, mode):
    return np.asarray(w, F)[:, kw, kh] if mode == "taps_transposed" else np.asarray(w, F)[:, kh, kw]


# ------------------------------------------------------------------------------------------------ fp32 restatement: convolution
def k_conv_fwd(x, w, tiled=True, mode="exact"):
    """head_conv_fwd_tiled_kernel (36 fmas per channel quad, taps outside, the quad's channels inside) or head_conv_fwd_kernel (per tap a
    four-term dot, then s = fma(ok, a, s)); the four quads are summed as the two DPP exchanges do: (s0 + s1) + (s2 + s3)."""
    x = np.asarray(x, F)
    N, H, W, _ = x.shape
    s = np.zeros((N, H, W, 4), F)
    with np.errstate(all="ignore"):
        for t in range(9):
            kh, kw = divmod(t, 3)
            v, wt = neigh(x, kh - 1, kw - 1, mode).reshape(N, H, W, 4, 4), _tap(w, kh, kw, mode).reshape(4, 4)
            if tiled:
                for j in range(4):
                    s = fma(v[..., j], wt[:, j], s)
            else:
                a = (v[..., 0] * wt[:, 0]).astype(F)
                for j in range(1, 4):
                    a = fma(v[..., j], wt[:, j], a)
                s = (a + s).astype(F)
        return ((s[..., 0] + s[..., 1]).astype(F) + (s[..., 2] + s[..., 3]).astype(F)).astype(F)


def k_conv_dgrad(dd, w, mode="exact"):
    """Both dgrad kernels: nine fmas in (kh, kw) order (a tap outside the image is skipped or multiplies a staged 0: the same bits)."""
    dd = np.asarray(dd, F)
    s = np.zeros(dd.shape + (C,), F)
    for kh in range(3):
        for kw in range(3):
            g = neigh(dd, kh - 1, kw - 1, mode) if mode == "dgrad_unflipped" else neigh(dd, 1 - kh, 1 - kw, mode)
            s = fma(g[..., None], _tap(w, kh, kw, mode), s)
    return s


def k_conv_wgrad(x, dd, blocks, mode="exact"):
    """head_conv_wgrad_kernel + launch_slab_reduce: block b owns pixels [b ppb, (b + 1) ppb), lane l the pixels b ppb + l + 64 k in
    increasing k; the 64 lanes are summed serially, the slabs as wgrad_chain describes."""
    x, dd = np.asarray(x, F), np.asarray(dd, F)
    P = dd.size
    ppb = cdiv(P, blocks)
    steps = cdiv(ppb, PL)
    sign = 1 if mode == "wgrad_sign" else -1
    g = np.stack([neigh(dd, sign * (t // 3 - 1), sign * (t % 3 - 1), mode).reshape(P) for t in range(9)], 1)          # [P, 9]
    xf = x.reshape(P, C)
    acc = np.zeros((blocks, PL, 9, C), F)
    for k in range(steps):
        off = k * PL + np.arange(PL)[None]
        idx = np.arange(blocks)[:, None] * ppb + off
        ok = (off < ppb) & (idx < P)
        idx = np.clip(idx, 0, P - 1)
        gv, xv = np.where(ok[..., None], g[idx], 0), np.where(ok[..., None], xf[idx], 0)
        acc = fma(gv[..., :, None], xv[..., None, :], acc)
    with np.errstate(all="ignore"):
        slabs = acc[:, 0]
        for l in range(1, PL):
            slabs = (slabs + acc[:, l]).astype(F)
        if mode == "slab_dropped":
            slabs = slabs[:-1] if blocks > 1 else np.zeros_like(slabs)
        J = min(len(slabs), 16)
        parts = []
        for j in range(J):
            s = slabs[j]
            for k in range(j + J, len(slabs), J):
                s = (s + slabs[k]).astype(F)
            parts.append(s)
        tot = parts[0]
        for s in parts[1:]:
            tot = (tot + s).astype(F)
    dw = np.ascontiguousarray(tot.T).reshape(C, 3, 3)
    return np.ascontiguousarray(dw.transpose(0, 2, 1)) if mode == "taps_transposed" else dw


# ------------------------------------------------------------------------------------------------ fp32 restatement: bilinear
def k_index(n_in, n_out, coord="fused", mode="exact", unclamped=False):
    """src_index for every output index -> (i0, i1, l1).  coord: "fused" -- l1 = fl(scale o - i0), what the compiled kernel does -- or
    "separate" -- fl(fl(scale o) - i0), ATen's."""
    o = np.arange(n_out).astype(F)
    if mode == "align_false":
        sc = F(n_in) / F(n_out)
        src = np.maximum((sc * (o + F(0.5))).astype(F) - F(0.5), F(0)).astype(F)
        exact = src.astype(D)
    else:
        sc = F(n_in - 1) / F(n_out - 1) if n_out > 1 else F(0)
        src = (sc * o).astype(F)
        exact = D(sc) * o.astype(D)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + 1 if unclamped else i0 + (i0 < n_in - 1)
    l1 = ((exact if coord == "fused" else src.astype(D)) - i0).astype(F)
    return i0, i1, np.clip(l1, F(0), F(1)).astype(F)


def k_bilinear_fwd(d, Ho, Wo, coord="fused", mode="exact"):
    """bilinear_fwd_kernel in plain fp32 (i1_unclamped: the row behind the last image is the NaN guard)."""
    d = np.asarray(d, F)
    N, Hs, Ws = d.shape
    y0, y1, ly = k_index(Hs, Ho, coord, mode, unclamped=mode == "i1_unclamped")
    x0, x1, lx = k_index(Ws, Wo, coord, mode)
    hy, hx = (F(1) - ly).astype(F), (F(1) - lx).astype(F)
    if mode == "lx_swapped":
        lx, hx = hx, lx
    rows = np.concatenate([d.reshape(N * Hs, Ws), np.full((1, Ws), np.nan, F)])
    at = lambda yy, xx: rows[(np.arange(N)[:, None, None] * Hs + yy[None, :, None]), xx[None, None, :]]
    hy, ly, hx, lx = hy[None, :, None], ly[None, :, None], hx[None, None, :], lx[None, None, :]
    with np.errstate(all="ignore"):
        top = ((hx * at(y0, x0)).astype(F) + (lx * at(y0, x1)).astype(F)).astype(F)
        bot = ((hx * at(y1, x0)).astype(F) + (lx * at(y1, x1)).astype(F)).astype(F)
        return ((hy * top).astype(F) + (ly * bot).astype(F)).astype(F)


def _gather_lists(n_in, n_out, coord, mode, short=False, swapped=False):
    """Per source index the output indices with a non-zero weight, in increasing order, and the weights as the kernel forms them
    (w = 0; if (i0 == i) w += 1 - l; if (i1 == i) w += l) -> (idx [n_in, K], weight [n_in, K]), padded with weight 0."""
    i0, i1, l = k_index(n_in, n_out, coord, mode)
    i = np.arange(n_in)[None]
    near, far = (l, (F(1) - l).astype(F)) if swapped else ((F(1) - l).astype(F), l)
    w = np.where(i0[:, None] == i, near[:, None], F(0)).astype(F)
    w = (w + np.where(i1[:, None] == i, far[:, None], F(0)).astype(F)).astype(F)          # [n_out, n_in]
    lists = [np.nonzero(w[:, k])[0] for k in range(n_in)]
    if short:
        lists = [v[:-1] for v in lists]
    K = max(1, max(len(v) for v in lists))
    idx, wt = np.zeros((n_in, K), np.int64), np.zeros((n_in, K), F)
    for k, v in enumerate(lists):
        idx[k, :len(v)], wt[k, :len(v)] = v, w[v, k]
    return idx, wt


def k_bilinear_bwd(dout, Hs, Ws, coord="fused", mode="exact"):
    """bilinear_bwd_kernel: s = fma(wy wx, dout[oy][ox], s) over the contributing output pixels, rows outside, columns inside
    (window_short: the last contributing row of every source pixel is missing from the candidate window)."""
    dout = np.asarray(dout, F)
    N, Ho, Wo = dout.shape
    iy, wy = _gather_lists(Hs, Ho, coord, mode, short=mode == "window_short")
    ix, wx = _gather_lists(Ws, Wo, coord, mode, swapped=mode == "lx_swapped")
    s = np.zeros((N, Hs, Ws), F)
    for j in range(iy.shape[1]):
        for i in range(ix.shape[1]):
            wgt = (wy[:, j][:, None] * wx[:, i][None]).astype(F)
            s = fma(wgt[None], dout[:, iy[:, j][:, None], ix[:, i][None]], s)
    return s

"""The cases tests/test_gpu_wino_fp64.py runs on the device and tests/test_wino_host.py shows to be sensitive to every shortcut of
wino_ref.MODES: shapes, data, the channel windows every operand lives in, the float64 results and the bars they are held to.

Output bar (u = 2^-24; per element, never a tensor-wide maximum; recounted against csrc/wino_split.hip):
    |out - want| <= K_OUT(R) u S,   S = sum_{i,j} |A^T[r,i]| |A^T[s,j]| sum_r |U_ij| (|B^T| |d| |B|)_ij + |addend|   (wino_ref.wino_magnitude)
    K_OUT(R) = 2                B^T d B: two levels of float32 additions (transform: t = rw -+ rw, then put(t -+ t)), one rounding each
             + 1                U: the float64 G g G^T rounded once to float32 (rd_wino_pack); its three pieces add up to it exactly,
                                and so do the three pieces of a transformed patch value (put: x - p0 and x - p0 - p1 are exact)
             + 3                the dropped products a1 b2, a2 b1, a2 b2: |a1| <= 2^-8 |a|, |a2| <= 2^-16 |a| (half an ulp of an 8-bit
                                significand, twice), so together (2^-24 + 2^-24 + 2^-32) |a b| = 2.004 u |a b|, counted as 3
             + 6 R + R / 16     the accumulators: six MFMA terms per 16-channel chunk, R products each, every piece product exact
                                (8 x 8 bits) and at most ONE rounding per accumulated product; the sum of the kept |piece products| is
                                at most (1 + 2^-8)^2 |a b|, which the R / 16 pays for
             + 5                the epilogue: z0 = m0 + m1 + m2 and z1 = m1 - m2 - m3 (two additions), y0 = z0 + z1 + z2 and
                                y1 = z1 - z2 - z3 (two), the addend (one)
             = 11 + 6.0625 R    (399 at 64 channels, 884 at 144)
    The one-rounding-per-product chain is documented for the f32 MFMA only; for v_mfma_f32_32x32x16_bf16 it is an ASSUMED upper bound.
    The bar is a worst case and wide for the arithmetic: it is there for masking, indexing, halos, rotation and windows.  The arithmetic
    is held bit for bit by the lattice classes below.
Statistics bars (per channel, against float64 sums of the float32 values the launch STORED, so they cover the summation only; the test
adds the partial rows in float64):
    a thread accumulates its four pixels (two items x two pixels) from zero: 3 roundings; the reduction adds 32 thread rows from zero:
    31 roundings; chain = 34
    sum y            34 u sum |y|
    sum y^2          35 u sum y^2                 (+ 1: the square)
    sum g            36 u sum |g|                 (+ 2: g = y * act', and 0.2f for 0.2)
    sum g (x - mean) 38 u sum |g| |x - mean|      (+ 2 more: the difference and the product)
Lattice classes (no tolerance): integer inputs on which every intermediate of the kernel -- B^T d B, the pieces, every partial sum of
the accumulators, z, y -- is an integer below 2^24 quanta, hence exact in float32 in ANY summation order; the stored output must equal
the float64 convolution bit for bit.  Each class makes one group of the six kept terms carry the result (LATTICE); the premise is
asserted in int64 by lattice_premise().  That the bf16 MFMA keeps sums which are exact in float32 is the hardware premise."""
import ctypes as C
import functools

import numpy as np

import norm_cases as NC
import pack_ref as PK
import wino_ref as R

F, D = np.float32, np.float64
U = R.U
K_SUM, K_SQ, K_G, K_GX = 34, 35, 36, 38
GUARD = 64


def k_out(red):
    return 11 + 6 * red + red // 16


# operand -> (elements the buffer is wider than the operand, first channel): pairwise different strides and offsets, offsets on the
# 4-element grid; "A": addend and bn_x end their buffer's rows, "B": in and out do
LAYOUTS = {"A": dict(x=(12, 4), out=(24, 8), addend=(20, 20), bn_x=(16, 16)),
           "B": dict(x=(8, 8), out=(4, 4), addend=(16, 0), bn_x=(28, 12))}
FORMS = ("fwd", "fwd_stat", "fwd_stat_cancel", "dgrad_add", "bnb_relu", "bnb_leaky")


def _c(form, shape, red, out, layout):
    return (form, shape, red, out, layout)


# (form, (N, H, W), reduction channels, output channels, layout).  A tile block is 4 x 8 tiles = 8 x 16 pixels.
GEOMETRY = [_c("fwd_stat", (1, 2, 2), 64, 64, "A"),                # one tile
            _c("dgrad_add", (2, 8, 16), 64, 64, "B"),              # exactly one block
            _c("bnb_leaky", (2, 7, 15), 64, 64, "A"),              # one pixel less in both directions
            _c("fwd_stat", (2, 9, 17), 64, 64, "B"),               # one more: a second block row and column, almost all outside
            _c("bnb_relu", (2, 3, 35), 64, 64, "B"),
            _c("dgrad_add", (3, 17, 33), 64, 64, "A"),             # 27 workgroups, pixel-block-major
            _c("fwd_stat_cancel", (2, 7, 15), 64, 64, "B")]
CHUNK_MAP = (2, 5, 7)
CHUNKS = [_c("fwd_stat" if i % 2 else "fwd", CHUNK_MAP, r, 64, "AB"[i % 2]) for i, r in enumerate((64, 80, 96, 112, 128, 144))] + \
         [_c("bnb_leaky" if i % 2 else "dgrad_add", CHUNK_MAP, r, 64, "BA"[i % 2]) for i, r in enumerate((64, 80, 96, 112, 128, 144))]
ORDERS = [_c("dgrad_add", (3, 8, 16), 64, 128, "A"),               # 6 workgroups, pixel-block-major with two channel blocks
          _c("bnb_relu", (3, 8, 16), 64, 256, "B"),                # 12 workgroups, channel-block-major
          _c("fwd_stat", (2, 7, 15), 80, 256, "A")]                # channel-block-major with masked edges
CASES = GEOMETRY + CHUNKS + ORDERS


def case_id(c):
    return "%s-%s-%dto%d-%s" % (c[0], "x".join(str(v) for v in c[1]), c[2], c[3], c[4])


def is_flip(form):
    return form.startswith("dgrad") or form.startswith("bnb")


def blocks(N, H, W):
    """Tile blocks of 4 x 8 tiles the map takes (= rows of the statistics buffer)."""
    th, tw = (H + 1) // 2, (W + 1) // 2
    return N * (-(-th // 4)) * (-(-tw // 8))


def workgroups(c):
    return blocks(*c[1]) * (c[3] // 64)


def strides(c):
    """operand -> (ld, c0) of the case."""
    form, _, red, out, layout = c
    width = dict(x=red, out=out, addend=out, bn_x=out)
    return {k: (width[k] + e, c0) for k, (e, c0) in LAYOUTS[layout].items()}


# ------------------------------------------------------------------------------------------------ data and expected results
def case_data(c, seed=0):
    """x [N,H,W,red] with per-channel scales 2^-3 .. 2^3; OIHW weights without any symmetry in (kh, kw); addend / bn_x of the output's
    shape; BatchNorm coefficients of either sign, with scale x + shift kept away from the activation's kink."""
    form, (N, H, W), red, out, _ = c
    rng = np.random.default_rng([31, seed, N, H, W, red, out, FORMS.index(form)])
    x = (2.0 ** rng.uniform(-3, 3, red) * rng.standard_normal((N, H, W, red))).astype(F)
    O, I = (red, out) if is_flip(form) else (out, red)
    w = ((rng.standard_normal((O, I, 3, 3)) + 0.3 * np.arange(9).reshape(3, 3) - 1.0) * (2.0 / (9 * red)) ** 0.5).astype(F)
    d = dict(case=c, x=x, w=w, flip=is_flip(form))
    if form == "dgrad_add":
        d["addend"] = (2.0 ** rng.uniform(-3, 3, out) * rng.standard_normal((N, H, W, out))).astype(F)
    if form == "fwd_stat_cancel":
        # the addend cancels all but 2^-16 of every result: the stored values are then the kernel's own low-order bits, and
        # statistics of anything but the stored values leave their bar
        y = R.conv(x, w)[0].astype(F)
        d["addend"] = -(y - y * F(2.0 ** -16))
    if form.startswith("bnb"):
        bx = (2.0 ** rng.uniform(-3, 3, out) * rng.standard_normal((N, H, W, out))).astype(F)
        scale = ((rng.uniform(0.5, 1.5, out)) * rng.choice([-1.0, 1.0], out)).astype(F)
        shift = (0.3 * rng.standard_normal(out)).astype(F)
        z = scale.astype(D) * bx + shift
        bx = np.where(np.abs(z) < 1e-3, bx + F(0.25) * np.sign(scale), bx).astype(F)      # (fp32 and float64 then agree on act')
        assert (np.abs(scale.astype(D) * bx + shift) > 1e-4).all()
        d.update(bn_x=bx, scale=scale, shift=shift, mean=(0.2 * rng.standard_normal(out) + 0.5).astype(F),
                 act=R.ACT_LEAKY if form == "bnb_leaky" else R.ACT_RELU)
    return d


def want_of(d):
    out, _ = R.conv(d["x"], d["w"], d["flip"])
    s = R.wino_magnitude(d["x"], d["w"], d["flip"])
    if "addend" in d:
        out, s = out + d["addend"], s + np.abs(d["addend"].astype(D))
    return dict(out=out, bar=k_out(d["case"][2]) * U * s)


@functools.lru_cache(maxsize=None)
def case(c):
    """(data, float64 result and bar) of a case: computed once, shared, never modified."""
    d = case_data(c)
    return d, want_of(d)


def stat_want(d, stored):
    """Per-channel (want, bar) pairs of the two statistics slots, from the float32 values the launch stored."""
    y = np.asarray(stored, D)
    if "bn_x" in d:
        s0, s1, a0, a1 = R.bn_terms(y, d["bn_x"], d["mean"], d["scale"], d["shift"], d["act"])
        return (s0, K_G * U * a0), (s1, K_GX * U * a1)
    s0, s1, a0 = R.stats(y)
    return (s0, K_SUM * U * a0), (s1, K_SQ * U * s1)


def fracs(d, want, out, stat=None):
    """out: the stored window [N,H,W,Q]; stat: the partial rows [rows][2 or 3][Q] -> {output: worst fraction of its bar}."""
    fr = {"out": NC.frac(out, want["out"], want["bar"])}
    if stat is not None:
        rows = np.asarray(stat, D)[:, :2].sum(0)
        for k, (w_, b_) in enumerate(stat_want(d, out)):
            fr["s%d" % k] = NC.frac(rows[k], w_, b_)
    return fr


def has_stat(form):
    return form != "fwd" and form != "dgrad_add"


CONV_MODES = ("taps_not_rotated", "channels_not_transposed", "row_wrap", "next_image")


def shortcut(c, mode="exact"):
    """What a kernel that took the shortcut `mode` would leave behind on a case: (stored window [N,H,W,Q] float32, statistics rows
    [1][2][Q] float64 or None).  "exact": the documented arithmetic (wino_ref.emulate), rounded once, then the addend in float32."""
    d, want = case(c)
    form, (N, H, W), red, out, _ = c
    P, st = N * H * W, strides(c)
    with np.errstate(all="ignore"):
        y = R.conv(d["x"], d["w"], d["flip"], mode)[0] if mode in CONV_MODES else R.emulate(d["x"], d["w"], d["flip"])
        y = y.astype(F)
        if "addend" in d:
            lda, ca = st["addend"]
            a = R.window(NC.wide(d["addend"].reshape(P, out), lda, ca), P, out, st["out"][0] if mode == "addend_at_out_stride" else lda, ca)
            y = (y + a.reshape(y.shape).astype(F)).astype(F)
        if not has_stat(form):
            return y, None
        v = want["out"] if mode == "stats_unrounded" else y.astype(D)
        if "bn_x" in d:
            ldb, cb = st["bn_x"]
            bx = R.window(NC.wide(d["bn_x"].reshape(P, out), ldb, cb), P, out, st["out"][0] if mode == "bn_x_at_out_stride" else ldb, cb)
            s0, s1 = R.bn_terms(v, bx.reshape(v.shape), d["mean"], d["scale"], d["shift"], d["act"], mode)[:2]
        else:
            s0, s1 = R.stats(v)[:2]
        if mode == "masked_counted":
            ext = R.conv_masked_extent(d["x"], d["w"], d["flip"])
            ext[:, :H, :W] = 0.0
            s0, s1 = s0 + ext.sum((0, 1, 2)), s1 + (ext * ext).sum((0, 1, 2))
    return y, np.stack([s0, s1])[None]


# ------------------------------------------------------------------------------------------------ the lattice classes
# class -> the kept terms (piece of the transformed patch, piece of U) that carry its result
LATTICE = {"A": ((0, 0), (1, 0), (2, 0)), "B": ((0, 0), (0, 1), (0, 2)), "C": ((0, 0), (0, 1), (1, 0), (1, 1))}
# (class, N, H, W, flip, log2 of the power of two x is scaled by)
LATTICE_CASES = [("A", 1, 7, 10, False, 0), ("B", 1, 7, 10, False, 0), ("C", 1, 7, 10, False, 0),
                 ("A", 2, 7, 10, True, 0), ("B", 2, 7, 10, True, 0), ("C", 2, 7, 10, True, 0),
                 ("A", 1, 7, 10, False, -40), ("B", 1, 7, 10, False, -40), ("C", 1, 7, 10, True, -40)]
LC = 64          # channels on either side


def lattice_id(c):
    return "%s-%dx%dx%d-%s-2^%d" % (c[0], c[1], c[2], c[3], "dgrad" if c[4] else "fwd", c[5])


@functools.lru_cache(maxsize=None)
def lattice_data(c):
    """Integer x and OIHW weights of a class.  The weights have ONE non-zero tap per (output, reduction channel) pair, drawn from all
    nine, and only `per` reduction channels per output channel are non-zero; g = +-4 m keeps U = G g G^T integral (+-m {4, 2, 1})."""
    cls, N, H, W, flip, e = c
    rng = np.random.default_rng([32, "ABC".index(cls), N, H, W, int(flip)])
    if cls == "A":
        x = rng.integers(-2 ** 17, 2 ** 17 + 1, (N, H, W, LC))
        per, m = 2, lambda n: np.ones(n, np.int64)
    elif cls == "B":
        x = rng.integers(-1, 2, (N, H, W, LC))
        per, m = 1, lambda n: 2 * rng.integers(2 ** 16, 2 ** 17, n) + 1
    else:
        x = rng.integers(-2 ** 8, 2 ** 8 + 1, (N, H, W, LC))
        per, m = 1, lambda n: 2 * rng.integers(2 ** 7, 2 ** 8, n) + 1
    g = np.zeros((LC, LC, 9), np.int64)          # [output][reduction][tap]
    for q in range(LC):
        rr = rng.choice(LC, per, replace=False)
        g[q, rr, rng.integers(0, 9, per)] = 4 * m(per) * rng.choice([-1, 1], per)
    g = g.reshape(LC, LC, 3, 3)
    # g is the kernel's view (output, reduction); the OIHW tensor of an input-gradient launch is its transposed, rotated form
    w = g.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1] if flip else g
    xf, wf = (x.astype(D) * 2.0 ** e).astype(F), np.ascontiguousarray(w).astype(F)
    assert np.array_equal(xf.astype(D), x * 2.0 ** e) and np.array_equal(wf.astype(np.int64), w)
    want = R.conv(xf, wf, flip)[0]
    return dict(case=c, x=xf, w=wf, flip=flip, xi=x, gi=g, quantum=2.0 ** e), want


def _bits(v):
    """Significant bits of the widest integer of an array."""
    v = np.abs(np.asarray(v, np.int64))
    v = v[v != 0]
    return int(max(int(a).bit_length() - (int(a) & -int(a)).bit_length() + 1 for a in np.unique(v))) if v.size else 0


def lattice_premise(c):
    """The premise of a lattice case in int64 along the kernel's data flow -- B^T d B, sum_r U V, z, y, with sums of absolute values so
    that it holds for any order -- and the piece counts the class claims (pack_ref.split3).  -> the figures, after asserting them."""
    d, want = lattice_data(c)
    cls = c[0]
    x, g = d["xi"], d["gi"]
    N, H, W, _ = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    g2 = np.stack([2 * g[:, :, 0], g[:, :, 0] + g[:, :, 1] + g[:, :, 2], g[:, :, 0] - g[:, :, 1] + g[:, :, 2], 2 * g[:, :, 2]], 2)          # 2 G g
    u4 = np.stack([2 * g2[..., 0], g2[..., 0] + g2[..., 1] + g2[..., 2], g2[..., 0] - g2[..., 1] + g2[..., 2], 2 * g2[..., 2]], 3)           # 4 U
    assert (u4 % 4 == 0).all(), "U is integral"
    u = u4 // 4
    assert np.array_equal(u.astype(D), PK.wino_gggt(g.astype(D))), "the int64 U is pack_ref's"
    p = np.zeros((N, 2 * th + 2, 2 * tw + 2, LC), np.int64)
    p[:, 1:H + 1, 1:W + 1] = x
    dd = np.stack([np.stack([p[:, a:a + 2 * th:2, b:b + 2 * tw:2] for b in range(4)], 3) for a in range(4)], 3)
    bt, at = R.BT.astype(np.int64), R.AT.astype(np.int64)
    t_abs = np.einsum("ia,ntxabc->ntxibc", np.abs(bt), np.abs(dd))
    v_abs = np.einsum("ntxibc,jb->ntxijc", t_abs, np.abs(bt))
    v = np.einsum("ia,ntxabc,jb->ntxijc", bt, dd, bt)
    m_abs = np.einsum("ntxijc,qcij->ntxijq", v_abs, np.abs(u))
    y_abs = np.einsum("ri,ntxijq,sj->ntrxsq", np.abs(at), m_abs, np.abs(at))
    worst = int(max(v_abs.max(), m_abs.max(), y_abs.max()))
    assert worst < 2 ** 24, "every partial sum is an integer below 2^24 quanta"
    # the pieces: of the float32 values the kernel splits
    vp = PK.split3((v.astype(D) * d["quantum"]).astype(F))
    up = PK.split3(u.astype(F))
    n_v = 1 + int((vp[1] << 1).any()) + int((vp[2] << 1).any())
    n_u = 1 + int((up[1] << 1).any()) + int((up[2] << 1).any())
    assert (n_v, n_u) == {"A": (3, 1), "B": (1, 3), "C": (2, 2)}[cls], (cls, n_v, n_u)
    # (with (3, 1), (1, 3) or (2, 2) pieces the dropped products a1 b2, a2 b1, a2 b2 are exactly zero)
    nz = float((want != 0).mean())
    assert nz >= 0.5, "at least half of the outputs are non-zero"
    y = np.einsum("ri,ntxijq,sj->ntrxsq", at, np.einsum("ntxijc,qcij->ntxijq", v, u), at).reshape(N, 2 * th, 2 * tw, LC)[:, :H, :W]
    assert np.array_equal(y.astype(D) * d["quantum"], want), "the int64 Winograd result is the float64 convolution"
    return dict(worst_log2=float(np.log2(worst)), v_bits=_bits(v), u_bits=_bits(u), nonzero=nz)


# ------------------------------------------------------------------------------------------------ on the device
def dev32(a):
    import torch
    a = np.ascontiguousarray(a, F).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.full(GUARD, np.nan, F)])).cuda()


def nan32(n):
    return dev32(np.full(n, np.nan, F))


def np32(t):
    a = t.cpu().numpy()
    assert np.isnan(a[a.size - GUARD:]).all(), "guard"
    return a[:a.size - GUARD]


def ptr(t, elems=0):
    return C.c_void_p(None if t is None else t.data_ptr() + elems * t.element_size())


def pack(L, st, w, flip):
    """rd_wino_pack on the device -> the packed operand (a bf16 tensor)."""
    import torch
    O, I = w.shape[:2]
    nbytes = int(L.rd_wino_packed_bytes(O, I, int(flip)))
    assert nbytes == 2 * PK.wino_packed_elems(O, I, int(flip))
    u = torch.zeros(nbytes // 2, dtype=torch.bfloat16, device="cuda")
    wd = dev32(w)
    rc = L.rd_wino_pack(ptr(wd), O, I, int(flip), ptr(u), st)
    assert rc == 0, L.rd_last_error()
    torch.cuda.synchronize()
    return u


def launch(d, strides_):
    """One launch of the case's form through the C ABI: every operand a channel window of a wider NaN-filled buffer with a NaN guard
    behind it, the output and statistics buffers NaN before the launch, LDS poisoned.  Asserts on the way: the return code, the guards,
    NaN everywhere outside the output window and finite values inside it, the statistics buffer fully finite (slot 2 of the _bnbwd layout
    untouched), the inputs unchanged.  -> (stored window [N,H,W,Q] float32, partial rows [rows][slots][Q] float32 or None)."""
    import torch
    from radar_depth_amd._lib import current_stream, lib
    L, st = lib(), current_stream()
    form, (N, H, W), red, out, _ = d["case"]
    P = N * H * W
    (ldx, cx), (ldo, co), (lda, ca), (ldb, cb) = (strides_[k] for k in ("x", "out", "addend", "bn_x"))
    assert len({ldx, ldo, lda, ldb}) == 4 and len({cx, co, ca, cb}) == 4 and not any(v % 4 for v in (ldx, ldo, lda, ldb, cx, co, ca, cb))
    assert L.rd_wino_supported(H, W, red, out, ldx, ldo) == 1, (H, W, red, out, ldx, ldo)
    u = pack(L, st, d["w"], d["flip"])
    xw = NC.wide(d["x"].reshape(P, red), ldx, cx)
    X, OUT = dev32(xw), nan32(P * ldo)
    rows = int(L.rd_wino_stat_tiles(N, H, W))
    assert rows == blocks(N, H, W)
    bnb = "bn_x" in d
    slots = 3 if bnb else 2
    STAT = nan32(rows * slots * out) if has_stat(form) else None
    keep = [(X, xw)]
    assert L.rd_debug_poison_lds(st) == 0, L.rd_last_error()
    if bnb:
        bw = NC.wide(d["bn_x"].reshape(P, out), ldb, cb)
        BX, M, S, T = dev32(bw), dev32(d["mean"]), dev32(d["scale"]), dev32(d["shift"])
        keep += [(BX, bw), (M, d["mean"]), (S, d["scale"]), (T, d["shift"])]
        rc = L.rd_wino_conv3x3_bnbwd(ptr(X, cx), N, H, W, red, ldx, ptr(u), ptr(OUT, co), out, ldo, ptr(BX, cb), ldb, ptr(M), ptr(S), ptr(T),
                                     d["act"], ptr(STAT), st)
    else:
        A = None
        if "addend" in d:
            aw = NC.wide(d["addend"].reshape(P, out), lda, ca)
            A = dev32(aw)
            keep.append((A, aw))
        rc = L.rd_wino_conv3x3(ptr(X, cx), N, H, W, red, ldx, ptr(u), ptr(OUT, co), out, ldo, ptr(A, ca) if A is not None else None,
                               lda if A is not None else 0, ptr(STAT) if STAT is not None else None, st)
    assert rc == 0, (rc, L.rd_last_error())
    torch.cuda.synchronize()
    ob = np32(OUT).reshape(P, ldo)
    assert NC.writes_ok(ob, ldo, co, out), "a write outside the output window, or a non-finite value inside it"
    for t, a in keep:
        assert np.array_equal(np32(t).view(np.uint32), np.ascontiguousarray(a, F).reshape(-1).view(np.uint32)), "an input was written"
    stat = None
    if STAT is not None:
        stat = np32(STAT).reshape(rows, slots, out)
        assert np.isfinite(stat[:, :2]).all(), "a statistics row was not written"
        assert slots == 2 or np.isnan(stat[:, 2]).all(), "slot 2 of the _bnbwd layout was written"
    return ob[:, co:co + out].reshape(N, H, W, out).copy(), stat


def run_case(c):
    d, want = case(c)
    out, stat = launch(d, strides(c))
    return fracs(d, want, out, stat)


def run_lattice(c):
    """-> (elements that differ from the float64 convolution, the first few of them)."""
    d, want = lattice_data(c)
    out, _ = launch(dict(d, case=("fwd", d["x"].shape[:3], LC, LC, "A")), strides(("fwd", None, LC, LC, "A")))
    bad = np.argwhere(out.astype(D) != want)
    return len(bad), [(tuple(int(v) for v in i), float(out[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]]


# ------------------------------------------------------------------------------------------------ the lattice classes without the transform
# The other forward kernels that rebuild fp32 products from six bf16 terms (y = sum over taps and channels of x w: no transform): the
# same three classes on one small descriptor each, against desc_emulator.run_desc in float64, bit for bit.
#   A: x 19 bits (three pieces), w = +-1;  B: x in {-1, 0, 1}, w 19 bits;  C: x and w two pieces each (10 x 10 bits).
#   `per` non-zero weights per output channel keep every partial sum below 2^24 quanta (asserted).
FLAT_KERNELS = ("gconv_split_3x3", "gconv_split_1x1", "gconv_split_pre_3x3", "gconv_split_pre_1x1", "gemm_taps_split_deconv2", "conv16_split")
FLAT_PER = {"A": 16, "B": 16, "C": 8}
# The descriptor kinds tests/test_gpu_split_lattice_tiles.py runs under every forced tile, for rd_gconv_split and rd_gconv_split_pre:
# kind -> weight slabs.  Multi-phase descriptors with short last tap groups, a 25-tap single phase and a 3x3 with partial channel blocks.
FLAT_TILE_KINDS = {"3x3": 9,                # conv_fwd(2, 7, 10, 64, 64, 3, 1, 1): the descriptor of FLAT_KERNELS
                   "upproj_fwd": 25,        # phases of 9 / 6 / 6 / 4 taps
                   "dgrad_s2": 9,           # conv_dgrad(2, 7, 10, 64, 64, 3, 2, 1): phases of 1 / 2 / 2 / 4 taps
                   "upproj_dgrad": 25,      # one phase of 25 taps
                   "3x3_partial": 9}        # conv_fwd(2, 13, 35, 96, 96, 3, 1, 1): partial 64-channel blocks on both sides
FLAT_TILE_KERNELS = tuple("%s_%s" % (e, k) for e in ("gconv_split", "gconv_split_pre") for k in FLAT_TILE_KINDS if k != "3x3")
FLAT_ALL = FLAT_KERNELS + FLAT_TILE_KERNELS          # (a kernel's index here seeds its data)


def flat_desc(kernel):
    """-> (descriptor, weight slabs)."""
    from radar_depth_amd import convdesc as cd
    if kernel == "conv16_split":
        return cd.conv_fwd(2, 7, 10, 16, 16, 3, 1, 1), 9
    if kernel == "gemm_taps_split_deconv2":
        return cd.deconv_fwd(2, 5, 4, 64, 64, 2), 4
    if kernel in FLAT_TILE_KERNELS:
        kind = kernel[len("gconv_split_pre_" if "_pre_" in kernel else "gconv_split_"):]
        d = {"upproj_fwd": lambda: cd.upproj_fwd(2, 7, 10, 64, 64), "dgrad_s2": lambda: cd.conv_dgrad(2, 7, 10, 64, 64, 3, 2, 1)[0],
             "upproj_dgrad": lambda: cd.upproj_dgrad(2, 7, 10, 64, 64), "3x3_partial": lambda: cd.conv_fwd(2, 13, 35, 96, 96, 3, 1, 1)}[kind]()
        return d, FLAT_TILE_KINDS[kind]
    k = 3 if kernel.endswith("3x3") else 1
    return cd.conv_fwd(2, 7, 10, 64, 64, k, 1, k // 2), k * k


@functools.lru_cache(maxsize=None)
def flat_data(kernel, cls, e=0):
    """-> (descriptor, x [N,Hi,Wi,Cin] float32, w [slabs,Cin,Cout] float32, float64 result with NaN where no phase writes)."""
    import torch
    from desc_emulator import run_desc
    d, S = flat_desc(kernel)
    rng = np.random.default_rng([33, FLAT_ALL.index(kernel), "ABC".index(cls)])
    shape = (d.N, d.Hi, d.Wi, d.Cin)
    per = min(FLAT_PER[cls], S * d.Cin)
    if cls == "A":
        x, m = rng.integers(-2 ** 18, 2 ** 18 + 1, shape), lambda n: np.ones(n, np.int64)
    elif cls == "B":
        x, m = rng.integers(-1, 2, shape), lambda n: 2 * rng.integers(2 ** 17, 2 ** 18, n) + 1
    else:
        x, m = rng.integers(-2 ** 9, 2 ** 9 + 1, shape), lambda n: 2 * rng.integers(2 ** 8, 2 ** 9, n) + 1
    w = np.zeros((S * d.Cin, d.Cout), np.int64)
    for q in range(d.Cout):
        w[rng.choice(S * d.Cin, per, replace=False), q] = m(per) * rng.choice([-1, 1], per)
    w = w.reshape(S, d.Cin, d.Cout)
    xf, wf = (x * 2.0 ** e).astype(F), w.astype(F)
    assert np.array_equal(xf.astype(D), x * 2.0 ** e) and np.array_equal(wf.astype(np.int64), w)
    want = run_desc(d, torch.from_numpy(xf).double(), torch.from_numpy(wf).double()).numpy()
    # the premise: sums of absolute values below 2^24 quanta, the piece counts of the class, at least half of the outputs non-zero
    worst = np.nanmax(run_desc(d, torch.from_numpy(np.abs(x)).double(), torch.from_numpy(np.abs(w)).double()).numpy())
    assert worst < 2 ** 24, (kernel, cls, worst)
    pieces = lambda a: 1 + int((PK.split3(a)[1] << 1).any()) + int((PK.split3(a)[2] << 1).any())
    assert (pieces(xf), pieces(wf)) == {"A": (3, 1), "B": (1, 3), "C": (2, 2)}[cls], (kernel, cls)
    written = ~np.isnan(want)
    assert (want[written] != 0).mean() >= 0.5
    return d, xf, wf, want


def flat_emulate(d, x, w, drop=None):
    """The six kept piece products of y = sum x w, summed exactly (float64)."""
    import torch
    from desc_emulator import run_desc
    xp = [torch.from_numpy(PK.bf16_to_f32(p).reshape(x.shape)).double() for p in PK.split3(x)]
    wp = [torch.from_numpy(PK.bf16_to_f32(p).reshape(w.shape)).double() for p in PK.split3(w)]
    return sum(run_desc(d, xp[a], wp[b]).numpy() for (a, b) in R.KEPT if (a, b) != drop)


def run_flat(kernel, cls):
    """One launch of the kernel on the class under poisoned LDS into a NaN-filled output -> (descriptor's plan marker or None,
    elements that differ from the float64 result, the first few)."""
    plan, n_bad, first = run_flat_plan(kernel, cls)
    return (None if plan is None else plan[7]), n_bad, first


def run_flat_plan(kernel, cls):
    """run_flat with the whole plan: -> (rd_gconv_split[_pre]_plan_info's eight figures under the tile choice of THIS process or None,
    differing elements, the first few)."""
    import torch
    from radar_depth_amd import ops
    from radar_depth_amd._lib import check, current_stream, lib
    L, st = lib(), current_stream()
    d, x, w, want = flat_data(kernel, cls)
    xg = torch.from_numpy(x).cuda()
    w_oihw = torch.from_numpy(np.ascontiguousarray(w.transpose(2, 1, 0)[..., None])).cuda()          # [Cout][Cin][slabs][1]
    out = torch.full((d.N, d.Ho, d.Wo, d.Cout), float("nan"), device="cuda")
    plan = None
    prev = L.rd_gconv_split_plan_all(1)
    try:
        check(L.rd_debug_poison_lds(st), "rd_debug_poison_lds")
        if kernel == "conv16_split":
            assert L.rd_conv16_split_supported(C.byref(d)) == 1
            wp = ops.pack_weights(w_oihw.reshape(d.Cout, d.Cin, 3, 3).contiguous())
            check(L.rd_conv16_split(C.byref(d), ptr(xg), ptr(wp), ptr(out), None, 0, None, st), kernel)
        elif kernel.startswith("gemm_taps"):
            assert ops.gemm_taps_split_supported(d)
            ops.gemm_taps_split(d, xg, ops.pack_weights_split(w_oihw), out)
        else:
            pre = "_pre_" in kernel
            info = (C.c_int32 * 8)()
            assert (L.rd_gconv_split_pre_supported if pre else L.rd_gconv_split_supported)(C.byref(d)) == 1, kernel
            assert (L.rd_gconv_split_pre_plan_info if pre else L.rd_gconv_split_plan_info)(C.byref(d), info) == 0
            plan = [int(v) for v in info]
            if pre:
                ops.gconv_split_pre(d, ops.split_pieces(xg), ops.pack_weights_split(w_oihw), out)
            else:
                ops.gconv_split(d, xg, ops.pack_weights_split(w_oihw), out)
        torch.cuda.synchronize()
    finally:
        L.rd_gconv_split_plan_all(1 if prev == 1 else 0)
    got = out.cpu().numpy().astype(D)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "exactly the phases' pixels are written"
    bad = np.argwhere((got != want) & ~np.isnan(want))
    return plan, len(bad), [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]]

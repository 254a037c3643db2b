"""The cases tests/test_gpu_norm_fp64.py runs on the device and tests/test_norm_host.py shows to be sensitive to every shortcut of
norm_ref.MODES: shapes, planted data, the channel windows every operand lives in, the expected results from the restatement and
the bars they are held to.  numpy only.

Bars (u = 2^-24; derived, not tuned):
  finalize / backward coefficients   the kernel evaluates the reference's double expressions and rounds once: 2u |want|
                                     (shift: 2u (|beta| + |mean gamma invstd|)); num_batches_tracked exact
  element-wise                       k u sum|addends|, k = roundings in the expression as the kernel writes it: 2 (fma, activation),
                                     3 with a residual, 4 for fma(A, g, fma(B, x - mean, K)) with the activation factor, 1 for
                                     g = dy * act'; pool gather: up to three additions and the slope, 4
  fp32 reductions                    chain u sum|term| per channel, chain = norm_ref.chain / pool_chain
Every comparison is per channel and per element: nothing is measured against a tensor-wide maximum."""
import numpy as np

import norm_ref as R

F, D = np.float32, np.float64
U = R.U
EPS, MOMENTUM = 1e-5, 0.1
SLOPE32 = float(F(0.2))          # the kernels' 0.2f

# (M, C, act, residual): RL = 256 / (C/4) row lanes -- C = 64: 16, so M = 15 and 17 are RL -+ 1; C = 1024: RL = 1; C = 80: 256 % 20 != 0,
# sixteen idle threads; (70000, 4): 1094 tiles in both rd_bn_stats and rd_bn_bwd_tiles, past the 768 of the four-tiles-per-trip loops
CHAIN = [(1, 4, 1, None), (3, 32, 1, "id"), (15, 64, 2, "bn"), (17, 64, 1, "bn"), (77, 80, 2, None), (48, 1024, 1, "id"),
         (700, 512, 2, "bn"), (5000, 16, 1, None), (70000, 4, 2, "bn"), (100, 8, 0, "bn")]
E2E = [(77, 80, 2, None), (48, 1024, 1, "id"), (700, 512, 2, "bn"), (5000, 16, 1, None), (70000, 4, 2, "bn"), (100, 8, 0, "bn")]
FIN_GEOM = [(None, 0, 64), (192, 64, 64), (640, 512, 128), (20, 16, 4)]          # (ld, c0, C); ld None: C
N_TILES = [1, 255, 256, 257, 768, 769, 1023, 1024, 1025, 1793, 2048, 4096]
# (N, H, W, C, act, forms): "all" also runs the stats / apply forms (C/4 must divide 256); (1, 224, 224, 64): 784 tiles
POOL = [(1, 1, 1, 4, 1, "all"), (2, 1, 5, 16, 2, "all"), (1, 2, 2, 128, 1, "all"), (1, 7, 9, 48, 2, "plain"), (3, 8, 9, 16, 1, "all"),
        (2, 49, 81, 64, 2, "all"), (1, 224, 224, 64, 1, "all")]
COND = [(5000, 16), (700, 512)]
COND_RATIOS = [0, 3, 30, 300]          # mean / std


def case_id(c):
    return "-".join("x" if v is None else str(v) for v in c)


# ------------------------------------------------------------------------------------------------ channel windows
def layout(C):
    """operand -> (ld, c0): every tensor operand is a channel window of a wider buffer, a different stride for each."""
    return dict(x1=(3 * C, C), x2=(2 * C, C), dy=(C + 16, 0), y=(C + 8, 4), g=(C + 4, 4), dx1=(C + 32, 16), dx2=(2 * C + 4, C),
                py=(C + 12, 8), pdy=(2 * C, C))


def wide(a, ld, c0, mode="exact"):
    """a [rows, C] as channels [c0, c0 + C) of a NaN-filled [rows, ld] float32 buffer ("neighbour_column": what a kernel that wrote
    one column too many would leave behind)."""
    a = np.asarray(a)
    a = a.reshape(-1, a.shape[-1])
    buf = np.full((a.shape[0], ld), np.nan, F)
    buf[:, c0:c0 + a.shape[1]] = a
    if mode == "neighbour_column":
        col = c0 + a.shape[1] if c0 + a.shape[1] < ld else c0 - 1
        buf[:, col] = a[:, -1]
    return buf


def writes_ok(buf, ld, c0, C):
    """NaN outside the written window, finite inside it."""
    b = np.asarray(buf).reshape(-1, ld)
    inside = np.zeros(ld, bool)
    inside[c0:c0 + C] = True
    return bool(np.isnan(b[:, ~inside]).all() and np.isfinite(b[:, inside]).all())


# ------------------------------------------------------------------------------------------------ comparison
def frac(got, want, bar):
    """Worst |got - want| / bar over the elements (0 where they agree exactly; inf where got is not finite or the bar is 0)."""
    got, want, bar = np.broadcast_arrays(np.asarray(got, D), np.asarray(want, D), np.asarray(bar, D))
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        f = np.where(err == 0, 0.0, err / bar)
    f = np.where(np.isfinite(got) & ~np.isnan(f), f, np.inf)
    return float(f.max())


def worst(fr):
    return max(fr.values()) if fr else 0.0


def _log_uniform(rng, lo, hi, n):
    a = 2.0 ** rng.uniform(lo, hi, n)
    a[0], a[-1] = 2.0 ** lo, 2.0 ** hi
    return a


# ------------------------------------------------------------------------------------------------ finalize on synthetic partial sums
def synth_partials(n_tiles, ld, c0, C, seed=0, small=False):
    """[n_tiles][2][ld] of integers (|s| <= 2^12, 0 <= q < 2^20: every summation order is exact in double), NaN outside the channel
    window.  With count = 7 * n_tiles: channel 0 gives a variance of exactly 0, channel 1 one of -1/count, the others are positive.
    small: |s| <= 8 and 400 <= q < 800 per tile, a positive variance at any count >= 1 with a few tiles."""
    rng = np.random.default_rng([11, seed, n_tiles, C])
    part = np.full((n_tiles, 2, ld), np.nan, F)
    base = rng.integers(-1500, 1501, C)
    part[:, 0, c0:c0 + C] = rng.integers(-8, 9, (n_tiles, C)) if small else base + rng.integers(-100, 101, (n_tiles, C))
    part[:, 1, c0:c0 + C] = rng.integers(400, 800, (n_tiles, C)) if small else rng.integers(1 << 19, 1 << 20, (n_tiles, C))
    part[:, 0, c0:c0 + 2], part[:, 1, c0:c0 + 2] = 21, 63          # mean 3, E[x^2] 9
    part[n_tiles // 2, 1, c0 + 1] = 62
    return part.reshape(-1)


def fin_case(n_tiles, geom, count=None, momentum=MOMENTUM, running=True, nbt=True, launches=1, seed=0):
    ld, c0, C = geom
    ld = C if ld is None else ld
    rng = np.random.default_rng([12, seed, n_tiles, C])
    gamma = (_log_uniform(rng, -10, 10, C) * np.where(rng.random(C) < 0.3, -1, 1)).astype(F)
    return dict(part=synth_partials(n_tiles, ld, c0, C, seed, small=count is not None), n_tiles=n_tiles, ld=ld, c0=c0, C=C, count=7 * n_tiles if count is None else count,
                gamma=gamma, beta=(np.abs(gamma) * rng.standard_normal(C)).astype(F), eps=float(F(EPS)), momentum=float(F(momentum)),
                rm=rng.standard_normal(C).astype(F) * 50 if running else None, rv=(rng.random(C) * 1e4 + 0.5).astype(F) if running else None,
                nbt=(0 if launches == 2 else int(rng.integers(3, 1000))) if nbt else None, launches=launches)          # (two launches from 0 leave 2)


def fin_cases():
    """Every tile count at one geometry each (all four appear), every geometry at n_tiles = 769, the running-statistics forms."""
    out = [fin_case(n, FIN_GEOM[i % 4]) for i, n in enumerate(N_TILES)] + [fin_case(769, g, seed=1) for g in FIN_GEOM]
    for count in (1, 2, 77):
        for momentum in (0.1, 1.0):
            out.append(fin_case(3, FIN_GEOM[1], count=count, momentum=momentum, seed=2))
    out += [fin_case(257, FIN_GEOM[3], running=False, seed=3), fin_case(257, FIN_GEOM[3], nbt=False, seed=4),
            fin_case(1025, FIN_GEOM[2], launches=2, seed=5), fin_case(1, FIN_GEOM[0], count=1, launches=2, seed=6)]
    return out


def fin_want(c, mode="exact"):
    """The state after c["launches"] calls on the same buffers (the running statistics are stored as fp32 in between)."""
    rm, rv, nbt = c["rm"], c["rv"], c["nbt"]
    for _ in range(c["launches"]):
        w = R.finalize(c["part"], c["n_tiles"], c["ld"], c["c0"], c["C"], c["count"], c["gamma"], c["beta"], c["eps"], c["momentum"], rm, rv, nbt,
                       mode)
        if rm is not None:
            with np.errstate(all="ignore"):
                rm, rv = w["rm"].astype(F), w["rv"].astype(F)
        nbt = w["nbt"]
    return w


def fin_fracs(got, want):
    fr = {k: frac(got[k], want[k], 2 * U * np.abs(want[k])) for k in ("mean", "invstd", "scale", "rm", "rv") if want[k] is not None}
    fr["shift"] = frac(got["shift"], want["shift"], 2 * U * want["shift_terms"])
    fr["nbt"] = 0.0 if got.get("nbt") == want["nbt"] else np.inf
    return fr


def synth_red(n_tiles, C, seed=0):
    """[n_tiles][3][C] of integers |.| <= 2^12 with a different offset per slot and channel, for the backward coefficient kernel."""
    rng = np.random.default_rng([13, seed, n_tiles, C])
    return (rng.integers(-3000, 3001, (1, 3, C)) + rng.integers(-1000, 1001, (n_tiles, 3, C))).astype(F).reshape(-1)


def coef_fracs(got, want):
    return {k: frac(got[k], want[k], 2 * U * np.abs(want[k])) for k in ("dgamma", "dbeta", "A", "B", "K")}


# ------------------------------------------------------------------------------------------------ the BatchNorm chain
def chain_data(M, C, act, res, seed=0, planted=True, e2e=False):
    """x1 [, x2], dy and the affine parameters: per-channel input scales 2^-12 .. 2^12 (mean / std = 0.25), gamma log-uniform in
    [2^-10, 2^10] with some negative.  planted (M >= 3): rows 0, M/2, M-1 of channels 1 and 2 are exact zeros (with shift = +0 / -0 --
    plant_shift -- channel 1 gives +0.0, channel 2, whose scale is negative, -0.0); channel 3 is the constant 0.1f.
    e2e: nothing planted and an output gradient whose backward sums are well conditioned (sum|t| / |sum t| small)."""
    rng = np.random.default_rng([14, seed, M, C])
    sign = lambda: np.where(rng.random(C) < 0.3, -1.0, 1.0)
    n1 = rng.standard_normal((M, C))
    d = dict(M=M, C=C, act=act, res=res, plant=None, x2=None, gamma2=None, beta2=None)
    d["x1"] = (_log_uniform(rng, -12, 12, C) * (n1 + 0.25)).astype(F)
    d["gamma1"] = (_log_uniform(rng, -10, 10, C) * sign()).astype(F)
    d["beta1"] = (np.abs(d["gamma1"]) * 0.3 * rng.standard_normal(C)).astype(F)
    t = np.sign(d["gamma1"]) * n1
    if res == "bn":
        n2 = rng.standard_normal((M, C))
        d["x2"] = (_log_uniform(rng, -12, 12, C)[::-1] * (n2 + 0.25)).astype(F)
        d["gamma2"] = (_log_uniform(rng, -10, 10, C) * sign()).astype(F)
        d["beta2"] = (np.abs(d["gamma2"]) * 0.3 * rng.standard_normal(C)).astype(F)
        t = t + np.sign(d["gamma2"]) * n2
    elif res == "id":
        d["x2"] = (np.abs(d["gamma1"]) * rng.standard_normal((M, C))).astype(F)
    ds = _log_uniform(rng, -6, 6, C)
    d["dy"] = (ds * (1.0 + 0.5 * t + 0.25 * rng.standard_normal((M, C))) if e2e else ds * rng.standard_normal((M, C))).astype(F)
    if planted and not e2e and M >= 3:
        rows = [0, M // 2, M - 1]
        d["plant"] = dict(rows=rows, pos=1, neg=2, const=3)
        d["gamma1"][1], d["gamma1"][2] = abs(d["gamma1"][1]), -abs(d["gamma1"][2])
        d["x1"][rows, 1], d["x1"][rows, 2], d["x1"][:, 3] = 0.0, 0.0, F(0.1)
        if res == "bn":
            d["gamma2"][1], d["gamma2"][2] = abs(d["gamma2"][1]), -abs(d["gamma2"][2])
            d["x2"][rows, 1], d["x2"][rows, 2] = 0.0, 0.0
        elif res == "id":
            d["x2"][rows, 1], d["x2"][rows, 2] = 0.0, -0.0
    return d


def plant_shift(d, co):
    """Coefficients with the planted channels' shift set to +0.0 / -0.0 (copies)."""
    co = {k: (None if v is None else np.array(v, F)) for k, v in co.items()}
    if d["plant"]:
        for k in ("shift1", "shift2"):
            if co.get(k) is not None:
                co[k][d["plant"]["pos"]], co[k][d["plant"]["neg"]] = 0.0, -0.0
    return co


def ref_coefs(d):
    """mean / invstd / scale / shift of both BatchNorms from the float64 statistics, rounded to fp32 (what the kernels are given)."""
    co = {}
    for k in ("1", "2"):
        if d["gamma" + k] is None:
            co.update({n + k: None for n in ("mean", "invstd", "scale", "shift")})
            continue
        w = R.finalize(R.stats_sums(d["x" + k])[0][None], 1, d["C"], 0, d["C"], d["M"], d["gamma" + k], d["beta" + k], EPS, MOMENTUM, None, None, None)
        co.update({n + k: w[n].astype(F) for n in ("mean", "invstd", "scale", "shift")})
    return co


def chain_want(d, co, mode="exact", slope=R.SLOPE, y_dev=None, g_dev=None, part=None, n_tiles=None, coef=None):
    """Everything the chain's kernels produce from the fp32 coefficients co.  On the device each stage is fed what the stage before
    it left there: y_dev (what rd_bn_bwd_reduce reads the sign from), g_dev (the masked gradient the sums are taken of), part / n_tiles
    (red_partial) and coef = {which: [3][C] coef_ws}.  Without them the reference feeds itself (rounded to fp32 where a kernel stores)."""
    f = lambda a: None if a is None else np.asarray(a, D)
    M, C, act, bn2 = d["M"], d["C"], d["act"], d["res"] == "bn"
    x1, x2, dy = f(d["x1"]), f(d["x2"]), f(d["dy"])
    s2, t2 = (f(co["scale2"]), f(co["shift2"])) if bn2 else (None, None)
    y, y_terms = R.bn_act(x1, f(co["scale1"]), f(co["shift1"]), x2, s2, t2, act, slope)
    out = dict(y=y, y_terms=y_terms, k_y=2 if x2 is None else 3)
    zq = R.pre_act(x1, f(co["scale1"]), f(co["shift1"]), x2, s2, t2, fp32=True)[0]
    out["g"] = R.bwd_g(dy, y.astype(F).astype(D) if y_dev is None else f(y_dev), act, slope, mode)          # sign read from y
    out["g_x"] = R.bwd_g(dy, zq, act, slope, mode)                                                          # ... recomputed from x
    g = out["g"].astype(F).astype(D) if g_dev is None else f(g_dev)
    out["sums"], out["sums_abs"] = R.bwd_sums(g, x1, f(co["mean1"]), x2 if bn2 else None, f(co["mean2"]) if bn2 else None, mode)
    if part is None:
        part, n_tiles = out["sums"].astype(F)[None], 1
    for w in (1, 2) if bn2 else (1,):
        k = str(w)
        cw = R.bwd_coeffs(part, n_tiles, C, w, M, d["gamma" + k], co["invstd" + k], mode)
        A, B, K = [f(a) for a in coef[w]] if coef else [cw[n].astype(F).astype(D) for n in "ABK"]
        out["coef" + k] = cw
        out["dx" + k], out["dx%s_terms" % k] = R.bwd_dx(g, f(d["x" + k]), f(co["mean" + k]), A, B, K, mode)
    return out


def chain_fracs(got, want, d):
    """got: y, g, sums ([3][C], summed over the tiles in float64), coef1 / coef2 (dicts), dx1 / dx2 -- whichever are present."""
    fr = {}
    if "y" in got:
        fr["y"] = frac(got["y"], want["y"], want["k_y"] * U * want["y_terms"])
    if "g" in got:
        fr["g"] = frac(got["g"], want["g"], U * np.abs(want["g"]))
    if "sums" in got:
        fr["sums"] = frac(got["sums"], want["sums"], R.chain(d["M"], d["C"], True) * U * want["sums_abs"])
    for k in ("1", "2"):
        if "coef" + k in got:
            fr.update({"coef%s.%s" % (k, n): v for n, v in coef_fracs(got["coef" + k], want["coef" + k]).items()})
        if "dx" + k in got:
            fr["dx" + k] = frac(got["dx" + k], want["dx" + k], 4 * U * want["dx%s_terms" % k])
    return fr


def rounded(want, keys):
    """An fp32-rounded copy of the correct results: what a correct kernel may return at best."""
    out = {}
    for k in keys:
        if k in want and want[k] is not None:
            with np.errstate(all="ignore"):
                out[k] = {n: v.astype(F) for n, v in want[k].items()} if isinstance(want[k], dict) else (
                    want[k].astype(F) if isinstance(want[k], np.ndarray) else want[k])
    return out


CHAIN_KEYS = ("y", "g", "sums", "coef1", "coef2", "dx1", "dx2")


# ------------------------------------------------------------------------------------------------ end to end
def e2e_want(d):
    """The whole chain from the raw inputs in float64 (no fp32 anywhere) -> y, dbeta1, dgamma1, dx1 [, dgamma2, dx2 | dx2 = g], and
    the conditioning of each stage: 1 + mean^2 / var of both inputs, sum|t| / |sum t| of the backward sums."""
    f = lambda a: None if a is None else np.asarray(a, D)
    M, C, act, bn2 = d["M"], d["C"], d["act"], d["res"] == "bn"
    co, cond = {}, {}
    for k in ("1", "2") if bn2 else ("1",):
        s = R.stats_sums(d["x" + k])[0]
        w = R.finalize(s[None], 1, C, 0, C, M, d["gamma" + k], d["beta" + k], float(F(EPS)), MOMENTUM, None, None, None)
        co.update({n + k: w[n] for n in ("mean", "invstd", "scale", "shift")})
        cond["stats" + k] = float((1 + w["mean"] ** 2 * w["invstd"] ** 2).max())
    y, _ = R.bn_act(f(d["x1"]), co["scale1"], co["shift1"], f(d["x2"]), co.get("scale2"), co.get("shift2"), act, SLOPE32)
    g = R.bwd_g(d["dy"], y, act, SLOPE32)
    sums, sabs = R.bwd_sums(g, f(d["x1"]), co["mean1"], f(d["x2"]) if bn2 else None, co.get("mean2"))
    out = dict(y=y, cond=cond)
    for w in (1, 2) if bn2 else (1,):
        k = str(w)
        cw = R.bwd_coeffs(sums[None], 1, C, w, M, d["gamma" + k], co["invstd" + k])
        out["dgamma" + k], out["dx" + k] = cw["dgamma"], R.bwd_dx(g, f(d["x" + k]), co["mean" + k], cw["A"], cw["B"], cw["K"])[0]
        cond["sum%d" % w] = float((sabs[w] / np.abs(sums[w])).max())
    out["dbeta1"] = sums[0]
    cond["sum0"] = float((sabs[0] / np.abs(sums[0])).max())
    if d["res"] == "id":
        out["dx2"] = g
    return out


E2E_FIGURES = dict(y=2e-5, dbeta1=2e-5, dgamma1=5e-5, dgamma2=5e-5, dx1=5e-5, dx2=5e-5)          # tests/test_gpu_norm.py's


def e2e_fracs(got, want):
    """Per channel: the worst error of the channel over the channel's largest magnitude, as a fraction of the figure."""
    fr = {}
    for k, fig in E2E_FIGURES.items():
        if k in got:
            a, b = np.asarray(got[k], D).reshape(-1, got[k].shape[-1]), np.asarray(want[k], D).reshape(-1, want[k].shape[-1])
            with np.errstate(all="ignore"):
                rel = np.abs(a - b).max(0) / np.abs(b).max(0)
            fr[k] = float(np.where(np.isfinite(rel), rel, np.inf).max()) / fig
    return fr


# ------------------------------------------------------------------------------------------------ conditioning
def cond_data(M, C, ratio, seed=0):
    rng = np.random.default_rng([15, seed, M, C, ratio])
    return (_log_uniform(rng, -3, 3, C) * (rng.standard_normal((M, C)) + ratio)).astype(F)


def cond_want(x, eps=float(F(EPS))):
    """-> invstd in float64, the contract's bound on its relative error (header: "accuracy of the training statistics") and
    1 + mean^2 / var, per channel."""
    x = np.asarray(x, D)
    M, C = x.shape
    m, q, a = x.mean(0), (x * x).mean(0), np.abs(x).mean(0)
    var = np.maximum(q - m * m, 0.0)
    return 1.0 / np.sqrt(var + eps), R.chain(M, C, False) * U * (q + 2 * np.abs(m) * a) / (2 * (var + eps)), 1 + m * m / var


# ------------------------------------------------------------------------------------------------ the stem's BN / act / max-pool
def pool_data(N, H, W, C, act, seed=0):
    """x [N,H,W,C], scale / shift (log-uniform scale, some negative), the pooled gradient dy, a mean for the fused sums.  Planted:
    channel 0 (scale 1, shift 0): a 4 x 4 block of -1 at the top left -- windows of nine equal values, all zero after ReLU -- and two
      equal maxima 5 side by side;
    channel 1 (scale 1, shift 0): the border ring of every image is 7, the interior below it -- every border window has several equal
      maxima, and what a kernel would find in the padded-away positions by wrapping (the previous row's or image's last cells, the next
      one's first) is never smaller than what the window really holds;
    channel 2 / 3: exact zeros with shift +0 / a negative scale and shift -0 (pre-activation +0.0 / -0.0)."""
    rng = np.random.default_rng([16, seed, N, H, W, C])
    x = (_log_uniform(rng, -6, 6, C) * (rng.standard_normal((N, H, W, C)) + 0.25)).astype(F)
    scale = (_log_uniform(rng, -8, 8, C) * np.where(rng.random(C) < 0.3, -1, 1)).astype(F)
    shift = (np.abs(scale) * _log_uniform(rng, -6, 6, C) * 0.3 * rng.standard_normal(C)).astype(F)
    scale[:4], shift[:4] = (1, 1, abs(scale[2]), -abs(scale[3])), (0.0, 0.0, 0.0, -0.0)
    x[..., 0] = rng.standard_normal((N, H, W))
    x[0, :4, :4, 0] = -1.0
    if H >= 3 and W >= 6:
        x[0, 2, 4:6, 0] = 5.0
    x[..., 1] = rng.random((N, H, W)) * 6
    x[:, [0, H - 1], :, 1] = 7.0
    x[:, :, [0, W - 1], 1] = 7.0
    zeros = rng.random((N, H, W)) < 0.2
    zeros[0, 0, 0] = True
    x[..., 2][zeros], x[..., 3][zeros] = 0.0, 0.0
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    dy = (_log_uniform(rng, -6, 6, C) * rng.standard_normal((N, Ho, Wo, C))).astype(F)
    mean = (x.reshape(-1, C).astype(D).mean(0) + 0.1 * x.reshape(-1, C).astype(D).std(0)).astype(F)
    gamma = (_log_uniform(rng, -10, 10, C) * np.where(rng.random(C) < 0.3, -1, 1)).astype(F)
    invstd = (1.0 / (x.reshape(-1, C).astype(D).std(0) + 1e-3)).astype(F)
    return dict(N=N, H=H, W=W, C=C, act=act, x=x, scale=scale, shift=shift, dy=dy, mean=mean, gamma=gamma, invstd=invstd, zeros=zeros)


def pool_want(p, mode="exact", slope=R.SLOPE, g_dev=None, part=None, n_tiles=None, coef=None):
    """Forward, gather, the fused sums and the fused dx.  The argmax is taken of the activation values as fp32 holds them (two values
    equal in fp32 tie there, whatever float64 makes of them); y is the float64 value at that position."""
    f = lambda a: np.asarray(a, D)
    N, H, W, C, act = p["N"], p["H"], p["W"], p["C"], p["act"]
    z, terms = R.pre_act(p["x"], f(p["scale"]), f(p["shift"]))
    zq = R.pre_act(p["x"], f(p["scale"]), f(p["shift"]), fp32=True)[0]
    _, idx = R.pool_fwd(R.act_fwd(zq, act, slope).astype(F).astype(D), mode)
    out = dict(idx=idx, y=R.pool_pick(R.act_fwd(z, act, slope), idx), y_terms=R.pool_pick(terms, idx))
    out["g"], out["g_abs"] = R.pool_bwd(p["dy"], idx, zq, act, slope, mode)
    g = (out["g"].astype(F).astype(D) if g_dev is None else f(g_dev)).reshape(-1, C)
    x, mean = f(p["x"]).reshape(-1, C), f(p["mean"])
    out["sums"], out["sums_abs"] = R.bwd_sums(g, x, mean, mode=mode)
    if part is None:
        part, n_tiles = out["sums"].astype(F)[None], 1
    out["coef"] = cw = R.bwd_coeffs(part, n_tiles, C, 1, N * H * W, p["gamma"], p["invstd"], mode)
    A, B, K = [f(a) for a in coef] if coef is not None else [cw[n].astype(F).astype(D) for n in "ABK"]
    # the fused dx takes g from registers: its roundings (g_abs) come on top of the three of x - mean and the two fmas
    dx, dx_terms = R.bwd_dx(out["g"].reshape(-1, C), x, mean, A, B, K, mode)
    out["dx"], out["dx_bar"] = dx.reshape(N, H, W, C), (U * (4 * np.abs(A) * out["g_abs"].reshape(-1, C) + 3 * dx_terms)).reshape(N, H, W, C)
    return out


def pool_fracs(got, want, p, tiles=1):
    fr = {}
    if "idx" in got:
        fr["idx"] = 0.0 if np.array_equal(got["idx"], want["idx"]) else np.inf
    if "y" in got:
        fr["y"] = frac(got["y"], want["y"], 2 * U * want["y_terms"])
    if "g" in got:
        fr["g"] = frac(got["g"], want["g"], 4 * U * want["g_abs"])
    if "sums" in got:
        fr["sums"] = frac(got["sums"][:2], want["sums"][:2], R.pool_chain(p["N"], p["H"], p["W"], p["C"], tiles) * U * want["sums_abs"][:2])
    if "coef" in got:
        fr.update({"coef." + n: v for n, v in coef_fracs(got["coef"], want["coef"]).items()})
    if "dx" in got:
        fr["dx"] = frac(got["dx"], want["dx"], want["dx_bar"])
    return fr


POOL_KEYS = ("idx", "y", "g", "sums", "coef", "dx")


# ------------------------------------------------------------------------------------------------ the launchers' source
# the functions of csrc/norm_act.hip that check arguments and launch (the extern "C" entry points forward to them)
LAUNCHERS = ["rd_bn_finalize", "rd_bn_stats_T", "rd_bn_act_T", "bn_bwd_reduce_impl", "rd_bn_bwd_apply_T", "rd_bn_bwd_apply_x_T", "rd_bn_bwd_apply_x2_T",
             "rd_bnact_maxpool_fwd_T", "rd_bnact_maxpool_bwd_T", "rd_bnact_maxpool_bwd_stats_T", "rd_bnact_maxpool_bwd_apply_T"]


def checks_precede_launches(source, function):
    """True when, in the body of `function` in csrc/norm_act.hip, argument checks exist and every one of them stands before the first
    kernel launch: only then may a refusal case be launched at all."""
    at = source.index(" " + function + "(")
    body = source[at:source.index("\n}\n", at)]
    checks = [i for i in range(len(body)) if body.startswith("RD_CHECK_ARG(", i)]
    # (a launch: hipLaunchKernelGGL, or the shared prologue of the kernels with > 64 KB of dynamic LDS, csrc/conv_host.h)
    launches = [i for i in (body.find("hipLaunchKernelGGL"), body.find("launch_dyn_lds<")) if i > 0]
    return bool(checks) and bool(launches) and max(checks) < min(launches)

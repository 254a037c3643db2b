"""The bf16-storage forms (dtype = RD_DTYPE_BF16) of csrc/norm_act.hip: the data, the float64 reference with the kernels' rounding
points, and the criterion tests/test_gpu_norm_bf16.py holds them to.  tests/test_norm_bf16_host.py shows that the criterion notices
every shortcut of MODES on these cases.  numpy only; the expressions are those of tests/norm_ref.py, the cases, planted data, channel
windows and fp32 bars those of tests/norm_cases.py.

Data: chain_data / pool_data / cond_data of norm_cases with every TENSOR operand (x1, x2, dy; the pool's x and dy) rounded to bf16, so
that it is exact in storage; per-channel vectors (gamma, beta, mean, scale, shift) stay fp32, as the kernels receive them.  The
planted exact zeros, the +0 / -0 shifts and the constant channel survive the rounding (0.1f becomes its bf16 neighbour): asserted.

Rounding points, as the code has them (bf16 values widen exactly on load; "rounds" = one round-to-nearest-even of the fp32 value in
the register, in st4 / round_store).  A stage that reads a stored bf16 tensor is fed what the stage before it left on the device; a
stage that keeps the value in registers is fed the unrounded value.

  entry point                    stores                  rounded                      reads / sums
  rd_bn_stats_t                  --                      --                           fp32 sums of the exact bf16 x
  rd_bn_act_t                    y                       once, AFTER the activation   --
  rd_bn_bwd_reduce_t             g                       once                         sign from the STORED y; sums of the UNROUNDED g
  rd_bn_bwd_reduce_x_t           g (optional)            once                         sign recomputed in fp32; sums of the UNROUNDED g
  rd_bn_bwd_reduce_x2_t          --                      --                           sign recomputed in fp32; sums of the UNROUNDED g
  rd_bn_bwd_apply_t              dx                      once                         the STORED (rounded) g
  rd_bn_bwd_apply_x_t            dx                      once                         g = dy * act' in registers: UNROUNDED
  rd_bn_bwd_apply_x2_t           dx1, dx2                once each                    g = dy * act' in registers: UNROUNDED
  rd_bnact_maxpool_fwd_t         y, idx                  y once (idx: fp32 argmax)    --
  rd_bnact_maxpool_bwd_t         g                       once                         --
  rd_bnact_maxpool_bwd_stats_t   g (optional)            once                         sums of the UNROUNDED g
  rd_bnact_maxpool_bwd_apply_t   dx                      g to bf16, then dx once      bit-identical to bwd_stats_t + rd_bn_bwd_apply_t
  rd_act_gate_t                  refuses RD_DTYPE_BF16 (RD_EPNP_DTYPE): an fp32-only entry point, it has no bf16 form

g = dy * act' is exact in bf16 for no activation and ReLU (a factor of 1 or 0), so "rounded" and "unrounded" g differ under
LeakyReLU only -- and in the pool, where up to four pooled gradients are added.  rd_bn_bwd_apply_x_t / _x2_t therefore differ from
reduce + rd_bn_bwd_apply_t under LeakyReLU by the bf16 rounding of g they do not perform: documented in the header, modelled here.

Criterion for a stored bf16 output: with the float64 value `want` and the fp32 bar b of norm_cases (k u sum|addends|, unchanged), a
correct kernel holds an fp32 value in [want - b, want + b] and rounds it once; rounding to nearest-even is monotone, so
    bf16(want - b) <= got <= bf16(want + b)          compared as values (-0.0 == +0.0).
The float64 endpoints go to fp32 with directed rounding (down / up) first: double rounding can then only widen the interval.  Behind
an activation the interval is taken on the pre-activation and both endpoints go through the (monotone) activation before they are
rounded.  No tensor-wide maximum, no ulp slack.  The constructed tie case (tie_data) multiplies 8-bit by 2-bit significands and adds
+0: every fp32 operation is exact there, so its bar is 0 and the stored value must be bf16(want) itself -- the only place where
ties-to-even can be told from ties-away.

fp32 outputs (partial sums, dgamma / dbeta, coef_ws, the conditioning contract) keep the fp32 bars of norm_cases: the inputs are
exact, and the chain length n + RL + 1 (n rows a thread adds: n - 1 additions; RL lanes: RL - 1 additions; x - mean, the product
and, under LeakyReLU, dy * 0.2f: 3) covers the sums of the unrounded g in float64.

Cap: for every case with M >= 15 rows and every stored output at most 5 % of the elements may have an interval that holds more than
one bf16 value (a property of reference and data, asserted on the CPU); smaller cases are interval-checked but exempt."""
import numpy as np

import norm_cases as NC
import norm_ref as R
import pack_ref as P

F, D = np.float32, np.float64
U = R.U
BF16 = 1          # RD_DTYPE_BF16
CAP, CAP_ROWS = 0.05, 15
MODES = ("truncate", "half_up", "halves_swapped", "ld_as_C", "c0_ignored", "sums_of_rounded_g", "dx_from_unrounded_g",
         "dx_x_from_rounded_g", "pool_dx_from_unrounded_g", "y_rounded_twice")


# ------------------------------------------------------------------------------------------------ bf16
def rb(a, mode="exact"):
    """float32 values rounded to bf16 (mode: pack_ref's truncate / half_up), as float32."""
    a = np.asarray(a, F)
    return P.bf16_to_f32(P.bf16_rne(a, mode if mode in ("truncate", "half_up") else "exact")).reshape(a.shape)


def bits(a):
    """bf16-exact float32 values -> their 16 bits."""
    return (np.ascontiguousarray(a, F).view(np.uint32) >> 16).astype(np.uint16)


def f32_directed(a, up):
    """float64 -> float32 rounded towards +inf (up) or -inf."""
    a = np.asarray(a, D)
    with np.errstate(all="ignore"):
        f = a.astype(F)
        bad = (f.astype(D) < a) if up else (f.astype(D) > a)
        return np.where(bad, np.nextafter(f, F(np.inf) if up else F(-np.inf)), f).astype(F)


def interval(lo64, hi64):
    """The bf16 values (as float64) a correct kernel may store for an fp32 value in [lo64, hi64]."""
    return rb(f32_directed(lo64, False)).astype(D), rb(f32_directed(hi64, True)).astype(D)


def held(got, lo64, hi64, mid64):
    """-> dict: out = elements outside their interval (non-finite ones included), wide = share of intervals holding more than one
    bf16 value, off = share of elements that are not the nearest bf16 of the reference itself (they sit on the other endpoint)."""
    lo, hi = interval(lo64, hi64)
    got = np.asarray(got, D)
    with np.errstate(all="ignore"):
        ok = (got >= lo) & (got <= hi)
        mid = rb(np.asarray(mid64, D).astype(F)).astype(D)
    return dict(out=int((~ok).sum()), n=int(got.size), wide=float((lo != hi).mean()) if got.size else 0.0,
                off=float((got != mid).mean()) if got.size else 0.0)


def _act_interval(z, b, act, slope):
    return R.act_fwd(z - b, act, slope), R.act_fwd(z + b, act, slope), R.act_fwd(z, act, slope)


# ------------------------------------------------------------------------------------------------ data
def chain_data(*case, **kw):
    d = NC.chain_data(*case, **kw)
    for k in ("x1", "x2", "dy"):
        if d[k] is not None:
            d[k] = rb(d[k])
    if d["plant"]:          # the plants are still what chain_data's comment says
        rows, pos, neg, const = d["plant"]["rows"], d["plant"]["pos"], d["plant"]["neg"], d["plant"]["const"]
        assert (d["x1"][rows][:, [pos, neg]] == 0).all() and d["gamma1"][pos] > 0 > d["gamma1"][neg]
        assert (d["x1"][:, const] == rb(F(0.1))).all() and rb(F(0.1)) != F(0.1)
        if d["x2"] is not None:
            assert (d["x2"][rows][:, [pos, neg]] == 0).all()
            assert d["res"] != "id" or (np.signbit(d["x2"][rows, neg]).all() and not np.signbit(d["x2"][rows, pos]).any())
    return d


def pool_data(*case, **kw):
    p = NC.pool_data(*case, **kw)
    p["x"], p["dy"] = rb(p["x"]), rb(p["dy"])
    H, W, x = p["H"], p["W"], p["x"]
    assert (x[0, :4, :4, 0] == -1).all() and (H < 3 or W < 6 or (x[0, 2, 4:6, 0] == 5).all())
    assert (x[:, [0, H - 1], :, 1] == 7).all() and (x[:, :, [0, W - 1], 1] == 7).all() and (H < 3 or W < 3 or x[:, 1:-1, 1:-1, 1].max() < 7)
    assert (x[..., 2][p["zeros"]] == 0).all() and (x[..., 3][p["zeros"]] == 0).all() and p["zeros"][0, 0, 0]
    assert p["shift"][2] == 0 and not np.signbit(p["shift"][2]) and p["shift"][3] == 0 and np.signbit(p["shift"][3]) and p["scale"][3] < 0
    return p


def cond_data(M, C, ratio):
    return rb(NC.cond_data(M, C, ratio))


def tie_data(act):
    """rd_bn_act_t, lone form, act 0 or 1, every fp32 operation exact: x runs through all 8-bit significands (both signs, one exponent
    per channel), scale has a 2-bit significand, shift is +0.  The exact products 1.5 x, 1.25 x, 0.75 x, 3 x are bf16 ties for about
    a quarter of the elements (235 of 1024; ties-to-even and ties-away differ on 118 of them)."""
    sig = np.arange(128, 256, dtype=D)
    x = np.stack([sig * 2.0 ** e for e in (-7, 0, 5, -20, 13, -3, 1, 9)], 1) * np.where(np.arange(128) % 3 == 0, -1.0, 1.0)[:, None]
    d = dict(M=128, C=8, act=act, res=None, plant=None, x1=x.astype(F), x2=None, dy=None, gamma2=None, beta2=None, exact=True)
    assert np.array_equal(rb(d["x1"]), d["x1"])
    co = dict(scale1=np.array([1.5, -1.5, 1.25, 0.75, 3.0, 1.0, -0.75, 2.0], F), shift1=np.zeros(8, F), scale2=None, shift2=None)
    return d, co


def n_ties(d, co):
    """Exact bf16 ties among the fp32 pre-activations of a tie case: (all, those where ties-to-even and ties-away differ)."""
    z = (d["x1"].astype(D) * co["scale1"].astype(D)).astype(F)
    assert np.array_equal(z.astype(D), d["x1"].astype(D) * co["scale1"].astype(D)), "the products are exact in fp32"
    tie = (z.view(np.uint32) & 0xffff) == 0x8000
    return int(tie.sum()), int((tie & (rb(z) != rb(z, "half_up"))).sum())


# ------------------------------------------------------------------------------------------------ what a shortcut reads
def _swap_halves(a):
    """The two 16-bit halves of every 32-bit word swapped on load: channels 2k and 2k + 1 exchanged."""
    a = np.asarray(a)
    return a.reshape(a.shape[:-1] + (-1, 2))[..., ::-1].reshape(a.shape)


def _load(a, ld, c0, mode):
    """[rows, C] as a kernel with the named shortcut reads it from its channel window (ld, c0) of the NaN-filled buffer."""
    if a is None:
        return None
    a = np.asarray(a, F)
    if mode == "halves_swapped":
        return _swap_halves(a)
    if mode in ("ld_as_C", "c0_ignored"):
        rows, C = a.shape
        flat = NC.wide(a, ld, c0).reshape(-1)
        at = np.arange(rows)[:, None] * (C if mode == "ld_as_C" else ld) + (c0 if mode == "ld_as_C" else 0) + np.arange(C)[None]
        return flat[at]
    return a


# ------------------------------------------------------------------------------------------------ the BatchNorm chain
def tile_bwd_sums(g, x1, m1, x2, m2, rpb):
    """norm_ref.bwd_sums per tile of rpb rows, as red_partial holds them -> ([tiles][3][C], the sums of the absolute terms): the
    chain bar bounds every partial sum, so each tile is held to it by itself."""
    starts = np.arange(0, g.shape[0], rpb)
    t = [g, g * (x1 - m1), np.zeros_like(g) if x2 is None else g * (x2 - m2)]
    return (np.stack([np.add.reduceat(v, starts, 0) for v in t], 1), np.stack([np.add.reduceat(np.abs(v), starts, 0) for v in t], 1))


def chain_want(d, co, slope=NC.SLOPE32, mode="exact", y_dev=None, g_dev=None, part=None, n_tiles=None, coef=None):
    """Everything the chain's bf16 forms produce from the fp32 coefficients co, as float64 values BEFORE the store's rounding, with
    the bars.  y_dev / g_dev (float64 of the stored bf16), part / n_tiles (red_partial) and coef = {which: [3][C]}: what the stages
    before left on the device; without them the reference feeds itself, rounding where a kernel stores.
    y: z (pre-activation), y_bar.  g (sign from the stored y) / g_x (sign recomputed in fp32), unrounded.  sums [tiles][3][C] of the
    unrounded g, one row per tile of red_partial.
    dx1 / dx2: rd_bn_bwd_apply_t, from the STORED g.  dx1_x / dx2_x: rd_bn_bwd_apply_x_t / _x2_t, from the unrounded g_x."""
    f = lambda a: None if a is None else np.asarray(a, D)
    M, C, act, bn2, lay = d["M"], d["C"], d["act"], d["res"] == "bn", NC.layout(d["C"])
    x1, x2 = f(_load(d["x1"], *lay["x1"], mode)), f(_load(d["x2"], *lay["x2"], mode))
    s2, t2 = (f(co["scale2"]), f(co["shift2"])) if bn2 else (None, None)
    with np.errstate(all="ignore"):
        z, terms = R.pre_act(x1, f(co["scale1"]), f(co["shift1"]), x2, s2, t2)
        if mode == "y_rounded_twice":
            z = rb(z.astype(F)).astype(D)
        out = dict(z=z, y=R.act_fwd(z, act, slope), y_bar=(0 if d.get("exact") else 2 if x2 is None else 3) * U * terms)
        if d["dy"] is None:
            return out
        dy = f(_load(d["dy"], *lay["dy"], mode))
        zq = R.pre_act(x1, f(co["scale1"]), f(co["shift1"]), x2, s2, t2, fp32=True)[0]
        out["g"] = R.bwd_g(dy, f(rb(out["y"].astype(F))) if y_dev is None else f(y_dev), act, slope)
        out["g_x"] = R.bwd_g(dy, zq, act, slope)
        g_st = f(rb(out["g"].astype(F))) if g_dev is None else f(g_dev)
        out["sums"], out["sums_abs"] = tile_bwd_sums(g_st if mode == "sums_of_rounded_g" else out["g"], x1, f(co["mean1"]), x2 if bn2 else None,
                                                     f(co["mean2"]) if bn2 else None, R.bwd_rows_per_block(M, C))
        if part is None:
            part, n_tiles = out["sums"].astype(F), out["sums"].shape[0]
        for w in (1, 2) if bn2 else (1,):
            k = str(w)
            cw = R.bwd_coeffs(part, n_tiles, C, w, M, d["gamma" + k], co["invstd" + k])
            A, B, K = [f(a) for a in coef[w]] if coef else [cw[n].astype(F).astype(D) for n in "ABK"]
            x = x1 if w == 1 else x2
            out["coef" + k] = cw
            out["dx" + k], out["dx%s_terms" % k] = R.bwd_dx(out["g"] if mode == "dx_from_unrounded_g" else g_st, x, f(co["mean" + k]), A, B, K)
            gx = f(rb(out["g_x"].astype(F))) if mode == "dx_x_from_rounded_g" else out["g_x"]
            out["dx%s_x" % k], out["dx%s_x_terms" % k] = R.bwd_dx(gx, x, f(co["mean" + k]), A, B, K)
    return out


CHAIN_STORED = ("y", "g", "g_x", "dx1", "dx2", "dx1_x", "dx2_x")


def stored(want, keys, mode="exact"):
    """What a kernel that computes `want` exactly in fp32 leaves in its bf16 tensors (mode: how it rounds); fp32 results as fp32."""
    out = {}
    with np.errstate(all="ignore"):
        for k in keys:
            if k in want and want[k] is not None:
                out[k] = rb(want[k].astype(F), mode).astype(D)
        for k in ("sums", "idx"):
            if k in want:
                out[k] = want[k].astype(F).astype(D) if k == "sums" else want[k]
        for k in ("coef1", "coef2", "coef"):
            if k in want:
                out[k] = {n: v.astype(F).astype(D) for n, v in want[k].items()}
    return out


def chain_held(got, want, d, slope=NC.SLOPE32):
    """-> ({stored output: held(...)}, {fp32 output: fraction of its bar}) for whichever outputs `got` has."""
    h, fr = {}, {}
    if "y" in got:
        h["y"] = held(got["y"], *_act_interval(want["z"], want["y_bar"], d["act"], slope))
    for k in ("g", "g_x"):
        if k in got:
            b = U * np.abs(want[k])
            h[k] = held(got[k], want[k] - b, want[k] + b, want[k])
    if "sums" in got:
        fr["sums"] = NC.frac(got["sums"], want["sums"], R.chain(d["M"], d["C"], True) * U * want["sums_abs"])
    for k in ("1", "2"):
        if "coef" + k in got:
            fr.update({"coef%s.%s" % (k, n): v for n, v in NC.coef_fracs(got["coef" + k], want["coef" + k]).items()})
        for n in ("dx" + k, "dx%s_x" % k):
            if n in got:
                b = 4 * U * want[n + "_terms"]
                h[n] = held(got[n], want[n] - b, want[n] + b, want[n])
    return h, fr


# ------------------------------------------------------------------------------------------------ the stem's BN / act / max-pool
def pool_want(p, slope=NC.SLOPE32, mode="exact", g_dev=None, part=None, n_tiles=None, coef=None):
    """Forward, gather, the fused sums (of the UNROUNDED g) and the two-pass dx (from g as bwd_stats_t stores it: rounded).  The argmax
    is taken of the fp32 activations of the bf16 x, first maximum wins; y is the float64 value at that position."""
    f = lambda a: np.asarray(a, D)
    N, H, W, C, act = p["N"], p["H"], p["W"], p["C"], p["act"]
    xin = _load(p["x"].reshape(-1, C), C, 0, mode).reshape(N, H, W, C) if mode == "halves_swapped" else p["x"]
    z, terms = R.pre_act(xin, f(p["scale"]), f(p["shift"]))
    zq = R.pre_act(xin, f(p["scale"]), f(p["shift"]), fp32=True)[0]
    _, idx = R.pool_fwd(R.act_fwd(zq, act, slope).astype(F).astype(D))
    out = dict(idx=idx, z=R.pool_pick(z, idx), y_bar=2 * U * R.pool_pick(terms, idx))
    out["y"] = R.act_fwd(out["z"], act, slope)
    out["g"], out["g_abs"] = R.pool_bwd(p["dy"], idx, zq, act, slope)
    g_st = (f(rb(out["g"].astype(F))) if g_dev is None else f(g_dev)).reshape(-1, C)
    x, mean = f(xin).reshape(-1, C), f(p["mean"])
    out["sums"], out["sums_abs"] = R.bwd_sums(g_st if mode == "sums_of_rounded_g" else out["g"].reshape(-1, C), x, mean)
    if part is None:
        part, n_tiles = out["sums"].astype(F)[None], 1
    out["coef"] = cw = R.bwd_coeffs(part, n_tiles, C, 1, N * H * W, p["gamma"], p["invstd"])
    A, B, K = [f(a) for a in coef] if coef is not None else [cw[n].astype(F).astype(D) for n in "ABK"]
    dx, dx_terms = R.bwd_dx(out["g"].reshape(-1, C) if mode == "pool_dx_from_unrounded_g" else g_st, x, mean, A, B, K)
    out["dx"], out["dx_terms"] = dx.reshape(N, H, W, C), dx_terms.reshape(N, H, W, C)
    return out


POOL_STORED = ("y", "g", "dx")


def pool_held(got, want, p, tiles=1, slope=NC.SLOPE32):
    h, fr = {}, {}
    if "idx" in got:
        fr["idx"] = 0.0 if np.array_equal(got["idx"], want["idx"]) else np.inf
    if "y" in got:
        h["y"] = held(got["y"], *_act_interval(want["z"], want["y_bar"], p["act"], slope))
    if "g" in got:
        b = 4 * U * want["g_abs"]
        h["g"] = held(got["g"], want["g"] - b, want["g"] + b, want["g"])
    if "sums" in got:
        fr["sums"] = NC.frac(got["sums"][:2], want["sums"][:2], R.pool_chain(p["N"], p["H"], p["W"], p["C"], tiles) * U * want["sums_abs"][:2])
    if "coef" in got:
        fr.update({"coef." + n: v for n, v in NC.coef_fracs(got["coef"], want["coef"]).items()})
    if "dx" in got:
        b = 4 * U * want["dx_terms"]
        h["dx"] = held(got["dx"], want["dx"] - b, want["dx"] + b, want["dx"])
    return h, fr


# ------------------------------------------------------------------------------------------------ reporting
def outside(h):
    return {k: v["out"] for k, v in h.items() if v["out"]}


def capped(h, rows):
    """The stored outputs whose share of multi-valued intervals exceeds the cap (cases below CAP_ROWS rows are exempt)."""
    return {k: v["wide"] for k, v in h.items() if rows >= CAP_ROWS and v["wide"] > CAP}


def line(what, h, fr=None):
    s = "BF16 %-44s" % what + " ".join("%s[out %d wide %.4f off %.4f]" % (k, v["out"], v["wide"], v["off"]) for k, v in sorted(h.items()))
    if fr:
        s += "  FRACTION worst %.3f %s" % (NC.worst(fr), " ".join("%s=%.3f" % kv for kv in sorted(fr.items())))
    return s

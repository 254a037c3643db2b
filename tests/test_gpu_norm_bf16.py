"""The bf16-storage forms of csrc/norm_act.hip (dtype = RD_DTYPE_BF16) -- rd_bn_stats_t, rd_bn_act_t, rd_bn_bwd_reduce_t / _x_t / _x2_t,
rd_bn_bwd_apply_t / _x_t / _x2_t, rd_bnact_maxpool_fwd_t / _bwd_t / _bwd_stats_t / _bwd_apply_t -- against the float64 reference of
tests/norm_bf16_cases.py, which models the rounding point of every form (the table in that module's docstring), on the cases of
tests/norm_cases.py.  rd_act_gate_t has no bf16 form: its documented refusal of RD_DTYPE_BF16 is what is tested.

Every tensor operand is a channel window of a wider buffer filled with bf16 NaN (strides and offsets on the 4-element grid the bf16
forms need: 8-byte accesses), with a NaN guard behind it: after each launch everything outside a written window is still NaN and
everything inside is finite.  Each stage is compared alone, fed what the stage before it left on the device.  A stored bf16 output
must lie in bf16(want - b) .. bf16(want + b), b the fp32 bar of norm_cases (no tensor-wide maximum, no ulp slack); fp32 outputs keep
their fp32 bars; the partial sums are held to the chain bar tile by tile.  tests/test_norm_bf16_host.py shows on the CPU that every
named shortcut (truncating or ties-away stores, swapped halves, a wrong stride or offset, sums of the rounded g, dx from the wrong g,
a y rounded twice) leaves these intervals, and that at most 5 % of the intervals hold more than one bf16 value.

Each test prints ("BF16 ..."; run with -s) per stored output the elements outside their interval, the share of intervals that hold
more than one bf16 value (wide) and the share of elements that are not the nearest bf16 of the float64 reference (off: they sit on the
other endpoint of such an interval), and the fractions of the fp32 bars.

Largest values observed on an MI355X when the file was added (records, not thresholds): no element outside its interval; wide 0.033
(y of 70000-4-2-bn; the pool's g 0.015; 0.003 elsewhere at 15 rows or more); off 0.0001 (the kernels store the nearest bf16 of the
float64 reference nearly everywhere); fp32 bars: backward partial sums per tile 0.44, rd_bn_stats_t sums 0.13, the pool's fused sums
0.13, finalize and coefficients 0.50 (one rounding of a double), conditioning contract 0.07."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import norm_bf16_cases as B
import norm_cases as NC
import norm_ref as R

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
BF16 = B.BF16          # RD_DTYPE_BF16
GUARD = 64             # elements of NaN behind every device buffer
NAN16 = 0x7fc0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _dev(a):
    """numpy array (fp32 / int64 / uint8) -> flat device tensor with a guard behind it (NaN, -1, 0xEE)."""
    a = np.ascontiguousarray(a).reshape(-1)
    tail = np.full(GUARD, 0xEE, np.uint8) if a.dtype == np.uint8 else np.full(GUARD, np.nan if a.dtype.kind == "f" else -1, a.dtype)
    return torch.from_numpy(np.concatenate([a, tail])).cuda()


def _nan(n):
    return _dev(np.full(n, np.nan, F))


def _np(t):
    a = t.cpu().numpy()
    assert np.isnan(a[a.size - GUARD:]).all() if a.dtype.kind == "f" else (a[a.size - GUARD:] == (0xEE if a.dtype == np.uint8 else -1)).all(), "guard"
    return a[:a.size - GUARD]


def _devb(a):
    """float32 values that are exact in bf16 (or NaN) -> flat device tensor of their 16 bits, GUARD bf16 NaNs behind it."""
    a = np.ascontiguousarray(a, F).reshape(-1)
    with np.errstate(all="ignore"):
        assert np.array_equal(B.rb(a), a, equal_nan=True), "the operand is not exact in bf16"
    u = np.concatenate([B.bits(a), np.full(GUARD, NAN16, np.uint16)])
    return torch.from_numpy(u.view(np.int16)).cuda()


def _nanb(n):
    return _devb(np.full(n, np.nan, F))


def _bitsb(t):
    """The 16-bit words of a bf16 device buffer (guard checked and dropped)."""
    u = t.cpu().numpy().view(np.uint16)
    assert (u[u.size - GUARD:] == NAN16).all(), "guard"
    return u[:u.size - GUARD]


def _npb(t):
    return (_bitsb(t).astype(np.uint32) << 16).view(F)


def _winb(t, rows, ld, c0, Cc):
    """The window [c0, c0 + C) of a bf16 device buffer as float64, after checking that nothing outside it was written."""
    a = _npb(t).reshape(rows, ld)
    assert NC.writes_ok(a, ld, c0, Cc), "a write outside the window, or a non-finite value inside it"
    return a[:, c0:c0 + Cc].astype(D)


def _p(t, elems=0):
    return C.c_void_p(None if t is None else t.data_ptr() + elems * t.element_size())


def _ok(rc, what):
    assert rc == 0, (what, rc, _L().rd_last_error())


def _i64(v):
    return C.c_int64(v)


def _report(what, h, fr, rows):
    print(B.line(what, h, fr))
    assert not B.outside(h), (what, "outside their interval", B.outside(h))
    assert NC.worst(fr) <= 1.0, (what, {k: v for k, v in fr.items() if v > 1.0})
    assert not B.capped(h, rows), (what, "more than 5 % of the intervals hold two bf16 values", B.capped(h, rows))


# ------------------------------------------------------------------------------------------------ the chain, stage by stage
def _stats_finalize(d, k, X, ld, c0, fr, running=True):
    """rd_bn_stats_t(BF16) on the window + rd_bn_finalize: the partial sums against float64 (chain u sum|term|), the finalize against
    the reference fed those partial sums (2u).  -> coefficients (float32 numpy)."""
    L, M, Cc = _L(), d["M"], d["C"]
    tiles = R.stats_tiles(M)
    part, nt = _nan(tiles * 2 * Cc), C.c_int32(0)
    _ok(L.rd_bn_stats_t(BF16, _p(X, c0), _i64(M), Cc, ld, _p(part), C.byref(nt), _st()), "rd_bn_stats_t")
    torch.cuda.synchronize()
    assert nt.value == tiles
    part_np = _np(part)
    sums, sabs = R.stats_sums(d["x" + k])
    fr["stats" + k] = NC.frac(part_np.astype(D).reshape(tiles, 2, Cc).sum(0), sums, R.chain(M, Cc, False) * NC.U * sabs)
    rng = np.random.default_rng(M + Cc)
    c = dict(n_tiles=tiles, ld=Cc, c0=0, C=Cc, count=M, eps=float(F(NC.EPS)), momentum=float(F(NC.MOMENTUM)), part=part_np, gamma=d["gamma" + k],
             beta=d["beta" + k], rm=rng.standard_normal(Cc).astype(F) if running else None, rv=(rng.random(Cc) + 0.5).astype(F) if running else None,
             nbt=5 if running else None, launches=1)
    rm, rv, nbt = (_dev(c["rm"]), _dev(c["rv"]), _dev(np.array([5], np.int64))) if running else (None, None, None)
    outs, gm, bt = [_nan(Cc) for _ in range(4)], _dev(c["gamma"]), _dev(c["beta"])
    _ok(L.rd_bn_finalize(_p(part), tiles, Cc, 0, Cc, _i64(M), _p(gm), _p(bt), C.c_float(c["eps"]), C.c_float(c["momentum"]),
                         _p(rm), _p(rv), _p(nbt), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _st()), "rd_bn_finalize")
    torch.cuda.synchronize()
    got = dict(zip(("mean", "invstd", "scale", "shift"), (_np(o).astype(D) for o in outs)))
    got.update(rm=_np(rm).astype(D) if running else None, rv=_np(rv).astype(D) if running else None, nbt=int(_np(nbt)[0]) if running else None)
    fr.update({"finalize%s.%s" % (k, n): v for n, v in NC.fin_fracs(got, NC.fin_want(c)).items()})
    return {n + k: got[n].astype(F) for n in ("mean", "invstd", "scale", "shift")}


def _run_chain(d, plant):
    """Every bf16 form of the chain on d's windows -> (coefficients, outputs as float64 windows, fractions of the stats / finalize bars)."""
    L, M, Cc, act, res = _L(), d["M"], d["C"], d["act"], d["res"]
    bn2, lay = res == "bn", NC.layout(d["C"])
    fr, out = {}, {}
    dev = {k: _devb(NC.wide(d[k], *lay[k])) for k in ("x1", "x2", "dy") if d[k] is not None}
    co = _stats_finalize(d, "1", dev["x1"], *lay["x1"], fr)
    co.update(_stats_finalize(d, "2", dev["x2"], *lay["x2"], fr, running=False) if bn2 else {n + "2": None for n in ("mean", "invstd", "scale", "shift")})
    if plant:
        co = NC.plant_shift(d, co)
    cd = {k: (None if v is None else _dev(v)) for k, v in co.items()}
    gam = {k: _dev(d["gamma" + k]) for k in ("1", "2") if d["gamma" + k] is not None}
    X1, X2, DY = _p(dev["x1"], lay["x1"][1]), (_p(dev["x2"], lay["x2"][1]) if res else None), _p(dev["dy"], lay["dy"][1])
    ldx1, ldx2, lddy = lay["x1"][0], (lay["x2"][0] if res else 0), lay["dy"][0]
    (ldy, cy), (ldg, cg), (ld1, c1), (ld2, c2) = lay["y"], lay["g"], lay["dx1"], lay["dx2"]
    # forward
    Y = _nanb(M * ldy)
    _ok(L.rd_bn_act_t(BF16, X1, ldx1, _p(cd["scale1"]), _p(cd["shift1"]), X2, ldx2, _p(cd["scale2"]), _p(cd["shift2"]), _p(Y, cy), ldy, _i64(M), Cc, act,
                      _st()), "rd_bn_act_t")
    # backward pass 1: the sign read from the stored y
    tiles = R.bwd_tiles(M, Cc)
    assert L.rd_bn_bwd_tiles(_i64(M), Cc) == tiles
    red, G = _nan(tiles * 3 * Cc), _nanb(M * ldg)
    _ok(L.rd_bn_bwd_reduce_t(BF16, DY, lddy, _p(Y, cy), ldy, X1, ldx1, _p(cd["mean1"]), X2 if bn2 else None, ldx2 if bn2 else 0, _p(cd["mean2"]), _p(G, cg),
                             ldg, _i64(M), Cc, act, _p(red), _st()), "rd_bn_bwd_reduce_t")
    torch.cuda.synchronize()
    out["y"], out["g"] = _winb(Y, M, ldy, cy, Cc), _winb(G, M, ldg, cg, Cc)
    red_np = _np(red).reshape(tiles, 3, Cc)
    assert np.isfinite(red_np).all()
    out["red"], out["tiles"], out["sums"] = red_np, tiles, red_np.astype(D)
    # backward pass 2: dx from the stored g
    for w in (1, 2) if bn2 else (1,):
        k = str(w)
        dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nanb(M * (ld1 if w == 1 else ld2))
        _ok(L.rd_bn_bwd_apply_t(BF16, _p(G, cg), ldg, X1 if w == 1 else X2, ldx1 if w == 1 else ldx2, _p(red), tiles, w, _p(gam[k]), _p(cd["mean" + k]),
                                _p(cd["invstd" + k]), _p(dG), _p(dB), _p(coef), _p(DX, c1 if w == 1 else c2), ld1 if w == 1 else ld2, _i64(M), Cc, _st()),
            "rd_bn_bwd_apply_t")
        torch.cuda.synchronize()
        cw = _np(coef).astype(D).reshape(3, Cc)
        out["coef" + k] = dict(dgamma=_np(dG).astype(D), dbeta=_np(dB).astype(D), A=cw[0], B=cw[1], K=cw[2])
        out["coef_ws" + k] = cw
        out["dx" + k] = _winb(DX, M, *((ld1, c1) if w == 1 else (ld2, c2)), Cc)
    # the forms that recompute the sign from x: bit-equal sums (and stored g); dx from the UNROUNDED g
    if act and res is None:
        red_x, Gx, red_n = _nan(tiles * 3 * Cc), _nanb(M * ldg), _nan(tiles * 3 * Cc)
        _ok(L.rd_bn_bwd_reduce_x_t(BF16, DY, lddy, X1, ldx1, _p(cd["mean1"]), _p(cd["scale1"]), _p(cd["shift1"]), _p(Gx, cg), ldg, _i64(M), Cc, act,
                                   _p(red_x), _st()), "rd_bn_bwd_reduce_x_t")
        _ok(L.rd_bn_bwd_reduce_x_t(BF16, DY, lddy, X1, ldx1, _p(cd["mean1"]), _p(cd["scale1"]), _p(cd["shift1"]), None, 0, _i64(M), Cc, act, _p(red_n),
                                   _st()), "rd_bn_bwd_reduce_x_t(g = NULL)")
        dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nanb(M * ld1)
        _ok(L.rd_bn_bwd_apply_x_t(BF16, DY, lddy, X1, ldx1, _p(red_n), tiles, _p(gam["1"]), _p(cd["mean1"]), _p(cd["invstd1"]), _p(cd["scale1"]),
                                  _p(cd["shift1"]), act, _p(dG), _p(dB), _p(coef), _p(DX, c1), ld1, _i64(M), Cc, _st()), "rd_bn_bwd_apply_x_t")
        torch.cuda.synchronize()
        rx, rn = _np(red_x).reshape(tiles, 3, Cc), _np(red_n).reshape(tiles, 3, Cc)
        out["g_x"] = _winb(Gx, M, ldg, cg, Cc)
        assert np.array_equal(_bitsb(Gx), _bitsb(G)), "reduce_x_t: the stored g bit for bit (NaN outside the window included)"
        assert np.array_equal(rx[:, :2], red_np[:, :2]) and np.array_equal(rn[:, :2], red_np[:, :2]), "reduce_x_t: sums bit for bit"
        assert np.array_equal(_np(coef).reshape(3, Cc), out["coef_ws1"].astype(F))
        out["dx1_x"] = _winb(DX, M, ld1, c1, Cc)
    if act and bn2:
        red2 = _nan(tiles * 3 * Cc)
        _ok(L.rd_bn_bwd_reduce_x2_t(BF16, DY, lddy, X1, ldx1, _p(cd["mean1"]), _p(cd["scale1"]), _p(cd["shift1"]), X2, ldx2, _p(cd["mean2"]),
                                    _p(cd["scale2"]), _p(cd["shift2"]), _i64(M), Cc, act, _p(red2), _st()), "rd_bn_bwd_reduce_x2_t")
        dg, db, coef6, DX1, DX2 = [_nan(Cc), _nan(Cc)], [_nan(Cc), _nan(Cc)], _nan(6 * Cc), _nanb(M * ld1), _nanb(M * ld2)
        _ok(L.rd_bn_bwd_apply_x2_t(BF16, DY, lddy, X1, ldx1, X2, ldx2, _p(red2), tiles, _p(gam["1"]), _p(cd["mean1"]), _p(cd["invstd1"]), _p(cd["scale1"]),
                                   _p(cd["shift1"]), _p(gam["2"]), _p(cd["mean2"]), _p(cd["invstd2"]), _p(cd["scale2"]), _p(cd["shift2"]), act, _p(dg[0]),
                                   _p(db[0]), _p(dg[1]), _p(db[1]), _p(coef6), _p(DX1, c1), ld1, _p(DX2, c2), ld2, _i64(M), Cc, _st()),
            "rd_bn_bwd_apply_x2_t")
        torch.cuda.synchronize()
        assert np.array_equal(_np(red2).reshape(tiles, 3, Cc), red_np), "reduce_x2_t: sums bit for bit"
        assert np.array_equal(_np(coef6).reshape(2, 3, Cc), np.stack([out["coef_ws1"], out["coef_ws2"]]).astype(F))
        assert np.array_equal(_np(dg[0]), out["coef1"]["dgamma"].astype(F)) and np.array_equal(_np(db[1]), out["coef2"]["dbeta"].astype(F))
        out["dx1_x"], out["dx2_x"] = _winb(DX1, M, ld1, c1, Cc), _winb(DX2, M, ld2, c2, Cc)
    return co, out, fr


def _chain_case(case, e2e):
    d = B.chain_data(*case, e2e=e2e)
    co, out, fr_fin = _run_chain(d, plant=not e2e)
    act = d["act"]
    want = B.chain_want(d, co, y_dev=out["y"], g_dev=out["g"], part=out["red"], n_tiles=out["tiles"],
                        coef={w: out["coef_ws%d" % w] for w in (1, 2) if "coef_ws%d" % w in out})
    keys = ("y", "g", "g_x", "sums", "coef1", "coef2", "dx1", "dx2", "dx1_x", "dx2_x")
    h, fr = B.chain_held({k: out[k] for k in keys if k in out}, want, d)
    assert np.array_equal(want["g"], want["g_x"]), "the sign of the stored y and of the recomputed pre-activation agree"
    if d["plant"] and act:
        rows, cols = d["plant"]["rows"], [d["plant"]["pos"], d["plant"]["neg"]]
        at = np.ix_(rows, cols)
        assert (out["y"][at] == 0).all() and (want["y"][at] == 0).all(), "planted zeros"
        k32 = F(0.0) if act == 1 else F(0.2)
        assert np.array_equal(out["g"][at].astype(F), B.rb(d["dy"][at] * k32)), "gradient at an output of exactly 0"
    _report(("e2e " if e2e else "") + NC.case_id(case), h, {**fr, **fr_fin}, d["M"])


@pytest.mark.parametrize("case", NC.CHAIN, ids=NC.case_id)
def test_chain_stage_by_stage(case):
    """rd_bn_stats_t -> rd_bn_finalize -> rd_bn_act_t -> rd_bn_bwd_reduce_t -> rd_bn_bwd_apply_t (and the _x_t / _x2_t pairs where the
    form applies) on channel windows of bf16 buffers, with the planted exact zeros, signed shifts and the constant channel."""
    _chain_case(case, e2e=False)


@pytest.mark.parametrize("case", NC.E2E, ids=NC.case_id)
def test_chain_on_the_end_to_end_data(case):
    """The same stages on the well-conditioned data of the fp32 end-to-end cases (nothing planted, the kernels' own coefficients
    throughout).  Under bf16 storage every stored stage carries a relative 2^-9, so there is no end-to-end figure to hold: each stage
    is held to its interval."""
    _chain_case(case, e2e=True)


@pytest.mark.parametrize("act", [0, 1])
def test_stores_round_ties_to_even(act):
    """rd_bn_act_t on the constructed tie case: every fp32 operation is exact, the bar is 0, and the stored value must be the
    ties-to-even bf16 of the exact product -- 235 exact ties per launch, 118 of them decided differently by ties-away."""
    d, co = B.tie_data(act)
    L, M, Cc, lay = _L(), d["M"], d["C"], NC.layout(d["C"])
    n, differ = B.n_ties(d, co)
    assert n >= 200 and differ >= 100
    (ldx, cx), (ldy, cy) = lay["x1"], lay["y"]
    X, Y, S, T = _devb(NC.wide(d["x1"], ldx, cx)), _nanb(M * ldy), _dev(co["scale1"]), _dev(co["shift1"])
    _ok(L.rd_bn_act_t(BF16, _p(X, cx), ldx, _p(S), _p(T), None, 0, None, None, _p(Y, cy), ldy, _i64(M), Cc, act, _st()),
        "rd_bn_act_t")
    torch.cuda.synchronize()
    want = B.chain_want(d, co)
    h, fr = B.chain_held(dict(y=_winb(Y, M, ldy, cy, Cc)), want, d)
    _report("ties act %d" % act, h, fr, M)
    assert h["y"]["wide"] == 0, "a bar of 0: every interval is one value"


# ------------------------------------------------------------------------------------------------ conditioning contract
@pytest.mark.parametrize("ratio", NC.COND_RATIOS)
@pytest.mark.parametrize("shape", NC.COND, ids=NC.case_id)
def test_conditioning_contract(shape, ratio):
    """invstd from rd_bn_stats_t(BF16) + rd_bn_finalize at mean / std = 0 .. 300 of bf16 data: the header's "accuracy of the training
    statistics" contract, unchanged (the inputs are exact, the sums fp32)."""
    M, Cc = shape
    x = B.cond_data(M, Cc, ratio)
    d = dict(M=M, C=Cc, x1=x, gamma1=np.ones(Cc, F), beta1=np.zeros(Cc, F))
    fr = {}
    co = _stats_finalize(d, "1", _devb(x), Cc, 0, fr)
    want, bound, cond = NC.cond_want(x)
    rel = np.abs(co["invstd1"].astype(D) - want) / want
    fr["invstd"] = float((rel / bound).max())
    print("conditioning mean/std %g: 1 + mean^2/var up to %.4g, relative error of invstd up to %.3g" % (ratio, cond.max(), rel.max()))
    _report("conditioning %s mean/std %g" % (NC.case_id(shape), ratio), {}, fr, M)


# ------------------------------------------------------------------------------------------------ the stem's BN / act / max-pool
@pytest.mark.parametrize("case", NC.POOL, ids=NC.case_id)
def test_stem_pool(case):
    """rd_bnact_maxpool_fwd_t / _bwd_t / _bwd_stats_t / _bwd_apply_t (BF16) on the planted ties, zeros and border rings, the pooled
    tensors as channel windows (x, g and dx have no stride in the signature): argmax bytes equal (the argmax is over the fp32
    activations of the bf16 x), y, g and dx in their intervals, the fused sums of the UNROUNDED g at the pool's chain bar, and the bit
    equalities: bwd_stats_t g == bwd_t g; two-pass dx == bwd_stats_t followed by rd_bn_bwd_apply_t."""
    N, H, W, Cc, act, forms = case
    L, p, lay = _L(), B.pool_data(N, H, W, Cc, act), NC.layout(Cc)
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    Mo, M = N * Ho * Wo, N * H * W
    (ldy, cy), (lddy, cdy) = lay["py"], lay["pdy"]
    X = _devb(p["x"])
    SC, SH, MEAN, GAM, INV = (_dev(p[k]) for k in ("scale", "shift", "mean", "gamma", "invstd"))
    Y, IDX, DY, G = _nanb(Mo * ldy), _dev(np.full(Mo * Cc, 0xEE, np.uint8)), _devb(NC.wide(p["dy"], lddy, cdy)), _nanb(M * Cc)
    _ok(L.rd_bnact_maxpool_fwd_t(BF16, _p(X), _p(SC), _p(SH), act, N, H, W, Cc, _p(Y, cy), ldy, _p(IDX), _st()), "rd_bnact_maxpool_fwd_t")
    _ok(L.rd_bnact_maxpool_bwd_t(BF16, _p(DY, cdy), lddy, _p(IDX), _p(X), _p(SC), _p(SH), act, N, H, W, Cc, _p(G), _st()), "rd_bnact_maxpool_bwd_t")
    torch.cuda.synchronize()
    got = dict(idx=_np(IDX).reshape(N, Ho, Wo, Cc), y=_winb(Y, Mo, ldy, cy, Cc).reshape(N, Ho, Wo, Cc), g=_npb(G).astype(D).reshape(N, H, W, Cc))
    tiles, kw = 1, {}
    if forms == "all":
        tiles = L.rd_bnact_maxpool_bwd_tiles(N, H, W, Cc)
        red, red_n, G2 = _nan(tiles * 3 * Cc), _nan(tiles * 3 * Cc), _nanb(M * Cc)
        _ok(L.rd_bnact_maxpool_bwd_stats_t(BF16, _p(DY, cdy), lddy, _p(IDX), _p(X), _p(SC), _p(SH), act, N, H, W, Cc, _p(G2), _p(MEAN), _p(red), _st()),
            "rd_bnact_maxpool_bwd_stats_t")
        _ok(L.rd_bnact_maxpool_bwd_stats_t(BF16, _p(DY, cdy), lddy, _p(IDX), _p(X), _p(SC), _p(SH), act, N, H, W, Cc, None, _p(MEAN), _p(red_n), _st()),
            "rd_bnact_maxpool_bwd_stats_t(g = NULL)")
        dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nanb(M * Cc)
        _ok(L.rd_bnact_maxpool_bwd_apply_t(BF16, _p(DY, cdy), lddy, _p(IDX), _p(X), _p(SC), _p(SH), act, N, H, W, Cc, _p(red_n), tiles, _p(GAM), _p(MEAN),
                                           _p(INV), _p(dG), _p(dB), _p(coef), _p(DX), _st()), "rd_bnact_maxpool_bwd_apply_t")
        dG1, dB1, coef1, DX1 = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nanb(M * Cc)
        _ok(L.rd_bn_bwd_apply_t(BF16, _p(G2), Cc, _p(X), Cc, _p(red), tiles, 1, _p(GAM), _p(MEAN), _p(INV), _p(dG1), _p(dB1), _p(coef1), _p(DX1), Cc, _i64(M),
                                Cc, _st()), "rd_bn_bwd_apply_t")
        torch.cuda.synchronize()
        red_np = _np(red).reshape(tiles, 3, Cc)
        assert np.array_equal(_bitsb(G2), _bitsb(G)), "bwd_stats_t: g bit for bit"
        assert np.array_equal(_np(red_n).reshape(tiles, 3, Cc)[:, :2], red_np[:, :2]), "sums with and without g"
        assert np.array_equal(_np(coef), _np(coef1)) and np.array_equal(_np(dG), _np(dG1)) and np.array_equal(_np(dB), _np(dB1))
        assert np.array_equal(_bitsb(DX), _bitsb(DX1)), "two-pass dx == bwd_stats_t g followed by rd_bn_bwd_apply_t, bit for bit"
        cw = _np(coef).astype(D).reshape(3, Cc)
        got.update(sums=red_np.astype(D).sum(0), coef=dict(dgamma=_np(dG).astype(D), dbeta=_np(dB).astype(D), A=cw[0], B=cw[1], K=cw[2]),
                   dx=_npb(DX).astype(D).reshape(N, H, W, Cc))
        kw = dict(part=red_np, n_tiles=tiles, coef=cw)
    assert np.isfinite(got["g"]).all() and ("dx" not in got or np.isfinite(got["dx"]).all())
    want = B.pool_want(p, g_dev=got["g"], **kw)
    if act == 1:
        assert (got["g"][..., 2][p["zeros"]] == 0).all() and (got["g"][..., 3][p["zeros"]] == 0).all(), "ReLU gradient at +0.0 / -0.0"
    h, fr = B.pool_held(got, want, p, tiles)
    _report("pool " + NC.case_id(case), h, fr, M)


# ------------------------------------------------------------------------------------------------ refusals
SENT = 0x7fc5a5a5          # a NaN with a payload: no kernel writes it


def test_refusals_of_the_storage_typed_forms():
    """Every storage-typed launcher refuses, before anything is launched (the source is read first: a case is only sent to a launcher
    whose checks all stand before its first launch), a dtype that is neither RD_DTYPE_F32 nor RD_DTYPE_BF16 and, with RD_DTYPE_BF16, a
    stride off the 4-element grid or below C on every strided operand.  rd_act_gate_t refuses RD_DTYPE_BF16 itself (RD_EPNP_DTYPE): it
    is an fp32-only entry point.  The sentinel-filled buffers stay untouched."""
    L = _L()
    src = open(os.path.join(REPO, "radar_depth_amd", "csrc", "norm_act.hip")).read()
    for fn in NC.LAUNCHERS:
        assert NC.checks_precede_launches(src, fn), fn
    pnp = open(os.path.join(REPO, "radar_depth_amd", "csrc", "pnp.hip")).read()
    gate = pnp[pnp.index('extern "C" int rd_act_gate_t('):]
    gate = gate[:gate.index("\n}\n")]
    assert 0 < gate.index("dtype == RD_DTYPE_F32") < gate.index("hipLaunchKernelGGL"), "rd_act_gate_t checks its dtype before it launches"
    bufs = [torch.from_numpy(np.full(4096, SENT, np.uint32).view(np.int32)).cuda() for _ in range(4)]
    I, O, O2, Bb = (C.c_void_p(b.data_ptr()) for b in bufs)          # inputs, outputs, more outputs, argmax bytes
    st, nt, i64 = _st(), C.c_int32(-7), _i64
    specs = {
        "rd_bn_stats_t": ([("x", I), ("M", i64(8)), ("C", 8), ("ldx", 8), ("part", O), ("nt", C.byref(nt)), ("st", st)], ("ldx",)),
        "rd_bn_act_t": ([("x1", I), ("ldx1", 8), ("s1", I), ("t1", I), ("x2", I), ("ldx2", 8), ("s2", I), ("t2", I), ("y", O), ("ldy", 8), ("M", i64(8)),
                         ("C", 8), ("act", 1), ("st", st)], ("ldx1", "ldx2", "ldy")),
        "rd_bn_bwd_reduce_t": ([("dy", I), ("lddy", 8), ("y", I), ("ldy", 8), ("x1", I), ("ldx1", 8), ("m1", I), ("x2", I), ("ldx2", 8), ("m2", I), ("g", O),
                                ("ldg", 8), ("M", i64(8)), ("C", 8), ("act", 1), ("red", O2), ("st", st)], ("lddy", "ldy", "ldx1", "ldx2", "ldg")),
        "rd_bn_bwd_reduce_x_t": ([("dy", I), ("lddy", 8), ("x1", I), ("ldx1", 8), ("m1", I), ("s1", I), ("t1", I), ("g", O), ("ldg", 8), ("M", i64(8)),
                                  ("C", 8), ("act", 2), ("red", O2), ("st", st)], ("lddy", "ldx1", "ldg")),
        "rd_bn_bwd_reduce_x2_t": ([("dy", I), ("lddy", 8), ("x1", I), ("ldx1", 8), ("m1", I), ("s1", I), ("t1", I), ("x2", I), ("ldx2", 8), ("m2", I),
                                   ("s2", I), ("t2", I), ("M", i64(8)), ("C", 8), ("act", 1), ("red", O2), ("st", st)], ("lddy", "ldx1", "ldx2")),
        "rd_bn_bwd_apply_t": ([("g", I), ("ldg", 8), ("x", I), ("ldx", 8), ("red", I), ("n_tiles", 1), ("which", 1), ("gamma", I), ("mean", I), ("invstd", I),
                               ("dgamma", O2), ("dbeta", O2), ("coef", O2), ("dx", O), ("lddx", 8), ("M", i64(8)), ("C", 8), ("st", st)],
                              ("ldg", "ldx", "lddx")),
        "rd_bn_bwd_apply_x_t": ([("dy", I), ("lddy", 8), ("x", I), ("ldx", 8), ("red", I), ("n_tiles", 1), ("gamma", I), ("mean", I), ("invstd", I),
                                 ("scale", I), ("shift", I), ("act", 1), ("dgamma", O2), ("dbeta", O2), ("coef", O2), ("dx", O), ("lddx", 8), ("M", i64(8)),
                                 ("C", 8), ("st", st)], ("lddy", "ldx", "lddx")),
        "rd_bn_bwd_apply_x2_t": ([("dy", I), ("lddy", 8), ("x1", I), ("ldx1", 8), ("x2", I), ("ldx2", 8), ("red", I), ("n_tiles", 1), ("g1", I), ("m1", I),
                                  ("i1", I), ("s1", I), ("t1", I), ("g2", I), ("m2", I), ("i2", I), ("s2", I), ("t2", I), ("act", 1), ("dg1", O2), ("db1", O2),
                                  ("dg2", O2), ("db2", O2), ("coef6", O2), ("dx1", O), ("lddx1", 8), ("dx2", O), ("lddx2", 8), ("M", i64(8)), ("C", 8),
                                  ("st", st)], ("lddy", "ldx1", "ldx2", "lddx1", "lddx2")),
        "rd_bnact_maxpool_fwd_t": ([("x", I), ("scale", I), ("shift", I), ("act", 1), ("N", 1), ("H", 4), ("W", 4), ("C", 8), ("y", O), ("ldy", 8), ("idx", Bb),
                                    ("st", st)], ("ldy",)),
        "rd_bnact_maxpool_bwd_t": ([("dy", I), ("lddy", 8), ("idx", I), ("x", I), ("scale", I), ("shift", I), ("act", 1), ("N", 1), ("H", 4), ("W", 4),
                                    ("C", 8), ("g", O), ("st", st)], ("lddy",)),
        "rd_bnact_maxpool_bwd_stats_t": ([("dy", I), ("lddy", 8), ("idx", I), ("x", I), ("scale", I), ("shift", I), ("act", 1), ("N", 1), ("H", 4), ("W", 4),
                                          ("C", 8), ("g", O), ("mean", I), ("red", O2), ("st", st)], ("lddy",)),
        "rd_bnact_maxpool_bwd_apply_t": ([("dy", I), ("lddy", 8), ("idx", I), ("x", I), ("scale", I), ("shift", I), ("act", 1), ("N", 1), ("H", 4),
                                          ("W", 4), ("C", 8), ("red", I), ("n_tiles", 1), ("gamma", I), ("mean", I), ("invstd", I), ("dgamma", O2),
                                          ("dbeta", O2), ("coef", O2), ("dx", O), ("st", st)], ("lddy",)),
    }
    n = 0
    for name, (spec, strides) in specs.items():
        fn = getattr(L, name)
        bad = [(7, {}), (-1, {}), (2, {})] + [(BF16, {k: v}) for k in strides for v in (10, 6, 4)]          # 10, 6: off the grid; 4: below C
        for dtype, over in bad:
            rc = fn(dtype, *[over.get(k, v) for k, v in spec])
            assert rc == -1, "%s(dtype %d, %r) returned %d: %s" % (name, dtype, over, rc, L.rd_last_error())
            assert L.rd_last_error(), name
            n += 1
    # rd_act_gate_t: no bf16 form
    rc = L.rd_act_gate_t(BF16, I, 8, C.c_void_p(I.value + 8192), 8, O, 8, 8, 8, 1, st)
    assert rc == -47, "rd_act_gate_t(RD_DTYPE_BF16) returned %d, not RD_EPNP_DTYPE" % rc
    torch.cuda.synchronize()
    for b in bufs:
        assert (b.cpu().numpy().view(np.uint32) == SENT).all(), "a refused call wrote"
    assert nt.value == -7
    print("refused %d calls" % (n + 1))

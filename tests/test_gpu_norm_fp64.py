"""The fp32 entry points of csrc/norm_act.hip -- rd_bn_stats, rd_bn_finalize, rd_bn_act, the three backward forms (reduce / apply,
reduce_x / apply_x, reduce_x2 / apply_x2) and the stem's fused BN / activation / max-pool (fwd, bwd, bwd_stats,
rd_bnact_maxpool_bwd_apply_t(RD_DTYPE_F32)) -- against tests/norm_ref.py, the numpy float64 restatement of the header.

Cases, planted data, channel windows and bars are those of tests/norm_cases.py (derived there, not tuned); tests/test_norm_host.py
proves the restatement against torch float64 and shows that each named shortcut misses these bars on these cases.  Every tensor
operand is a channel window of a wider NaN-filled buffer with its own stride: after each launch everything outside a written window
must still be NaN.  Each stage is compared with the reference fed what the stage before it left on the device (the kernel's own fp32
coefficients, y, g, partial sums), so a figure measures one kernel alone; the end-to-end test then runs the chain from the raw inputs.
Each test prints the largest fraction of its bars it observed ("FRACTION <class> ..."); run with -s to see them.

Largest fractions of the bars observed on an MI355X when the file was added: finalize and coefficients 0.50 (one rounding of a double),
element-wise 0.95 (g = dy * 0.2f, a single rounding held to u |g|; 0.66 on everything else), fp32 reductions 0.20, conditioning contract
0.06, end to end 0.017 of the figures."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import norm_cases as NC
import norm_ref as R

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
GUARD = 64          # floats of NaN behind every device buffer
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _dev(a):
    """numpy array -> flat device tensor with GUARD NaNs (0xEE bytes for uint8) behind it."""
    a = np.ascontiguousarray(a).reshape(-1)
    tail = np.full(GUARD, 0xEE, np.uint8) if a.dtype == np.uint8 else np.full(GUARD, np.nan if a.dtype.kind == "f" else -1, a.dtype)
    return torch.from_numpy(np.concatenate([a, tail])).cuda()


def _nan(n):
    return _dev(np.full(n, np.nan, F))


def _np(t, n=None):
    a = t.cpu().numpy()
    assert np.isnan(a[a.size - GUARD:]).all() if a.dtype.kind == "f" else (a[a.size - GUARD:] == (0xEE if a.dtype == np.uint8 else -1)).all(), "guard"
    return a[:a.size - GUARD] if n is None else a[:n]


def _p(t, elems=0):
    return C.c_void_p(None if t is None else t.data_ptr() + elems * t.element_size())


def _ok(rc, what):
    assert rc == 0, (what, rc, _L().rd_last_error())


def _i64(v):
    return C.c_int64(v)


def _win(t, rows, ld, c0, Cc):
    """The window [c0, c0 + C) of a device buffer as float64, after checking that nothing outside it was written."""
    a = _np(t).reshape(rows, ld)
    assert NC.writes_ok(a, ld, c0, Cc), "a write outside the window, or a non-finite value inside it"
    return a[:, c0:c0 + Cc].astype(D)


def _report(cls, what, fr):
    print("FRACTION %-12s %-40s worst %.3f  %s" % (cls, what, NC.worst(fr), " ".join("%s=%.3f" % kv for kv in sorted(fr.items()))))
    assert NC.worst(fr) <= 1.0, (cls, what, {k: v for k, v in fr.items() if v > 1.0})


# ------------------------------------------------------------------------------------------------ finalize / coefficients: exact integers
def _finalize(c, part, gamma, beta, rm, rv, nbt):
    Cc = c["C"]
    outs = [_nan(Cc) for _ in range(4)]
    for _ in range(c.get("launches", 1)):
        _ok(_L().rd_bn_finalize(_p(part), c["n_tiles"], c["ld"], c["c0"], Cc, _i64(c["count"]), _p(gamma), _p(beta), C.c_float(c["eps"]),
                                C.c_float(c["momentum"]), _p(rm), _p(rv), _p(nbt), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _st()),
            "rd_bn_finalize")
    torch.cuda.synchronize()
    got = dict(zip(("mean", "invstd", "scale", "shift"), (_np(o).astype(D) for o in outs)))
    got.update(rm=None if rm is None else _np(rm).astype(D), rv=None if rv is None else _np(rv).astype(D), nbt=None if nbt is None else int(_np(nbt)[0]))
    return got, outs


FIN = NC.fin_cases()


@pytest.mark.parametrize("i", range(len(FIN)), ids=lambda i: "t%d-ld%d-c%d-C%d-n%s-m%g-x%d%s%s" % (
    FIN[i]["n_tiles"], FIN[i]["ld"], FIN[i]["c0"], FIN[i]["C"], FIN[i]["count"], FIN[i]["momentum"], FIN[i]["launches"],
    "" if FIN[i]["rm"] is not None else "-norun", "" if FIN[i]["nbt"] is not None else "-nonbt"))
def test_finalize_on_exact_integer_partials(i):
    """Synthetic [n_tiles][2][ld] partial sums of integers, NaN outside the channel window: every tile count around the 768 and 1024
    of the four-tiles-per-trip loop, every (ld, c0, C), nonzero running statistics, momentum 0.1 and 1, count 1 / 2 / M, running
    statistics or num_batches_tracked absent, two launches on the same buffers.  The kernel evaluates the reference's double
    expressions and rounds once: 2u on everything, num_batches_tracked exact."""
    c = FIN[i]
    rm, rv = (None, None) if c["rm"] is None else (_dev(c["rm"]), _dev(c["rv"]))
    nbt = None if c["nbt"] is None else _dev(np.array([c["nbt"]], np.int64))
    got, _ = _finalize(c, _dev(c["part"]), _dev(c["gamma"]), _dev(c["beta"]), rm, rv, nbt)
    want = NC.fin_want(c)
    _report("finalize", "n_tiles %d" % c["n_tiles"], NC.fin_fracs(got, want))
    if c["count"] == 7 * c["n_tiles"]:          # channel 0: variance exactly 0; channel 1: -1/count, clamped
        r0 = 1.0 / np.sqrt(c["eps"])
        assert np.all(np.abs(got["invstd"][:2] - r0) <= 2 * NC.U * r0) and np.array_equal(want["invstd"][:2], [r0, r0])
    if c["launches"] == 2 and c["nbt"] is not None:
        assert got["nbt"] == 2


@pytest.mark.parametrize("n_tiles", NC.N_TILES)
def test_backward_coefficients_on_exact_integer_partials(n_tiles):
    """The same for bn_bwd_coeffs_kernel: one synthetic [n_tiles][3][C] array through rd_bn_bwd_apply (which = 1 and 2), _x, _x2 and
    rd_bnact_maxpool_bwd_apply_t(RD_DTYPE_F32) with a small M: dgamma, dbeta and the A, B, K they apply, 2u each."""
    L, Cc, N, H, W = _L(), 16, 1, 1, 5
    M, Wo = N * H * W, R.pool_out(W)
    rng = np.random.default_rng(n_tiles)
    red_np = NC.synth_red(n_tiles, Cc, 1)
    red = _dev(red_np)
    gm = [(NC._log_uniform(rng, -10, 10, Cc) * np.where(rng.random(Cc) < 0.3, -1, 1)).astype(F) for _ in range(2)]
    inv = [NC._log_uniform(rng, -8, 8, Cc).astype(F) for _ in range(2)]
    vec = lambda: _dev(rng.standard_normal(Cc).astype(F))
    ten = lambda rows=M: _dev(rng.standard_normal((rows, Cc)).astype(F))
    G, X, X2, mean, sc, sh, DYp = ten(), ten(), ten(), vec(), vec(), vec(), ten(Wo)
    gmd, invd = [_dev(a) for a in gm], [_dev(a) for a in inv]
    idx = _dev(np.full(Wo * Cc, 4, np.uint8))
    fr = {}

    def compare(tag, which, dG, dB, coef, off=0):
        cw = _np(coef).astype(D)[off:off + 3 * Cc].reshape(3, Cc)
        got = dict(dgamma=_np(dG).astype(D), dbeta=_np(dB).astype(D), A=cw[0], B=cw[1], K=cw[2])
        want = R.bwd_coeffs(red_np, n_tiles, Cc, which, M, gm[which - 1], inv[which - 1])
        fr.update({tag + "." + k: v for k, v in NC.coef_fracs(got, want).items()})

    for which in (1, 2):
        dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nan(M * Cc)
        _ok(L.rd_bn_bwd_apply(_p(G), Cc, _p(X), Cc, _p(red), n_tiles, which, _p(gmd[which - 1]), _p(mean), _p(invd[which - 1]), _p(dG), _p(dB),
                              _p(coef), _p(DX), Cc, _i64(M), Cc, _st()), "rd_bn_bwd_apply")
        torch.cuda.synchronize()
        compare("apply%d" % which, which, dG, dB, coef)
        assert np.isfinite(_np(DX)).all()
    dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nan(M * Cc)
    _ok(L.rd_bn_bwd_apply_x(_p(G), Cc, _p(X), Cc, _p(red), n_tiles, _p(gmd[0]), _p(mean), _p(invd[0]), _p(sc), _p(sh), 1, _p(dG), _p(dB), _p(coef),
                            _p(DX), Cc, _i64(M), Cc, _st()), "rd_bn_bwd_apply_x")
    torch.cuda.synchronize()
    compare("apply_x", 1, dG, dB, coef)
    dg, db, coef6, DX1, DX2 = [_nan(Cc), _nan(Cc)], [_nan(Cc), _nan(Cc)], _nan(6 * Cc), _nan(M * Cc), _nan(M * Cc)
    _ok(L.rd_bn_bwd_apply_x2(_p(G), Cc, _p(X), Cc, _p(X2), Cc, _p(red), n_tiles, _p(gmd[0]), _p(mean), _p(invd[0]), _p(sc), _p(sh), _p(gmd[1]), _p(mean),
                             _p(invd[1]), _p(sc), _p(sh), 2, _p(dg[0]), _p(db[0]), _p(dg[1]), _p(db[1]), _p(coef6), _p(DX1), Cc, _p(DX2), Cc, _i64(M), Cc,
                             _st()), "rd_bn_bwd_apply_x2")
    torch.cuda.synchronize()
    compare("apply_x2.1", 1, dg[0], db[0], coef6)
    compare("apply_x2.2", 2, dg[1], db[1], coef6, 3 * Cc)
    dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nan(M * Cc)
    _ok(L.rd_bnact_maxpool_bwd_apply_t(0, _p(DYp), Cc, _p(idx), _p(X), _p(sc), _p(sh), 1, N, H, W, Cc, _p(red), n_tiles, _p(gmd[0]), _p(mean), _p(invd[0]),
                                       _p(dG), _p(dB), _p(coef), _p(DX), _st()), "rd_bnact_maxpool_bwd_apply_t")
    torch.cuda.synchronize()
    compare("pool_apply", 1, dG, dB, coef)
    assert np.isfinite(_np(DX)).all()
    _report("finalize", "coefficients, n_tiles %d" % n_tiles, fr)


# ------------------------------------------------------------------------------------------------ the chain, stage by stage
def _stats_finalize(d, k, X, lay, fr, running=True):
    """rd_bn_stats + rd_bn_finalize of operand k on its window; the partial sums against float64 (chain u sum|term|), the finalize
    against the reference fed those partial sums (2u).  -> coefficients (float32 numpy)."""
    L, M, Cc = _L(), d["M"], d["C"]
    ld, c0 = lay["x" + k]
    tiles = R.stats_tiles(M)
    assert L.rd_bn_stats_tiles(_i64(M)) == tiles
    part, nt = _nan(tiles * 2 * Cc), C.c_int32(0)
    _ok(L.rd_bn_stats(_p(X, c0), _i64(M), Cc, ld, _p(part), C.byref(nt), _st()), "rd_bn_stats")
    torch.cuda.synchronize()
    assert nt.value == tiles
    part_np = _np(part)
    sums, sabs = R.stats_sums(d["x" + k])
    fr["stats" + k] = NC.frac(part_np.astype(D).reshape(tiles, 2, Cc).sum(0), sums, R.chain(M, Cc, False) * NC.U * sabs)
    rng = np.random.default_rng(M + Cc)
    c = dict(n_tiles=tiles, ld=Cc, c0=0, C=Cc, count=M, eps=float(F(NC.EPS)), momentum=float(F(NC.MOMENTUM)), part=part_np, gamma=d["gamma" + k],
             beta=d["beta" + k], rm=rng.standard_normal(Cc).astype(F) if running else None, rv=(rng.random(Cc) + 0.5).astype(F) if running else None,
             nbt=5 if running else None, launches=1)
    got, outs = _finalize(c, part, _dev(c["gamma"]), _dev(c["beta"]), None if c["rm"] is None else _dev(c["rm"]),
                          None if c["rv"] is None else _dev(c["rv"]), None if c["nbt"] is None else _dev(np.array([5], np.int64)))
    fr.update({"finalize%s.%s" % (k, n): v for n, v in NC.fin_fracs(got, NC.fin_want(c)).items()})
    return {n + k: got[n].astype(F) for n in ("mean", "invstd", "scale", "shift")}


def _run_chain(d, plant):
    """Every kernel of the chain on d's windows.  -> (coefficients, outputs as float64 windows, fractions of the stats / finalize bars,
    the device-side facts the bit-equality promises are about)."""
    L, M, Cc, act, res = _L(), d["M"], d["C"], d["act"], d["res"]
    bn2, lay = res == "bn", NC.layout(d["C"])
    fr, out = {}, {}
    dev = {k: _dev(NC.wide(d[k], *lay[k])) for k in ("x1", "x2", "dy") if d[k] is not None}
    co = _stats_finalize(d, "1", dev["x1"], lay, fr)
    co.update(_stats_finalize(d, "2", dev["x2"], lay, fr, running=False) if bn2 else {n + "2": None for n in ("mean", "invstd", "scale", "shift")})
    if plant:
        co = NC.plant_shift(d, co)
    cd = {k: (None if v is None else _dev(v)) for k, v in co.items()}
    gam = {k: _dev(d["gamma" + k]) for k in ("1", "2") if d["gamma" + k] is not None}
    X1, X2, DY = _p(dev["x1"], lay["x1"][1]), (_p(dev["x2"], lay["x2"][1]) if res else None), _p(dev["dy"], lay["dy"][1])
    ldx1, ldx2, lddy = lay["x1"][0], (lay["x2"][0] if res else 0), lay["dy"][0]
    (ldy, cy), (ldg, cg), (ld1, c1), (ld2, c2) = lay["y"], lay["g"], lay["dx1"], lay["dx2"]
    # forward
    Y = _nan(M * ldy)
    _ok(L.rd_bn_act(X1, ldx1, _p(cd["scale1"]), _p(cd["shift1"]), X2, ldx2, _p(cd["scale2"]), _p(cd["shift2"]), _p(Y, cy), ldy, _i64(M), Cc, act, _st()),
        "rd_bn_act")
    # backward pass 1: the sign read from y
    tiles = R.bwd_tiles(M, Cc)
    assert L.rd_bn_bwd_tiles(_i64(M), Cc) == tiles
    red, G = _nan(tiles * 3 * Cc), _nan(M * ldg)
    _ok(L.rd_bn_bwd_reduce(DY, lddy, _p(Y, cy), ldy, X1, ldx1, _p(cd["mean1"]), X2 if bn2 else None, ldx2 if bn2 else 0, _p(cd["mean2"]), _p(G, cg), ldg,
                           _i64(M), Cc, act, _p(red), _st()), "rd_bn_bwd_reduce")
    torch.cuda.synchronize()
    out["y"], out["g"] = _win(Y, M, ldy, cy, Cc), _win(G, M, ldg, cg, Cc)
    red_np = _np(red).reshape(tiles, 3, Cc)
    assert np.isfinite(red_np).all()
    out["red"], out["tiles"], out["sums"] = red_np, tiles, red_np.astype(D).sum(0)
    # backward pass 2
    for w in (1, 2) if bn2 else (1,):
        k = str(w)
        dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nan(M * (ld1 if w == 1 else ld2))
        _ok(L.rd_bn_bwd_apply(_p(G, cg), ldg, X1 if w == 1 else X2, ldx1 if w == 1 else ldx2, _p(red), tiles, w, _p(gam[k]), _p(cd["mean" + k]),
                              _p(cd["invstd" + k]), _p(dG), _p(dB), _p(coef), _p(DX, c1 if w == 1 else c2), ld1 if w == 1 else ld2, _i64(M), Cc, _st()),
            "rd_bn_bwd_apply")
        torch.cuda.synchronize()
        cw = _np(coef).astype(D).reshape(3, Cc)
        out["coef" + k] = dict(dgamma=_np(dG).astype(D), dbeta=_np(dB).astype(D), A=cw[0], B=cw[1], K=cw[2])
        out["coef_ws" + k] = cw
        out["dx" + k] = _win(DX, M, *((ld1, c1) if w == 1 else (ld2, c2)), Cc)
    # the forms that recompute the sign from x: bit-equal sums (and g), the same dx to the same bars
    if act and res is None:
        red_x, Gx, red_n = _nan(tiles * 3 * Cc), _nan(M * ldg), _nan(tiles * 3 * Cc)
        _ok(L.rd_bn_bwd_reduce_x(DY, lddy, X1, ldx1, _p(cd["mean1"]), _p(cd["scale1"]), _p(cd["shift1"]), _p(Gx, cg), ldg, _i64(M), Cc, act, _p(red_x),
                                 _st()), "rd_bn_bwd_reduce_x")
        _ok(L.rd_bn_bwd_reduce_x(DY, lddy, X1, ldx1, _p(cd["mean1"]), _p(cd["scale1"]), _p(cd["shift1"]), None, 0, _i64(M), Cc, act, _p(red_n), _st()),
            "rd_bn_bwd_reduce_x(g = NULL)")
        dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nan(M * ld1)
        _ok(L.rd_bn_bwd_apply_x(DY, lddy, X1, ldx1, _p(red_n), tiles, _p(gam["1"]), _p(cd["mean1"]), _p(cd["invstd1"]), _p(cd["scale1"]), _p(cd["shift1"]),
                                act, _p(dG), _p(dB), _p(coef), _p(DX, c1), ld1, _i64(M), Cc, _st()), "rd_bn_bwd_apply_x")
        torch.cuda.synchronize()
        rx, rn = _np(red_x).reshape(tiles, 3, Cc), _np(red_n).reshape(tiles, 3, Cc)
        assert np.array_equal(_np(Gx).view(np.uint32), _np(G).view(np.uint32)), "reduce_x: g bit for bit (NaN outside the window included)"
        assert np.array_equal(rx[:, :2], red_np[:, :2]) and np.array_equal(rn[:, :2], red_np[:, :2]), "reduce_x: sums bit for bit"
        assert np.array_equal(_np(coef).reshape(3, Cc), out["coef_ws1"].astype(F))
        out["dx1_x"] = _win(DX, M, ld1, c1, Cc)
    if act and bn2:
        red2 = _nan(tiles * 3 * Cc)
        _ok(L.rd_bn_bwd_reduce_x2(DY, lddy, X1, ldx1, _p(cd["mean1"]), _p(cd["scale1"]), _p(cd["shift1"]), X2, ldx2, _p(cd["mean2"]), _p(cd["scale2"]),
                                  _p(cd["shift2"]), _i64(M), Cc, act, _p(red2), _st()), "rd_bn_bwd_reduce_x2")
        dg, db, coef6, DX1, DX2 = [_nan(Cc), _nan(Cc)], [_nan(Cc), _nan(Cc)], _nan(6 * Cc), _nan(M * ld1), _nan(M * ld2)
        _ok(L.rd_bn_bwd_apply_x2(DY, lddy, X1, ldx1, X2, ldx2, _p(red2), tiles, _p(gam["1"]), _p(cd["mean1"]), _p(cd["invstd1"]), _p(cd["scale1"]),
                                 _p(cd["shift1"]), _p(gam["2"]), _p(cd["mean2"]), _p(cd["invstd2"]), _p(cd["scale2"]), _p(cd["shift2"]), act, _p(dg[0]),
                                 _p(db[0]), _p(dg[1]), _p(db[1]), _p(coef6), _p(DX1, c1), ld1, _p(DX2, c2), ld2, _i64(M), Cc, _st()), "rd_bn_bwd_apply_x2")
        torch.cuda.synchronize()
        assert np.array_equal(_np(red2).reshape(tiles, 3, Cc), red_np), "reduce_x2: sums bit for bit"
        assert np.array_equal(_np(coef6).reshape(2, 3, Cc), np.stack([out["coef_ws1"], out["coef_ws2"]]).astype(F))
        assert np.array_equal(_np(dg[0]), out["coef1"]["dgamma"].astype(F)) and np.array_equal(_np(db[1]), out["coef2"]["dbeta"].astype(F))
        out["dx1_x"], out["dx2_x"] = _win(DX1, M, ld1, c1, Cc), _win(DX2, M, ld2, c2, Cc)
    return co, out, fr


@pytest.mark.parametrize("case", NC.CHAIN, ids=NC.case_id)
def test_chain_stage_by_stage(case):
    """rd_bn_stats -> rd_bn_finalize -> rd_bn_act -> reduce -> apply (and the _x / _x2 pairs where the form applies) on channel
    windows, with the planted exact zeros and the constant channel; every stage against float64 at its own bar."""
    d = NC.chain_data(*case)
    co, out, fr_fin = _run_chain(d, plant=True)
    M, Cc, act = d["M"], d["C"], d["act"]
    want = NC.chain_want(d, co, slope=NC.SLOPE32, y_dev=out["y"], g_dev=out["g"], part=out["red"], n_tiles=out["tiles"],
                         coef={w: out["coef_ws%d" % w] for w in (1, 2) if "coef_ws%d" % w in out})
    fr = NC.chain_fracs({k: out[k] for k in NC.CHAIN_KEYS if k in out}, want, d)
    for k in ("1", "2"):          # apply_x / apply_x2: g = dy * act' is formed in registers -- the same four roundings
        if "dx%s_x" % k in out:
            fr["dx%s_x" % k] = NC.frac(out["dx%s_x" % k], want["dx" + k], 4 * NC.U * want["dx%s_terms" % k])
    assert np.array_equal(want["g"], want["g_x"]), "the sign of y and of the recomputed pre-activation agree"
    if d["plant"] and act:
        rows, cols = d["plant"]["rows"], [d["plant"]["pos"], d["plant"]["neg"]]
        at = np.ix_(rows, cols)
        assert (out["y"][at] == 0).all() and (want["y"][at] == 0).all(), "planted zeros"
        k32 = F(0.0) if act == 1 else F(0.2)
        assert np.array_equal(out["g"][at].astype(F), d["dy"][at] * k32), "gradient at an output of exactly 0"
    _report("reduction", NC.case_id(case), {k: v for k, v in {**fr, **fr_fin}.items() if k.startswith(("stats", "sums"))})
    _report("finalize", NC.case_id(case), {k: v for k, v in {**fr, **fr_fin}.items() if k.startswith(("finalize", "coef"))})
    _report("element-wise", NC.case_id(case), {k: v for k, v in fr.items() if k.startswith(("y", "g", "dx"))})


@pytest.mark.parametrize("case", NC.E2E, ids=NC.case_id)
def test_end_to_end_from_raw_inputs(case):
    """stats -> finalize -> act -> reduce -> apply from the raw inputs against the whole chain in float64, per channel, at the figures
    of tests/test_gpu_norm.py (2e-5 for y and dbeta, 5e-5 for dgamma and dx) on the well-conditioned cases (tests/test_norm_host.py
    bounds their conditioning)."""
    d = NC.chain_data(*case, e2e=True)
    _, out, _ = _run_chain(d, plant=False)
    want = NC.e2e_want(d)
    got = dict(y=out["y"], dbeta1=out["coef1"]["dbeta"][None], dgamma1=out["coef1"]["dgamma"][None], dx1=out["dx1"])
    want = dict(want, dbeta1=want["dbeta1"][None], dgamma1=want["dgamma1"][None])
    if d["res"] == "bn":
        got.update(dgamma2=out["coef2"]["dgamma"][None], dx2=out["dx2"])
        want["dgamma2"] = want["dgamma2"][None]
    elif d["res"] == "id":
        got["dx2"] = out["g"]
    print("conditioning", NC.case_id(case), want["cond"])
    _report("end-to-end", NC.case_id(case), NC.e2e_fracs(got, want))


# ------------------------------------------------------------------------------------------------ conditioning contract
@pytest.mark.parametrize("ratio", NC.COND_RATIOS)
@pytest.mark.parametrize("shape", NC.COND, ids=NC.case_id)
def test_conditioning_contract(shape, ratio):
    """invstd from rd_bn_stats + rd_bn_finalize at mean / std = 0 .. 300: relative error within
    chain u (E[x^2] + 2 |mean| E|x|) / (2 (var + eps)), the header's "accuracy of the training statistics" contract."""
    M, Cc = shape
    x = NC.cond_data(M, Cc, ratio)
    d = dict(M=M, C=Cc, x1=x, gamma1=np.ones(Cc, F), beta1=np.zeros(Cc, F))
    co = _stats_finalize(d, "1", _dev(x), dict(x1=(Cc, 0)), {})
    want, bound, cond = NC.cond_want(x)
    rel = np.abs(co["invstd1"].astype(D) - want) / want
    print("conditioning mean/std %g: 1 + mean^2/var up to %.4g, relative error of invstd up to %.3g, bound %.3g" % (ratio, cond.max(), rel.max(), bound[rel.argmax()]))
    _report("conditioning", "%s mean/std %g" % (NC.case_id(shape), ratio), dict(invstd=float((rel / bound).max())))


# ------------------------------------------------------------------------------------------------ the stem's BN / act / max-pool
@pytest.mark.parametrize("case", NC.POOL, ids=NC.case_id)
def test_stem_pool(case):
    """rd_bnact_maxpool_fwd / _bwd / _bwd_stats / rd_bnact_maxpool_bwd_apply_t(F32) on the planted ties, zeros and border rings, the
    pooled tensors as channel windows: argmax bytes equal, y and the gather at their bars, the fused sums at the pool's chain, and the
    promised bit equalities (bwd_stats g == bwd g; two-pass dx == one-pass g followed by rd_bn_bwd_apply)."""
    N, H, W, Cc, act, forms = case
    L, p, lay = _L(), NC.pool_data(N, H, W, Cc, act), NC.layout(Cc)
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    Mo, M = N * Ho * Wo, N * H * W
    (ldy, cy), (lddy, cdy) = lay["py"], lay["pdy"]
    X, SC, SH, MEAN, GAM, INV = (_dev(p[k]) for k in ("x", "scale", "shift", "mean", "gamma", "invstd"))
    Y, IDX, DY, G = _nan(Mo * ldy), _dev(np.full(Mo * Cc, 0xEE, np.uint8)), _dev(NC.wide(p["dy"], lddy, cdy)), _nan(M * Cc)
    _ok(L.rd_bnact_maxpool_fwd(_p(X), _p(SC), _p(SH), act, N, H, W, Cc, _p(Y, cy), ldy, _p(IDX), _st()), "rd_bnact_maxpool_fwd")
    _ok(L.rd_bnact_maxpool_bwd(_p(DY, cdy), lddy, _p(IDX), _p(X), _p(SC), _p(SH), act, N, H, W, Cc, _p(G), _st()), "rd_bnact_maxpool_bwd")
    torch.cuda.synchronize()
    got = dict(idx=_np(IDX).reshape(N, Ho, Wo, Cc), y=_win(Y, Mo, ldy, cy, Cc).reshape(N, Ho, Wo, Cc), g=_np(G).astype(D).reshape(N, H, W, Cc))
    tiles, kw = 1, {}
    if forms == "all":
        tiles = L.rd_bnact_maxpool_bwd_tiles(N, H, W, Cc)
        red, red_n, G2 = _nan(tiles * 3 * Cc), _nan(tiles * 3 * Cc), _nan(M * Cc)
        _ok(L.rd_bnact_maxpool_bwd_stats(_p(DY, cdy), lddy, _p(IDX), _p(X), _p(SC), _p(SH), act, N, H, W, Cc, _p(G2), _p(MEAN), _p(red), _st()), "bwd_stats")
        _ok(L.rd_bnact_maxpool_bwd_stats(_p(DY, cdy), lddy, _p(IDX), _p(X), _p(SC), _p(SH), act, N, H, W, Cc, None, _p(MEAN), _p(red_n), _st()),
            "bwd_stats(g = NULL)")
        dG, dB, coef, DX = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nan(M * Cc)
        _ok(L.rd_bnact_maxpool_bwd_apply_t(0, _p(DY, cdy), lddy, _p(IDX), _p(X), _p(SC), _p(SH), act, N, H, W, Cc, _p(red_n), tiles, _p(GAM), _p(MEAN),
                                           _p(INV), _p(dG), _p(dB), _p(coef), _p(DX), _st()), "bwd_apply_t")
        dG1, dB1, coef1, DX1 = _nan(Cc), _nan(Cc), _nan(3 * Cc), _nan(M * Cc)
        _ok(L.rd_bn_bwd_apply(_p(G2), Cc, _p(X), Cc, _p(red), tiles, 1, _p(GAM), _p(MEAN), _p(INV), _p(dG1), _p(dB1), _p(coef1), _p(DX1), Cc, _i64(M), Cc,
                              _st()), "rd_bn_bwd_apply")
        torch.cuda.synchronize()
        red_np = _np(red).reshape(tiles, 3, Cc)
        assert np.array_equal(_np(G2), _np(G)), "bwd_stats: g bit for bit"
        assert np.array_equal(_np(red_n).reshape(tiles, 3, Cc)[:, :2], red_np[:, :2]), "sums with and without g"
        assert np.array_equal(_np(coef), _np(coef1)) and np.array_equal(_np(dG), _np(dG1)) and np.array_equal(_np(dB), _np(dB1))
        assert np.array_equal(_np(DX), _np(DX1)), "two-pass dx == one-pass g followed by rd_bn_bwd_apply, bit for bit"
        cw = _np(coef).astype(D).reshape(3, Cc)
        got.update(sums=red_np.astype(D).sum(0), coef=dict(dgamma=_np(dG).astype(D), dbeta=_np(dB).astype(D), A=cw[0], B=cw[1], K=cw[2]),
                   dx=_np(DX).astype(D).reshape(N, H, W, Cc))
        kw = dict(part=red_np, n_tiles=tiles, coef=cw)
    want = NC.pool_want(p, slope=NC.SLOPE32, g_dev=got["g"], **kw)
    assert np.isfinite(got["g"]).all()
    if act == 1:
        assert (got["g"][..., 2][p["zeros"]] == 0).all() and (got["g"][..., 3][p["zeros"]] == 0).all(), "ReLU gradient at +0.0 / -0.0"
    fr = NC.pool_fracs(got, want, p, tiles)
    _report("reduction", "pool " + NC.case_id(case), {k: v for k, v in fr.items() if k == "sums"})
    _report("finalize", "pool " + NC.case_id(case), {k: v for k, v in fr.items() if k.startswith("coef")})
    _report("element-wise", "pool " + NC.case_id(case), {k: v for k, v in fr.items() if k in ("idx", "y", "g", "dx")})


# ------------------------------------------------------------------------------------------------ refusals
SENT = 0x7fc5a5a5          # a NaN with a payload: no kernel writes it


def _call(fn, spec, **over):
    assert all(k in dict(spec) for k in over), over
    return fn(*[over[n] if n in over else v for n, v in spec])


def test_refusals_are_uniform_and_touch_nothing():
    """Every launcher refuses (RD_EINVAL, before anything is launched -- the source is read first: a case is only sent to a launcher
    whose checks all stand before its first hipLaunchKernelGGL) C < 4, C % 4, a stride that is no multiple of 4 or narrower than C on
    an operand that is given, M / n_tiles / N / H / W <= 0, which outside {1, 2} and a NULL required pointer; the reduce and stats
    forms C > 1024; the pool's stats and apply forms a C/4 that does not divide 256.  The sentinel-filled buffers stay untouched."""
    L = _L()
    src = open(os.path.join(REPO, "radar_depth_amd", "csrc", "norm_act.hip")).read()
    for fn in NC.LAUNCHERS:
        assert NC.checks_precede_launches(src, fn), fn
    bufs = [torch.from_numpy(np.full(4096, SENT, np.uint32).view(np.int32)).cuda() for _ in range(4)]
    I, O, O2, B = (C.c_void_p(b.data_ptr()) for b in bufs)          # inputs, outputs, more outputs, argmax bytes
    st, f, nt = _st(), C.c_float(0.1), C.c_int32(-7)
    i64 = _i64
    zero, big = (("C", 0), ("C", 2), ("C", 6)), (("C", 1028),)
    specs = {
        "rd_bn_finalize": ([("part", I), ("n_tiles", 1), ("ld", 8), ("c0", 0), ("C", 8), ("count", i64(8)), ("gamma", I), ("beta", I), ("eps", f), ("mom", f),
                            ("rm", O2), ("rv", O2), ("nbt", O2), ("mean", O), ("invstd", O), ("scale", O), ("shift", O), ("st", st)],
                           zero + (("n_tiles", 0), ("count", i64(0)), ("ld", 6), ("ld", 10), ("ld", 4), ("c0", -4), ("c0", 4), ("part", None), ("gamma", None),
                                   ("mean", None), ("shift", None), ("rm", None), ("rv", None))),
        "rd_bn_stats": ([("x", I), ("M", i64(8)), ("C", 8), ("ldx", 8), ("part", O), ("nt", C.byref(nt)), ("st", st)],
                        zero + big + (("M", i64(0)), ("M", i64(-3)), ("ldx", 10), ("ldx", 4), ("x", None), ("part", None))),
        "rd_bn_act": ([("x1", I), ("ldx1", 8), ("s1", I), ("t1", I), ("x2", I), ("ldx2", 8), ("s2", I), ("t2", I), ("y", O), ("ldy", 8), ("M", i64(8)), ("C", 8),
                       ("act", 1), ("st", st)],
                      zero + (("M", i64(0)), ("ldx1", 10), ("ldx1", 4), ("ldx2", 6), ("ldx2", 4), ("ldy", 10), ("ldy", 4), ("x1", None), ("s1", None), ("t1", None),
                              ("y", None), ("t2", None))),
        "rd_bn_bwd_reduce": ([("dy", I), ("lddy", 8), ("y", I), ("ldy", 8), ("x1", I), ("ldx1", 8), ("m1", I), ("x2", I), ("ldx2", 8), ("m2", I), ("g", O),
                              ("ldg", 8), ("M", i64(8)), ("C", 8), ("act", 1), ("red", O2), ("st", st)],
                             zero + big + (("M", i64(0)), ("lddy", 10), ("lddy", 4), ("ldy", 6), ("ldx1", 4), ("ldx2", 10), ("ldg", 4), ("ldg", 9), ("dy", None),
                                           ("red", None), ("m1", None), ("m2", None), ("y", None))),
        "rd_bn_bwd_reduce_x": ([("dy", I), ("lddy", 8), ("x1", I), ("ldx1", 8), ("m1", I), ("s1", I), ("t1", I), ("g", O), ("ldg", 8), ("M", i64(8)), ("C", 8),
                                ("act", 2), ("red", O2), ("st", st)],
                               zero + big + (("M", i64(0)), ("lddy", 6), ("ldx1", 4), ("ldg", 10), ("dy", None), ("red", None), ("s1", None), ("t1", None),
                                             ("x1", None), ("m1", None))),
        "rd_bn_bwd_reduce_x2": ([("dy", I), ("lddy", 8), ("x1", I), ("ldx1", 8), ("m1", I), ("s1", I), ("t1", I), ("x2", I), ("ldx2", 8), ("m2", I), ("s2", I),
                                 ("t2", I), ("M", i64(8)), ("C", 8), ("act", 1), ("red", O2), ("st", st)],
                                zero + big + (("M", i64(0)), ("lddy", 4), ("ldx1", 10), ("ldx2", 6), ("dy", None), ("red", None), ("x2", None), ("s2", None),
                                              ("m2", None), ("act", 0))),
        "rd_bn_bwd_apply": ([("g", I), ("ldg", 8), ("x", I), ("ldx", 8), ("red", I), ("n_tiles", 1), ("which", 1), ("gamma", I), ("mean", I), ("invstd", I),
                             ("dgamma", O2), ("dbeta", O2), ("coef", O2), ("dx", O), ("lddx", 8), ("M", i64(8)), ("C", 8), ("st", st)],
                            zero + (("which", 0), ("which", 3), ("n_tiles", 0), ("n_tiles", -1), ("M", i64(0)), ("ldg", 10), ("ldx", 4), ("lddx", 6), ("g", None),
                                    ("x", None), ("red", None), ("gamma", None), ("mean", None), ("invstd", None), ("coef", None), ("dx", None))),
        "rd_bn_bwd_apply_x": ([("dy", I), ("lddy", 8), ("x", I), ("ldx", 8), ("red", I), ("n_tiles", 1), ("gamma", I), ("mean", I), ("invstd", I), ("scale", I),
                               ("shift", I), ("act", 1), ("dgamma", O2), ("dbeta", O2), ("coef", O2), ("dx", O), ("lddx", 8), ("M", i64(8)), ("C", 8), ("st", st)],
                              zero + (("n_tiles", 0), ("M", i64(0)), ("lddy", 10), ("ldx", 4), ("lddx", 6), ("dy", None), ("x", None), ("red", None),
                                      ("scale", None), ("shift", None), ("coef", None), ("dx", None))),
        "rd_bn_bwd_apply_x2": ([("dy", I), ("lddy", 8), ("x1", I), ("ldx1", 8), ("x2", I), ("ldx2", 8), ("red", I), ("n_tiles", 1), ("g1", I), ("m1", I), ("i1", I),
                                ("s1", I), ("t1", I), ("g2", I), ("m2", I), ("i2", I), ("s2", I), ("t2", I), ("act", 1), ("dg1", O2), ("db1", O2), ("dg2", O2),
                                ("db2", O2), ("coef6", O2), ("dx1", O), ("lddx1", 8), ("dx2", O), ("lddx2", 8), ("M", i64(8)), ("C", 8), ("st", st)],
                               zero + (("n_tiles", 0), ("M", i64(0)), ("lddy", 10), ("ldx1", 4), ("ldx2", 6), ("lddx1", 4), ("lddx2", 10), ("dy", None), ("x2", None),
                                       ("red", None), ("i2", None), ("t2", None), ("coef6", None), ("dx1", None), ("dx2", None))),
        "rd_bnact_maxpool_fwd": ([("x", I), ("scale", I), ("shift", I), ("act", 1), ("N", 1), ("H", 4), ("W", 4), ("C", 8), ("y", O), ("ldy", 8), ("idx", B),
                                  ("st", st)],
                                 zero + (("N", 0), ("H", 0), ("W", -1), ("ldy", 10), ("ldy", 4), ("x", None), ("scale", None), ("shift", None), ("y", None),
                                         ("idx", None))),
        "rd_bnact_maxpool_bwd": ([("dy", I), ("lddy", 8), ("idx", I), ("x", I), ("scale", I), ("shift", I), ("act", 1), ("N", 1), ("H", 4), ("W", 4), ("C", 8),
                                  ("g", O), ("st", st)],
                                 zero + (("N", 0), ("H", -2), ("W", 0), ("lddy", 10), ("lddy", 4), ("dy", None), ("idx", None), ("x", None), ("g", None))),
        "rd_bnact_maxpool_bwd_stats": ([("dy", I), ("lddy", 8), ("idx", I), ("x", I), ("scale", I), ("shift", I), ("act", 1), ("N", 1), ("H", 4), ("W", 4),
                                        ("C", 8), ("g", O), ("mean", I), ("red", O2), ("st", st)],
                                       zero + (("C", 48), ("C", 80), ("N", 0), ("H", 0), ("W", 0), ("lddy", 10), ("lddy", 4), ("dy", None), ("idx", None),
                                               ("mean", None), ("red", None))),
        "rd_bnact_maxpool_bwd_apply_t": ([("dtype", 0), ("dy", I), ("lddy", 8), ("idx", I), ("x", I), ("scale", I), ("shift", I), ("act", 1), ("N", 1), ("H", 4),
                                          ("W", 4), ("C", 8), ("red", I), ("n_tiles", 1), ("gamma", I), ("mean", I), ("invstd", I), ("dgamma", O2), ("dbeta", O2),
                                          ("coef", O2), ("dx", O), ("st", st)],
                                         zero + (("C", 48), ("C", 80), ("dtype", 7), ("n_tiles", 0), ("N", 0), ("H", 0), ("W", 0), ("lddy", 10), ("lddy", 4),
                                                 ("dy", None), ("idx", None), ("red", None), ("gamma", None), ("coef", None), ("dx", None))),
    }
    n = 0
    for name, (spec, bad) in specs.items():
        for key, value in bad:
            rc = _call(getattr(L, name), spec, **{key: value})
            assert rc == -1, "%s(%s = %r) returned %d: %s" % (name, key, getattr(value, "value", value), rc, L.rd_last_error())
            assert L.rd_last_error(), name
            n += 1
    assert L.rd_bn_bwd_tiles(i64(8), 6) == -1 and L.rd_bn_bwd_tiles(i64(0), 8) == -1
    torch.cuda.synchronize()
    for b in bufs:
        assert (b.cpu().numpy().view(np.uint32) == SENT).all(), "a refused call wrote"
    assert nt.value == -7
    print("refused %d calls" % n)

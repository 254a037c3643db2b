"""The cases tests/test_gpu_head.py runs on the device and tests/test_head_host.py shows to be sensitive to every shortcut of
head_ref.MODES: shapes, data, the channel windows x and dx live in, the float64 results and the bars they are held to.

Bars (u = 2^-24; derived from csrc/head.hip, per element, never a tensor-wide maximum):
  conv forward, tiled      38 u sum|x w|: a channel quad's 36 fmas (9 taps x 4 channels into one accumulator), then the two DPP additions
  conv forward, untiled    15 u sum|x w|: per tap a four-term dot (a product and three fmas: 4), the tap's accumulation s = fma(ok, a, s)
                           (9 of them behind the first addend), the two DPP additions
  conv dgrad, both forms   9 u sum|dd w|: nine fmas into one accumulator
  conv wgrad               chain u sum|x dd| per (channel, tap), chain = head_ref.wgrad_chain(pixels, blocks) with the block count the
                           library reports (rd_head_conv_bwd_workspace_floats / (9 C) - 16)
  bilinear                 head_ref.bilinear_fwd / bilinear_bwd: 6u resp. (K + 4) u on the weighted absolute values plus the coordinate
                           terms (the kernel's coordinate within 2u s(o) of the exact one, the hat function 1-Lipschitz)
  bf16 dx                  the interval criterion of norm_bf16_cases with b = 9 u sum|dd w|; x in bf16 is exact, so d and dw keep their bars
Run as a script (RD_HEAD_FWD_TILED=0 RD_HEAD_DGRAD_TILED=0 in the environment: the knobs are read once per process) it runs UNTILED
on the device and writes the fractions as JSON to the path given."""
import functools
import hashlib
import json
import os
import sys

import numpy as np

import head_ref as R
import norm_bf16_cases as B
import norm_cases as NC

F, D = np.float32, np.float64
U, C = R.U, R.C
K_FWD_TILED, K_FWD_UNTILED, K_DGRAD = 38, 15, 9
BF16 = B.BF16
CAP, CAP_ELEMS = 0.05, 1000          # at most 5 % multi-valued intervals on every bf16 dx of at least 1000 elements

# (N, H, W): the tile is 8 x 32 -- (1, 8, 32) is exactly one, (2, 7, 31) / (2, 9, 33) one less / more in both directions, (3, 17, 70) 3 x 3
# tiles with ragged edges; N >= 2 wherever a kernel could leak across an image boundary
CONV = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (2, 5, 7), (1, 8, 32), (2, 7, 31), (2, 9, 33), (3, 17, 70), (2, 64, 64), (1, 65, 127)]
# the weight gradient's regime each case is there for (blocks = cdiv(pixels, 512), at most 4 per CU): asserted against the library
REGIME = {(1, 1, 1): "one", (2, 1, 5): "one", (2, 5, 1): "one", (2, 5, 7): "one", (1, 8, 32): "one", (2, 7, 31): "one", (2, 9, 33): "direct",
          (3, 17, 70): "direct", (2, 64, 64): "direct", (1, 65, 127): "two_stage"}
BLOCKS = {(2, 9, 33): 2, (3, 17, 70): 7, (2, 64, 64): 16, (1, 65, 127): 17}          # (1 where the regime is "one")
UNTILED = [(2, 5, 7), (2, 9, 33), (3, 17, 70)]
# operand -> (ld, c0): channel windows of wider NaN-filled buffers, different strides, offsets on the 4-element grid
LAYOUTS = {"window": dict(x=(48, 16), dx=(20, 4)), "tight": dict(x=(16, 0), dx=(16, 0))}
# (N, Hs, Ws, Ho, Wo, the backward's path): identity, output 1 x 1, source 1 x 1, downscale (source pixels without a gradient), exact
# integer coordinates (17, 33 -> 33, 65: scale 1/2), the generic loop through either axis, the workload's own size
BIL = [(2, 5, 7, 5, 7, "fast"), (2, 5, 7, 1, 1, "fast"), (2, 1, 1, 4, 6, "fast"), (2, 7, 9, 3, 4, "fast"), (2, 4, 4, 10, 10, "fast"),
       (2, 6, 11, 13, 45, "mix"), (2, 3, 40, 40, 70, "generic"), (2, 30, 50, 57, 100, "fast"), (2, 17, 33, 33, 65, "fast"),
       (1, 240, 400, 450, 800, "fast")]


def case_id(c):
    return "-".join(str(v) for v in c)


def cap_shape(cap):
    """A two-image shape with more than 512 cap pixels: the weight gradient's block count is capped (about (2, 450, 600) at 256 CUs)."""
    return (2, R.cdiv(512 * cap + 1, 2 * 600) + 1, 600)


# ------------------------------------------------------------------------------------------------ data and expected results
def conv_data(shape, bf16=False, seed=0):
    """x [N,H,W,C] with per-channel scales 2^-3 .. 2^3 (rounded to bf16 for bf16 storage: exact there), w [C,3,3] without any symmetry
    in (kh, kw), the gradient map dd [N,H,W]."""
    N, H, W = shape
    rng = np.random.default_rng([21, seed, N, H, W])
    x = (2.0 ** rng.uniform(-3, 3, C) * rng.standard_normal((N, H, W, C))).astype(F)
    w = (0.1 * rng.standard_normal((C, 3, 3)) + 0.02 * np.arange(9).reshape(3, 3)).astype(F)
    dd = rng.standard_normal((N, H, W)).astype(F)
    return dict(shape=shape, x=B.rb(x) if bf16 else x, w=w, dd=dd, bf16=bf16)


def conv_want(dat):
    d, d_abs = R.conv_fwd(dat["x"], dat["w"])
    dx, dx_abs = R.conv_dgrad(dat["dd"], dat["w"])
    dw, dw_abs = R.conv_wgrad(dat["x"], dat["dd"])
    return dict(d=d, d_abs=d_abs, dx=dx, dx_abs=dx_abs, dw=dw, dw_abs=dw_abs)


@functools.lru_cache(maxsize=None)
def conv_case(shape, bf16):
    """(data, float64 results) of a case: computed once, shared, never modified."""
    dat = conv_data(shape, bf16)
    return dat, conv_want(dat)


def tie_data():
    """bf16 dgrad with every fp32 operation exact, so the bar is 0 and the stored value must be bf16(want) itself: 128 images of 3 x 3 with
    one non-zero gradient pixel in the middle -- all 8-bit significands, both signs -- and weights with 2-bit significands: every dx is
    ONE product (the other eight addends are exact zeros), 9 or 10 significant bits, a bf16 tie whenever bit 9 is its last."""
    sig = np.arange(128, 256, dtype=D) * 2.0 ** (np.arange(128) % 5 - 9) * np.where(np.arange(128) % 3 == 0, -1.0, 1.0)
    dd = np.zeros((128, 3, 3), F)
    dd[:, 1, 1] = sig
    vals = np.array([1.5, -1.5, 1.25, 0.75, 3.0, 1.0, -0.75, 2.0, -1.25, 0.5, 6.0], F)
    w = vals[(np.arange(C)[:, None] * 5 + np.arange(9)[None] * 3) % len(vals)].reshape(C, 3, 3)
    dx, dx_abs = R.conv_dgrad(dd, w)
    assert np.array_equal(dx.astype(F).astype(D), dx) and np.array_equal(np.abs(dx), dx_abs), "every result is one exact product"
    return dict(shape=(128, 3, 3), dd=dd, w=w, bf16=True, exact=True), dict(dx=dx, dx_abs=dx_abs)


def n_ties(want):
    """Exact bf16 ties among the tie case's results: (all, those where ties-to-even and ties-away differ)."""
    z = want["dx"].astype(F)
    tie = (z.view(np.uint32) & 0xffff) == 0x8000
    return int(tie.sum()), int((tie & (B.rb(z) != B.rb(z, "half_up"))).sum())


def conv_fracs(got, want, dat, k_fwd, blocks):
    """got: d, dx, dw as float64 -- whichever are present -> ({fp32 output: fraction of its bar}, {bf16 output: held(...)})."""
    fr, h = {}, {}
    if "d" in got:
        fr["d"] = NC.frac(got["d"], want["d"], k_fwd * U * want["d_abs"])
    if "dw" in got:
        fr["dw"] = NC.frac(got["dw"], want["dw"], R.wgrad_chain(dat["dd"].size, blocks) * U * want["dw_abs"])
    if "dx" in got:
        b = (0 if dat.get("exact") else K_DGRAD) * U * want["dx_abs"]
        if dat["bf16"]:
            h["dx"] = B.held(got["dx"], want["dx"] - b, want["dx"] + b, want["dx"])
        else:
            fr["dx"] = NC.frac(got["dx"], want["dx"], b)
    return fr, h


def capped(h):
    return {k: v["wide"] for k, v in h.items() if v["n"] >= CAP_ELEMS and v["wide"] > CAP}


def bil_data(case, seed=0):
    N, Hs, Ws, Ho, Wo = case[:5]
    rng = np.random.default_rng([22, seed, N, Hs, Ws, Ho, Wo])
    return dict(d=rng.standard_normal((N, Hs, Ws)).astype(F), dout=rng.standard_normal((N, Ho, Wo)).astype(F))


@functools.lru_cache(maxsize=None)
def bil_case(case):
    dat = bil_data(case)
    out, out_bar = R.bilinear_fwd(dat["d"], case[3], case[4])
    dd, dd_bar = R.bilinear_bwd(dat["dout"], case[1], case[2])
    return dat, dict(out=out, out_bar=out_bar, dd=dd, dd_bar=dd_bar)


def bil_fracs(got, want):
    return {k: NC.frac(got[k], want[k], want[k + "_bar"]) for k in ("out", "dd") if k in got}


# ------------------------------------------------------------------------------------------------ the launchers' source
LAUNCHERS = ["head_conv_fwd_T", "head_conv_dgrad_T", "head_conv_wgrad_T", "rd_bilinear_fwd", "rd_bilinear_bwd"]


def bwd_checks_precede_halves(source):
    """head_conv_bwd_T launches nothing itself: all of its checks stand before the first of the two halves it calls."""
    at = source.index(" head_conv_bwd_T(")
    body = source[at:source.index("\n}\n", at)]
    checks = [i for i in range(len(body)) if body.startswith("RD_CHECK_ARG(", i)]
    return len(checks) >= 4 and max(checks) < body.index("head_conv_dgrad_T<T>(") < body.index("head_conv_wgrad_T<T>(")


# ------------------------------------------------------------------------------------------------ on the device
GUARD = 64             # elements of NaN behind every device buffer
NAN16 = 0x7fc0


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


def dev16(a):
    """float32 values exact in bf16 (or NaN) -> flat device tensor of their 16 bits, GUARD bf16 NaNs behind it."""
    import torch
    a = np.ascontiguousarray(a, F).reshape(-1)
    with np.errstate(all="ignore"):
        assert np.array_equal(B.rb(a), a, equal_nan=True), "the operand is not exact in bf16"
    return torch.from_numpy(np.concatenate([B.bits(a), np.full(GUARD, NAN16, np.uint16)]).view(np.int16)).cuda()


def nan16(n):
    return dev16(np.full(n, np.nan, F))


def np16(t):
    u = t.cpu().numpy().view(np.uint16)
    assert (u[u.size - GUARD:] == NAN16).all(), "guard"
    return (u[:u.size - GUARD].astype(np.uint32) << 16).view(F)


def ptr(t, elems=0):
    import ctypes
    return ctypes.c_void_p(None if t is None else t.data_ptr() + elems * t.element_size())


def window(a, rows, ld, c0):
    """The window [c0, c0 + C) of a buffer read back, after checking that nothing outside it was written and all inside is finite."""
    a = a.reshape(rows, ld)
    assert NC.writes_ok(a, ld, c0, C), "a write outside the window, or a non-finite value inside it"
    return a[:, c0:c0 + C]


def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_conv(shape, bf16, layout, k_fwd, case=None, legacy=True):
    """rd_head_conv_fwd_t / dgrad_t / wgrad_t / bwd_t (and, fp32, rd_head_conv_fwd / rd_head_conv_bwd) on the case's windows.
    -> dict(fr, h, blocks, d / dx digests).  Asserts on the way: return codes, guards, windows, NaN-prefilled dw overwritten, inputs
    untouched, bwd_t == dgrad_t + wgrad_t and the untyped forms == the typed ones bit for bit."""
    import torch
    from radar_depth_amd._lib import current_stream, lib
    L, st = lib(), current_stream()
    N, H, W = shape
    P = N * H * W
    dat, want = case or conv_case(shape, bf16)
    (ldx, cx), (ldd, cd) = LAYOUTS[layout]["x"], LAYOUTS[layout]["dx"]
    dt, dev, nan, back = (BF16, dev16, nan16, np16) if bf16 else (0, dev32, nan32, np32)

    def ok(rc, what):
        assert rc == 0, (what, rc, L.rd_last_error())

    x_wide = NC.wide(dat["x"].reshape(P, C), ldx, cx)
    X, Wt, DD = dev(x_wide), dev32(dat["w"]), dev32(dat["dd"])
    floats = int(L.rd_head_conv_bwd_workspace_floats(N, H, W, C))
    blocks = floats // (9 * C) - 16
    Dm, DX, DW, WS = nan32(P), nan(P * ldd), nan32(9 * C), nan32(floats)
    ok(L.rd_head_conv_fwd_t(dt, ptr(X, cx), ldx, ptr(Wt), N, H, W, C, ptr(Dm), st), "rd_head_conv_fwd_t")
    ok(L.rd_head_conv_dgrad_t(dt, ptr(Wt), ptr(DD), N, H, W, C, ptr(DX, cd), ldd, st), "rd_head_conv_dgrad_t")
    ok(L.rd_head_conv_wgrad_t(dt, ptr(X, cx), ldx, ptr(DD), N, H, W, C, ptr(DW), ptr(WS), st), "rd_head_conv_wgrad_t")
    DX2, DW2, WS2 = nan(P * ldd), nan32(9 * C), nan32(floats)
    ok(L.rd_head_conv_bwd_t(dt, ptr(X, cx), ldx, ptr(Wt), ptr(DD), N, H, W, C, ptr(DX2, cd), ldd, ptr(DW2), ptr(WS2), st), "rd_head_conv_bwd_t")
    torch.cuda.synchronize()
    d, dx_buf, dw = np32(Dm), back(DX), np32(DW)
    np32(WS), np32(WS2)          # the guards behind the workspaces
    assert np.isfinite(d).all() and np.isfinite(dw).all(), "d / dw: an element was not written (dw does not accumulate: NaN before the launch)"
    dx = window(dx_buf, P, ldd, cd)
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert same(back(DX2), dx_buf) and same(np32(DW2), dw), "rd_head_conv_bwd_t == dgrad_t + wgrad_t, bit for bit"
    assert same(back(X), x_wide.reshape(-1)) and same(np32(Wt), dat["w"].reshape(-1)) and same(np32(DD), dat["dd"].reshape(-1)), "an input was written"
    if not bf16 and legacy:
        D3, DX3, DW3, WS3 = nan32(P), nan32(P * ldd), nan32(9 * C), nan32(floats)
        ok(L.rd_head_conv_fwd(ptr(X, cx), ldx, ptr(Wt), N, H, W, C, ptr(D3), st), "rd_head_conv_fwd")
        ok(L.rd_head_conv_bwd(ptr(X, cx), ldx, ptr(Wt), ptr(DD), N, H, W, C, ptr(DX3, cd), ldd, ptr(DW3), ptr(WS3), st), "rd_head_conv_bwd")
        torch.cuda.synchronize()
        np32(WS3)
        assert same(np32(D3), d) and same(np32(DX3), dx_buf) and same(np32(DW3), dw), "the untyped forms == the _t forms, bit for bit"
    got = dict(d=d.astype(D).reshape(N, H, W), dx=dx.astype(D).reshape(N, H, W, C), dw=dw.astype(D).reshape(C, 3, 3))
    fr, h = conv_fracs(got, want, dat, k_fwd, blocks)
    return dict(fr=fr, h=h, blocks=blocks, d_bits=_digest(d), dx_bits=_digest(dx))


def run_untiled():
    """The untiled forward and dgrad kernels on UNTILED, both storage types, the windowed layout."""
    assert os.environ.get("RD_HEAD_FWD_TILED") == "0" and os.environ.get("RD_HEAD_DGRAD_TILED") == "0"
    recs = []
    for shape in UNTILED:
        for bf16 in (False, True):
            r = run_conv(shape, bf16, "window", K_FWD_UNTILED)
            recs.append(dict(shape=list(shape), bf16=bf16, **r))
    return recs


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[1], "w") as fh:
        json.dump(run_untiled(), fh)

"""The network head at kernel level (csrc/head.hip): rd_head_conv_fwd_t / _dgrad_t / _wgrad_t / _bwd_t in fp32 and bf16 storage -- the
forms the engine calls -- with rd_head_conv_fwd / rd_head_conv_bwd beside them, and rd_bilinear_fwd / rd_bilinear_bwd, against the
float64 reference of tests/head_ref.py on the cases and at the bars of tests/head_cases.py (derived there from the code, per element).
tests/test_head_host.py shows on the CPU that every named shortcut leaves these bars on these cases.

x and dx are channel windows of wider NaN-filled buffers ((ld, c0) = (48, 16) and (20, 4), and (16, 0)), every buffer has a NaN guard
behind it, dw and the workspace are NaN before the launch: after each launch everything outside a written window is still NaN, all
inside is finite, the inputs are untouched.  rd_head_conv_bwd_t must equal dgrad_t + wgrad_t and the untyped fp32 forms the typed
ones, bit for bit.  A stored bf16 dx lies in bf16(want - b) .. bf16(want + b), b = 9 u sum|dd w| (no ulp slack); the constructed tie
case has b = 0.  The weight gradient's block count is read from the library and every case is asserted to land in the regime it is
there for; the bilinear backward's path of every case is asserted from the restated window formula.  The untiled forward and dgrad
kernels (RD_HEAD_FWD_TILED=0, RD_HEAD_DGRAD_TILED=0: read once per process) run in one child process, tests/head_cases.py as a script.

Each test prints ("FRACTION ..." / "BF16 ..."; run with -s) the worst fraction of each bar and, for bf16, the elements outside their
interval, the share of multi-valued intervals (wide) and of elements that are not the nearest bf16 of the reference (off).

Largest values observed on an MI355X when the file was added (records, not thresholds): forward d 0.069 of 38 u tiled (the capped map;
0.049 below it) and 0.102 of 15 u untiled; fp32 dx 0.469 of 9 u (the capped map, 8.4 M elements; 0.323 below it), the same figure for
both dgrad forms, which agree bit for bit; dw 0.030 of its chain bar; bf16 dx: no element outside its interval, wide 0.0036, off 0.0009,
the tie case (3968 ties, 1997 of them rounded differently by ties-away) exact; bilinear forward 0.261, backward 0.228 (0.179 / 0.175 at
240 x 400 -> 450 x 800); 170 refused calls.  No kernel had to be changed."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_cases as HC
import head_ref as R
import norm_bf16_cases as B
import norm_cases as NC

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _cap():
    """The weight gradient's block cap (four per CU), from the workspace query of a map with far more than 512 pixels per block."""
    return int(_L().rd_head_conv_bwd_workspace_floats(64, 4096, 4096, R.C)) // (9 * R.C) - 16


def _report(what, r):
    fr, h = r["fr"], r["h"]
    print("FRACTION %-34s blocks %-5d worst %.3f  %s" % (what, r["blocks"], NC.worst(fr), " ".join("%s=%.3f" % kv for kv in sorted(fr.items()))))
    if h:
        print(B.line(what, h))
    assert NC.worst(fr) <= 1.0, (what, {k: v for k, v in fr.items() if v > 1.0})
    assert not B.outside(h), (what, "outside their interval", B.outside(h))
    assert not HC.capped(h), (what, "more than 5 % of the intervals hold two bf16 values", HC.capped(h))


@pytest.fixture(scope="module", autouse=True)
def untiled_worker(tmp_path_factory):
    """The child process of the untiled forms, started with the first test of the file and collected by the last."""
    out = tmp_path_factory.mktemp("head_untiled")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RD_")}
    env.update(RD_HEAD_FWD_TILED="0", RD_HEAD_DGRAD_TILED="0", OMP_NUM_THREADS="1")
    log = open(out / "untiled.log", "w")
    p = subprocess.Popen([sys.executable, os.path.join(HERE, "head_cases.py"), str(out / "untiled.json")], env=env, stdout=log, stderr=subprocess.STDOUT)
    yield p, out / "untiled.json", out / "untiled.log"
    if p.poll() is None:
        p.kill()
        p.wait()
    log.close()


# ------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", HC.CONV, ids=HC.case_id)
def test_conv_forms_storage_and_windows(shape, bf16):
    """Forward (38 u), dgrad (9 u; bf16: the interval), wgrad (chain u) on both layouts, the weight gradient in its stated regime."""
    for layout in HC.LAYOUTS:
        r = HC.run_conv(shape, bf16, layout, HC.K_FWD_TILED)
        assert R.wgrad_regime(r["blocks"], _cap()) == HC.REGIME[shape] and r["blocks"] == HC.BLOCKS.get(shape, 1), (shape, r["blocks"], _cap())
        _report("%s %s %s" % (HC.case_id(shape), "bf16" if bf16 else "fp32", layout), r)


def test_conv_over_the_block_cap():
    """More than 512 pixels per block: the weight gradient's grid is capped, its blocks start at arbitrary (row, column) positions and
    walk more than eight pixels per lane; fp32, the plain layout."""
    cap = _cap()
    shape = HC.cap_shape(cap)
    dat = HC.conv_data(shape)
    r = HC.run_conv(shape, False, "tight", HC.K_FWD_TILED, case=(dat, HC.conv_want(dat)))
    assert r["blocks"] == cap and R.wgrad_regime(r["blocks"], cap) == "cap" and R.cdiv(int(np.prod(shape)), cap) > 512, (shape, r["blocks"], cap)
    _report("%s fp32 tight (cap %d)" % (HC.case_id(shape), cap), r)


def test_bf16_dgrad_rounds_ties_to_even():
    """The constructed tie case: every fp32 operation exact, bar 0 -- the stored dx is bf16(want) itself, ties to even."""
    L = _L()
    dat, want = HC.tie_data()
    N, H, W = dat["shape"]
    P, (ld, c0) = N * H * W, HC.LAYOUTS["window"]["dx"]
    Wt, DD, DX = HC.dev32(dat["w"]), HC.dev32(dat["dd"]), HC.nan16(P * ld)
    rc = L.rd_head_conv_dgrad_t(HC.BF16, HC.ptr(Wt), HC.ptr(DD), N, H, W, R.C, HC.ptr(DX, c0), ld, _st())
    assert rc == 0, L.rd_last_error()
    torch.cuda.synchronize()
    got = HC.window(HC.np16(DX), P, ld, c0).astype(D).reshape(N, H, W, R.C)
    _, h = HC.conv_fracs(dict(dx=got), want, dat, 0, 1)
    n, differ = HC.n_ties(want)
    print(B.line("tie case: %d ties, %d where even != away" % (n, differ), h))
    assert h["dx"]["out"] == 0 and h["dx"]["wide"] == 0 and h["dx"]["off"] == 0 and differ > 400, h


def test_untiled_forms_in_a_child_process(untiled_worker):
    """head_conv_fwd_kernel (15 u) and head_conv_dgrad_kernel (9 u) on three small shapes, both storage types, windows as above."""
    p, res, log = untiled_worker
    rc = p.wait(timeout=300)
    assert rc == 0, open(log).read()[-4000:]
    recs = json.load(open(res))
    assert [(tuple(r["shape"]), r["bf16"]) for r in recs] == [(s, b) for s in HC.UNTILED for b in (False, True)]
    fwd_differs = 0
    for r in recs:
        shape = tuple(r["shape"])
        _report("untiled %s %s" % (HC.case_id(shape), "bf16" if r["bf16"] else "fp32"), r)
        tiled = HC.run_conv(shape, r["bf16"], "window", HC.K_FWD_TILED, legacy=False)
        fwd_differs += tiled["d_bits"] != r["d_bits"]
        print("    tiled == untiled bit for bit: d %s, dx %s" % (tiled["d_bits"] == r["d_bits"], tiled["dx_bits"] == r["dx_bits"]))
    assert fwd_differs, "the child ran the tiled forward: its summation order, hence some bits, must differ from the untiled kernel's"


# ------------------------------------------------------------------------------------------------ bilinear
@pytest.mark.parametrize("case", HC.BIL, ids=HC.case_id)
def test_bilinear_forward_and_backward(case):
    L = _L()
    N, Hs, Ws, Ho, Wo, path = case
    assert R.bilinear_bwd_paths(Hs, Ws, Ho, Wo) == path, "the backward's path, from the restated window formula"
    dat, want = HC.bil_case(case)
    Dm, DOUT, OUT, DDm = HC.dev32(dat["d"]), HC.dev32(dat["dout"]), HC.nan32(N * Ho * Wo), HC.nan32(N * Hs * Ws)
    assert L.rd_bilinear_fwd(HC.ptr(Dm), N, Hs, Ws, HC.ptr(OUT), Ho, Wo, _st()) == 0, L.rd_last_error()
    assert L.rd_bilinear_bwd(HC.ptr(DOUT), N, Ho, Wo, HC.ptr(DDm), Hs, Ws, _st()) == 0, L.rd_last_error()
    torch.cuda.synchronize()
    got = dict(out=HC.np32(OUT).astype(D).reshape(N, Ho, Wo), dd=HC.np32(DDm).astype(D).reshape(N, Hs, Ws))
    assert np.isfinite(got["out"]).all() and np.isfinite(got["dd"]).all(), "an element was not written"
    assert np.array_equal(HC.np32(Dm), dat["d"].reshape(-1)) and np.array_equal(HC.np32(DOUT), dat["dout"].reshape(-1)), "an input was written"
    fr = HC.bil_fracs(got, want)
    print("FRACTION bilinear %-22s %-8s out=%.3f dd=%.3f" % (HC.case_id(case[:5]), path, fr["out"], fr["dd"]))
    assert NC.worst(fr) <= 1.0, (case, fr)


# ------------------------------------------------------------------------------------------------ refusals
SENT = 0x7fc5a5a5          # a NaN with a payload: no kernel writes it


def test_refusals_name_the_entry_point_and_touch_nothing():
    """Every head entry point refuses (-1, before anything is launched -- the source is read first) C != 16, N / H / W < 1, a stride that
    is no multiple of 4 or narrower than C, a NULL pointer, x / dx off the four-element grid of their storage type (16 B fp32, 8 B bf16),
    a workspace off 16 B and, the _t forms, an unknown dtype; rd_last_error names the entry point; the sentinel-filled buffers stay
    untouched.  Every call is given buffers in which a launch would stay in bounds even if a check were missing."""
    L = _L()
    src = open(os.path.join(REPO, "radar_depth_amd", "csrc", "head.hip")).read()
    for fn in HC.LAUNCHERS:
        assert NC.checks_precede_launches(src, fn), fn
    assert HC.bwd_checks_precede_halves(src)
    bufs = [torch.from_numpy(np.full(4096, SENT, np.uint32).view(np.int32)).cuda() for _ in range(4)]
    at = lambda b, nbytes=0: C.c_void_p(bufs[b].data_ptr() + nbytes)
    I, O, O2, WS = at(0), at(1), at(2), at(3)
    st = _st()
    geom = [dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(W=-3), dict(C=8), dict(C=32), dict(C=0)]
    ldx = [dict(ldx=18), dict(ldx=12), dict(ldx=0), dict(ldx=-16), dict(x=None), dict(x=at(0, 4)), dict(x=at(0, 8))]
    lddx = [dict(lddx=18), dict(lddx=12), dict(lddx=0), dict(dx=None), dict(dx=at(1, 4)), dict(dx=at(1, 8))]
    ws = [dict(ws=None), dict(ws=at(3, 4)), dict(ws=at(3, 8)), dict(dw=None)]
    typed = [dict(dtype=7), dict(dtype=-1), dict(dtype=2)]
    bf_x = [dict(dtype=1, x=at(0, 2)), dict(dtype=1, x=at(0, 4)), dict(dtype=1, ldx=18), dict(dtype=1, ldx=8)]
    bf_dx = [dict(dtype=1, dx=at(1, 2)), dict(dtype=1, dx=at(1, 4)), dict(dtype=1, lddx=18), dict(dtype=1, lddx=8)]
    shape = [("N", 1), ("H", 4), ("W", 4), ("C", 16)]
    specs = {
        "rd_head_conv_fwd": ([("x", I), ("ldx", 16), ("w", I)] + shape + [("d", O), ("st", st)], geom + ldx + [dict(w=None), dict(d=None)]),
        "rd_head_conv_fwd_t": ([("dtype", 0), ("x", I), ("ldx", 16), ("w", I)] + shape + [("d", O), ("st", st)],
                               geom + ldx + typed + bf_x + [dict(w=None), dict(d=None)]),
        "rd_head_conv_dgrad_t": ([("dtype", 0), ("w", I), ("dd", I)] + shape + [("dx", O), ("lddx", 16), ("st", st)],
                                 geom + lddx + typed + bf_dx + [dict(w=None), dict(dd=None)]),
        "rd_head_conv_wgrad_t": ([("dtype", 0), ("x", I), ("ldx", 16), ("dd", I)] + shape + [("dw", O2), ("ws", WS), ("st", st)],
                                 geom + ldx + ws + typed + bf_x + [dict(dd=None)]),
        "rd_head_conv_bwd": ([("x", I), ("ldx", 16), ("w", I), ("dd", I)] + shape + [("dx", O), ("lddx", 16), ("dw", O2), ("ws", WS), ("st", st)],
                             geom + ldx + lddx + ws + [dict(w=None), dict(dd=None)]),
        "rd_head_conv_bwd_t": ([("dtype", 0), ("x", I), ("ldx", 16), ("w", I), ("dd", I)] + shape + [("dx", O), ("lddx", 16), ("dw", O2), ("ws", WS),
                                                                                                    ("st", st)],
                               geom + ldx + lddx + ws + typed + bf_x + bf_dx + [dict(w=None), dict(dd=None)]),
        "rd_bilinear_fwd": ([("d", I), ("N", 1), ("Hs", 4), ("Ws", 4), ("out", O), ("Ho", 8), ("Wo", 8), ("st", st)],
                            [dict(d=None), dict(out=None), dict(N=0), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=0)]),
        "rd_bilinear_bwd": ([("dout", I), ("N", 1), ("Ho", 8), ("Wo", 8), ("dd", O), ("Hs", 4), ("Ws", 4), ("st", st)],
                            [dict(dout=None), dict(dd=None), dict(N=0), dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=0)]),
    }
    n = 0
    for name, (spec, bad) in specs.items():
        for over in bad:
            assert all(k in dict(spec) for k in over), (name, over)
            rc = getattr(L, name)(*[over[k] if k in over else v for k, v in spec])
            shown = {k: getattr(v, "value", v) for k, v in over.items()}
            assert rc == -1, "%s(%r) returned %d: %s" % (name, shown, rc, L.rd_last_error())
            assert name.encode() in L.rd_last_error(), (name, shown, L.rd_last_error())
            n += 1
    torch.cuda.synchronize()
    for b in bufs:
        assert (b.cpu().numpy().view(np.uint32) == SENT).all(), "a refused call wrote"
    print("refused %d calls" % n)

"""The bf16-operand matrix-core kernels bit for bit: gconv_bf16_kernel<MT,NT,PIPE,IO16> (20 instantiations), gconv_bf16p_kernel<MT,NT>
(4), wgrad_bf16_kernel<FULL,NK,IO16> (12) + rd_wgrad_bf16_reduce and stem_fwd_bf16_kernel<NT> (2) on the integer-lattice classes of
tests/bf16_lattice_cases.py (P products, R rounding on store, D conversion on load, S statistics, T statistics source; the premises and the
fault table: tests/test_bf16_lattice_host.py).  On these inputs the stored result IS the exact result -- the integer, or RNE_bf16 of it in a
bf16 tensor -- so every comparison is an equality of bit patterns: there is no tolerance in this file.

Every launch runs under poisoned LDS into NaN-filled outputs, statistics rows and workspaces with a canary block behind them; a gradient
lies between two canary blocks; operands must keep their bits; nothing outside a channel window may be written.  The library's own plan
runs in this process; rd_gconv_bf16's five (MT, NT) tiles are forced through RD_GCONV_BF16_FORCE, which is read once per process: one
worker per index (tests/bf16_lattice_cases.py run as a script), all five started together and waited on with a limit, two of them with
RD_GCONV_BF16P_MT set as well; a worker that ended on a signal fails every configuration after it without anything being run again.
The last test asserts from the plan queries that every instantiation ran, with zero differing elements.  `pytest -s` prints one line per
(kernel, case, instantiation, tensor type) with its launches per class and what differs, and every differing launch in full
(profiles/r20_bf16_lattice.txt)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import bf16_lattice_cases as B
import stem_lattice_cases as SL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILES = [(2, 2), (2, 1), (3, 2), (1, 2), (1, 1)]          # cfgs[] of plan_gconv_bf16: the index RD_GCONV_BF16_FORCE takes
FORCED = {"force-%d" % i: {"RD_GCONV_BF16_FORCE": str(i)} for i in range(5)}
FORCED["force-0"]["RD_GCONV_BF16P_MT"] = "2"              # (the library's own plan puts these small maps on MT 1)
FORCED["force-1"]["RD_GCONV_BF16P_MT"] = "1"
ORDER = sorted(FORCED)
# Observed on an MI355X: the five workers, started together, had all ended 10.3 s later (the slowest spent 7.9 s of that in its 435
# launches, data and references included; the rest is the interpreter, torch and the library loading).  The wait is 20 times the slowest
# worker.
WAIT = 200


def _env():
    from radar_depth_amd._lib import check, current_stream, lib
    return lib(), check, current_stream()


def _ok(rec):
    assert rec["n_bad"] == 0 and not rec.get("n_bad_stat") and not rec.get("n_bad_acc"), rec


def _n_conv_jobs():
    return sum(len(B.conv_jobs(k)) for k in B.GCONV_KINDS) + len(B.BF16P_GRIDS) * sum(len(B.conv_jobs(k)) for k in B.BF16P_KINDS)


def _check_conv(records, tile=None, mt=None):
    """Every job of the tables ran once, on the expected tile, with nothing differing."""
    ran = [r for r in records if "seconds" not in r]
    assert len(ran) == _n_conv_jobs()
    want = {(k, tuple(j), 0) for k in B.GCONV_KINDS for j in B.conv_jobs(k)} | {(k, tuple(j), g) for g in B.BF16P_GRIDS for k in B.BF16P_KINDS for j in B.conv_jobs(k)}
    assert {(r["kind"], (r["cls"], r["e"], r["io16"], r["ep"]), r["grid"]) for r in ran} == want
    for r in ran:
        _ok(r)
        if r["kernel"] == "gconv_bf16":
            assert r["plan"][2] < 2000 and (tile is None or tuple(r["plan"][:2]) == tile), r
        else:
            assert r["plan"][2] >= 2000 and (mt is None or r["plan"][0] == mt), r
        if r["cls"] in "ST":
            assert r["n_bad_stat"] == 0, r
    # the tall maps: the launched plan's TH x TW fills every wave and M-block of the tile (full M-tiles under the vec / add epilogues and
    # the statistics jobs, non-zero partials from all four waves), with the pipelined loop as far as a plan allows
    B.check_fill({r["kind"]: r["plan"] for r in ran if r["kernel"] == "gconv_bf16"}, tile)
    for k in B.TALL_KINDS:
        assert {(r["cls"][0], r["io16"]) for r in ran if r["kind"] == k} == {("P", 0), ("P", 1), ("R", 1), ("D", 0), ("S", 0), ("S", 1), ("T", 1)}
        assert all(B.fills(r["plan"]) for r in ran if r["kind"] == k)
    return ran


# ------------------------------------------------------------------------------------------------ the convolutions
@pytest.fixture(scope="module")
def default_records():
    for k in ("RD_GCONV_BF16_FORCE", "RD_GCONV_BF16_CKP", "RD_GCONV_BF16_NOPIPE", "RD_GCONV_BF16_NOVEC4", "RD_GCONV_BF16P", "RD_GCONV_BF16P_MT"):
        assert k not in os.environ, "%s is set: this process would not run the library's own plan" % k
    return B.run_conv_all()


@pytest.fixture(scope="module")
def workers(tmp_path_factory):
    """name -> (return code or None when it ran out of time, records file, log file, seconds); every worker has ended when this returns."""
    out = tmp_path_factory.mktemp("bf16_lattice")
    procs = {}
    t0 = time.monotonic()
    for name in ORDER:
        env = {k: v for k, v in os.environ.items() if not k.startswith("RD_")}
        env.update(FORCED[name], OMP_NUM_THREADS="3")          # (five workers on 16 CPUs)
        log = open(out / (name + ".log"), "w")
        procs[name] = (subprocess.Popen([sys.executable, os.path.join(HERE, "bf16_lattice_cases.py"), str(out / (name + ".json"))], env=env,
                                        stdout=log, stderr=subprocess.STDOUT), log)
    assert len(procs) == 5
    done = {}
    try:
        for name in ORDER:
            p = procs[name][0]
            try:
                rc = p.wait(timeout=max(1.0, t0 + WAIT - time.monotonic()))
            except subprocess.TimeoutExpired:
                rc = None
            done[name] = (rc, out / (name + ".json"), out / (name + ".log"), time.monotonic() - t0)
    finally:
        for p, log in procs.values():          # leftovers: out of time, or the wait itself was interrupted
            if p.poll() is None:
                p.kill()
                p.wait()
            log.close()
    yield done


def _records(name, workers):
    """The records of a forced configuration, after asserting that it and every configuration before it ended well."""
    for prev in ORDER[:ORDER.index(name)]:
        rc = workers[prev][0]
        assert rc is None or rc >= 0, "worker %s ended on signal %d: nothing after it counts" % (prev, -rc)
    rc, res, log, secs = workers[name]
    assert rc is not None, "worker %s did not finish within %d s" % (name, WAIT)
    assert rc == 0, open(log).read()[-4000:]
    recs = json.load(open(res))
    print("BF16-LATTICE %s: worker had ended %.1f s after the five were started (its launches, data and references: %.1f s; wait: %d s)" % (
        name, secs, recs[-1]["seconds"], WAIT))
    return recs


def test_conv_lattice_default_plan(default_records):
    """Every kind, class, tensor type and epilogue under the tiles the planners pick; bf16 tensors on these small maps stay on
    gconv_bf16_kernel unless rd_gconv_bf16p_plan_all(1) is set, then on the persistent kernel under the grid caps 0 / 1 / 3."""
    B.summarize(default_records, "default")
    ran = _check_conv(default_records)
    assert {r["ckp"] for r in ran if r["kernel"] == "gconv_bf16"} == {64, 32, 16}
    assert {(r["inst"][2], r["inst"][3]) for r in ran if r["kernel"] == "gconv_bf16"} == {(0, 0), (0, 1), (1, 0), (1, 1)}      # (PIPE, IO16)
    assert {r["inst"][1] for r in ran if r["kernel"] == "gconv_bf16p"} == {1, 2}
    d, _ = B.conv_desc("p_3x3")
    assert B.conv_plan(d, 1)[2] < 2000, "rd_gconv_bf16p_plan_all is restored"


@pytest.mark.parametrize("name", ORDER)
def test_conv_lattice_forced_tile(name, workers):
    """One (MT, NT) of gconv_bf16_kernel forced (and, in two workers, the persistent kernel's MT)."""
    recs = _records(name, workers)
    B.summarize(recs, name)
    mt = FORCED[name].get("RD_GCONV_BF16P_MT")
    _check_conv(recs, tile=TILES[int(name.split("-")[1])], mt=int(mt) if mt else None)


def test_conv_bad_arguments_are_refused_before_the_launch():
    """bf16 tensors with an input channel stride that is no multiple of 8: gconv_bf16_impl's first checks, nothing is launched."""
    L, _, st = _env()
    d, _ = B.conv_desc("3x3")
    d.ldi = d.Cin + 4
    buf = torch.zeros(d.N * d.Hi * d.Wi * d.ldi + d.N * d.Ho * d.Wo * d.ldo, dtype=torch.bfloat16, device="cuda")
    assert L.rd_gconv_bf16_t(B.BF16, C.byref(d), B._vp(buf), B._vp(buf), B._vp(buf), None, 0, 0, None, 0, None, st) != 0
    assert b"multiple of 8" in L.rd_last_error(), L.rd_last_error()
    assert L.rd_gconv_bf16_t(7, C.byref(d), B._vp(buf), B._vp(buf), B._vp(buf), None, 0, 0, None, 0, None, st) != 0
    torch.cuda.synchronize()
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ the weight gradient
@pytest.mark.parametrize("case", B.WGRAD_CASES, ids=lambda c: c.id)
def test_wgrad_bf16_lattice(case):
    """P (also at 2^-40) on fp32 and bf16 tensors, D on fp32 tensors; the UpProj cases reduce their two column ranges and once more with
    accumulate = 1."""
    recs = [B.run_wgrad_case(case.id, cls, e, io16) for cls, e, io16 in B.wgrad_jobs(case)]
    B.summarize(recs)
    for rec in recs:
        _ok(rec)
        assert case.kind != "upproj" or rec["cls"] != "P" or rec["n_bad_acc"] == 0


@pytest.mark.parametrize("case_id", B.WGRAD_WINDOW_CASES)
def test_wgrad_bf16_lattice_on_channel_windows(case_id):
    """ldi = Cin + 8, ldo = Cout + 8, first channel 8, every other channel NaN; a base off the 16-byte grid and, with bf16 tensors, a
    channel stride that is no multiple of 8 are refused before anything is launched (wgrad_bf16_impl's first checks)."""
    case = B.WGRAD_BY_ID[case_id]
    recs = [B.run_wgrad_case(case_id, cls, e, io16, True) for cls, e, io16 in B.wgrad_jobs(case)]
    B.summarize(recs)
    for rec in recs:
        _ok(rec)
    L, _, st = _env()
    d = B.wgrad_desc(case, True)
    buf = torch.zeros(max(d.N * d.Hi * d.Wi * d.ldi, d.N * d.Ho * d.Wo * d.ldo) + 8, device="cuda")
    ws = torch.full((int(L.rd_wgrad_bf16_workspace_floats(C.byref(d))),), float("nan"), device="cuda")
    for xo, yo in ((4, 0), (0, 8), (12, 12)):          # bytes
        assert L.rd_wgrad_bf16(C.byref(d), C.c_void_p(buf.data_ptr() + xo), C.c_void_p(buf.data_ptr() + yo), B._vp(ws), st) != 0, (xo, yo)
        assert b"unaligned" in L.rd_last_error(), L.rd_last_error()
        assert L.rd_wgrad_bf16_t(B.BF16, C.byref(d), C.c_void_p(buf.data_ptr() + xo), C.c_void_p(buf.data_ptr() + yo), B._vp(ws), st) != 0
    d.ldi = case.cin + 4
    assert L.rd_wgrad_bf16_t(B.BF16, C.byref(d), B._vp(buf), B._vp(buf), B._vp(ws), st) != 0
    assert b"multiples of 8" in L.rd_last_error(), L.rd_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all()), "a refused call launched nothing"


# ------------------------------------------------------------------------------------------------ the stem
@pytest.mark.parametrize("cfg", B.STEM_CONFIGS, ids=SL.fwd_id)
def test_stem_bf16_lattice(cfg):
    recs = [B.run_stem(cfg, shape, cls, io16) for shape in B.STEM_SHAPES for cls, io16 in B.stem_jobs(cfg)]
    B.summarize(recs)
    for rec in recs:
        _ok(rec)
        assert rec["cls"] not in "ST" or rec["n_bad_stat"] == 0


def _walk_shape():
    L, check, _ = _env()
    n_cu = C.c_int(0)
    name = C.create_string_buffer(128)
    check(L.rd_device_info(C.byref(n_cu), name, 128), "rd_device_info")
    return n_cu.value, B.stem_walk_shape(n_cu.value)


def test_stem_bf16_tile_walk():
    """More 8 x 32 output tiles than the persistent grid of 2 workgroups per CU (Cout 64): the grid-stride tile walk and its prefetch of the
    next tile's patch, class S, both output types."""
    n_cu, shape = _walk_shape()
    assert int(np.prod(SL.stat_tiles(shape))) > 2 * n_cu
    recs = [B.run_stem((1, 64), shape, "S", io16) for io16 in (0, 1)]
    B.summarize(recs, "walk")
    for rec in recs:
        _ok(rec)
        assert rec["n_bad_stat"] == 0 and rec["tiles"] > 2 * n_cu


# ------------------------------------------------------------------------------------------------ every form
def test_every_instantiation_ran_bit_for_bit(default_records, workers):
    """20 gconv_bf16_kernel<MT,NT,PIPE,IO16> + 4 gconv_bf16p_kernel<MT,NT> + 12 wgrad_bf16_kernel<FULL,NK,IO16> + 2 stem_fwd_bf16_kernel<NT>,
    each with zero differing elements, as the plan queries report them."""
    conv, pers = set(), {}
    for recs in [default_records] + [_records(name, workers) for name in ORDER]:
        for r in recs:
            if "seconds" in r:
                continue
            _ok(r)
            if r["kernel"] == "gconv_bf16":
                conv.add(tuple(r["inst"]))
            else:
                pers.setdefault(tuple(r["inst"]), set()).add(r["grid"])
    assert conv == {(mt, nt, pipe, io) for (mt, nt) in TILES for pipe in (0, 1) for io in (0, 1)} and len(conv) == 20, sorted(conv)
    assert pers == {(mt, nt): set(B.BF16P_GRIDS) for mt in (1, 2) for nt in (1, 2)}, pers
    wg = set()
    for case in B.WGRAD_CASES:
        for cls, e, io16 in B.wgrad_jobs(case):
            rec = B.run_wgrad_case(case.id, cls, e, io16)
            _ok(rec)
            wg.add(tuple(rec["inst"]))
    assert wg == {(f, nk, io) for f in (0, 1) for nk in (1, 2, 4) for io in (0, 1)} and len(wg) == 12, sorted(wg)
    assert any(B.run_wgrad_case(c.id, "P", 0, 0)["plan"][3] > 1 for c in B.WGRAD_CASES), "several pixel splits"
    stem = set()
    for cfg in B.STEM_CONFIGS:
        for shape in B.STEM_SHAPES:
            for cls, io16 in B.stem_jobs(cfg):
                rec = B.run_stem(cfg, shape, cls, io16)
                _ok(rec)
                stem.add((rec["inst"][0], io16))
    assert stem == {(nt, io) for nt in (1, 2) for io in (0, 1)}, stem
    _, shape = _walk_shape()
    assert all(B.run_stem((1, 64), shape, "S", io)["n_bad"] == 0 for io in (0, 1)), "the stem's tile walk"

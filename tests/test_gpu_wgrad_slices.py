"""Every weight-gradient family on CHANNEL SLICES of wider NHWC buffers (ldi > Cin, ldo > Cout, the other channels NaN) against
desc_emulator.run_wgrad in float64 and, bit for bit, against the same launch on dense operands (tests/wgrad_slice_cases.py holds the
cases).  Each sub-kernel has its own copy of the address arithmetic -- the generic tile, column-strip and immediate-offset forms of
csrc/wgrad.hip, wgrad16.hip, wgrad1x1.hip, wgrad_split.hip (buffer resources sized Hi*Wi*ldi*4) and wgrad_bf16.hip -- so a Cin written
where ldi belongs, or a missing channel guard on a partial 64-channel block, fails HERE with the kernel and the stride in the test id.

Per case: the plan queries do not depend on the strides; the strided gradient is finite and torch.equal to the dense twin's; both are
within the family's own bar of float64 (5e-5 of the gradient's largest magnitude for rd_wgrad / rd_wgrad_split / _pre as in
test_gpu_wgrad.py / test_gpu_wgrad_split.py, 2e-5 on the bf16-rounded operands for rd_wgrad_bf16[_t] as in test_wgrad_bf16); the slab
workspace is exactly *_workspace_floats(d) floats, NaN-filled, with a canary tail that keeps its bits; the gradient is a view between two
canary blocks; the operand buffers, NaN channels included, keep their bits.  `pytest -s` prints every case's error
(profiles/r14_wgrad_slices.txt)."""
import ctypes as C

import pytest
import torch

import wgrad_slice_cases as wc

pytestmark = pytest.mark.gpu

BAR = {"wgrad": 5e-5, "wgrad_split": 5e-5, "wgrad_split_pre": 5e-5, "wgrad_bf16": 2e-5}
CANARY = 4096           # floats behind the slab workspace and on both sides of the gradient
CANARY_VALUE = -1234.5
ENTRY = {   # family -> (workspace query, supported query, reduce, (plan query, ints))
    "wgrad": ("rd_wgrad_workspace_floats", None, "rd_wgrad_reduce", ("rd_wgrad_plan_info", 9)),
    "wgrad_split": ("rd_wgrad_split_workspace_floats", "rd_wgrad_split_supported", "rd_wgrad_split_reduce", ("rd_wgrad_split_plan_info", 4)),
    "wgrad_split_pre": ("rd_wgrad_split_workspace_floats", "rd_wgrad_split_pre_supported", "rd_wgrad_split_reduce", ("rd_wgrad_split_plan_info", 4)),
    "wgrad_bf16": ("rd_wgrad_bf16_workspace_floats", "rd_wgrad_bf16_supported", "rd_wgrad_bf16_reduce", ("rd_wgrad_bf16_plan_info", 7)),
}


def _lib():
    from radar_depth_amd._lib import lib
    return lib()


def _vp(addr):
    return C.c_void_p(addr)


def _rel(a, b):
    return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def queries(fam, d):
    """(supported, workspace floats, plan) of a descriptor: what must not depend on ldi / ldo."""
    from radar_depth_amd._lib import check
    L = _lib()
    ws_q, sup_q, _, (info_q, n_info) = ENTRY[fam]
    sup = getattr(L, sup_q)(C.byref(d)) if sup_q else 1
    assert sup == 1, (fam, L.rd_last_error())
    nws = int(getattr(L, ws_q)(C.byref(d)))
    if nws < 0:
        check(nws, ws_q)
    info = (C.c_int32 * n_info)()
    check(getattr(L, info_q)(C.byref(d), info), info_q)
    return sup, nws, tuple(info)


def launch(fam, d, xb, cx, yb, cy, ws):
    """The family's weight-gradient launch on the slices xb[..., cx:cx+Cin], yb[..., cy:cy+Cout] (fp32 or bf16 buffers)."""
    from radar_depth_amd import ops
    from radar_depth_amd._lib import check, current_stream
    L = _lib()
    es = xb.element_size()
    xp, yp = _vp(xb.data_ptr() + es * cx), _vp(yb.data_ptr() + es * cy)
    if fam == "wgrad":
        check(L.rd_wgrad(C.byref(d), xp, yp, _vp(ws.data_ptr()), current_stream()), "rd_wgrad")
    elif fam == "wgrad_split":
        check(L.rd_wgrad_split(C.byref(d), xp, yp, _vp(ws.data_ptr()), current_stream()), "rd_wgrad_split")
    elif fam == "wgrad_split_pre":
        xpc = ops.split_pieces(xb[..., cx:cx + d.Cin])
        ypc = ops.split_pieces(yb[..., cy:cy + d.Cout])
        check(L.rd_wgrad_split_pre(C.byref(d), _vp(xpc.data_ptr()), C.c_int64(xpc[0].numel()), _vp(ypc.data_ptr()), C.c_int64(ypc[0].numel()),
                                   _vp(ws.data_ptr()), current_stream()), "rd_wgrad_split_pre")
        torch.cuda.synchronize()          # (the piece planes are temporaries)
    elif xb.dtype == torch.bfloat16:
        check(L.rd_wgrad_bf16_t(1, C.byref(d), xp, yp, _vp(ws.data_ptr()), current_stream()), "rd_wgrad_bf16_t")
    else:
        check(L.rd_wgrad_bf16(C.byref(d), xp, yp, _vp(ws.data_ptr()), current_stream()), "rd_wgrad_bf16")


def reduce(fam, d, ws, grad, co_off=0, accumulate=0):
    from radar_depth_amd._lib import check, current_stream
    o, i, kh, kw = grad.shape
    assert grad.is_contiguous()
    check(getattr(_lib(), ENTRY[fam][2])(C.byref(d), _vp(ws.data_ptr()), _vp(grad.data_ptr()), o, i, kh, kw, co_off, accumulate, current_stream()),
          ENTRY[fam][2])


def operands(case, dense, dtype=torch.float32):
    """(descriptor, x buffer, cx, dy buffer, cy) on the GPU: the slices inside NaN-filled wide buffers, or the dense twin."""
    d = wc.desc(case, dense)
    xv, yv = wc.values(case)
    cx, cy = (0, 0) if dense else (case.cx, case.cy)
    return d, wc.widen(xv, cx, d.ldi, dtype).cuda(), cx, wc.widen(yv, cy, d.ldo, dtype).cuda(), cy


def run(fam, case, dense, dtype=torch.float32):
    """One launch + reduction with every guard of the module docstring around it -> (gradient on the CPU, plan queries)."""
    d, xb, cx, yb, cy = operands(case, dense, dtype)
    x0, y0 = xb.clone(), yb.clone()
    q = queries(fam, d)
    ws = torch.full((q[1] + CANARY,), float("nan"), device="cuda")
    kh, kw = wc.kernel_shape(case)
    nel = case.cout * case.cin * kh * kw
    gbuf = torch.full((2 * CANARY + nel,), CANARY_VALUE, device="cuda")
    grad = gbuf[CANARY:CANARY + nel].view(case.cout, case.cin, kh, kw)
    grad.fill_(float("nan"))
    launch(fam, d, xb, cx, yb, cy, ws)
    if case.kind == "upproj":       # the two branch weights: column ranges of one slab set, in increasing co_off order
        half = case.cout // 2
        reduce(fam, d, ws, grad[:half], 0)
        reduce(fam, d, ws, grad[half:], half)
    else:
        reduce(fam, d, ws, grad)
    torch.cuda.synchronize()
    nan_bits = _bits(torch.full((1,), float("nan")))[0].item()
    assert bool((_bits(ws[q[1]:]) == nan_bits).all()), "%s %s: wrote behind the slab workspace" % (fam, case.id)
    assert bool((gbuf[:CANARY] == CANARY_VALUE).all()) and bool((gbuf[CANARY + nel:] == CANARY_VALUE).all()), \
        "%s %s: wrote outside the gradient tensor" % (fam, case.id)
    assert torch.equal(_bits(xb), _bits(x0)) and torch.equal(_bits(yb), _bits(y0)), "%s %s: an operand buffer changed" % (fam, case.id)
    return grad.cpu().clone(), q


def check_case(fam, case, dtype=torch.float32):
    gs, qs = run(fam, case, False, dtype)
    gd, qd = run(fam, case, True, dtype)
    ref = wc.reference(case, fam == "wgrad_bf16")
    es, ed = _rel(gs, ref), _rel(gd, ref)
    print("%-16s %-5s %-44s strided %.3e dense %.3e (bar %.0e)  plan %s" % (fam, "bf16" if dtype == torch.bfloat16 else "fp32", case.id, es, ed,
                                                                           BAR[fam], qs[2]))
    assert qs == qd, "%s %s: supported / workspace / plan depend on the strides: %s vs dense %s" % (fam, case.id, qs, qd)
    assert bool(torch.isfinite(gs).all()), "%s %s: non-finite gradient from a slice with NaN neighbours" % (fam, case.id)
    assert torch.equal(gs, gd), "%s %s: strided and dense gradients differ by %.3e" % (fam, case.id, (gs - gd).abs().max().item())
    assert es < BAR[fam] and ed < BAR[fam], (fam, case.id, es, ed)
    return qs


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------ one test per family and case
@pytest.mark.parametrize("case", wc.SPLIT_CONV + wc.SPLIT_UPPROJ, ids=_ids(wc.SPLIT_CONV + wc.SPLIT_UPPROJ))
def test_wgrad_split_slices(case):
    check_case("wgrad_split", case)


@pytest.mark.parametrize("case", wc.SPLIT_PRE, ids=_ids(wc.SPLIT_PRE))
def test_wgrad_split_pre_slices(case):
    """Piece planes made by ops.split_pieces from the same slices; bit-identical to rd_wgrad_split on the slices."""
    check_case("wgrad_split_pre", case)
    pre, _ = run("wgrad_split_pre", case, False)
    fly, _ = run("wgrad_split", case, False)
    assert torch.equal(pre, fly)


@pytest.mark.parametrize("case", wc.WGRAD, ids=_ids(wc.WGRAD))
def test_wgrad_slices(case):
    check_case("wgrad", case)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32_tensors", "bf16_tensors"])
@pytest.mark.parametrize("case", wc.BF16, ids=_ids(wc.BF16))
def test_wgrad_bf16_slices(case, dtype):
    """rd_wgrad_bf16 rounds fp32 tensors while it stages them, rd_wgrad_bf16_t(RD_DTYPE_BF16) reads tensors that hold the same roundings:
    one float64 reference (on the rounded operands) serves both."""
    assert case.cx % 8 == 0 and case.cy % 8 == 0 and case.ldi % 8 == 0 and case.ldo % 8 == 0
    check_case("wgrad_bf16", case, dtype)


# ------------------------------------------------------------------------------------------------ the cases reach the paths they name
def test_split_cases_reach_both_tile_geometries_and_a_short_last_split():
    geoms, many, short = set(), [], []
    for case in wc.SPLIT_CONV + wc.SPLIT_UPPROJ:
        n_splits, tps, _, tiles = queries("wgrad_split", wc.desc(case))[2]
        tall, total = (tiles >> 30) & 1, tiles & ((1 << 30) - 1)
        print("%-44s splits %3d tiles/split %3d tiles %4d %s" % (case.id, n_splits, tps, total, "4x16" if tall else "2x32"))
        geoms.add(tall)
        if n_splits > 1:
            many.append(case.id)
            if total - (n_splits - 1) * tps < tps:
                short.append(case.id)
    assert geoms == {0, 1} and many and short, (geoms, many, short)


def test_wgrad_cases_reach_every_sub_kernel():
    """out[0..8] of rd_wgrad_plan_info = taps per group (0: wgrad16.hip), MFMA size, layout A (-1: wgrad1x1.hip), shared B, LDS pitch,
    taps per row, per-phase launches, splits, column-strip kernel."""
    seen = set()
    for case in wc.WGRAD:
        tg, mf, la, shb, pitch, rw, per_phase, splits, strip = queries("wgrad", wc.desc(case))[2]
        kind = ("strip" if strip else "wgrad16" if tg == 0 else "wgrad1x1" if la == -1 else "pitch" if pitch > 0 else "generic")
        print("%-44s %-8s layoutA %2d per-phase %d splits %3d" % (case.id, kind, la, per_phase, splits))
        seen.add(kind)
        seen.add("layoutA" if la == 1 else "layoutB" if la == 0 else "1x1")
        if per_phase:
            seen.add("per_phase")
        if splits > 1:
            seen.add("splits>1")
    assert seen >= {"strip", "pitch", "generic", "wgrad16", "wgrad1x1", "layoutA", "layoutB", "per_phase", "splits>1"}, seen


# ------------------------------------------------------------------------------------------------ the slab reductions
RED_CASE = {"wgrad": wc.SPLIT_CONV[0], "wgrad_split": wc.SPLIT_CONV[0],
            # (rd_wgrad_bf16 needs channel counts that are multiples of 16: 96 columns as [0, 40) + [40, 96) instead of 88)
            "wgrad_bf16": wc.make_case("conv", 2, (64, 8, 80), (96, 16, 128), 9, 35)}


@pytest.mark.parametrize("fam", ["wgrad", "wgrad_split", "wgrad_bf16"])
def test_reduce_column_ranges_and_accumulate(fam):
    """Two column ranges reduced separately, in increasing co_off order, concatenate to the full reduction bit for bit; accumulate = 1 onto
    an unrelated g0 gives float32(g0 + r) exactly, r being the non-accumulated result: launch_slab_reduce (csrc/wgrad.hip) sums the slabs
    into a register first and adds the old value LAST (`*dst + s`), one rounding, so there is nothing to bound."""
    case = RED_CASE[fam]
    assert case.kind == "conv" and case.k == 3 and case.cout > 40
    d, xb, cx, yb, cy = operands(case, False)
    ws = torch.full((queries(fam, d)[1],), float("nan"), device="cuda")
    launch(fam, d, xb, cx, yb, cy, ws)
    full = torch.full((case.cout, case.cin, 3, 3), float("nan"), device="cuda")
    reduce(fam, d, ws, full)
    parts = torch.full_like(full, float("nan"))
    reduce(fam, d, ws, parts[:40], 0)
    reduce(fam, d, ws, parts[40:], 40)
    g0 = torch.randn(full.shape, generator=torch.Generator().manual_seed(21)).cuda()
    acc = g0.clone()
    reduce(fam, d, ws, acc, 0, accumulate=1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(full).all()) and _rel(full.cpu(), wc.reference(case, fam == "wgrad_bf16")) < BAR[fam]
    assert torch.equal(parts, full)
    assert torch.equal(acc, g0 + full)


def test_reduce_batched_on_strided_upproj_and_bf16_jobs():
    """rd_wgrad_reduce_batched: one batch with jobs from strided descriptors, an UpProj pair (two column ranges of one slab set) and a
    bf16_kernel = 1 job, bit-identical to the per-tensor entry points."""
    from radar_depth_amd import ops
    jobs, want, keep = [], [], []
    upproj = [c for c in wc.WGRAD if c.kind == "upproj"][0]
    for fam, case in (("wgrad", wc.WGRAD[0]), ("wgrad", wc.WGRAD[2]), ("wgrad", upproj), ("wgrad_bf16", wc.BF16[0])):
        d, xb, cx, yb, cy = operands(case, False)
        ws = torch.full((queries(fam, d)[1],), float("nan"), device="cuda")
        launch(fam, d, xb, cx, yb, cy, ws)
        kh, kw = wc.kernel_shape(case)
        ranges = [(0, case.cout // 2), (case.cout // 2, case.cout // 2)] if case.kind == "upproj" else [(0, case.cout)]
        for off, o in ranges:
            ref = torch.full((o, case.cin, kh, kw), float("nan"), device="cuda")
            reduce(fam, d, ws, ref, off)
            want.append(ref)
            jobs.append((d, ws, torch.full_like(ref, float("nan")), off, int(fam == "wgrad_bf16")))
        keep.append((xb, yb))
    nb1, nb2 = ops.wgrad_reduce_batched(jobs)
    torch.cuda.synchronize()
    assert nb2 > 0
    for job, ref in zip(jobs, want):
        assert bool(torch.isfinite(ref).all()) and torch.equal(job[2], ref)

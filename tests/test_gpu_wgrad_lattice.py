"""The split weight-gradient and stem kernels bit for bit: rd_wgrad_split / rd_wgrad_split_pre (csrc/wgrad_split.hip: 3x3 / 2x3 / 3x2 /
2x2 tap rectangles x wide or tall pixel tiles x staged or pre-split = 16 instantiations), rd_stem_wgrad_split_t (csrc/stem_wgrad_split.hip:
8 plain instantiations) and rd_stem_fwd_split (csrc/stem_split.hip, its own term list) on the integer-lattice classes A-C, the
one-product-per-element class D and, for the stem forward's BatchNorm partial sums, class S (tests/wgrad_lattice_cases.py,
tests/stem_lattice_cases.py; the premises and the kept-term proof: tests/test_wgrad_lattice_host.py).  On these inputs the stored result
IS the float64 result: every comparison is equality, there is no tolerance in this file.

Every launch runs under poisoned LDS into NaN-filled gradients / outputs and a NaN-filled workspace with a canary behind the
floats the workspace query asks for; the gradient lies between two canary blocks; nothing NaN may be left and no canary may change.
Every launch goes through one cached function, and the coverage tests at the end call it for everything the tables list: that each
instantiation ran, with zero differing elements, is asserted there.  `pytest -s` prints one line per launch
(profiles/r19_split_lattice_forms.txt)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import stem_lattice_cases as SL
import wgrad_lattice_cases as WL
from test_gpu_wgrad_slices import CANARY, CANARY_VALUE, _bits, _vp, reduce
from wgrad_slice_cases import widen

pytestmark = pytest.mark.gpu

D = np.float64


def _env():
    from radar_depth_amd._lib import check, current_stream, lib
    return lib(), check, current_stream()


def _first(got, want, bad):
    return [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:6]]


def _canary_ok(t, n):
    """The tail behind the first n floats keeps the canary's bits."""
    return bool((_bits(t[n:]) == _bits(torch.full((1,), CANARY_VALUE))[0].item()).all())


def _workspace(n):
    ws = torch.full((n + CANARY,), float("nan"), device="cuda")
    ws[n:] = CANARY_VALUE
    return ws


def _gradient(shape):
    nel = int(np.prod(shape))
    gbuf = torch.full((2 * CANARY + nel,), CANARY_VALUE, device="cuda")
    grad = gbuf[CANARY:CANARY + nel].view(*shape)
    grad.fill_(float("nan"))
    return gbuf, grad, nel


# ------------------------------------------------------------------------------------------------ rd_wgrad_split[_pre]
def instantiations(case):
    """The (tap rows, tap columns, tall, ) rectangles x geometry the case's launches instantiate, from the plan the device reports."""
    L, check, _ = _env()
    d = WL.desc(case)
    info = (C.c_int32 * 4)()
    check(L.rd_wgrad_split_plan_info(C.byref(d), info), "rd_wgrad_split_plan_info")
    tall = (info[3] >> 30) & 1
    return {(d.phase[i].dh_max - d.phase[i].dh_min + 1, d.phase[i].dw_max - d.phase[i].dw_min + 1, tall) for i in range(d.n_phases)}, list(info)


@functools.lru_cache(maxsize=None)
def run_wgrad(case_id, cls, e, pre, window=False):
    """One launch + reduction -> record."""
    from radar_depth_amd import ops
    L, check, st = _env()
    case = WL.BY_ID[case_id]
    d = WL.desc(case, window)
    x, dy, want = WL.data(case_id, cls, e)
    off = WL.WINDOW_OFF if window else 0
    xb, yb = widen(torch.from_numpy(x), off, d.ldi).cuda(), widen(torch.from_numpy(dy), off, d.ldo).cuda()
    x0, y0 = xb.clone(), yb.clone()
    assert L.rd_wgrad_split_supported(C.byref(d)) == 1 and (not pre or L.rd_wgrad_split_pre_supported(C.byref(d)) == 1)
    nws = int(L.rd_wgrad_split_workspace_floats(C.byref(d)))
    assert nws > 0
    ws = _workspace(nws)
    kh, kw = WL.kernel_shape(case)
    gbuf, grad, nel = _gradient((case.cout, case.cin, kh, kw))
    xp, yp = _vp(xb.data_ptr() + 4 * off), _vp(yb.data_ptr() + 4 * off)
    assert xp.value % 16 == 0 and yp.value % 16 == 0
    if pre:
        xpc, ypc = ops.split_pieces(xb[..., off:off + d.Cin]), ops.split_pieces(yb[..., off:off + d.Cout])
    check(L.rd_debug_poison_lds(st), "rd_debug_poison_lds")
    if pre:
        check(L.rd_wgrad_split_pre(C.byref(d), _vp(xpc.data_ptr()), C.c_int64(xpc[0].numel()), _vp(ypc.data_ptr()), C.c_int64(ypc[0].numel()),
                                   _vp(ws.data_ptr()), st), "rd_wgrad_split_pre")
    else:
        check(L.rd_wgrad_split(C.byref(d), xp, yp, _vp(ws.data_ptr()), st), "rd_wgrad_split")
    fam = "wgrad_split_pre" if pre else "wgrad_split"
    ranges = [(0, case.cout // 2), (case.cout // 2, case.cout // 2)] if case.kind == "upproj" else [(0, case.cout)]
    for lo, n in ranges:          # (UpProj: the two branch tensors are column ranges of one slab set)
        reduce(fam, d, ws, grad[lo:lo + n], lo)
    acc = None
    if case.kind == "upproj" and cls != "D":
        # once more with accumulate = 1 onto an integer-lattice gradient: G0 + dW is still exact
        q = 2.0 ** e
        assert np.abs(want).max() / q + 2 ** 10 < 2 ** 24
        g0 = torch.randint(-2 ** 10, 2 ** 10 + 1, grad.shape, generator=torch.Generator().manual_seed(5)).double() * q
        acc = g0.float().cuda()
        for lo, n in ranges:
            reduce(fam, d, ws, acc[lo:lo + n], lo, accumulate=1)
    torch.cuda.synchronize()
    assert _canary_ok(ws, nws), "%s %s: wrote behind the %d workspace floats" % (fam, case_id, nws)
    assert bool((gbuf[:CANARY] == CANARY_VALUE).all()) and bool((gbuf[CANARY + nel:] == CANARY_VALUE).all()), "wrote outside the gradient"
    assert torch.equal(_bits(xb), _bits(x0)) and torch.equal(_bits(yb), _bits(y0)), "an operand buffer changed"
    got = grad.cpu().numpy().astype(D)
    assert not np.isnan(got).any(), "%s %s: the NaN-filled gradient is not fully overwritten" % (fam, case_id)
    bad = np.argwhere(got != want)
    n_acc = 0
    if acc is not None:
        n_acc = int((acc.cpu().numpy().astype(D) != g0.numpy() + want).sum())
    inst, plan = instantiations(case)
    assert ((plan[3] >> 30) & 1, plan[3] & ((1 << 30) - 1)) == (case.tall, case.tiles), (case_id, plan)
    rec = dict(kernel=fam, case=case_id, cls=cls, e=e, window=window, plan=plan, inst=sorted(inst), n_bad=len(bad), n_bad_acc=n_acc,
               first=_first(got, want, bad))
    print("LATTICE %-16s %-28s class %s 2^%-3d %s plan %s differing elements: %d (accumulated: %s) %s" % (
        fam, case_id, cls, e, "window" if window else "dense ", plan, len(bad), n_acc if acc is not None else "-", rec["first"]))
    return rec


def _wgrad_jobs():
    for case in WL.CASES:
        for pre in (False, True) if case.pre else (False,):
            for cls, e in WL.VARIANTS:
                yield (case.id, cls, e, pre, False)
    for cid in WL.WINDOW_CASES:
        for cls, e in WL.VARIANTS:
            yield (cid, cls, e, False, True)


def _ok(rec):
    assert rec["n_bad"] == 0 and rec.get("n_bad_acc", 0) == 0, rec


@pytest.mark.parametrize("pre", [False, True], ids=["staged", "pre"])
@pytest.mark.parametrize("case", WL.CASES, ids=lambda c: c.id)
def test_wgrad_split_lattice(case, pre):
    """Every class of a case on one entry point; the pre-split entry point takes channel counts that are multiples of 16 only (the
    72 -> 96 case is refused there, which is asserted instead)."""
    if pre and not case.pre:
        L, _, _ = _env()
        assert L.rd_wgrad_split_pre_supported(C.byref(WL.desc(case))) == 0
        return
    for cls, e in WL.VARIANTS:
        _ok(run_wgrad(case.id, cls, e, pre))


@pytest.mark.parametrize("case_id", WL.WINDOW_CASES)
def test_wgrad_split_lattice_on_channel_windows(case_id):
    """ldi = Cin + 8, ldo = Cout + 8, first channel 4, every other channel NaN; a base off the 16-byte grid is refused."""
    for cls, e in WL.VARIANTS:
        _ok(run_wgrad(case_id, cls, e, False, True))
    L, _, st = _env()
    d = WL.desc(WL.BY_ID[case_id], True)
    buf = torch.zeros(max(d.N * d.Hi * d.Wi * d.ldi, d.N * d.Ho * d.Wo * d.ldo) + 8, device="cuda")
    ws = torch.zeros(int(L.rd_wgrad_split_workspace_floats(C.byref(d))), device="cuda")
    for xo, yo in ((4, 0), (0, 8), (12, 12)):          # bytes: a window that starts at channel 1, 2 or 3
        assert L.rd_wgrad_split(C.byref(d), _vp(buf.data_ptr() + xo), _vp(buf.data_ptr() + yo), _vp(ws.data_ptr()), st) == -1, (xo, yo)
        assert b"unaligned" in L.rd_last_error(), L.rd_last_error()


def test_wgrad_split_every_instantiation_ran_bit_for_bit():
    """All 16 instantiations of wgrad_split_kernel -- (3,3) (2,3) (3,2) (2,2) x wide / tall x staged / pre -- and every case, class and
    entry point of the tables, zero differing elements each."""
    seen, keys = set(), set()
    for job in _wgrad_jobs():
        rec = run_wgrad(*job)
        _ok(rec)
        keys.add(job)
        seen |= {(tr, tc, tall, job[3]) for (tr, tc, tall) in rec["inst"]}
    assert seen == {(tr, tc, tall, pre) for tr in (2, 3) for tc in (2, 3) for tall in (0, 1) for pre in (False, True)}, sorted(seen)
    assert len(keys) == (2 * len(WL.CASES) - 1 + len(WL.WINDOW_CASES)) * len(WL.VARIANTS)
    assert any(run_wgrad(*j)["plan"][0] > 16 for j in keys), "the two-stage slab reduction"


# ------------------------------------------------------------------------------------------------ the stems
def _planes(xw, cin):
    """Planes 1.. of a wider NCHW tensor with strided images (as tests/test_gpu_stem.py)."""
    n, ctot, h, w = xw.shape
    planes = (C.c_void_p * 4)(*[xw.data_ptr() + 4 * h * w * (1 + c) if c < cin else None for c in range(4)])
    strides = (C.c_int64 * 4)(*[ctot * h * w if c < cin else 0 for c in range(4)])
    return planes, strides


def _wide_nchw(x):
    n, c, h, w = x.shape
    xw = torch.full((n, c + 1, h, w), float("nan"))
    xw[:, 1:] = torch.from_numpy(x)
    return xw.cuda()


@functools.lru_cache(maxsize=None)
def run_stem_wgrad(cfg, shape, cls, e):
    L, check, st = _env()
    n, h, w = shape
    x, dout, want = SL.wgrad_data(cfg, shape, cls, e)
    xw = _wide_nchw(x)
    dg = torch.from_numpy(dout).to(torch.bfloat16 if cfg.bf16 else torch.float32).cuda()
    assert np.array_equal(dg.float().cpu().numpy(), dout), "the bf16 tensor holds the same numbers"
    x0, d0 = xw.clone(), dg.clone()
    planes, strides = _planes(xw, cfg.cin)
    assert L.rd_stem_wgrad_split_supported(cfg.cin, cfg.cout) == 1
    nws = int(L.rd_stem_wgrad_workspace_floats(n, h, w, cfg.cin, cfg.cout))
    ws = _workspace(nws)
    gbuf, grad, nel = _gradient((cfg.cout, cfg.cin, 7, 7))
    check(L.rd_debug_poison_lds(st), "rd_debug_poison_lds")
    check(L.rd_stem_wgrad_split_t(cfg.bf16, planes, strides, cfg.cin, n, h, w, _vp(dg.data_ptr()), cfg.cout, _vp(grad.data_ptr()), _vp(ws.data_ptr()), st),
          "rd_stem_wgrad_split_t")
    torch.cuda.synchronize()
    assert _canary_ok(ws, nws), "wrote behind the workspace"
    assert bool((gbuf[:CANARY] == CANARY_VALUE).all()) and bool((gbuf[CANARY + nel:] == CANARY_VALUE).all()), "wrote outside the gradient"
    assert torch.equal(_bits(xw), _bits(x0)) and torch.equal(_bits(dg), _bits(d0)), "an operand changed"
    got = grad.cpu().numpy().astype(D)
    assert not np.isnan(got).any(), "the NaN-filled gradient is not fully overwritten"
    bad = np.argwhere(got != want)
    rec = dict(kernel="stem_wgrad_split", cfg=cfg, shape=shape, cls=cls, e=e, n_bad=len(bad), first=_first(got, want, bad),
               inst=(-(-49 * cfg.cin // 32), 2 if cfg.cout > 32 else 1, cfg.bf16))
    print("LATTICE stem_wgrad_split %-10s %-10s class %s 2^%-3d instantiation %s differing elements: %d %s" % (
        SL.wgrad_id(cfg), "x".join(map(str, shape)), cls, e, rec["inst"], len(bad), rec["first"]))
    return rec


@functools.lru_cache(maxsize=None)
def run_stem_fwd(cfg, shape, cls):
    L, check, st = _env()
    cin, cout = cfg
    n, h, w = shape
    x, wt, want = SL.fwd_data(cfg, shape, cls)
    xw, wg = _wide_nchw(x), torch.from_numpy(wt).cuda()
    x0, w0 = xw.clone(), wg.clone()
    planes, strides = _planes(xw, cin)
    ho, wo = SL.out_size(h), SL.out_size(w)
    tiles = int(L.rd_stem_stat_tiles(n, h, w))
    assert tiles == int(np.prod(SL.stat_tiles(shape)))
    nel = n * ho * wo * cout
    obuf = torch.full((nel + CANARY,), float("nan"), device="cuda")
    obuf[nel:] = CANARY_VALUE
    sbuf = torch.full((tiles * 2 * cout + CANARY,), float("nan"), device="cuda")
    sbuf[tiles * 2 * cout:] = CANARY_VALUE
    check(L.rd_debug_poison_lds(st), "rd_debug_poison_lds")
    check(L.rd_stem_fwd_split(planes, strides, cin, n, h, w, _vp(wg.data_ptr()), cout, _vp(obuf.data_ptr()), _vp(sbuf.data_ptr()), st), "rd_stem_fwd_split")
    torch.cuda.synchronize()
    assert _canary_ok(obuf, nel) and _canary_ok(sbuf, tiles * 2 * cout), "wrote behind the output or the partial sums"
    assert torch.equal(_bits(xw), _bits(x0)) and torch.equal(_bits(wg), _bits(w0)), "an operand changed"
    got = obuf[:nel].view(n, ho, wo, cout).cpu().numpy().astype(D)
    stat = sbuf[:tiles * 2 * cout].view(tiles, 2, cout).cpu().numpy().astype(D)
    assert not np.isnan(got).any() and np.isfinite(stat).all(), "the output and every partial-sum row are written"
    bad = np.argwhere(got != want)
    n_stat = None
    if cls == "S":
        # integers, |y| <= 8: every partial sum is exact, so the rows add up to the integer sums of the stored output
        sums = np.stack([got.sum((0, 1, 2)), (got * got).sum((0, 1, 2))])
        n_stat = int((stat.sum(0) != sums).sum())
    rec = dict(kernel="stem_fwd_split", cfg=cfg, shape=shape, cls=cls, n_bad=len(bad), n_bad_stat=n_stat, first=_first(got, want, bad))
    print("LATTICE stem_fwd_split   %-10s %-10s class %s tiles %d differing elements: %d, statistics: %s %s" % (
        SL.fwd_id(cfg), "x".join(map(str, shape)), cls, tiles, len(bad), "-" if n_stat is None else n_stat, rec["first"]))
    return rec


def _ok_stem(rec):
    assert rec["n_bad"] == 0 and not rec.get("n_bad_stat"), rec


@pytest.mark.parametrize("cfg", SL.WGRAD_CONFIGS, ids=SL.wgrad_id)
def test_stem_wgrad_split_lattice(cfg):
    for shape in SL.wgrad_shapes(cfg):
        for cls, e in SL.wgrad_variants(cfg):
            _ok_stem(run_stem_wgrad(cfg, shape, cls, e))


@pytest.mark.parametrize("cfg", SL.FWD_CONFIGS, ids=SL.fwd_id)
def test_stem_fwd_split_lattice(cfg):
    for shape in SL.FWD_SHAPES:
        for cls in SL.FWD_CLASSES:
            _ok_stem(run_stem_fwd(cfg, shape, cls))


def test_stems_every_instantiation_ran_bit_for_bit():
    """The eight plain instantiations of stem_wgrad_split_kernel (K tiles, N tiles, bf16 dout) and the ten (Cin, Cout) forms of the stem
    forward, every shape and class of the tables, zero differing elements; the statistics of class S exact on every form and shape."""
    seen = set()
    for cfg in SL.WGRAD_CONFIGS:
        for shape in SL.wgrad_shapes(cfg):
            for cls, e in SL.wgrad_variants(cfg):
                rec = run_stem_wgrad(cfg, shape, cls, e)
                _ok_stem(rec)
                seen.add(rec["inst"])
    assert seen == {(5, 2, 0), (5, 2, 1), (2, 1, 0), (2, 1, 1), (4, 1, 0), (4, 1, 1), (7, 2, 0), (2, 2, 0)}, sorted(seen)
    assert run_stem_wgrad(SL.WGRAD_CONFIGS[0], SL.WGRAD_BIG, "A", 0)["n_bad"] == 0
    done = set()
    for cfg in SL.FWD_CONFIGS:
        for shape in SL.FWD_SHAPES:
            for cls in SL.FWD_CLASSES:
                rec = run_stem_fwd(cfg, shape, cls)
                _ok_stem(rec)
                assert cls != "S" or rec["n_bad_stat"] == 0
                done.add((cfg, cls))
    assert done == {(c, k) for c in SL.FWD_CONFIGS for k in SL.FWD_CLASSES} and len(SL.FWD_CONFIGS) == 10

"""No GPU: everything tests/test_gpu_bf16_lattice.py rests on (tests/bf16_lattice_cases.py).  Per case and class, in int64: operands
that are bf16 numbers where they must be, sums of absolute products below 2^24 along every reduction, exact statistics on the largest tile
any plan can use, ties of both directions in every class-R expectation, class D's planted patterns in the gathered output.  The
references are desc_emulator.run_desc / run_wgrad, held here to torch's float64 convolutions and autograd; the RNE_bf16 helper is held to
torch.Tensor.bfloat16().  In place of device mutation runs, each operation is restated with one named fault and must then leave the
expectation of the class that carries the fault, on every case the fault applies to.  The plan facts the cases were chosen for are
asserted through the plan queries (they answer without a device, for 256 CUs)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import bf16_lattice_cases as B
import stem_lattice_cases as SL

D = np.float64


def _L():
    from radar_depth_amd._lib import lib
    return lib()


# ------------------------------------------------------------------------------------------------ the rounding helper
def test_rne_bf16_is_torch_bfloat16():
    rng = np.random.default_rng(1)
    hi = np.arange(0x0080, 0x7f80, dtype=np.uint32)                       # every positive normal upper half
    lows = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], np.uint32)
    u = np.concatenate([((hi[:, None] << 16) | lows[None]).reshape(-1), rng.integers(0x00800000, 0x7f800000, 1 << 16).astype(np.uint32),
                        np.array(B.PLANTED, np.uint32)])
    u = np.concatenate([u, u | np.uint32(0x80000000)])
    a = u.view(np.float32)
    got = B.bf16_bits(a)
    want = torch.from_numpy(a.copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)
    finite = np.isfinite(B.bf16_value(want))                              # (the largest upper half rounds up to infinity: both say so)
    assert np.array_equal(got, want) and finite.sum() > finite.size - 8
    assert (B.bf16_bits(a, "trunc") != got).any() and (B.bf16_bits(a, "half_away") != got).any()
    assert [hex(v) for v in B.bf16_bits(np.array(B.PLANTED, np.uint32).view(np.float32))] == ["0x4040", "0x4042", "0x4040", "0x4041", "0x3f80"]
    assert B.ties(np.array(B.PLANTED, np.uint32).view(np.float32)) == (1, 2)


# ------------------------------------------------------------------------------------------------ references against torch
def _oihw(b, k):
    """[k*k][I][O] -> [O][I][k][k]."""
    return torch.from_numpy(np.ascontiguousarray(b.reshape(k, k, b.shape[1], b.shape[2]).transpose(3, 2, 0, 1))).double()


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, D).transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


CONV_FWD = {"3x3_tall": (3, 1), "1x1_320_tall": (1, 1), "1x1_320_wide": (1, 1), "3x3": (3, 1), "3x3_partial": (3, 1), "1x1": (1, 1), "3x3_320": (3, 1), "1x1_320": (1, 1), "3x3_48": (3, 1), "3x3_16": (3, 1),
            "p_3x3": (3, 1), "p_ragged": (3, 1), "p_wide": (3, 1)}


@pytest.mark.parametrize("kind", B.ALL_KINDS)
def test_conv_reference_is_torch_float64(kind):
    """run_desc on class P against F.conv2d / autograd in float64, and the numpy restatement the faults are built from against run_desc."""
    d, S = B.conv_desc(kind)
    dd = B.conv_data(kind, "P")
    a, b, y = dd["a"].astype(D), dd["b"].astype(D), dd["y"]
    assert np.array_equal(B.emulate_conv(d, a, b), y, equal_nan=True)
    x = _nchw(a)
    if kind in CONV_FWD:
        k, s = CONV_FWD[kind]
        ref = _nhwc(TF.conv2d(x, _oihw(b, k), None, s, k // 2))
    elif kind in ("upproj_fwd", "p_upproj", "upproj_tall"):
        up = torch.zeros(d.N, d.Cin, 2 * d.Hi, 2 * d.Wi, dtype=torch.float64)
        up[:, :, ::2, ::2] = x
        ref = _nhwc(TF.conv2d(up, _oihw(b, 5), None, 1, 2))
    elif kind == "upproj_dgrad":       # b is [25][forward Cout][forward Cin]: the transposed operand
        w = _oihw(b, 5).permute(1, 0, 2, 3)
        ref = _nhwc(TF.conv_transpose2d(x, w, padding=2)[:, :, ::2, ::2])
    else:
        k, s = {"dgrad_s2": (3, 2), "dgrad_1x1_s2": (1, 2), "p_dgrad": (3, 1)}[kind]
        w = _oihw(b, k).permute(1, 0, 2, 3).contiguous()
        ref = _nhwc(torch.nn.grad.conv2d_input((d.N, d.Cout, d.Ho, d.Wo), w, x, s, k // 2))
    written = ~np.isnan(y)
    assert np.array_equal(y[written], ref[written]) and not ref[~written].any()
    assert written.all() == (kind != "dgrad_1x1_s2")
    # the epilogue, once: relu on the first columns of conv + bias + addend
    if kind == "3x3":
        e = B.conv_data(kind, "P", 0, "scalar")
        z = ref + e["bias"].astype(D) + e["addend"].astype(D)
        z[..., :e["act_cols"]] = np.maximum(z[..., :e["act_cols"]], 0)
        assert e["act_cols"] == 30 and np.array_equal(z, e["want"]) and (e["want"][..., :30] == 0).any() and (e["want"][..., 30:] < 0).any()


@pytest.mark.parametrize("case", B.WGRAD_CASES, ids=lambda c: c.id)
def test_wgrad_reference_is_torch_float64(case):
    d = B.wgrad_desc(case)
    kh, kw = B.kernel_shape(case)
    x, dy, want = B.wgrad_data(case.id, "P")
    assert np.array_equal(B.oihw(case, B.emulate_wgrad(d, x, dy, kh * kw)), want)
    xt, gt = _nchw(x), _nchw(dy)
    if case.kind == "upproj":
        up = torch.zeros(case.n, case.cin, 2 * case.h, 2 * case.w, dtype=torch.float64)
        up[:, :, ::2, ::2] = xt
        ref = torch.nn.grad.conv2d_weight(up, (case.cout, case.cin, 5, 5), gt, 1, 2)
    else:
        k, s = {"conv3": (3, 1), "conv3s2": (3, 2), "conv1": (1, 1)}[case.kind]
        ref = torch.nn.grad.conv2d_weight(xt, (case.cout, case.cin, k, k), gt, s, k // 2)
    assert np.array_equal(ref.numpy(), want)


@pytest.mark.parametrize("cfg", B.STEM_CONFIGS, ids=SL.fwd_id)
def test_stem_reference_is_torch_float64(cfg):
    for shape in B.STEM_SHAPES:
        x, w, want = B.stem_data(cfg, shape, "P")
        wt = torch.from_numpy(np.ascontiguousarray(w.reshape(7, 7, cfg[0], cfg[1]).transpose(3, 2, 0, 1))).double()
        assert np.array_equal(_nhwc(TF.conv2d(torch.from_numpy(x).double(), wt, None, 2, 3)), want)


# ------------------------------------------------------------------------------------------------ premises
@pytest.mark.parametrize("kind", B.ALL_KINDS)
def test_conv_premises(kind, capsys):
    seen = set()
    for cls, e, io16, ep in B.conv_jobs(kind):
        if (cls, e, ep) in seen:
            continue
        seen.add((cls, e, ep))
        fig = B.conv_premise(kind, cls, e, ep)
        with capsys.disabled():
            print("\n%-14s class %s 2^%-3d %-6s %s" % (kind, cls, e, ep, fig), end="")
    assert {c[0] for c, _, _ in seen} == ({"P", "S"} if kind == "1x1_320_wide" else {"P", "R", "S", "T"} if kind in B.BF16P_KINDS else set(B.CONV_CLASSES))


@pytest.mark.parametrize("case", B.WGRAD_CASES, ids=lambda c: c.id)
def test_wgrad_premises(case, capsys):
    for cls, e in {(c, e) for c, e, _ in B.wgrad_jobs(case)}:
        fig = B.wgrad_premise(case, cls, e)
        with capsys.disabled():
            print("\n%-28s class %s 2^%-3d %s" % (case.id, cls, e, fig), end="")


@pytest.mark.parametrize("cfg", B.STEM_CONFIGS, ids=SL.fwd_id)
def test_stem_premises(cfg):
    for shape in B.STEM_SHAPES:
        for cls in sorted({c for c, _ in B.stem_jobs(cfg)}):
            B.stem_premise(cfg, shape, cls)
    x, w, want = B.stem_data((1, 64), B.stem_walk_shape(4), "S")          # the tile-walk case's generator, at a toy CU count
    assert want.shape == (3, 16, 64, 64) and np.abs(want).max() <= 8


# ------------------------------------------------------------------------------------------------ the named faults
def _differs(pair):
    want, got = pair
    return not np.array_equal(want, got, equal_nan=True)


def test_every_conv_fault_moves_the_class_that_carries_it():
    """On every kind a fault applies to.  The stores and the statistics source concern bf16 tensors, the load conversion fp32 ones."""
    applies = {m: 0 for m in B.CONV_SHORTCUTS}
    kinds = [k for k in B.ALL_KINDS if k != "1x1_320_wide"]          # (the wide map runs P and S only: it is there for one plan)
    for kind in kinds:
        for mode in B.CONV_SHORTCUTS:
            if mode == "truncating_load" and kind in B.BF16P_KINDS:
                continue                       # (bf16 tensors only: nothing is converted on load)
            pair = B.conv_shortcut(kind, mode)
            if pair is None:
                continue
            assert _differs(pair), (kind, mode)
            applies[mode] += 1
    assert all(applies.values()), applies
    assert applies["dropped_tap"] == applies["dropped_k_step"] == len(kinds) and applies["upproj_phases_swapped"] == 3


def test_every_wgrad_fault_moves_the_class_that_carries_it():
    applies = {m: 0 for m in B.WGRAD_SHORTCUTS}
    for case in B.WGRAD_CASES:
        for mode in B.WGRAD_SHORTCUTS:
            pair = B.wgrad_shortcut(case, mode)
            if pair is None:
                continue
            assert _differs(pair), (case.id, mode)
            applies[mode] += 1
    assert all(applies.values()), applies
    assert applies["dropped_split"] == applies["dropped_k_step"] == len(B.WGRAD_CASES) and applies["upproj_phases_swapped"] == 2


@pytest.mark.parametrize("cfg", B.STEM_CONFIGS, ids=SL.fwd_id)
def test_every_stem_fault_moves_the_class_that_carries_it(cfg):
    for shape in B.STEM_SHAPES:
        r = B.stem_data(cfg, shape, "R")[2]
        assert (B.bf16_bits(r) != B.bf16_bits(r, "trunc")).any() and (B.bf16_bits(r) != B.bf16_bits(r, "half_away")).any()
        x, w, want = B.stem_data(cfg, shape, "D")
        assert not np.array_equal(SL.fwd_ref(B.rne(x, "trunc"), w), want)
        t = B.stem_data(cfg, shape, "T")[2]
        assert (B.stem_stat_rows(shape, t)[:, 0] != B.stem_stat_rows(shape, B.rne(t))[:, 0]).any()
        x, w, want = B.stem_data(cfg, shape, "P")
        w2 = w.copy()
        w2[48] = 0                                                         # one dropped tap
        assert not np.array_equal(SL.fwd_ref(x, w2), want)


# ------------------------------------------------------------------------------------------------ plan facts
def test_conv_plan_facts():
    """What the kinds are there for, under the library's own plan: PIPE through the 320-channel kinds, CKP 64 / 32 / 16, small maps with
    bf16 tensors off the persistent kernel, every statistics tile within MAX_STAT_TILE."""
    L = _L()
    plans = {}
    for kind in B.GCONV_KINDS:
        d, _ = B.conv_desc(kind)
        plans[kind] = B.conv_plan(d, 1)
        assert plans[kind] == B.conv_plan(d, 0) and plans[kind][2] < 2000, (kind, plans[kind])
        assert plans[kind][3] * plans[kind][4] <= B.MAX_STAT_TILE
    assert plans["3x3_320"][2] // 1000 == 1 and plans["1x1_320"][2] // 1000 == 1 and plans["3x3"][2] // 1000 == 0
    assert {p[2] % 1000 for p in plans.values()} == {64, 32, 16}
    assert plans["3x3"][2] == 64 and plans["3x3_partial"][2] == 32 and plans["3x3_48"][2] == 16 and plans["3x3_16"][2] == 16
    prev = L.rd_gconv_bf16p_plan_all(1)
    try:
        for kind in B.BF16P_KINDS:
            d, _ = B.conv_desc(kind)
            p = B.conv_plan(d, 1)
            assert p[2] >= 2000 and p[1] == (2 if d.Cout % 64 == 0 else 1) and p[3] * p[4] <= 256, (kind, p)
            if kind == "p_wide":
                assert -(-d.Wo // p[4]) > 1, "several tile columns"
        assert {B.conv_plan(B.conv_desc(k)[0], 1)[1] for k in B.BF16P_KINDS} == {1, 2}
    finally:
        L.rd_gconv_bf16p_plan_all(1 if prev == 1 else 0)
    d, _ = B.conv_desc("p_3x3")
    assert B.conv_plan(d, 1)[2] < 2000, "restored: the small map is back on gconv_bf16_kernel"


def test_tall_maps_fill_every_wave_under_every_forced_tile(tmp_path):
    """RD_GCONV_BF16_FORCE is read once per process: five plan-query processes (no device), started together."""
    import json
    import os
    import subprocess
    import sys
    tiles = [(2, 2), (2, 1), (3, 2), (1, 2), (1, 1)]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bf16_lattice_cases.py")
    procs = []
    for i in range(5):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RD_")}
        env.update(RD_GCONV_BF16_FORCE=str(i), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, script, "--plans", str(tmp_path / ("%d.json" % i))], env=env))
    for i, p in enumerate(procs):
        assert p.wait(timeout=120) == 0
        plans = json.load(open(tmp_path / ("%d.json" % i)))
        B.check_fill(plans, tiles[i])
        assert all(tuple(v[:2]) == tiles[i] for v in plans.values())
    B.check_fill(B.forced_plans())          # the library's own plan
    # what the small maps give, which is why the tall ones are there: one M-block of wave 0
    assert not B.fills(B.conv_plan(B.conv_desc("3x3")[0], 0))


def test_wgrad_plan_facts():
    L = _L()
    inst = {}
    for case in B.WGRAD_CASES:
        d = B.wgrad_desc(case)
        assert L.rd_wgrad_bf16_supported(C.byref(d)) == 1
        kh, kw = B.kernel_shape(case)
        plan = B.wgrad_plan(d)
        inst.setdefault(B.wgrad_inst(d, kh * kw, plan, 0)[:2], []).append(case.id)
        dw = B.wgrad_desc(case, window=True)
        assert (dw.ldi, dw.ldo) == (case.cin + 8, case.cout + 8) and B.wgrad_plan(dw) == plan
    assert set(inst) == {(f, nk) for f in (0, 1) for nk in (1, 2, 4)}, inst
    assert B.wgrad_plan(B.wgrad_desc(B.WGRAD_BY_ID["conv3_4x23x40_64to64"]))[3] > 1, "several pixel splits"
    assert B.wgrad_plan(B.wgrad_desc(B.WGRAD_BY_ID["conv3_2x7x10_80to96"]))[2] == 4, "partial 64-channel blocks on both sides"
    from radar_depth_amd import convdesc as cd
    kind, n, h, w, ci, co = B.WGRAD_REFUSED
    assert L.rd_wgrad_bf16_supported(C.byref(cd.conv_fwd(n, h, w, ci, co, 3, 1, 1))) == 0, "72 channels: not a multiple of 16"

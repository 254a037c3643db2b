"""No GPU: the premises behind tests/test_gpu_wgrad_lattice.py and the stem lattices (tests/wgrad_lattice_cases.py,
tests/stem_lattice_cases.py).  Per case and class, in int64: every sum of absolute values below 2^24 quanta, the piece counts the
class claims, at least half of the result non-zero.  A numpy emulation of the six kept piece products (exact float64 sums) gives the
float64 result on every class, and loses it exactly on the classes that claim a term when that term is dropped.  Class D's expected
tensor is a gather; the stem references are torch's float64 convolution and weight gradient.  A short list of indexing shortcuts each moves a lattice case off the expected gradient.  The plan facts the
weight-gradient cases were chosen for are asserted through rd_wgrad_split_plan_info."""
import ctypes as C

import numpy as np
import pytest

import stem_lattice_cases as SL
import wgrad_lattice_cases as WL
from wino_ref import KEPT


def _L():
    from radar_depth_amd._lib import lib
    return lib()


# ------------------------------------------------------------------------------------------------ rd_wgrad_split[_pre]
@pytest.mark.parametrize("case", WL.CASES, ids=lambda c: c.id)
def test_wgrad_plan_facts(case):
    """out[0..3] of rd_wgrad_split_plan_info = splits, tiles per split, workgroups, pixel tiles (+ 2^30: the tall 4 x 16 tile)."""
    L = _L()
    d = WL.desc(case)
    assert L.rd_wgrad_split_supported(C.byref(d)) == 1
    assert L.rd_wgrad_split_pre_supported(C.byref(d)) == int(case.pre)
    info = (C.c_int32 * 4)()
    assert L.rd_wgrad_split_plan_info(C.byref(d), info) == 0
    assert ((info[3] >> 30) & 1, info[0], info[1], info[3] & ((1 << 30) - 1)) == (case.tall, case.splits, case.tiles_per_split, case.tiles), list(info)
    dw = WL.desc(case, window=True)
    assert (dw.ldi, dw.ldo) == (case.cin + 8, case.cout + 8) and L.rd_wgrad_split_supported(C.byref(dw)) == 1


def test_wgrad_cases_reach_what_they_are_there_for():
    by = {c.id: c for c in WL.CASES}
    assert {(c.kind, c.tall) for c in WL.CASES} == {("conv", 0), ("conv", 1), ("upproj", 0), ("upproj", 1)}
    assert any(c.splits > 16 for c in WL.CASES), "the two-stage slab reduction"
    assert any(c.cin % 64 and c.cout % 64 for c in WL.CASES), "partial 64-channel blocks on both sides"
    assert any(c.tiles == 1 for c in WL.CASES) and any(c.splits > 1 and c.tiles % c.tiles_per_split == 0 for c in WL.CASES)
    assert {by[i].kind for i in WL.WINDOW_CASES} == {"conv", "upproj"}
    # the UpProj phases are the four tap rectangles
    d = WL.desc(WL.CASES[7])
    rects = {(d.phase[i].dh_max - d.phase[i].dh_min + 1, d.phase[i].dw_max - d.phase[i].dw_min + 1) for i in range(d.n_phases)}
    assert rects == {(3, 3), (2, 3), (3, 2), (2, 2)}


@pytest.mark.parametrize("case", WL.CASES, ids=lambda c: c.id)
def test_wgrad_premises_and_kept_terms(case, capsys):
    for cls, e in WL.VARIANTS:
        fig = WL.premise(case, cls, e)
        with capsys.disabled():
            print("\n%-28s class %s 2^%-3d worst sum of |products| 2^%.1f, %.1f %% non-zero" % (case.id, cls, e, fig["worst_log2"], 100 * fig["nonzero"]),
                  end="")
        if e:
            continue
        x, dy, want = WL.data(case.id, cls)
        tm = WL.terms(case, x, dy)
        assert np.array_equal(WL.emulate(tm), want), (case.id, cls)
        for term in KEPT:
            changed = int((WL.emulate(tm, drop=term) != want).sum())
            assert (changed > 0) == (term in WL.CARRIED[cls]), (case.id, cls, term, changed)


def test_wgrad_class_d_places_the_hot_pixels():
    for case in WL.CASES:
        _, _, where = WL.one_hot(case)
        os_ = 2 if case.kind == "upproj" else 1
        logical = {(n, oh // os_, ow // os_) for (_, n, oh, ow, _, _) in where}
        assert set(WL.hot_pixels(case)) <= logical, case.id
        r, tw = WL.tile_shape(case)
        rows, cols = {p[1] for p in logical}, {p[2] for p in logical}
        assert {0, case.h - 1} <= rows and {0, case.w - 1} <= cols
        assert case.w <= tw or {tw - 1, tw} <= cols, case.id
        assert case.h <= r or {r - 1, r} <= rows, case.id
        assert {k for (_, _, _, _, k, _) in where} == set(range(-3, 4)) and {s for (_, _, _, _, _, s) in where} == {-1, 1}


@pytest.mark.parametrize("mode", WL.SHORTCUTS)
def test_wgrad_indexing_shortcuts_are_seen(mode):
    """Each shortcut moves class D -- one product per element, so a wrong address is a wrong element -- off the expected gradient on
    every case it applies to, and the lattice classes A-C on at least one."""
    seen = 0
    for case in WL.CASES[:4] + WL.CASES[7:]:
        for cls in WL.CLASSES:
            x, dy, want = WL.data(case.id, cls)
            got = WL.shortcut(case, x, dy, mode)
            if got is None:
                continue
            moved = int((got != want).sum())
            assert cls != "D" or moved > 0, (mode, case.id)
            seen += int(cls != "D" and moved > 0)
    assert seen > 0, mode


# ------------------------------------------------------------------------------------------------ the stems
@pytest.mark.parametrize("cfg", SL.WGRAD_CONFIGS, ids=SL.wgrad_id)
def test_stem_wgrad_premises_and_kept_terms(cfg, capsys):
    assert _L().rd_stem_wgrad_split_supported(cfg.cin, cfg.cout) == 1
    for shape in SL.wgrad_shapes(cfg)[:2]:          # (the kept-term proof does not depend on the map; the premises of the others: below)
        for cls in SL.wgrad_classes(cfg):
            x, dout, want = SL.wgrad_data(cfg, shape, cls)
            tm = SL.wgrad_terms(x, dout)
            assert np.array_equal(SL.emulate(tm), want), (cfg, shape, cls)
            for term in KEPT:
                changed = int((SL.emulate(tm, drop=term) != want).sum())
                assert (changed > 0) == (term in SL.CARRIED[cls]), (cfg, shape, cls, term, changed)
    for shape in SL.wgrad_shapes(cfg):
        for cls, e in SL.wgrad_variants(cfg):
            fig = SL.wgrad_premise(cfg, shape, cls, e)
            with capsys.disabled():
                print("\nstem wgrad %-16s %-10s class %s 2^%-3d worst 2^%.1f, %.1f %% non-zero" % (
                    SL.wgrad_id(cfg), "x".join(map(str, shape)), cls, e, fig["worst_log2"], 100 * fig["nonzero"]), end="")


def test_stem_wgrad_shapes_reach_the_tile_edges_and_the_two_stage_reduction():
    """The output tile is 4 x 32: a map narrower than a tile with one row past it, exactly one tile, one row and one column past it, and
    45 tiles for the 3 -> 64 stem."""
    tiles = lambda s: (s[0], -(-((s[1] - 1) // 2 + 1) // 4), -(-((s[2] - 1) // 2 + 1) // 32))
    assert [tiles(s) for s in SL.WGRAD_SHAPES] == [(2, 2, 1), (1, 1, 1), (2, 2, 2)] and tiles(SL.WGRAD_BIG) == (3, 5, 3)
    assert ((8 - 1) // 2 + 1, (64 - 1) // 2 + 1) == (4, 32)
    assert {(c.cin, c.cout, c.bf16) for c in SL.WGRAD_CONFIGS} == {(3, 64, 0), (1, 16, 0), (2, 16, 0), (4, 64, 0), (1, 64, 0), (3, 64, 1), (1, 16, 1),
                                                                   (2, 16, 1)}
    assert [c for c in SL.WGRAD_CONFIGS if SL.WGRAD_BIG in SL.wgrad_shapes(c)] == [SL.WGRAD_CONFIGS[0]]


@pytest.mark.parametrize("cfg", SL.FWD_CONFIGS, ids=SL.fwd_id)
def test_stem_fwd_premises_and_kept_terms(cfg, capsys):
    for shape in SL.FWD_SHAPES:
        for cls in SL.FWD_CLASSES:
            fig = SL.fwd_premise(cfg, shape, cls)
            with capsys.disabled():
                print("\nstem fwd %-8s %-10s class %s worst 2^%.1f, %.1f %% non-zero" % (SL.fwd_id(cfg), "x".join(map(str, shape)), cls,
                                                                                         fig["worst_log2"], 100 * fig["nonzero"]), end="")
            if shape != SL.FWD_SHAPES[0]:
                continue
            x, w, want = SL.fwd_data(cfg, shape, cls)
            tm = SL.fwd_terms(x, w)
            assert np.array_equal(SL.emulate(tm), want), (cfg, shape, cls)
            for term in KEPT:
                changed = int((SL.emulate(tm, drop=term) != want).sum())
                assert (changed > 0) == (term in SL.CARRIED[cls]), (cfg, shape, cls, term, changed)


def test_stem_fwd_shapes_and_configs():
    """The output tile is 8 x 32: smaller than a tile, exactly one, one past it in both directions."""
    tiles = lambda s: (s[0], -(-((s[1] - 1) // 2 + 1) // 8), -(-((s[2] - 1) // 2 + 1) // 32))
    assert [tiles(s) for s in SL.FWD_SHAPES] == [(2, 1, 1), (1, 1, 1), (2, 2, 2)] and ((16 - 1) // 2 + 1, (64 - 1) // 2 + 1) == (8, 32)
    L = _L()
    for s in SL.FWD_SHAPES:
        assert L.rd_stem_stat_tiles(*s) == int(np.prod(tiles(s))), s
    assert set(SL.FWD_CONFIGS) == {(ci, co) for ci in (1, 2, 3) for co in (16, 32, 64)} | {(4, 64)}


def test_stem_references_are_torch_float64():
    """stem_lattice_cases.fwd_ref / wgrad_ref against torch's float64 conv2d and conv2d_weight (7x7, stride 2, pad 3), odd and even maps."""
    import torch
    import torch.nn.functional as TF
    rng = np.random.default_rng(3)
    for n, c, h, w, o in ((2, 3, 9, 11, 5), (1, 2, 8, 64, 4)):
        x, wt = rng.standard_normal((n, c, h, w)), rng.standard_normal((o, c, 7, 7))
        y = TF.conv2d(torch.tensor(x), torch.tensor(wt), stride=2, padding=3)
        got = SL.fwd_ref(x, wt.transpose(2, 3, 1, 0).reshape(49, c, o))
        assert np.abs(got - y.permute(0, 2, 3, 1).numpy()).max() <= 1e-13 * np.abs(y.numpy()).max()
        dout = rng.standard_normal(tuple(y.permute(0, 2, 3, 1).shape))
        g = torch.nn.grad.conv2d_weight(torch.tensor(x), wt.shape, torch.tensor(dout).permute(0, 3, 1, 2).contiguous(), stride=2, padding=3)
        assert np.abs(SL.wgrad_ref(x, dout) - g.numpy()).max() <= 1e-13 * np.abs(g.numpy()).max()

"""Host-side checks of the plan tests of the fp32 convolution (tests/gconv_plan_cases.py; no GPU needed -- the planner's host entry
points run on the CPU, where the CU count falls back to the library's default):

  * the float64 reference (tests/desc_emulator.run_desc + the epilogue of gconv_plan_cases) against torch.nn.functional -- conv2d,
    conv_transpose2d, the unpool + 5x5 construction and their input gradients -- in float64, for every case kind;
  * the exactness budgets of every case on both grids;
  * the candidate sets: nothing truncated, every pin accepted and reported back by rd_gconv_plan_info, all five register tiles,
    both patch chunks, split-K 1 / 2 / 4 and the three loop forms covered, several column tiles on every register tile for c3w;
  * every (MT, NT, CKP, ksplit, loop form) point that radar_depth_amd/tuned_plans.json pins occurs among the candidates of a case."""
import ctypes as C
import json

import pytest
import torch

import gconv_plan_cases as G
from radar_depth_amd._lib import lib

TILES = {(2, 2), (2, 1), (3, 2), (1, 2), (1, 1)}


@pytest.fixture(scope="module")
def cand_sets():
    """Candidates of every case, every pin checked; the descriptors go back to the heuristic afterwards."""
    L = lib()
    out = {}
    for case in G.CASES:
        d = case.desc()
        assert L.rd_gconv_plan_state(C.byref(d), 1) == 0, "%s is already planned in this process: change the case's shape" % case.name
        cands = G.candidates(L, d)
        for c in cands:
            G.pin(L, d, c)
            assert L.rd_gconv_plan_state(C.byref(d), 1) == 1
        if cands:
            G.pin(L, d, None)
        out[case.name] = cands
    return out


@pytest.mark.parametrize("case", G.CASES + [G.WINO_EXTRA], ids=repr)
def test_reference_matches_torch_functional(case):
    d = case.desc()
    for grid in ("quarter", "unit"):
        data = G.make_data(case, grid)
        y = G.conv_ref(d, data["x"], data["w"])
        assert not torch.isnan(y).any() and G.covers_output(d), "every case tiles its whole output"
        assert tuple(y.shape) == (d.N, d.Ho, d.Wo, d.Cout)
        want = G.torch_ref(case, data["x"], data["w"])
        assert torch.equal(y, want), (case.name, grid, float((y - want).abs().max()))     # exact data: float64 is exact in any order
    # the epilogue: bias, addend, activation on the first act_cols channels; LeakyReLU = one float32 multiply
    data = G.make_data(case, "quarter")
    y = G.conv_ref(d, data["x"], data["w"])
    ac = d.Cout // 2 + 2
    for act in (G.ACT_RELU, G.ACT_LEAKY02):
        got = G.epilogue_ref(y, data["bias"], data["addend"], act, ac)
        z = (y + data["bias"] + data["addend"]).float()
        neg = torch.zeros_like(z) if act == G.ACT_RELU else z * 0.2
        want = torch.cat((torch.where(z[..., :ac] > 0, z[..., :ac], neg[..., :ac]), z[..., ac:]), -1)
        assert want.dtype == torch.float32 and torch.equal(got, want)
        assert bool((got[..., ac:] < 0).any()) and bool((z[..., :ac] < 0).any()), "the boundary must be visible in the data"
    assert torch.equal(G.epilogue_ref(y, data["bias"], None, G.ACT_NONE, 0), (y + data["bias"]).float())


def test_randn_reference_matches_torch_functional():
    for name in ("c3", "up", "dgs2", "updg", "dc3", "dc2"):
        case = G.BY_NAME[name]
        data = G.make_randn(case)
        y = G.conv_ref(case.desc(), data["x"], data["w"])
        want = G.torch_ref(case, data["x"], data["w"])
        assert float((y - want).abs().max()) <= 1e-12 * float(want.abs().max()), name


@pytest.mark.parametrize("case", G.CASES + [G.WINO_EXTRA], ids=repr)
def test_exactness_budgets(case):
    figs = {grid: G.check_budget(case, grid, G.make_data(case, grid)) for grid in ("quarter", "unit")}
    print(case.name, figs)
    # the unit-grid statistics are not trivial: some channel's sums are non-zero, and the BatchNorm-backward gate both opens and closes
    data = G.make_data(case, "unit")
    y = G.conv_ref(case.desc(), data["x"], data["w"])
    s0, s1 = G.bnbwd_ref(y, data["bn_x"], data["mean"], data["scale"], data["shift"])
    assert bool((s0 != 0).any()) and bool((s1 != 0).any()) and bool((y != 0).any())
    z = data["scale"] * data["bn_x"] + data["shift"]
    assert bool((z > 0).any()) and bool((z == 0).any()) and bool((z < 0).any())


def test_budget_check_refuses_inexact_data():
    case = G.BY_NAME["c3"]
    data = G.make_data(case, "unit")
    data["x"] = data["x"] * 4096.0
    with pytest.raises(AssertionError):
        G.check_budget(case, "unit", data)
    data = G.make_data(case, "quarter")
    data["w"] = data["w"] + 1.0 / 3.0
    with pytest.raises(AssertionError):
        G.check_budget(case, "quarter", data)


def test_candidates_cover_the_planner(cand_sets):
    allc = [c for v in cand_sets.values() for c in v]
    print({k: len(v) for k, v in cand_sets.items()}, "total", len(allc))
    assert cand_sets["c16"] == [], "the conv16 kernel has one tiling"
    for name, v in cand_sets.items():
        if name != "c16":
            assert len(v) > 1 and len(set(v)) == len(v), name
    assert {(c[0], c[1]) for c in allc} == TILES
    assert {c[4] for c in allc} == {16, 32}
    assert {c[7] for c in allc} == {1, 2, 4}
    assert {c[8] for c in allc} == {0, 1, 2}
    # every register tile runs every loop form and every split somewhere
    for t in TILES:
        mine = [c for c in allc if (c[0], c[1]) == t]
        assert {c[8] for c in mine} == {0, 1, 2} and {c[7] for c in mine} == {1, 2, 4}, t
    assert all(c[7] == 1 for c in cand_sets["c3s"]), "a channel slice of a wider output buffer cannot split (ldo != Cout)"
    assert {c[4] for c in cand_sets["c3r"]} == {16}


def test_c3w_has_several_column_tiles_on_every_register_tile(cand_sets):
    d = G.BY_NAME["c3w"].desc()
    for t in TILES:
        tws = [c[6] for c in cand_sets["c3w"] if (c[0], c[1]) == t]
        assert tws and all(-(-d.Wo // tw) > 1 for tw in tws), (t, tws)


def test_cases_are_ragged_under_some_register_tile(cand_sets):
    for case in G.CASES:
        if case.name == "c16":
            continue
        d = case.desc()
        ragged = False
        for c in cand_sets[case.name]:
            for i in range(d.n_phases):
                p = d.phase[i]
                ragged = ragged or p.lh % c[5] != 0 or p.lw % c[6] != 0 or c[5] * c[6] != c[0] * c[2] * 32 or d.Cout % (c[1] * c[3] * 32) != 0
        assert ragged, case.name


def test_tuned_table_points_are_covered(cand_sets):
    from radar_depth_amd import autotune
    with open(autotune.TABLE_PATH) as f:
        plans = json.load(f)["plans"]
    have = {(c[0], c[1], c[4], c[7], c[8]) for v in cand_sets.values() for c in v}
    want = {(p["plan"][0], p["plan"][1], p["plan"][4], p["plan"][7], p["plan"][8]) for p in plans.values()}
    print("tuned table: %d plans on %d points; the cases offer %d points" % (len(plans), len(want), len(have)))
    assert want and want <= have, sorted(want - have)
    assert sum(p["plan"][8] == 2 for p in plans.values()) > 0 and sum(p["plan"][7] > 1 for p in plans.values()) > 0

"""CPU-only checks of what tests/test_gpu_head.py stands on (tests/head_ref.py, tests/head_cases.py):

  - the float64 reference is torch's float64 conv2d / interpolate(align_corners=True) and their autograd;
  - the fp32 restatement of every kernel (head_ref.k_*) stays inside every bar and interval on every case -- the bilinear one with the
    fused coordinate the compiled kernel uses and with ATen's separately rounded one, and ATen's own fp32 interpolate does too;
  - the cap: at most 5 % of the intervals of a bf16 dx of at least 1000 elements hold more than one bf16 value;
  - the criterion has teeth: every shortcut of head_ref.MODES leaves the bars or intervals, and where it cannot show the test says why;
  - the weight gradient's regimes and the bilinear backward's paths are what head_cases states;
  - the argument checks of csrc/head.hip stand before the launches."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import head_cases as HC
import head_ref as R
import norm_bf16_cases as B
import norm_cases as NC

F, D = np.float32, np.float64
C = R.C
CAP_BLOCKS = 4 * 256          # four blocks per CU on the MI355X's 256 CUs
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocks(shape):
    return R.wgrad_blocks(int(np.prod(shape)), CAP_BLOCKS)


def _restated(shape, bf16, mode="exact", tiled=True, layout="window"):
    """d, dx (as the window holds it after the store), dw of the restated kernels under `mode`."""
    dat, _ = HC.conv_case(shape, bf16)
    (ldx, cx), (ldd, cd) = HC.LAYOUTS[layout]["x"], HC.LAYOUTS[layout]["dx"]
    x = R.load(dat["x"], ldx, cx, mode)
    with np.errstate(all="ignore"):
        dx = R.k_conv_dgrad(dat["dd"], dat["w"], mode)
        if bf16:
            dx = B.rb(dx, mode)
        return dict(d=R.k_conv_fwd(x, dat["w"], tiled, mode).astype(D), dx=R.store(dx, ldd, cd, mode).astype(D),
                    dw=R.k_conv_wgrad(x, dat["dd"], _blocks(shape), mode).astype(D))


def _missed(fr, h):
    """The outputs that left their bar or interval."""
    return {k for k, v in fr.items() if v > 1.0} | {k for k, v in h.items() if v["out"]}


# ------------------------------------------------------------------------------------------------ the reference is the operation
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 9, 33)], ids=HC.case_id)
def test_conv_reference_is_torch_float64(shape):
    dat = HC.conv_data(shape)
    want = HC.conv_want(dat)
    x = torch.tensor(dat["x"], dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
    w = torch.tensor(dat["w"], dtype=torch.float64)[None].requires_grad_(True)
    d = TF.conv2d(x, w, padding=1)
    d.backward(torch.tensor(dat["dd"], dtype=torch.float64)[:, None])
    for got, ref in ((want["d"], d[:, 0]), (want["dx"], x.grad.permute(0, 2, 3, 1)), (want["dw"], w.grad[0])):
        assert np.abs(got - ref.detach().numpy()).max() <= 1e-13 * np.abs(got).max()


@pytest.mark.parametrize("case", HC.BIL[:9], ids=HC.case_id)
def test_bilinear_reference_is_torch_float64(case):
    dat, want = HC.bil_case(case)
    d = torch.tensor(dat["d"], dtype=torch.float64)[:, None].requires_grad_(True)
    out = TF.interpolate(d, size=case[3:5], mode="bilinear", align_corners=True)
    out.backward(torch.tensor(dat["dout"], dtype=torch.float64)[:, None])
    assert np.abs(want["out"] - out[:, 0].detach().numpy()).max() <= 1e-13
    assert np.abs(want["dd"] - d.grad[:, 0].numpy()).max() <= 1e-13 * max(1.0, np.abs(want["dd"]).max())


# ------------------------------------------------------------------------------------------------ the correct kernels pass
def test_regimes_and_paths_are_as_stated():
    for shape in HC.CONV:
        b = _blocks(shape)
        assert R.wgrad_regime(b, CAP_BLOCKS) == HC.REGIME[shape] and b == HC.BLOCKS.get(shape, 1), shape
    big = HC.cap_shape(CAP_BLOCKS)
    assert big == (2, 438, 600) and R.wgrad_regime(_blocks(big), CAP_BLOCKS) == "cap"
    assert {HC.REGIME[s] for s in HC.CONV} == {"one", "direct", "two_stage"}
    for case in HC.BIL:
        assert R.bilinear_bwd_paths(*case[1:5]) == case[5], case
    assert {c[5] for c in HC.BIL} == {"fast", "mix", "generic"}
    # the generic loop is reached through the rows (3 -> 40) and through the columns (11 -> 45) alike
    assert R.bilinear_bwd_paths(3, 40, 40, 41) == "generic" and R.bilinear_bwd_paths(6, 11, 7, 45) == "mix"


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_the_restated_conv_kernels_pass_and_the_cap_holds(bf16, capsys):
    lines = []
    for shape in HC.CONV:
        dat, want = HC.conv_case(shape, bf16)
        for tiled in (True, False):
            fr, h = HC.conv_fracs(_restated(shape, bf16, tiled=tiled), want, dat, HC.K_FWD_TILED if tiled else HC.K_FWD_UNTILED, _blocks(shape))
            assert not _missed(fr, h), (shape, tiled, fr, h)
            assert not HC.capped(h), (shape, h)
            assert set(fr) | set(h) == {"d", "dx", "dw"}
        lines.append("%-12s %s %s" % (HC.case_id(shape), " ".join("%s=%.3f" % kv for kv in sorted(fr.items())), B.line("", h) if h else ""))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_tie_case_holds_ties_and_tells_the_roundings_apart():
    dat, want = HC.tie_data()
    n, differ = HC.n_ties(want)
    assert (n, differ) == (3968, 1997) and want["dx"].size == 18432
    with np.errstate(all="ignore"):
        dx = R.k_conv_dgrad(dat["dd"], dat["w"])
    assert np.array_equal(dx.astype(D), want["dx"]), "every fp32 operation of the restated kernel is exact"
    outs = {m: HC.conv_fracs(dict(dx=B.rb(dx, m).astype(D)), want, dat, 0, 1)[1]["dx"]["out"] for m in ("exact", "half_up", "truncate")}
    assert outs["exact"] == 0 and outs["half_up"] == differ and outs["truncate"] >= differ, outs


@pytest.mark.parametrize("case", HC.BIL, ids=HC.case_id)
def test_the_restated_bilinear_kernels_and_aten_pass(case, capsys):
    dat, want = HC.bil_case(case)
    N, Hs, Ws, Ho, Wo = case[:5]
    worst = {}
    for coord in ("fused", "separate"):
        got = dict(out=R.k_bilinear_fwd(dat["d"], Ho, Wo, coord).astype(D), dd=R.k_bilinear_bwd(dat["dout"], Hs, Ws, coord).astype(D))
        worst[coord] = fr = HC.bil_fracs(got, want)
        assert NC.worst(fr) <= 1.0, (case, coord, fr)
    d = torch.tensor(dat["d"])[:, None].requires_grad_(True)
    out = TF.interpolate(d, size=(Ho, Wo), mode="bilinear", align_corners=True)
    out.backward(torch.tensor(dat["dout"])[:, None])
    worst["aten"] = fr = HC.bil_fracs(dict(out=out[:, 0].detach().numpy().astype(D), dd=d.grad[:, 0].numpy().astype(D)), want)
    assert NC.worst(fr) <= 1.0, (case, "aten", fr)
    with capsys.disabled():
        print("\n%-22s %s" % (HC.case_id(case[:5]), "  ".join("%s out=%.3f dd=%.3f" % (k, v["out"], v["dd"]) for k, v in worst.items())))


# ------------------------------------------------------------------------------------------------ the shortcuts do not
# mode -> (storage, outputs that must leave their bar or interval, the cases on which the shortcut cannot show and why)
ONE_PIXEL = {(1, 1, 1)}
CONV_WHERE = {
    "taps_transposed": (False, {"d", "dx", "dw"}, ONE_PIXEL),                                  # only the centre tap is inside a 1 x 1 image
    "dgrad_unflipped": (False, {"dx"}, ONE_PIXEL),
    "wgrad_sign": (False, {"dw"}, ONE_PIXEL),
    "no_col_mask": (False, {"d", "dx", "dw"}, ONE_PIXEL),                                      # no neighbouring row or image in memory
    "no_image_mask": (False, {"d", "dx", "dw"}, {s for s in HC.CONV if s[0] == 1}),            # one image: nothing but zeros around it
    "ld_as_C": (False, {"d", "dx", "dw"}, ONE_PIXEL),                                          # the stride is never used with one pixel
    "c0_ignored": (False, {"d", "dx", "dw"}, set()),
    "truncate": (True, {"dx"}, set()),
    "slab_dropped": (False, {"dw"}, set()),
}


@pytest.mark.parametrize("mode", sorted(CONV_WHERE))
def test_conv_shortcuts_leave_the_bars(mode):
    bf16, outputs, blind = CONV_WHERE[mode]
    for shape in HC.CONV:
        dat, want = HC.conv_case(shape, bf16)
        for tiled in (True, False):
            fr, h = HC.conv_fracs(_restated(shape, bf16, mode, tiled), want, dat, HC.K_FWD_TILED if tiled else HC.K_FWD_UNTILED, _blocks(shape))
            assert _missed(fr, h) == (set() if shape in blind else outputs), (mode, shape, tiled, fr, h)


def test_ties_away_shows_on_the_tie_case_only():
    """Random data holds no exact tie: a ties-away store passes every random case and is caught by the constructed one (above)."""
    for shape in HC.CONV:
        dat, want = HC.conv_case(shape, True)
        assert not _missed(*HC.conv_fracs(_restated(shape, True, "half_up"), want, dat, HC.K_FWD_TILED, _blocks(shape))), shape


# the bilinear cases on which a shortcut cannot show: identity and a 1 x 1 source have the same weights with either scale; every
# weight of a 1 x 1 source falls on the one pixel whichever way round
IDENTITY, SOURCE_1 = HC.BIL[0], HC.BIL[2]
BIL_WHERE = {"align_false": ({"out", "dd"}, {IDENTITY, SOURCE_1}), "lx_swapped": ({"out", "dd"}, {SOURCE_1}), "window_short": ({"dd"}, set()),
             "i1_unclamped": ({"out"}, None)}


@pytest.mark.parametrize("mode", sorted(BIL_WHERE))
def test_bilinear_shortcuts_leave_the_bars(mode):
    outputs, blind = BIL_WHERE[mode]
    seen = 0
    for case in HC.BIL:
        dat, want = HC.bil_case(case)
        N, Hs, Ws, Ho, Wo = case[:5]
        for coord in ("fused", "separate"):
            with np.errstate(all="ignore"):
                got = dict(out=R.k_bilinear_fwd(dat["d"], Ho, Wo, coord, mode).astype(D), dd=R.k_bilinear_bwd(dat["dout"], Hs, Ws, coord, mode).astype(D))
            missed = {k for k, v in HC.bil_fracs(got, want).items() if v > 1.0}
            if blind is None:
                # an unclamped i1 reads the row behind the image wherever the last output row's i0 is the last source row (it always is
                # unless the rounded product falls short of Hs - 1): with weight 0 or not, the NaN guard behind the last image shows
                reads_behind = R.k_index(Hs, Ho, coord)[0][-1] == Hs - 1
                assert missed == (outputs if reads_behind else set()), (mode, case, coord)
                seen += reads_behind
            else:
                assert missed == (set() if case in blind else outputs), (mode, case, coord, missed)
    assert blind is not None or seen >= 16, "the unclamped row shows on at least eight of the ten shapes, with either coordinate"


# ------------------------------------------------------------------------------------------------ the launchers' source
def test_argument_checks_precede_the_launches():
    src = open(os.path.join(REPO, "radar_depth_amd", "csrc", "head.hip")).read()
    for fn in HC.LAUNCHERS:
        assert NC.checks_precede_launches(src, fn), fn
    assert HC.bwd_checks_precede_halves(src)

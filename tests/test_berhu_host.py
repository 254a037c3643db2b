"""MaskedBerHuLoss without a GPU: the numpy restatement (tests/berhu_ref.py) against the vectors of the reference's own class
(tests/golden/berhu.npz), what that fixture claims to cover, the RD_EBERHU_* argument checks (nothing is launched: the pointers are host
dummies that are never followed), and the Python surface."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import berhu_ref as B  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "berhu.npz"))
CASES = ("rand", "ladder", "ladder2", "thresh1", "equal", "tail")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(name):
    return G[name + "_pred"], G[name + "_target"], float(G[name + "_thresh"])


# ------------------------------------------------------------------------------------------------ restatement and fixture
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(name):
    pred, target, thresh = case(name)
    want_loss, want_grad = float(G[name + "_loss"]), G[name + "_grad"]
    r = B.berhu(pred, target, thresh, coef=3.0)
    if name == "equal":
        assert np.isnan(want_loss) and np.isnan(r.loss) and not want_grad.any() and not r.grad.any()
        assert np.isnan(r.term[r.valid]).all() and not r.term[~r.valid].any()
        return
    print(name, "loss rel", abs(r.loss - want_loss) / abs(want_loss), "grad", np.abs(r.grad - want_grad).max() / np.abs(want_grad).max())
    assert abs(r.loss - want_loss) <= 1e-6 * abs(want_loss)
    assert np.abs(r.grad - want_grad).max() <= 1e-6 * np.abs(want_grad).max()
    assert np.array_equal(r.grad == 0, want_grad == 0)


def test_restatement_matches_reference_big():
    pred, target = B.big_planes(int(G["big_seed"]))
    assert np.array_equal(np.array([pred.astype(np.float64).sum(), target.astype(np.float64).sum()]), G["big_check"])
    assert pred.size > 1024 * 256 * 8
    r = B.berhu(pred, target, float(G["big_thresh"]))
    print("big loss rel", abs(r.loss - float(G["big_loss"])) / float(G["big_loss"]))
    assert abs(r.loss - float(G["big_loss"])) <= 1e-6 * float(G["big_loss"])


def test_fixture_covers_what_it_claims():
    # rand: two frames of an odd size, about 40 % valid, predictions on both sides, an invalid pixel beyond the valid maximum
    pred, target, _ = case("rand")
    v = target > 0
    d = np.abs(target - pred)
    assert pred.shape == (2, 1, 33, 47) and 0.3 < v.mean() < 0.5 and (pred > target)[v].any() and (pred < target)[v].any()
    bad = int(G["rand_outlier"])
    assert not v.reshape(-1)[bad] and d.reshape(-1)[bad] > d[v].max() and d.reshape(-1)[bad] == d.max()
    # ladder: delta = 10 exactly; the rungs sit at delta and its float32 neighbours; at least three valid pixels are in neither branch
    for name, exact in (("ladder", True), ("ladder2", False)):
        pred, target, thresh = case(name)
        r = B.berhu(pred, target, thresh)
        assert pred.shape == (1, 1, 9, 13) and r.delta == float(G[name + "_delta"]) and (float(np.float32(r.delta)) == r.delta) == exact
        pos, steps = G[name + "_pos"], G[name + "_steps"]
        diff = np.abs(target - pred).reshape(-1)[pos]
        assert r.valid.reshape(-1)[pos].all() and sorted(set(steps.tolist())) == [-2, -1, 0, 1, 2]
        for dd, k in zip(diff, steps):
            x = np.float32(r.delta)
            for _ in range(abs(int(k))):
                x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
            assert dd == x
    pred, target, thresh = case("ladder")
    r = B.berhu(pred, target, thresh)
    assert r.delta == 10.0
    neither = r.valid & ~r.in1 & ~r.in2
    assert int(neither.sum()) >= 3 and not r.term[neither].any() and not r.grad[neither].any()
    assert (r.in1 & r.in2).sum() == 0
    # the shortcuts miss the reference's ladder loss by more than 1e-4 relative (the exact restatement: within 1e-6, above)
    want = float(G["ladder_loss"])
    for mode in ("single_compare", "textbook"):
        assert abs(B.berhu(pred, target, thresh, mode=mode).loss - want) > 1e-4 * want, mode
    # thresh1: the pixel holding the maximum is in neither branch
    pred, target, thresh = case("thresh1")
    r = B.berhu(pred, target, thresh)
    top = np.abs(target - pred) == r.max
    assert thresh == 1.0 and (top & r.valid).sum() >= 1 and not r.in1[top & r.valid].any() and not r.in2[top & r.valid].any()
    assert G["thresh1_grad"][top & r.valid].tolist() == [0.0] * int((top & r.valid).sum())
    # equal: valid pixels equal the prediction, invalid ones do not
    pred, target, _ = case("equal")
    assert (target > 0).any() and np.array_equal(pred[target > 0], target[target > 0]) and (pred != target)[target <= 0].all()
    # tail: five elements, the maximum in the last
    pred, target, _ = case("tail")
    d = np.where(target > 0, np.abs(target - pred), 0).reshape(-1)
    assert pred.shape == (1, 1, 1, 5) and d.argmax() == 4 and d[4] > d[:4].max()


def test_reciprocal_shortcut_changes_terms():
    """Multiplying by 1 / den is not the division: over the big planes some terms differ in the last bit."""
    pred, target = B.big_planes(int(G["big_seed"]), shape=(1, 1, 90, 80))
    a, b = B.berhu(pred, target, 0.2), B.berhu(pred, target, 0.2, mode="reciprocal")
    assert (a.term != b.term).any()


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_new_symbols_are_exported(L):
    for name in ("rd_berhu_workspace_floats", "rd_masked_berhu_sums", "rd_masked_berhu_sums_metrics", "rd_masked_berhu_bwd"):
        assert hasattr(L, name), name
    from radar_depth_amd import _lib as E
    tiles = L.rd_loss_tiles(C.c_int64(5)), L.rd_loss_tiles(C.c_int64(3 * 900 * 800))
    assert tiles == (1, 1024)
    # twelve doubles per tile for the partial sums, one 32-bit maximum per tile
    assert [L.rd_berhu_workspace_floats(5), L.rd_berhu_workspace_floats(3 * 900 * 800)] == [2 * 12 + 2, 2 * 12 * 1024 + 1024]
    assert L.rd_berhu_workspace_floats(0) == E.RD_EBERHU_RANGE and L.rd_berhu_workspace_floats(-3) == E.RD_EBERHU_RANGE
    for name in ("rd_masked_berhu_sums", "rd_masked_berhu_sums_metrics", "rd_masked_berhu_bwd"):      # replayable by the op table
        assert L.rd_optable_entry_args(name.encode()) == {"rd_masked_berhu_sums": 7}.get(name, 8)


def test_abi_rejects_bad_arguments_without_gpu(L):
    """Every rejection happens before anything reaches the GPU, each with a code of its own."""
    from radar_depth_amd import _lib as E
    big = C.create_string_buffer(1 << 12)
    base = (C.addressof(big) + 15) & ~15
    opt = lambda v: None if v is None else C.c_void_p(base + v)        # noqa: E731

    def sums(pred=0, target=64, n=5, thresh=0.2, ws=128, sums=512, msums=None, metrics=False):
        if metrics:
            return L.rd_masked_berhu_sums_metrics(opt(pred), opt(target), n, thresh, opt(ws), opt(sums), opt(msums), None)
        return L.rd_masked_berhu_sums(opt(pred), opt(target), n, thresh, opt(ws), opt(sums), None)

    def bwd(pred=0, target=64, n=5, sums=512, coef=600, dpred=640):
        return L.rd_masked_berhu_bwd(opt(pred), opt(target), n, opt(sums), opt(coef), opt(dpred), 0, None)

    assert [sums(pred=None), sums(target=None), sums(ws=None), sums(sums=None), sums(metrics=True), bwd(pred=None), bwd(target=None),
            bwd(sums=None), bwd(coef=None), bwd(dpred=None)] == [E.RD_EBERHU_NULL] * 10 and b"null" in L.rd_last_error()
    assert [sums(n=0), sums(n=-1), sums(n=0, metrics=True, msums=560), bwd(n=0)] == [E.RD_EBERHU_RANGE] * 4 and b"n = 0" in L.rd_last_error()
    assert [sums(thresh=0.0), sums(thresh=-0.2), sums(thresh=float("nan")), sums(thresh=float("inf")),
            sums(thresh=0.0, metrics=True, msums=560)] == [E.RD_EBERHU_THRESH] * 5 and b"thresh" in L.rd_last_error()
    assert [sums(ws=132), sums(sums=516), sums(metrics=True, msums=564), bwd(sums=516)] == [E.RD_EBERHU_ALIGN] * 4 and b"8-byte" in L.rd_last_error()
    codes = [E.RD_EBERHU_NULL, E.RD_EBERHU_RANGE, E.RD_EBERHU_THRESH, E.RD_EBERHU_ALIGN]
    assert codes == list(range(E.RD_EVIS_OVERLAP - 1, E.RD_EVIS_OVERLAP - 5, -1))                 # the numbering goes on after RD_EVIS_OVERLAP
    hdr = open(os.path.join(ROOT, "include", "radar_depth_hip.h")).read()
    for name in ("NULL", "RANGE", "THRESH", "ALIGN"):
        assert "#define RD_EBERHU_%s (%d)" % (name, getattr(E, "RD_EBERHU_" + name)) in hdr


# ------------------------------------------------------------------------------------------------ Python surface
def test_signatures_are_the_references():
    from radar_depth_amd.evaluation import criteria_new
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]        # noqa: E731
    empty = inspect.Parameter.empty
    assert sig(criteria_new.MaskedBerHuLoss.__init__) == [("self", empty), ("thresh", 0.2)]
    assert sig(criteria_new.MaskedBerHuLoss.forward) == [("self", empty), ("pred", empty), ("target", empty)]
    assert criteria_new.MaskedBerHuLoss().thresh == 0.2 and criteria_new.MaskedBerHuLoss(0.5).thresh == 0.5
    import torch
    with pytest.raises(RuntimeError, match="MI355X only"):
        criteria_new.MaskedBerHuLoss()(torch.zeros(1, 1, 2, 2), torch.ones(1, 1, 2, 2))
    with pytest.raises(AssertionError, match="inconsistent dimensions"):
        criteria_new.MaskedBerHuLoss()(torch.zeros(1, 2, 2), torch.ones(1, 1, 2, 2))


def test_criterion_names():
    from radar_depth_amd import main, utils
    base = ["-a", "resnet18_latefusion", "--data", "nuscenes"]
    assert utils.parse_command(base).criterion == "l1"
    for name in ("l1", "l2", "berhu"):
        assert utils.parse_command(base + ["-c", name]).criterion == name
    with pytest.raises(SystemExit):
        utils.parse_command(base + ["-c", "huber"])
    assert main.CRITERIA == ("l1", "l2", "berhu")
    from radar_depth_amd.evaluation import criteria_new
    args = utils.parse_command(base + ["-c", "berhu"])
    crit = main.create_criterion(args, berhu_thresh=0.3)
    assert list(crit) == ["depth"] and isinstance(crit["depth"], criteria_new.MaskedBerHuLoss) and crit["depth"].thresh == 0.3
    args.arch, args.criterion = "resnet18_multistage_uncertainty_fixs", "l2"
    crit = main.create_criterion(args)
    assert isinstance(crit["depth"], criteria_new.MaskedMSELoss) and isinstance(crit["smooth"], criteria_new.SmoothnessLoss)
    args.criterion = "huber"
    with pytest.raises(ValueError, match=r"\[Error\] Unknown criterion"):
        main.create_criterion(args)


def test_train_step_rejects_an_unknown_criterion():
    from radar_depth_amd.main import HipTrainStep
    assert inspect.signature(HipTrainStep.__init__).parameters["berhu_thresh"].default == 0.2
    with pytest.raises(ValueError, match=r"\[Error\] Unknown criterion"):       # before the model or the GPU is touched
        HipTrainStep(None, 1, 8, 8, criterion="huber")

"""MaskedBerHuLoss on the GPU (csrc/loss_opt.hip: rd_masked_berhu_sums / _sums_metrics / _bwd; evaluation.criteria_new.MaskedBerHuLoss;
HipTrainStep(criterion="berhu")) against the numpy restatement of tests/berhu_ref.py and the reference's own values in
tests/golden/berhu.npz.

Bars: the maximum, delta and the count are exact.  The sum of the terms is within 1e-10 relative of the restatement's float64 sum of its
float32 terms -- both sides add the same float32 terms in double, only the order differs -- and the same bar holds the device meters to
Result.evaluate.  The gradient is exactly 0 wherever the restatement's is and within 1e-6 of each pixel's own value elsewhere.  Against
the reference's float32 loss and gradient the bars are those of tests/test_berhu_host.py (1e-6 relative; 1e-6 of the gradient's maximum).
The fused step is compared with a torch-CPU autograd restatement on the oracle model at the 2e-3 of the `-c l2` step test."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import berhu_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "berhu.npz"))
CASES = ("rand", "ladder", "ladder2", "thresh1", "equal", "tail")
NAMES = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10", "delta1", "delta2", "delta3")
COEF = 3.0


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _ok(rc, what):
    from radar_depth_amd._lib import check
    check(rc, what)


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _nan64(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)


def _bits(t):
    return t.cpu().view(torch.int64)


_PLANES = {}


def planes(name):
    """pred, target, thresh of a fixture case and the restatement's result on them, computed once."""
    if name not in _PLANES:
        if name == "big":
            pred, target = B.big_planes(int(G["big_seed"]))
        elif name == "none":                                  # no valid pixel: zeros and negatives
            pred = G["rand_pred"]
            target = np.where(G["rand_target"] > 0, np.float32(0), np.float32(-1.5)).astype(np.float32)
        else:
            pred, target = G[name + "_pred"], G[name + "_target"]
        thresh = 0.2 if name == "none" else float(G[name + "_thresh"])
        _PLANES[name] = (pred, target, thresh, B.berhu(pred, target, thresh, coef=COEF))
    return _PLANES[name]


def _sums(P, T, thresh, metrics=False):
    L = _L()
    n = P.numel()
    nfl = int(L.rd_berhu_workspace_floats(n))
    assert nfl > 0
    ws, sums, msums = _nan64((nfl + 1) // 2), _nan64(4), _nan64(10)
    if metrics:
        _ok(L.rd_masked_berhu_sums_metrics(_p(P), _p(T), n, thresh, _p(ws), _p(sums), _p(msums), _st()), "rd_masked_berhu_sums_metrics")
    else:
        _ok(L.rd_masked_berhu_sums(_p(P), _p(T), n, thresh, _p(ws), _p(sums), _st()), "rd_masked_berhu_sums")
    return sums, msums


def _bwd(P, T, sums, coef, dpred, accumulate):
    _ok(_L().rd_masked_berhu_bwd(_p(P), _p(T), P.numel(), _p(sums), _p(coef), _p(dpred), accumulate, _st()), "rd_masked_berhu_bwd")


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("name", CASES + ("big", "none"))
def test_kernels_against_restatement_and_reference(name):
    pred, target, thresh, r = planes(name)
    P, T = torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV)
    sums, _ = _sums(P, T, thresh)
    coef = torch.tensor([COEF], device=DEV)
    dp = torch.full(pred.shape, float("nan"), device=DEV)
    _bwd(P, T, sums, coef, dp, 0)
    d0 = torch.randn(pred.shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    acc = d0.clone()
    _bwd(P, T, sums, coef, acc, 1)
    sums_m, msums = _sums(P, T, thresh, metrics=True)
    L = _L()
    n = P.numel()
    mws, want_m = _nan64(10 * L.rd_loss_tiles(C.c_int64(n))), _nan64(10)
    _ok(L.rd_depth_metrics(_p(P), _p(T), C.c_int64(n), _p(mws), _p(want_m), _st()), "rd_depth_metrics")
    torch.cuda.synchronize()
    s = sums.cpu().numpy()
    got = dp.cpu().numpy()
    # ---- the threshold: exact, and it never left the device
    assert s[3] == float(r.max) and s[2] == r.delta and s[1] == r.count, (s, float(r.max), r.delta, r.count)
    # ---- the sum of the terms
    if name in ("equal", "none"):
        with np.errstate(invalid="ignore"):
            assert (math.isnan(s[0]) if name == "equal" else s[0] == 0.0) and math.isnan(s[0] / s[1]) and math.isnan(r.loss)
    else:
        print("%s: sum of terms within %.2e of the restatement" % (name, abs(s[0] - r.total) / abs(r.total)))
        assert abs(s[0] - r.total) <= 1e-10 * abs(r.total), (s[0], r.total)
    # ---- the gradient
    zero = r.grad == 0
    assert not np.isnan(got).any(), "accumulate = 0 must overwrite"
    assert not got[zero].any(), "exactly 0 on invalid pixels, where t == p and where a pixel is in neither branch"
    assert (np.abs(got[~zero] - r.grad[~zero]) <= 1e-6 * np.abs(r.grad[~zero])).all()
    if name in ("ladder", "ladder2"):
        pos = G[name + "_pos"]
        assert np.array_equal(got.reshape(-1)[pos] == 0, (r.valid & ~r.in1 & ~r.in2).reshape(-1)[pos])
    assert torch.equal(acc, d0 + dp), "accumulate = 1 adds onto what dpred held"
    # ---- the reference's own loss and gradient
    if name not in ("equal", "none"):
        want = float(G[name + "_loss"])
        assert abs(s[0] / s[1] - want) <= 1e-6 * want, (s[0] / s[1], want)
    if name not in ("big", "none"):
        wg = G[name + "_grad"]
        assert np.abs(got - wg).max() <= 1e-6 * max(np.abs(wg).max(), 1e-30) and np.array_equal(got == 0, wg == 0)
    # ---- with the metric sums riding along: the same bits as the plain call and as rd_depth_metrics
    assert torch.equal(_bits(sums_m), _bits(sums))
    assert torch.equal(_bits(msums), _bits(want_m))
    assert float(msums[0].item()) == r.count


# ------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("name", CASES)
def test_module_against_reference(name):
    from radar_depth_amd.evaluation.criteria_new import MaskedBerHuLoss
    pred, target, thresh, _ = planes(name)
    P = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    loss = MaskedBerHuLoss(thresh)(P, torch.from_numpy(target).to(DEV))
    (COEF * loss).backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    want, wg = float(G[name + "_loss"]), G[name + "_grad"]
    got = P.grad.cpu().numpy()
    if name == "equal":
        assert math.isnan(loss.item()) and math.isnan(want) and not got.any()
        return
    assert abs(loss.item() - want) <= 1e-6 * want
    assert np.abs(got - wg).max() <= 1e-6 * np.abs(wg).max() and np.array_equal(got == 0, wg == 0)


def test_module_honours_thresh_and_an_all_invalid_target():
    from radar_depth_amd.evaluation.criteria_new import MaskedBerHuLoss
    pred, target, _, r02 = planes("rand")
    r05 = B.berhu(pred, target, 0.5)
    P, T = torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV)
    l02, l05 = MaskedBerHuLoss()(P, T).item(), MaskedBerHuLoss(0.5)(P, T).item()
    assert abs(l02 - r02.loss) <= 1e-6 * r02.loss and abs(l05 - r05.loss) <= 1e-6 * r05.loss and abs(r05.loss - r02.loss) > 1e-2 * r02.loss
    # a diverged prediction: a NaN difference is the largest bit pattern, so it becomes the maximum and reaches the loss, as the
    # reference's torch.max carries it
    Pn = P.clone()
    Pn.view(-1)[int(np.flatnonzero(target.reshape(-1) > 0)[5])] = float("nan")
    assert math.isnan(MaskedBerHuLoss()(Pn, T).item())
    # the one difference from the reference, whose torch.max raises here
    P = P.clone().requires_grad_(True)
    loss = MaskedBerHuLoss()(P, torch.zeros_like(T))
    loss.backward()
    assert math.isnan(loss.item()) and not P.grad.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ the fused step
def berhu_torch(pred, target, thresh=0.2):
    """The definition of tests/berhu_ref.py in torch, for CPU autograd on the oracle model."""
    v = target > 0
    diff = (target[v] - pred[v]).abs()
    delta = thresh * float(diff.detach().max())
    thr, d2, den = (torch.tensor(x, dtype=torch.float32) for x in (-delta, delta * delta, 2.0 * delta))
    y = diff * diff - d2
    part1 = torch.where(-diff > thr, diff, torch.zeros_like(diff))
    part2 = (torch.where(y > 0, y, -d2) + d2) / den
    return (part1 + part2).mean()


def _latefusion_pair(h, w):
    from oracle.models import ResNet_latefusion as ORef
    from radar_depth_amd.model.models import ResNet_latefusion
    from radar_depth_amd.synthetic import procedural_fill_
    torch.manual_seed(0)
    m = ResNet_latefusion(18, "upproj", [h, w], 4, False)
    procedural_fill_(m)
    o = ORef(18, "upproj", [h, w], 4, False)
    procedural_fill_(o)
    return m.cuda().train(), o.train()


GEOM = (2, 97, 161)
STEPS = 3


def _batches():
    from radar_depth_amd.synthetic import make_batch
    b, h, w = GEOM
    return [make_batch(b, h, w, 40 + it, ref_pixels=h * w) for it in range(STEPS)]


def _run(**kw):
    """STEPS fused steps of a freshly filled latefusion model; returns the losses, the step object and the last prediction."""
    from radar_depth_amd.main import HipTrainStep
    b, h, w = GEOM
    m, _ = _latefusion_pair(h, w)
    ts = HipTrainStep(m, b, h, w, lr=0.01, momentum=0.9, weight_decay=1e-4, criterion="berhu", **kw)
    losses = []
    for x, t in _batches():
        loss, pred = ts.step(x.cuda(), t.cuda())
        losses.append(loss.clone())
    torch.cuda.synchronize()
    return [v.item() for v in losses], ts, pred


@pytest.fixture(scope="module")
def plain():
    losses, ts, _ = _run()
    names = [fn.__name__ for _, fn, _ in ts._ops]
    ts.close()
    return losses, names


def test_step_vs_oracle_autograd(plain):
    b, h, w = GEOM
    losses, names = plain
    assert names.count("rd_masked_berhu_sums") == 1 and names.count("rd_masked_berhu_bwd") == 1 and not [k for k in names if "masked_l1" in k]
    _, o = _latefusion_pair(h, w)
    opt = torch.optim.SGD(o.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    for it, (x, t) in enumerate(_batches()[:2]):
        lo = berhu_torch(o(x), t)
        opt.zero_grad()
        lo.backward()
        opt.step()
        assert abs(losses[it] - lo.item()) / lo.item() < 2e-3, (it, losses[it], lo.item())


def test_step_graph_replay_is_bit_identical(plain):
    losses, ts, _ = _run(use_graph=True)
    assert ts.graphs, "the later steps were replayed from captured graphs"
    ts.close()
    assert losses == plain[0], (losses, plain[0])


def test_step_with_metrics_keeps_the_loss(plain):
    from radar_depth_amd.evaluation.metrics import Result
    losses, ts, pred = _run(metrics=True)
    names = [fn.__name__ for _, fn, _ in ts._ops]
    assert names.count("rd_masked_berhu_sums_metrics") == 1 and "rd_masked_berhu_sums" not in names
    assert losses == plain[0], (losses, plain[0])
    r = Result()
    r.evaluate(pred, _batches()[-1][1].cuda())
    last, want = ts.meter.last(), np.array([getattr(r, k) for k in NAMES], dtype=np.float64)
    got = np.array([getattr(last, k) for k in NAMES], dtype=np.float64)
    # (lg10 is NaN on both sides while the barely trained network still predicts negative depths: NaN has to meet NaN)
    ok = ~np.isnan(want)
    assert ts.meter.count() == float(GEOM[0] * STEPS) and np.array_equal(np.isnan(got), np.isnan(want)) and ok.sum() >= 9, (got, want)
    assert (np.abs(got[ok] - want[ok]) <= 1e-10 * np.abs(want[ok])).all(), (got, want)
    ts.close()


def test_eager_loop_body_agrees_with_the_step(plain):
    """pred = model(x); loss = criterion(pred, t); loss.backward() through the drop-in module."""
    from radar_depth_amd.evaluation.criteria_new import MaskedBerHuLoss
    b, h, w = GEOM
    m, _ = _latefusion_pair(h, w)
    x, t = _batches()[0]
    loss = MaskedBerHuLoss()(m(x.cuda()), t.cuda())
    loss.backward()
    assert abs(loss.item() - plain[0][0]) / plain[0][0] < 2e-3
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_step_data_parallel_path(plain, tmp_path, monkeypatch):
    """Bucketed pieces with the native communicator on one rank: the losses of the single-GPU step."""
    from radar_depth_amd import comm
    comm.init_from_file(str(tmp_path / "rccl_token"), 0, 1)
    try:
        monkeypatch.setenv("RD_FORCE_DP", "1")
        losses, ts, _ = _run()
        assert ts.dp and ts.comm == "rccl"
        ts.close()
    finally:
        comm.destroy()
    assert losses == plain[0], (losses, plain[0])


def test_step_multistage_uncertainty_stage_losses():
    """Both stage losses of the uncertainty-weighted total are BerHu: loss4[0] and loss4[1] against the module on the two predictions."""
    from radar_depth_amd import main as hmain
    from radar_depth_amd.evaluation.criteria_new import MaskedBerHuLoss
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    b, h, w = GEOM
    torch.manual_seed(0)
    args = types.SimpleNamespace(arch="resnet18_multistage_uncertainty_fixs", decoder="upproj", modality="rgbd", pretrained=False)
    model, lw = hmain.create_model(args, [h, w])
    procedural_fill_(model)
    ts = hmain.HipTrainStep(model.cuda().train(), b, h, w, lr=0.01, momentum=0.9, weight_decay=1e-4, loss_weights=lw, criterion="berhu",
                            berhu_thresh=0.3)
    x, t = make_batch(b, h, w, 41, ref_pixels=h * w)
    t = t.cuda()
    loss, pred = ts.step(x.cuda(), t)
    torch.cuda.synchronize()
    names = [fn.__name__ for _, fn, _ in ts._ops]
    assert names.count("rd_masked_berhu_sums") == 2 and names.count("rd_masked_berhu_bwd") == 2 and not [k for k in names if "masked_l1" in k]
    crit = MaskedBerHuLoss(0.3)
    d1, d2 = crit(ts.plans[0].pred, t).item(), crit(pred, t).item()
    got = ts.loss4.cpu().numpy()
    assert abs(got[0] - d1) <= 1e-6 * d1 and abs(got[1] - d2) <= 1e-6 * d2 and d1 != d2, (got, d1, d2)
    assert math.isfinite(loss.item()) and abs(MaskedBerHuLoss(0.2)(pred, t).item() - d2) > 1e-3 * d2
    ts.close()

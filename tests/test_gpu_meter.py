"""On-device metric meters (csrc/loss_opt.hip: rd_masked_l1/l2_sums_metrics, rd_depth_metrics_frames, rd_meter_update;
evaluation.metrics.DeviceAverageMeter / evaluate_batch; HipTrainStep(metrics=True)).

Bars: the fused and per-frame kernels form the SAME fp32 terms as rd_depth_metrics and differ from it at most in the order of the
float64 summation (1e-10 relative; counts exact); the loss sums of the fused kernel are bit-identical to rd_masked_l1/l2_sums; the
meter against the reference's own CPU results (tests/golden/meter.npz) is held to 1e-5 relative -- 1.4e-7 between the reference's
fp32 means and a float64 mean of the same terms, plus at most ~2e-6 from 1-ulp logf differences in lg10 -- and against the existing
synchronising route (Result.evaluate + AverageMeter on the host, float64 on both sides) to 1e-10."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10", "delta1", "delta2", "delta3")


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


def _f64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _vec(result):
    return np.array([getattr(result, n) for n in NAMES], dtype=np.float64)


def _rel(got, want):
    """Worst relative error; NaN must meet NaN."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)).max())


def _pair(n, share, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, generator=g) * 79.5 + 0.5
    o = t * (torch.rand(n, generator=g) * 1.7 + 0.5)
    t = torch.where(torch.rand(n, generator=g) < share, t, torch.zeros(n))
    return o.to(DEV), t.to(DEV)


def _depth_metrics(o, t):
    L = _L()
    n = o.numel()
    ws, out = _f64(10 * L.rd_loss_tiles(C.c_int64(n))), _f64(10)
    _ok(L.rd_depth_metrics(_p(o), _p(t), C.c_int64(n), _p(ws), _p(out), _st()), "rd_depth_metrics")
    return out


def _sums_close(got, want, bar):
    got, want = got.cpu().numpy(), want.cpu().numpy()
    for k in (0, 5, 6, 7):
        assert got[k] == want[k], (k, got, want)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    assert (err <= bar).all(), (err, bar)
    return float(err.max())


# ------------------------------------------------------------------------------------------------ fused loss + metric sums
@pytest.mark.parametrize("share", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049, 3922, 2048 * 1024 + 3])       # the last: past the 1024-block cap, a second trip
def test_fused_sums_and_metrics(n, share):
    L = _L()
    o, t = _pair(n, share, 700 + n % 1000)
    tiles = L.rd_loss_tiles(C.c_int64(n))
    want_m = _depth_metrics(o, t)
    for kind in ("l1", "l2"):
        ws2, want = _f64(2 * tiles), _f64(2)
        _ok(getattr(L, "rd_masked_%s_sums" % kind)(_p(o), _p(t), C.c_int64(n), _p(ws2), _p(want), _st()), kind)
        ws12, got, got_m = _f64(12 * tiles), _f64(2), _f64(10)
        _ok(getattr(L, "rd_masked_%s_sums_metrics" % kind)(_p(o), _p(t), C.c_int64(n), _p(ws12), _p(got), _p(got_m), _st()), kind + " fused")
        torch.cuda.synchronize()
        assert torch.equal(got, want), (kind, got, want)                     # bit-identical loss sums
        worst = _sums_close(got_m, want_m, 1e-10)
        print("fused %s n=%d share=%.1f: metric sums within %.2e of rd_depth_metrics" % (kind, n, share, worst))


# ------------------------------------------------------------------------------------------------ per-frame sums
@pytest.mark.parametrize("frames,hw", [(1, 1), (3, 1961), (5, 2049), (2, 15617)])
def test_per_frame_sums(frames, hw):
    L = _L()
    o, t = _pair(frames * hw, 1.0 if hw == 1 else 0.3, 900 + hw % 1000)
    o, t = o.view(frames, hw), t.view(frames, hw).clone()
    if frames > 1:
        t[1] = 0                                                              # a frame without a valid pixel
    nfl = int(L.rd_depth_metrics_frames_workspace_floats(frames, hw))
    assert nfl == 2 * 10 * frames * L.rd_loss_tiles(C.c_int64(hw))
    ws, got = _f64(nfl // 2), _f64(frames, 10)
    _ok(L.rd_depth_metrics_frames(_p(o), _p(t), frames, hw, _p(ws), _p(got), _st()), "rd_depth_metrics_frames")
    torch.cuda.synchronize()
    for f in range(frames):
        _sums_close(got[f], _depth_metrics(o[f].contiguous(), t[f].contiguous()), 1e-10)
    if frames > 1:
        assert torch.equal(got[1].cpu(), torch.zeros(10, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ meter vs the reference's CPU results
def test_meter_vs_reference_fixture():
    from radar_depth_amd.evaluation.metrics import DeviceAverageMeter
    gold = np.load(os.path.join(HERE, "golden", "meter.npz"))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    worst = 0.0
    # 1. four steps, one Result per step, weights 3, 3, 2, 3
    m = DeviceAverageMeter()
    for k in range(4):
        m.update(dev(gold["step_out"][k]), dev(gold["step_target"][k]), n=float(gold["step_weights"][k]))
        worst = max(worst, _rel(_vec(m.last()), gold["step_results"][k]), _rel(_vec(m.average()), gold["step_averages"][k]))
    assert m.count() == 11.0
    # 2. five frames into three meters: one batch-1 update per frame, and one update of all five frames
    fo, ft, masks = dev(gold["frame_out"]), dev(gold["frame_target"]), [int(v) for v in gold["frame_groups"]]
    one, five = DeviceAverageMeter(groups=3), DeviceAverageMeter(groups=3)
    for k in range(5):
        one.update(fo[k:k + 1], ft[k:k + 1], per_frame=True, groups=[masks[k]])
    five.update(fo, ft, per_frame=True, groups=torch.tensor(masks, dtype=torch.int32, device=DEV))
    for g in range(3):
        for meter in (one, five):
            worst = max(worst, _rel(_vec(meter.average(g)), gold["frame_averages"][g]))
        assert one.count(g) == five.count(g) == sum(1 for v in masks if v >> g & 1)
    # 3. no valid pixel: NaN in all ten, and into the meter, in both modes
    for per_frame in (False, True):
        e = DeviceAverageMeter()
        e.update(dev(gold["empty_out"]), dev(gold["empty_target"]), per_frame=per_frame)
        assert np.isnan(_vec(e.last())).all() and np.isnan(_vec(e.average())).all() and e.count() == 1.0
        _rel(_vec(e.last()), gold["empty_result"])
    with pytest.raises(ZeroDivisionError):
        DeviceAverageMeter().average()
    t = DeviceAverageMeter()
    t.update(fo[:1], ft[:1])
    t.add_times(0.5, 0.25, 1)
    assert t.average().gpu_time == 0.5 and t.average().data_time == 0.25
    print("device meter vs the reference's CPU results: worst relative error %.3e" % worst)
    assert worst <= 1e-5


# ------------------------------------------------------------------------------------------------ the training step
def _model(arch, h, w):
    from radar_depth_amd import main as hmain
    from radar_depth_amd.model.models import ResNet
    from radar_depth_amd.synthetic import procedural_fill_
    torch.manual_seed(0)
    if arch == "resnet_rgb":
        m, lw = ResNet(18, "deconv2", [h, w], 3, False), None
    else:
        made = hmain.create_model(types.SimpleNamespace(arch=arch, decoder="upproj", modality="rgbd", pretrained=False), [h, w])
        m, lw = made if isinstance(made, tuple) else (made, None)
    procedural_fill_(m)
    return m.cuda().train(), lw


def _batches(arch, b, h, w, steps):
    from radar_depth_amd.synthetic import make_batch
    out = []
    for k in range(steps):
        x, t = make_batch(b, h, w, 300 + k, ref_pixels=h * w)
        out.append(((x[:, :3] if arch == "resnet_rgb" else x).contiguous().cuda(), t.cuda()))
    return out


def _step_check(arch, use_graph, criterion="l1", steps=3):
    from radar_depth_amd.evaluation.metrics import AverageMeter, Result
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 2, 97, 161
    data = _batches(arch, b, h, w, steps + 1)
    runs = {}
    for metrics in (False, True):
        m, lw = _model(arch, h, w)
        ts = HipTrainStep(m, b, h, w, lr=0.01, momentum=0.9, weight_decay=1e-4, loss_weights=lw, use_graph=use_graph, criterion=criterion,
                          metrics=metrics)
        host = [AverageMeter(), AverageMeter()]
        losses, results = [], []
        for x, t in data[:steps]:
            loss, pred = ts.step(x, t)
            losses.append(loss.clone())
            if metrics:                     # the synchronising route, on the predictions of the same step
                preds = [pred] + ([ts.plans[0].pred] if ts.multistage else [])
                results = []
                for am, pr in zip(host, preds):
                    r = Result()
                    r.evaluate(pr, t)
                    am.update(r, 0, 0, n=b)
                    results.append(r)
        torch.cuda.synchronize()
        runs[metrics] = ([v.item() for v in losses], [p.detach().clone() for p in m.parameters()], ts, host, results)
    l0, p0, ts0, _, _ = runs[False]
    l1, p1, ts, host, results = runs[True]
    assert ts0.meter is None and ts0.meter_stage1 is None
    assert not [name for name, _, _ in ts0._ops if "metrics" in name or "meter" in name]
    assert [name for name, _, _ in ts._ops if "metrics" in name] and [name for name, _, _ in ts._ops if "meter" in name]
    assert l0 == l1, (l0, l1)                                                   # bit-equal losses
    assert all(torch.equal(a, c) for a, c in zip(p0, p1))
    meters = [ts.meter] + ([ts.meter_stage1] if ts.multistage else [])
    assert (ts.meter_stage1 is not None) == ts.multistage
    worst = 0.0
    for dm, am, r in zip(meters, host, results):
        assert dm.count() == float(b * steps)                                   # a captured step counts once
        assert float(dm.buf[0, 11].item()) == float(steps)
        worst = max(worst, _rel(_vec(dm.average()), _vec(am.average())), _rel(_vec(dm.last()), _vec(r)))
    print("step %s graph=%s %s: device meter within %.2e of Result.evaluate + AverageMeter" % (arch, use_graph, criterion, worst))
    assert worst <= 1e-10
    for dm in meters:
        dm.reset()
    ts.step(*data[steps])
    torch.cuda.synchronize()
    for dm in meters:
        assert dm.count() == float(b)
    ts.close()
    ts0.close()


@pytest.mark.parametrize("use_graph", [False, True])
def test_step_latefusion(use_graph):
    _step_check("resnet18_latefusion", use_graph)


def test_step_multistage_uncertainty():
    _step_check("resnet18_multistage_uncertainty_fixs", False)


def test_step_early_fusion_l2():
    _step_check("resnet_rgb", False, criterion="l2")


def test_step_data_parallel(tmp_path, monkeypatch):
    """The data-parallel path (bucketed pieces, native communicator, one rank): the meter ops sit in the head piece, the meters are
    per rank and hold what the single-GPU step's hold."""
    from radar_depth_amd import comm
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 2, 97, 161
    data = _batches("resnet18_latefusion", b, h, w, 3)
    m_ref, _ = _model("resnet18_latefusion", h, w)
    ts_ref = HipTrainStep(m_ref, b, h, w, metrics=True)
    comm.init_from_file(str(tmp_path / "rccl_token"), 0, 1)
    try:
        monkeypatch.setenv("RD_FORCE_DP", "1")
        m, _ = _model("resnet18_latefusion", h, w)
        ts = HipTrainStep(m, b, h, w, metrics=True)
        assert ts.dp and ts.comm == "rccl" and not ts_ref.dp
        for x, t in data:
            l0, _ = ts_ref.step(x, t)
            l1, _ = ts.step(x, t)
            torch.cuda.synchronize()
            assert l0.item() == l1.item()
        kinds = [kind for kind, bgn, end in ts._ranges if any("meter" in name for name, _, _ in ts._ops[bgn:end])]
        assert kinds == ["piece"]
        assert ts.meter.count() == float(b * len(data))
        assert _rel(_vec(ts.meter.average()), _vec(ts_ref.meter.average())) <= 1e-10
        assert _rel(_vec(ts.meter.last()), _vec(ts_ref.meter.last())) <= 1e-10
        ts.close()
    finally:
        comm.destroy()
    ts_ref.close()


def test_step_metrics_off():
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 2, 97, 161
    m, lw = _model("resnet18_latefusion", h, w)
    ts = HipTrainStep(m, b, h, w, metrics=False)
    ts.step(*_batches("resnet18_latefusion", b, h, w, 1)[0])
    torch.cuda.synchronize()
    assert ts.meter is None
    assert not [name for name, _, _ in ts._ops if "metrics" in name or "meter" in name]
    ts.close()


# ------------------------------------------------------------------------------------------------ batched validation
def test_evaluate_batch():
    from radar_depth_amd.evaluation.metrics import AverageMeter, DeviceAverageMeter, Result, evaluate_batch
    from radar_depth_amd.main import HipInference
    b, h, w = 4, 97, 161
    m, _ = _model("resnet18_latefusion", h, w)
    x, t = _batches("resnet18_latefusion", b, h, w, 1)[0]
    pred = HipInference(m, b, h, w, use_graph=False)(x)
    masks = [0b001, 0b011, 0b101, 0b111]
    dm, dm1 = DeviceAverageMeter(groups=3), DeviceAverageMeter(groups=3)
    evaluate_batch(dm, pred, t, groups=masks)
    other = pred * 1.1 + 0.3
    evaluate_batch((dm, dm1), {"stage1": pred, "stage2": other}, t, groups=masks)      # dm: stage 2 of the dict on top of the first call
    host, host2 = [AverageMeter() for _ in range(3)], [AverageMeter() for _ in range(3)]
    for k in range(b):
        for src, meters in ((pred, host), (pred, host2), (other, host2)):
            r = Result()
            r.evaluate(src[k:k + 1], t[k:k + 1])
            for g in range(3):
                if masks[k] >> g & 1:
                    meters[g].update(r, 0, 0, 1)
    worst = 0.0
    for g in range(3):
        worst = max(worst, _rel(_vec(dm1.average(g)), _vec(host[g].average())), _rel(_vec(dm.average(g)), _vec(host2[g].average())))
        assert dm1.count(g) == host[g].count
    print("evaluate_batch vs four batch-1 Result.evaluate calls: %.2e" % worst)
    assert worst <= 1e-10

"""The early-fusion ResNet (--arch resnet18 / resnet34; modality rgbd, rgb, d) on the MI355X plans, against float64 steps of the
reference (tests/golden/make_golden_resnet.py): one step per fixture case through the drop-in modules (split and fp32 plans) and the
eval forward, the fused step against the eager loop and with hipGraph replay, HipInference, a checkpoint round trip, the zero-copy
input binding, and one step at the geometry users run.  The bars are those of tests/test_gpu_decoders.py / tests/test_gpu_model.py."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# case -> (layers, decoder, channel slice of the [N,4,H,W] batch): make_golden_resnet.CASES
CASES = {"rgbd_upproj": (18, "upproj", (0, 4)), "rgb_deconv2": (18, "deconv2", (0, 3)), "d_deconv3": (18, "deconv3", (3, 4)),
         "rgbd34_upconv": (34, "upconv", (0, 4))}
OPERANDS = ("split", "fp32")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def net(case, h=97, w=161):
    from radar_depth_amd.model.models import ResNet
    from radar_depth_amd.synthetic import procedural_fill_
    layers, dec, ch = CASES[case]
    torch.manual_seed(0)
    m = ResNet(layers, dec, [h, w], ch[1] - ch[0], False)
    procedural_fill_(m)
    return m.cuda()


def batch(case, b, h, w, seed):
    from radar_depth_amd.synthetic import make_batch
    ch = CASES[case][2]
    x, t = make_batch(b, h, w, seed, ref_pixels=h * w)
    return x[:, ch[0]:ch[1]].contiguous().cuda(), t.cuda()


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("case", list(CASES))
def test_step_vs_golden(case, operands):
    """pred = model(x); loss.backward(); opt.step() against the reference's float64 step, and the eval forward on the same batch."""
    from radar_depth_amd.engine import ResNetPlan
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    want = np.load(os.path.join(GOLD, "resnet_net_%s.npz" % case))
    b, h, w = 2, 97, 161
    m = net(case, h, w)
    m.operands = operands
    x, t = batch(case, b, h, w, 4321)
    m.eval()
    with torch.no_grad():
        e_eval = rel(m(x).cpu().numpy(), want["eval_out"])
    m.train()
    opt = torch.optim.SGD(m.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    y = m(x)
    plan = m._plan(b, h, w, True, split=operands == "split")
    assert isinstance(plan, ResNetPlan) and plan.generation == 1 and plan.split == (operands == "split")
    e_train = rel(y.detach().cpu().numpy(), want["train_out"])
    loss = MaskedL1Loss()(y, t)
    e_loss = abs(loss.item() - want["loss"][0]) / want["loss"][0]
    print("resnet %s %s: eval %.2e, train %.2e, loss %.2e" % (case, operands, e_eval, e_train, e_loss))
    assert e_eval < 1e-3 and e_train < 1e-3 and e_loss < 1e-4
    opt.zero_grad()
    loss.backward()
    names = [n for n, _ in m.named_parameters()]
    assert names == list(want["param_names"])
    gn = np.array([p.grad.double().norm().item() for p in m.parameters()])
    floor = 1e-6 * want["grad_norms"].max()
    print("    worst gradient norm: %.2e" % max(abs(a - c) / c for a, c in zip(gn, want["grad_norms"])))
    bad = [(n, a, c) for n, a, c in zip(names, gn, want["grad_norms"]) if abs(a - c) > 1e-2 * c + floor]
    assert not bad, bad[:8]
    opt.step()
    pn = np.array([p.double().norm().item() for p in m.parameters()])
    assert np.abs(pn - want["param_norms1"]).max() / want["param_norms1"].max() < 1e-4
    assert rel(m.bn1.running_mean.cpu().numpy(), want["bn1_running_mean"]) < 1e-4
    assert rel(m.bn1.running_var.cpu().numpy(), want["bn1_running_var"]) < 1e-4
    assert all(int(v) == 1 for k, v in m.state_dict().items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("case", ["rgbd_upproj", "rgb_deconv2"])
def test_fused_step_matches_eager_loop(case):
    """HipTrainStep (fused loss + backward + SGD on the split plan) and the eager loop on the same split plan: losses and parameters
    within 1e-6 of their magnitude after three steps (the loss reduction and the update come from different kernels on the two routes)."""
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 2, 97, 161
    fused, eager = net(case, h, w).train(), net(case, h, w).train()
    ts = HipTrainStep(fused, b, h, w, lr=0.01, momentum=0.9, weight_decay=1e-4, use_graph=False, operands="split")
    opt = torch.optim.SGD(eager.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    crit = MaskedL1Loss()
    for it in range(3):
        x, t = batch(case, b, h, w, 55 + it)
        lf, _ = ts.step(x, t)
        le = crit(eager(x), t)
        opt.zero_grad()
        le.backward()
        opt.step()
        torch.cuda.synchronize()
        assert abs(lf.item() - le.item()) <= 1e-6 * abs(le.item()), (it, lf.item(), le.item())
    for (n, p), q in zip(fused.named_parameters(), eager.parameters()):
        assert torch.equal(p, q) or (p - q).abs().max().item() <= 1e-6 * q.abs().max().item(), n


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("case", ["rgbd_upproj", "rgb_deconv2"])
def test_graph_replay_equals_plain_launches(case, operands):
    """use_graph=True (replay from the second call on) against use_graph=False over three steps: equal losses, equal parameters."""
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 2, 97, 161
    mg, mp = net(case, h, w), net(case, h, w)
    tg = HipTrainStep(mg, b, h, w, use_graph=True, operands=operands)
    tp = HipTrainStep(mp, b, h, w, use_graph=False, operands=operands)
    for it in range(3):
        x, t = batch(case, b, h, w, 300 + it)
        lg, _ = tg.step(x, t)
        lp, _ = tp.step(x, t)
        torch.cuda.synchronize()
        assert lg.item() == lp.item(), (it, lg.item(), lp.item())
    assert tg.graphs is not None and tp.graphs is None
    for (n, p), q in zip(mg.named_parameters(), mp.parameters()):
        assert torch.equal(p, q), n


@pytest.mark.parametrize("case", ["rgbd_upproj", "d_deconv3"])
def test_inference_equals_eval_forward(case):
    from radar_depth_amd.main import HipInference
    h, w = 97, 161
    m = net(case, h, w).eval()
    inf = HipInference(m, 1, h, w)
    for it in range(3):          # (plain launches, capture, replay)
        x, _ = batch(case, 1, h, w, 5 + it)
        with torch.no_grad():
            want = m(x)
        got = inf(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, want), it


@pytest.mark.parametrize("case", ["rgb_deconv2", "rgbd34_upconv"])
def test_checkpoint_round_trip(case):
    """state_dict save / load into a fresh module: identical keys and tensors, identical eval-mode forward."""
    from radar_depth_amd.model.models import ResNet
    h, w = 97, 161
    layers, dec, ch = CASES[case]
    m = net(case, h, w).eval()
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    m2 = ResNet(layers, dec, [h, w], ch[1] - ch[0], False)
    m2.load_state_dict(torch.load(buf, map_location="cpu", weights_only=True))
    m2 = m2.cuda().eval()
    assert list(m2.state_dict()) == list(m.state_dict())
    x, _ = batch(case, 1, h, w, 5)
    with torch.no_grad():
        a, b_ = m(x), m2(x)
    assert torch.equal(a, b_)


def test_zero_copy_input_binding(monkeypatch):
    """A contiguous caller-owned [N,4,H,W] batch is read in place (the stem's four plane pointers are re-pointed); the copying route
    (RD_ZERO_COPY_INPUT=0) gives the same losses and parameters."""
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 2, 97, 161
    mz, mc = net("rgbd_upproj", h, w), net("rgbd_upproj", h, w)
    tz = HipTrainStep(mz, b, h, w)
    monkeypatch.setenv("RD_ZERO_COPY_INPUT", "0")
    tc = HipTrainStep(mc, b, h, w)
    assert tz._zero_copy and not tc._zero_copy
    for it in range(2):
        x, t = batch("rgbd_upproj", b, h, w, 800 + it)
        lz, _ = tz.step(x, t)
        lc, _ = tc.step(x, t)
        torch.cuda.synchronize()
        assert tz.plan._x_bound == x.data_ptr() and tc.plan._x_bound == tc.plan.x_in.data_ptr()
        assert lz.item() == lc.item()
    for p, q in zip(mz.parameters(), mc.parameters()):
        assert torch.equal(p, q)


def test_data_parallel_path_single_rank(monkeypatch):
    """The data-parallel code path (one hipGraph per backward segment or plain launches, an all-reduce per gradient bucket, SGD scaled
    by 1/world) on a 1-rank nccl group reproduces the single-GPU step exactly: the plan's four buckets cover every parameter."""
    import torch.distributed as dist
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 2, 97, 161
    case = "rgbd_upproj"
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29623")
    ref = net(case, h, w)
    ts_ref = HipTrainStep(ref, b, h, w, use_graph=True)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        monkeypatch.setenv("RD_FORCE_DP", "1")
        m, m2 = net(case, h, w), net(case, h, w)
        ts = HipTrainStep(m, b, h, w, use_graph=True)
        ts2 = HipTrainStep(m2, b, h, w)
        assert ts.dp and ts2.dp and len(ts._buckets) == 4
        for it in range(3):
            x, t = batch(case, b, h, w, 300 + it)
            l0, _ = ts_ref.step(x, t)
            l1, _ = ts.step(x, t)
            l2, _ = ts2.step(x, t)
            torch.cuda.synchronize()
            assert l0.item() == l1.item() == l2.item()
        for p, q, r in zip(ref.parameters(), m.parameters(), m2.parameters()):
            assert torch.equal(p, q) and torch.equal(p, r)
    finally:
        dist.destroy_process_group()


def test_wrong_channel_count_raises():
    m = net("rgb_deconv2").eval()
    with pytest.raises(RuntimeError, match="expected input"):
        m(torch.zeros(1, 4, 97, 161, device="cuda"))


def test_full_geometry_two_steps():
    """(18, rgbd, upproj) at b = 16, 450x800: two fused split steps, loss and every parameter finite; the first-step loss within 1e-3 of
    the fp32-operand plan's on the same batch."""
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 16, 450, 800
    losses = {}
    for operands in ("split", "fp32"):
        m = net("rgbd_upproj", h, w)
        ts = HipTrainStep(m, b, h, w, operands=operands)
        x, t = batch("rgbd_upproj", b, h, w, 42)
        l1, _ = ts.step(x, t)
        torch.cuda.synchronize()
        losses[operands] = l1.item()
        if operands == "split":
            l2, _ = ts.step(x, t)
            torch.cuda.synchronize()
            assert np.isfinite(l1.item()) and np.isfinite(l2.item())
            assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
        ts.close()
        del ts, m
        torch.cuda.empty_cache()
    print("full geometry: split %.6f, fp32 %.6f" % (losses["split"], losses["fp32"]))
    assert abs(losses["split"] - losses["fp32"]) <= 1e-3 * abs(losses["fp32"])

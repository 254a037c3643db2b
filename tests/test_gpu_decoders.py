"""The deconv2 / deconv3 / upconv decoders on the MI355X plans, against vectors generated from the reference
(tests/golden/make_golden_decoders.py): stand-alone decoders, one resnet18_latefusion step per decoder (split and fp32 plans),
the eval forward, one multistage deconv3 step, the fused step against the eager loop, and a checkpoint round trip."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECODERS = ("deconv2", "deconv3", "upconv")
OPERANDS = ("split", "fp32")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def module_inputs(y_shape=None):
    """Same counter-based inputs as make_golden_decoders.module_inputs."""
    from radar_depth_amd.synthetic import normal01
    shape = (2, 256, 3, 3)
    x = torch.from_numpy(normal01(int(np.prod(shape)), 31).reshape(shape)).float()
    if y_shape is None:
        return x
    return x, torch.from_numpy(normal01(int(np.prod(y_shape)), 32).reshape(y_shape)).float()


def net(dec, h=97, w=161):
    from radar_depth_amd.model.models import ResNet_latefusion
    from radar_depth_amd.synthetic import procedural_fill_
    torch.manual_seed(0)
    m = ResNet_latefusion(18, dec, [h, w], 4, False)
    procedural_fill_(m)
    return m.cuda()


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("dec", DECODERS)
def test_standalone_decoder_vs_golden(dec, operands):
    """DeConv(256, k) / UpConv(256) called on their own: output, input gradient, every parameter gradient and the running statistics,
    at 1e-4 of each tensor's max (the UpProj module test's bar)."""
    from radar_depth_amd.model.models import choose_decoder
    from radar_depth_amd.synthetic import procedural_fill_
    want = np.load(os.path.join(GOLD, "decoders_module_%s.npz" % dec))
    m = choose_decoder(dec, 256)
    procedural_fill_(m)
    m = m.cuda().train()
    m.operands = operands
    x = module_inputs().cuda().requires_grad_(True)
    y = m(x)
    assert rel(y.detach().cpu().numpy(), want["y"]) < 1e-4
    _, gy = module_inputs(tuple(y.shape))
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    assert rel(x.grad.cpu().numpy(), want["gx"]) < 1e-4
    for n, p in m.named_parameters():
        g = p.grad.cpu().numpy().ravel()
        assert abs(np.abs(g).max() - want["gmax/" + n][0]) <= 1e-4 * want["gmax/" + n][0], n
        assert np.abs(g[::int(want["gstride/" + n][0])] - want["grad/" + n]).max() <= 1e-4 * want["gmax/" + n][0], n
    sd = m.state_dict()
    for k in want.files:
        if k.startswith("buf/"):
            assert rel(sd[k[4:]].cpu().numpy(), want[k]) < 1e-4, k


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("dec", DECODERS)
def test_latefusion_step_vs_golden(dec, operands):
    """One resnet18_latefusion step through the drop-in surface (pred = model(x); loss.backward(); opt.step()) against the reference's
    float64 step, at the fp32 bars of the existing configuration tests; and the eval forward on the same batch."""
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    from radar_depth_amd.synthetic import make_batch
    want = np.load(os.path.join(GOLD, "decoders_net_%s.npz" % dec))
    b, h, w = 2, 97, 161
    m = net(dec, h, w)
    m.operands = operands
    x, t = make_batch(b, h, w, 4321, ref_pixels=h * w)
    x, t = x.cuda(), t.cuda()
    m.eval()
    with torch.no_grad():
        assert rel(m(x).cpu().numpy(), want["eval_out"]) < 1e-3
    m.train()
    opt = torch.optim.SGD(m.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    y = m(x)
    plan = m._plan(b, h, w, True, split=operands == "split")
    assert plan.generation == 1 and plan.split == (operands == "split")
    assert rel(y.detach().cpu().numpy(), want["train_out"]) < 1e-3
    loss = MaskedL1Loss()(y, t)
    assert abs(loss.item() - want["loss"][0]) / want["loss"][0] < 1e-4
    opt.zero_grad()
    loss.backward()
    names = [n for n, _ in m.named_parameters()]
    assert names == list(want["param_names"])
    gn = np.array([p.grad.double().norm().item() for p in m.parameters()])
    floor = 1e-6 * want["grad_norms"].max()
    bad = [(n, a, c) for n, a, c in zip(names, gn, want["grad_norms"]) if abs(a - c) > 1e-2 * c + floor]
    assert not bad, bad[:8]
    opt.step()
    pn = np.array([p.double().norm().item() for p in m.parameters()])
    assert np.abs(pn - want["param_norms1"]).max() / want["param_norms1"].max() < 1e-4


def test_multistage_deconv3_vs_golden():
    """ResNet_multistage with deconv3 + the uncertainty-weighted loss (main.py:416-429): the four loss terms, the stage weights'
    gradients, per-parameter gradient norms (stage 2 -> stage 1 coupling included) and a finite update."""
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss, SmoothnessLoss
    from radar_depth_amd.model.multistage_model import ResNet_multistage
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    want = np.load(os.path.join(GOLD, "decoders_ms_deconv3.npz"))
    b, h, w = 2, 97, 161
    torch.manual_seed(0)
    m = ResNet_multistage(18, "deconv3", [h, w], False)
    w1, w2 = torch.nn.Parameter(torch.tensor(1.0)), torch.nn.Parameter(torch.tensor(1.0))
    m.register_parameter("w_stage1", w1)
    m.register_parameter("w_stage2", w2)
    procedural_fill_(m)
    m = m.cuda().train()
    x, t = make_batch(b, h, w, 777, ref_pixels=h * w)
    x[:, 3, ::7, ::11] = torch.where(x[:, 3, ::7, ::11] > 0, x[:, 3, ::7, ::11], torch.full_like(x[:, 3, ::7, ::11], 60.0))
    x, t = x.cuda(), t.cuda()
    assert [n for n, _ in m.named_parameters()] == list(want["param_names"])
    opt = torch.optim.SGD(m.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    crit, smooth = MaskedL1Loss(), SmoothnessLoss()
    o = m(x)
    p1, p2 = o["stage1"], o["stage2"]
    d1, d2, sm = crit(p1, t), crit(p2, t), smooth(p1, x)
    W1, W2 = m.w_stage1, m.w_stage2
    loss = torch.exp(-W1) * (d1 + 0.1 * sm) + torch.exp(-W2) * d2 + (W1 + W2)
    got = np.array([d1.item(), d2.item(), sm.item(), loss.item()])
    assert np.abs(got - want["losses"]).max() / np.abs(want["losses"]).max() < 1e-4, (got, want["losses"])
    opt.zero_grad()
    loss.backward()
    assert np.abs(np.array([W1.grad.item(), W2.grad.item()]) - want["w_grads"]).max() < 1e-4 * np.abs(want["w_grads"]).max()
    gn = np.array([p.grad.double().norm().item() for p in m.parameters()])
    floor = 1e-6 * want["grad_norms"].max()
    bad = [(n, a, c) for n, a, c in zip(want["param_names"], gn, want["grad_norms"]) if abs(a - c) > 2e-2 * c + floor]
    assert not bad, bad[:8]
    opt.step()
    pn = np.array([p.double().norm().item() for p in m.parameters()])
    assert np.isfinite(pn).all()
    assert np.abs(pn - want["param_norms1"]).max() / want["param_norms1"].max() < 1e-4


@pytest.mark.parametrize("dec", DECODERS)
def test_fused_step_matches_eager_loop(dec):
    """HipTrainStep (fused loss + backward + SGD on the split plan) and the eager loop (model(x); loss.backward(); opt.step()) on the
    same split plan leave the same parameters after two steps.  Not bit for bit: the two routes share every convolution / BatchNorm
    launch, but the loss and its gradient come from the fused loss kernel on one route and from torch's MaskedL1Loss (another reduction
    order) on the other, and the update from the fused SGD kernel vs torch.optim.SGD; hence 1e-6 of each tensor's magnitude."""
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    from radar_depth_amd.main import HipTrainStep
    from radar_depth_amd.synthetic import make_batch
    b, h, w = 2, 97, 161
    fused, eager = net(dec, h, w).train(), net(dec, h, w).train()
    ts = HipTrainStep(fused, b, h, w, lr=0.01, momentum=0.9, weight_decay=1e-4, use_graph=False, operands="split")
    opt = torch.optim.SGD(eager.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    crit = MaskedL1Loss()
    for it in range(2):
        x, t = make_batch(b, h, w, 55 + it, ref_pixels=h * w)
        x, t = x.cuda(), t.cuda()
        lf, _ = ts.step(x, t)
        le = crit(eager(x), t)
        opt.zero_grad()
        le.backward()
        opt.step()
        torch.cuda.synchronize()
        assert abs(lf.item() - le.item()) <= 1e-6 * abs(le.item()), (it, lf.item(), le.item())
    for (n, p), q in zip(fused.named_parameters(), eager.parameters()):
        assert torch.equal(p, q) or (p - q).abs().max().item() <= 1e-6 * q.abs().max().item(), n


@pytest.mark.parametrize("dec", DECODERS)
def test_checkpoint_round_trip(dec):
    """state_dict save / load into a fresh module: identical keys and tensors, identical eval-mode forward."""
    from radar_depth_amd.model.models import ResNet_latefusion
    from radar_depth_amd.synthetic import make_batch
    h, w = 97, 161
    m = net(dec, h, w).eval()
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    m2 = ResNet_latefusion(18, dec, [h, w], 4, False)
    m2.load_state_dict(torch.load(buf, map_location="cpu", weights_only=True))
    m2 = m2.cuda().eval()
    assert list(m2.state_dict()) == list(m.state_dict())
    x, _ = make_batch(1, h, w, 5, ref_pixels=h * w)
    with torch.no_grad():
        a, b_ = m(x.cuda()), m2(x.cuda())
    assert torch.equal(a, b_)

"""End-to-end GPU parity of the HIP-backed ResNet_latefusion against the golden vectors generated from the real
reference (tests/golden/*.npz) and against the CPU oracle run live.

Tolerances (fp32): forward maps <= 1e-3 relative to the map's max magnitude (BASELINE.json north_star; measured
~2e-5), per-module statistics <= 2e-3, loss <= 1e-4.  Gradients: each backward kernel is verified to <= 5e-5 in
tests/test_gpu_{gconv,wgrad,norm}.py; END-TO-END gradients are limited by conditioning, not by the kernels -- a
forward difference of 1e-5 flips the ReLU mask of an element that is ~0 in the reference, and on the small test
geometry (4x6 bottleneck, 192 rows per BN channel) one such flip moves downstream gradients by up to a few percent
(tools/diag_bwd.py measures exactly one flip, at |z| = 3e-6 of the map's max, with the fp32 CPU oracle showing the
same behaviour against an fp64 oracle).  Hence: gradient norms <= 1e-2, gradient elements <= 3e-2 of the tensor max."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def stats(t):
    t = t.float()
    return np.array([t.mean().item(), t.abs().mean().item(), t.abs().max().item()])


def tap_stats(plan, gold_name):
    """Statistic triplet of the plan tensor that corresponds to a reference leaf-module output."""
    taps = plan.taps
    if gold_name in taps:
        return stats(taps[gold_name].view())
    parts = gold_name.split(".")
    if parts[-1] == "relu" and ".".join(parts[:-1]) in taps:            # block / UpProj module output
        return stats(taps[".".join(parts[:-1])].view())
    if gold_name.endswith("upper_branch.conv1") or gold_name.endswith("bottom_branch.conv"):
        base = ".".join(parts[:2]) + ".conv5x5"
        a = taps[base]
        half = a.C // 2
        return stats(a.chan(0, half).view() if "upper" in gold_name else a.chan(half, half).view())
    return None


def build(h, w):
    from radar_depth_amd.model.models import ResNet_latefusion
    from radar_depth_amd.synthetic import procedural_fill_
    torch.manual_seed(0)
    m = ResNet_latefusion(18, "upproj", [h, w], 4, False)
    procedural_fill_(m)
    return m.cuda()


def run_case(npz, batch, h, w, seed, sub, dense_small, fwd_tol=1e-3, operands="split"):
    """The reference's loop body (main.py:440-445) through the drop-in surface: pred = model(x); loss = criterion(pred, t);
    optimizer.zero_grad(); loss.backward(); optimizer.step() -- on the module's eager plan, `operands` = its arithmetic
    (model.operands: "split", the default since round 6, or "fp32")."""
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    from radar_depth_amd.synthetic import make_batch
    want = np.load(os.path.join(GOLD, npz))
    m = build(h, w)
    m.operands = operands
    ref_px = h * w if dense_small else 450 * 800
    x, t = make_batch(batch, h, w, seed, ref_pixels=ref_px)
    x, t = x.cuda(), t.cuda()
    crit = MaskedL1Loss()
    m.eval()
    with torch.no_grad():
        y_eval = m(x)
    assert rel(y_eval.cpu().numpy()[:, :, ::sub, ::sub], want["eval_out"]) < fwd_tol

    m.train()
    opt = torch.optim.SGD(m.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    y = m(x)
    plan = m._plan(batch, h, w, True, split=operands == "split")
    assert plan.generation == 1 and plan.split == (operands == "split")      # the plan the call above ran on, not a fresh one
    torch.cuda.synchronize()
    # per-module statistics: localises any divergence to a layer
    worst = ("", 0.0)
    checked = 0
    for name, val in zip(want["stat_names"], want["stat_values"]):
        got = tap_stats(plan, str(name))
        if got is None:
            continue
        checked += 1
        err = np.abs(got - val).max() / max(np.abs(val).max(), 1e-6)
        if err > worst[1]:
            worst = (str(name), err)
        assert err < 2e-3, (str(name), got, val)
    assert checked >= 60, checked
    assert rel(y.detach().cpu().numpy()[:, :, ::sub, ::sub], want["train_out"]) < fwd_tol, worst
    loss = crit(y, t)
    assert abs(loss.item() - want["loss"][0]) / want["loss"][0] < 1e-4
    opt.zero_grad()
    loss.backward()
    names = [n for n, _ in m.named_parameters()]
    assert names == list(want["param_names"])
    gn = np.array([p.grad.double().norm().item() for p in m.parameters()])
    # bn_fusion.bias has an exactly-zero true gradient (a per-channel constant in front of a training-mode BN): its
    # computed value is roundoff noise on both sides, hence the absolute floor relative to the overall gradient scale
    floor = 1e-6 * want["grad_norms"].max()
    bad = [(n, a, b) for n, a, b in zip(names, gn, want["grad_norms"]) if abs(a - b) > 1e-2 * b + floor]
    assert not bad, bad[:8]
    for k in want.files:
        if k.startswith("grad/"):
            g = dict(m.named_parameters())[k[5:]].grad.cpu().numpy()
            assert np.abs(g - want[k]).max() <= 3e-2 * np.abs(want[k]).max() + 1e-9, k
    opt.step()
    sd = m.state_dict()
    for k in want.files:
        if k.startswith("buf1/"):
            assert rel(sd[k[5:]].cpu().numpy(), want[k]) < 1e-3, k
    assert int(sd["bn1.num_batches_tracked"]) == int(want["nbt1"][0])
    x2, t2 = make_batch(batch, h, w, seed + 1, ref_pixels=ref_px)
    y2 = m(x2.cuda())
    loss2 = crit(y2, t2.cuda())
    opt.zero_grad()
    loss2.backward()
    opt.step()
    assert abs(loss2.item() - want["loss2"][0]) / want["loss2"][0] < 2e-3
    pn = np.array([p.double().norm().item() for p in m.parameters()])
    assert np.abs(pn - want["param_norms2"]).max() / want["param_norms2"].max() < 1e-4
    for k in want.files:
        if k.startswith("param2/"):
            assert rel(dict(m.named_parameters())[k[7:]].detach().cpu().numpy(), want[k]) < 3e-2, k   # two SGD steps on conditioning-limited gradients (see module docstring)
    return m


@pytest.mark.parametrize("operands", ["split", "fp32"])
def test_latefusion_small_vs_golden(operands):
    run_case("latefusion_small.npz", 2, 97, 161, 4321, 1, True, operands=operands)


@pytest.mark.parametrize("operands", ["split", "fp32"])
def test_latefusion_full_vs_golden(operands):
    run_case("latefusion_full.npz", 2, 450, 800, 1234, 8, False, operands=operands)


def test_eager_default_is_the_split_plan(monkeypatch):
    """`pred = model(x)` runs the plan the headline is measured on unless told otherwise (model.operands / RD_EAGER_OPERANDS)."""
    from radar_depth_amd.model import models
    m = build(64, 96)
    assert models.eager_operands(m) == "split" and models.eager_operands(m.layer1[0]) == "split"
    m.operands = "fp32"
    assert models.eager_operands(m) == "fp32" and models.eager_operands(m.layer1[0]) == "fp32"      # sub-modules follow their network
    del m.operands
    monkeypatch.setenv("RD_EAGER_OPERANDS", "fp32")
    assert models.eager_operands(m) == "fp32"
    monkeypatch.delenv("RD_EAGER_OPERANDS")
    x = torch.rand(1, 4, 64, 96, device="cuda")
    m.train()
    m(x)
    plans = list(m.__dict__["_plans"].values())
    assert len(plans) == 1 and plans[0].split
    m.operands = "bogus"
    with pytest.raises(ValueError):
        m(x)


def test_fused_step_matches_oracle():
    """HipTrainStep (fused loss + backward + SGD, graph replay from step 2) against the CPU oracle for 3 steps."""
    from oracle.criteria import MaskedL1Loss as OL1
    from oracle.models import ResNet_latefusion as ORef
    from radar_depth_amd.main import HipTrainStep
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    b, h, w = 2, 97, 161
    m = build(h, w)
    torch.manual_seed(0)
    o = ORef(18, "upproj", [h, w], 4, False)
    procedural_fill_(o)
    o.train()
    opt = torch.optim.SGD(o.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    ts = HipTrainStep(m, b, h, w, lr=0.01, momentum=0.9, weight_decay=1e-4, use_graph=True)
    crit = OL1()
    for it in range(3):
        x, t = make_batch(b, h, w, 99 + it, ref_pixels=h * w)
        lo = crit(o(x), t)
        opt.zero_grad()
        lo.backward()
        opt.step()
        lg, pred = ts.step(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        assert abs(lg.item() - lo.item()) / lo.item() < 2e-3, (it, lg.item(), lo.item())
    po = np.array([p.double().norm().item() for p in o.parameters()])
    pg = np.array([p.double().norm().item() for p in m.parameters()])
    assert np.abs(po - pg).max() / po.max() < 5e-3
    # Element-wise comparison after several steps is only meaningful for well-conditioned tensors: the reference network is
    # chaotic in its multi-step trajectory (tests/test_conditioning.py: a 5e-4 weight perturbation moves the next step's
    # gradients by ~20 % in the CPU oracle itself), so only the head weight is compared element-wise.
    a_, c_ = m.conv3.weight.detach().cpu().double(), o.conv3.weight.detach().double()
    assert ((a_ - c_).norm() / c_.norm()).item() < 5e-3


def test_no_cpu_fallback():
    from radar_depth_amd.model.models import ResNet_latefusion
    m = ResNet_latefusion(18, "upproj", [97, 161], 4, False)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 4, 97, 161))


def test_multistage_vs_golden():
    """ResNet_multistage + uncertainty-weighted loss (main.py:416-429): outputs, mask, losses, w gradients, stage coupling,
    parameter norms after one SGD step, through the torch.autograd-compatible path."""
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss, SmoothnessLoss
    from radar_depth_amd.model.multistage_model import ResNet_multistage
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    want = np.load(os.path.join(GOLD, "multistage_small.npz"))
    b, h, w = 2, 97, 161
    torch.manual_seed(0)
    m = ResNet_multistage(18, "upproj", [h, w], False)
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
    for k in ("stage1", "stage2", "radar_filtered"):
        assert rel(o[k].detach().cpu().numpy(), want["out/" + k]) < 1e-3, k
    assert (o["mask"].cpu().numpy() != want["out/mask"]).mean() < 1e-4
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
    for k in ("stage1.conv3.weight", "stage2.conv1_depth.weight"):
        g = dict(m.named_parameters())[k].grad.cpu().numpy()
        assert np.abs(g - want["grad/" + k]).max() <= 3e-2 * np.abs(want["grad/" + k]).max(), k
    opt.step()
    pn = np.array([p.double().norm().item() for p in m.parameters()])
    assert np.abs(pn - want["param_norms1"]).max() / want["param_norms1"].max() < 1e-4


@pytest.mark.slow
def test_multistage_fused_step_matches_oracle():
    """HipTrainStep on resnet18_multistage_uncertainty_fixs (fused losses, stage coupling, SGD incl. w_stage1/2) vs the oracle."""
    import types

    from oracle import train as otrain
    from radar_depth_amd import main as hmain
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    b, h, w = 2, 97, 161
    args = types.SimpleNamespace(arch="resnet18_multistage_uncertainty_fixs", decoder="upproj", modality="rgbd", pretrained=False)
    torch.manual_seed(0)
    hm, hw_ = hmain.create_model(args, [h, w])
    om, ow = otrain.create_model(args, [h, w])
    procedural_fill_(hm)
    procedural_fill_(om)
    hm = hm.cuda()
    om.train()
    opt = torch.optim.SGD(om.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    crit = otrain.make_criterion(args.arch)
    ts = hmain.HipTrainStep(hm, b, h, w, lr=0.01, momentum=0.9, weight_decay=1e-4, loss_weights=hw_, use_graph=True)
    for it in range(3):
        x, t = make_batch(b, h, w, 500 + it, ref_pixels=h * w)
        lo, _, _ = otrain.train_step(args.arch, om, crit, opt, x, t, ow)
        lg, _ = ts.step(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        assert abs(lg.item() - lo.item()) / abs(lo.item()) < 2e-3, (it, lg.item(), lo.item())
    assert abs(hm.w_stage1.item() - om.w_stage1.item()) < 1e-3 and abs(hm.w_stage2.item() - om.w_stage2.item()) < 1e-3   # 3 chaotic steps, losses agree to 2e-3
    po = np.array([p.double().norm().item() for p in om.parameters()])
    pg = np.array([p.double().norm().item() for p in hm.parameters()])
    assert np.abs(po - pg).max() / po.max() < 5e-3          # 3 chaotic steps (tests/test_conditioning.py)


def test_step_is_bitwise_reproducible_under_concurrency():
    """Two identically initialised models stepped on the same batches must stay bit-identical: the step runs ~650 kernels on
    three streams, so any race in a kernel's own synchronisation (e.g. reading an LDS buffer an asynchronous copy has not
    finished filling) or a missing cross-stream edge shows up as a last-bit difference here."""
    from radar_depth_amd.main import HipTrainStep
    from radar_depth_amd.synthetic import make_batch
    b, h, w = 5, 97, 161        # the geometry at which uninitialised-LDS NaNs in the strip weight-gradient kernel first showed
    m1, m2 = build(h, w), build(h, w)
    t1, t2 = HipTrainStep(m1, b, h, w), HipTrainStep(m2, b, h, w)
    for it in range(10):
        x, t = make_batch(b, h, w, 900 + it, ref_pixels=h * w)
        l1, _ = t1.step(x.cuda(), t.cuda())
        l2, _ = t2.step(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        assert l1.item() == l2.item(), it
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p, q)


def test_data_parallel_path_single_rank(monkeypatch):
    """The DP code path (one hipGraph per backward segment, async RCCL all-reduce per gradient bucket, wait, SGD scaled by
    1/world) on a 1-rank nccl group must reproduce the single-graph step exactly."""
    import torch.distributed as dist
    from radar_depth_amd.main import HipTrainStep
    from radar_depth_amd.synthetic import make_batch
    b, h, w = 2, 97, 161
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29611")
    ref = build(h, w)
    ts_ref = HipTrainStep(ref, b, h, w, use_graph=True)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        monkeypatch.setenv("RD_FORCE_DP", "1")
        m, m2 = build(h, w), build(h, w)
        ts = HipTrainStep(m, b, h, w, use_graph=True)         # data-parallel path as segment graphs
        ts2 = HipTrainStep(m2, b, h, w)                       # ... and as plain stream launches (the default)
        assert ts.dp and ts2.dp
        ts._build_table()
        assert sum(1 for kind, _, _ in ts._ranges if kind == "piece") == len(ts._buckets) + 1
        for it in range(3):
            x, t = make_batch(b, h, w, 300 + it, ref_pixels=h * w)
            l0, _ = ts_ref.step(x.cuda(), t.cuda())
            l1, _ = ts.step(x.cuda(), t.cuda())
            l2, _ = ts2.step(x.cuda(), t.cuda())
            torch.cuda.synchronize()
            assert l0.item() == l1.item() == l2.item()
        for p, q, r in zip(ref.parameters(), m.parameters(), m2.parameters()):
            assert torch.equal(p, q) and torch.equal(p, r)
    finally:
        dist.destroy_process_group()


def test_checkpoint_loads_and_eval_forward_matches_oracle():
    """A reference-format state_dict loaded into the HIP module reproduces the oracle's eval-mode forward (running-stat BN)."""
    from oracle.models import ResNet_latefusion as ORef
    from radar_depth_amd.model.models import ResNet_latefusion
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    h, w = 97, 161
    o = ORef(18, "upproj", [h, w], 4, False)
    procedural_fill_(o)
    o.eval()
    m = ResNet_latefusion(18, "upproj", [h, w], 4, False)
    m.load_state_dict(o.state_dict())
    m = m.cuda().eval()
    x, _ = make_batch(1, h, w, 5, ref_pixels=h * w)          # validate() uses batch size 1 (main.py:636)
    with torch.no_grad():
        want = o(x)
        got = m(x.cuda())
    assert rel(got.cpu().numpy(), want.numpy()) < 1e-3


def test_large_geometry_900x1600():
    """configs[4] geometry (900x1600, 4x the activations of 450x800): forward + loss + gradient norms vs the CPU oracle, b=1."""
    from oracle.criteria import MaskedL1Loss as OL1
    from oracle.models import ResNet_latefusion as ORef
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    h, w = 900, 1600
    m = build(h, w).train()
    torch.manual_seed(0)
    o = ORef(18, "upproj", [h, w], 4, False)
    procedural_fill_(o)
    o.train()
    x, t = make_batch(1, h, w, 31)
    yo = o(x)
    lo = OL1()(yo, t)
    lo.backward()
    y = m(x.cuda())
    lg = MaskedL1Loss()(y, t.cuda())
    lg.backward()
    assert rel(y.detach().cpu().numpy(), yo.detach().numpy()) < 1e-3
    assert abs(lg.item() - lo.item()) / lo.item() < 1e-4
    go = np.array([p.grad.double().norm().item() for p in o.parameters()])
    gg = np.array([p.grad.double().norm().item() for p in m.parameters()])
    assert np.abs(go - gg).max() / go.max() < 2e-2


def test_inference_graph_matches_module_forward():
    """HipInference (graph-captured eval forward, folded BatchNorm) == module.eval()(x) == oracle eval forward."""
    from oracle.models import ResNet_latefusion as ORef
    from radar_depth_amd.main import HipInference
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    h, w = 97, 161
    m = build(h, w).eval()
    o = ORef(18, "upproj", [h, w], 4, False)
    procedural_fill_(o)
    o.eval()
    inf = HipInference(m, 2, h, w)
    for it in range(3):
        x, _ = make_batch(2, h, w, 40 + it, ref_pixels=h * w)
        got = inf(x.cuda()).clone()
        with torch.no_grad():
            want = o(x)
            direct = m(x.cuda())
        torch.cuda.synchronize()
        assert rel(got.cpu().numpy(), want.numpy()) < 1e-3, it
        assert torch.equal(got, direct)


@pytest.mark.parametrize("b,h,w", [(1, 97, 161), (3, 64, 64), (1, 131, 77), (2, 228, 304), (5, 50, 90)])
def test_geometries_forward_backward_vs_oracle(b, h, w):
    """Edge geometries (batch 1, odd batch, square, portrait, NYU-sized, small): train-mode forward + loss + gradient norms
    against the CPU oracle.  Exercises ragged tiles of every conv plan, odd pooled sizes and the stride-2 parity phases."""
    from oracle.criteria import MaskedL1Loss as OL1
    from oracle.models import ResNet_latefusion as ORef
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    m = build(h, w).train()
    torch.manual_seed(0)
    o = ORef(18, "upproj", [h, w], 4, False)
    procedural_fill_(o)
    o.train()
    x, t = make_batch(b, h, w, 900 + b, ref_pixels=h * w)
    yo = o(x)
    lo = OL1()(yo, t)
    lo.backward()
    y = m(x.cuda())
    lg = MaskedL1Loss()(y, t.cuda())
    lg.backward()
    assert rel(y.detach().cpu().numpy(), yo.detach().numpy()) < 1e-3
    assert abs(lg.item() - lo.item()) / lo.item() < 1e-4
    go = np.array([p.grad.double().norm().item() for p in o.parameters()])
    gg = np.array([p.grad.double().norm().item() for p in m.parameters()])
    # small bottlenecks (2x2 ... 8x10 pixels) make deep gradients very sensitive to single ReLU flips: compare the
    # well-conditioned tail of the network tightly and everything else loosely
    names = [n for n, _ in o.named_parameters()]
    tail = [i for i, n in enumerate(names) if n.startswith(("decoder.layer4", "decoder.layer3", "conv3"))]
    assert np.abs(go[tail] - gg[tail]).max() / go[tail].max() < 1e-3
    assert np.abs(go - gg).max() / go.max() < 0.1


def test_eager_multistage_forward_backward_is_bitwise_reproducible():
    """The autograd (eager plan) path of the multistage network at config 4's geometry, repeated in one process: outputs (the radar
    filter's mask included -- it turns a one-ulp difference of stage 1 into a percent-level change of stage 2) and every parameter
    gradient must be bit-identical every time.  This is the detector that found the missing LDS wait in front of the pipelined
    gconv loop's barrier (tools/stress_eager.py is the long form)."""
    import types
    from radar_depth_amd.main import create_model
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    b, h, w = 2, 450, 800
    args = types.SimpleNamespace(arch="resnet18_multistage_uncertainty_fixs", decoder="upproj", modality="rgbd", pretrained=False)
    torch.manual_seed(0)
    m, _ = create_model(args, [h, w])
    procedural_fill_(m)
    m = m.cuda().train()
    x, _ = make_batch(b, h, w, 77, ref_pixels=h * w)
    x = x.cuda()
    ref = None
    for it in range(12):
        m.zero_grad(set_to_none=True)
        o = m(x)
        keys = [k for k in sorted(o) if torch.is_tensor(o[k])]
        sum(o[k].float().mean() for k in keys if o[k].dtype.is_floating_point).backward()
        torch.cuda.synchronize()
        cur = [o[k].detach().clone() for k in keys] + [p.grad.detach().clone() for p in m.parameters() if p.grad is not None]
        if ref is None:
            ref = cur
        else:
            assert all(torch.equal(a_, b_) for a_, b_ in zip(ref, cur)), "repetition %d differs" % it
        junk = [torch.empty(int(1e6 * (1 + (it * 7 + k) % 5)), device="cuda") for k in range(3)]      # shuffle the allocator
        del junk


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_batched_slab_reductions_step_is_bit_identical(monkeypatch, storage):
    """RD_WGRAD_REDUCE_BATCH=4 (rd_wgrad_reduce_batched: the slab reductions of several weight tensors in two launches) against the
    default one-reduction-per-tensor plan: same summation order, so three training steps end in bit-identical parameters."""
    from radar_depth_amd.main import HipTrainStep
    from radar_depth_amd.synthetic import make_batch
    b, h, w = 2, 97, 161
    runs = []
    for batch in ("0", "4"):
        monkeypatch.setenv("RD_WGRAD_REDUCE_BATCH", batch)
        m = build(h, w)
        # (the fp32-MFMA plan: the batched reduction is an option of rd_wgrad's slabs; the default split plan keeps its own per-tensor form)
        ts = HipTrainStep(m, b, h, w, storage=storage, operands="fp32" if storage == "fp32" else None)
        assert bool(ts.plan.reduce_batches) == (batch != "0")
        for it in range(3):
            x, t = make_batch(b, h, w, 700 + it, ref_pixels=h * w)
            ts.step(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        runs.append([p.detach().clone() for p in m.parameters()])
    for p, q in zip(*runs):
        assert torch.equal(p, q)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_stem_backward_two_pass_is_bit_identical(monkeypatch, storage):
    """The stem's pool + BatchNorm backward without the materialised full-resolution gradient (rd_bnact_maxpool_bwd_stats_t with
    g == NULL, then rd_bnact_maxpool_bwd_apply_t repeating the gather) against the one-pass form that stores g: same expressions,
    same rounding of g under bf16 storage -> bit-identical parameters after three steps."""
    from radar_depth_amd.main import HipTrainStep
    from radar_depth_amd.synthetic import make_batch
    b, h, w = 2, 97, 161
    runs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("RD_STEM_BWD_TWO_PASS", mode)
        m = build(h, w)
        ts = HipTrainStep(m, b, h, w, storage=storage)
        names = [n for n, _, _ in ts.plan.bwd]
        assert ("conv1.bn.bn1.bwd_apply" in names) and (mode == "0" or names.count("conv1.pool_bwd") == 1)
        for it in range(3):
            x, t = make_batch(b, h, w, 800 + it, ref_pixels=h * w)
            ts.step(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        runs.append([p.detach().clone() for p in m.parameters()])
    for p, q in zip(*runs):
        assert torch.equal(p, q)


def test_op_table_replay_ranges_streams_and_errors():
    """rd_optable_run on the GPU: a sub-range issues exactly its ops, stream arguments are taken from the slots of THAT run, float
    arguments arrive bit-exact, and a failing op stops the run and reports its index (the ops behind it are not issued)."""
    import ctypes as C
    from radar_depth_amd._lib import RadarDepthHipError, lib, ptr
    from radar_depth_amd.optable import OpTable
    L = lib()
    t = torch.zeros(4, 1024, device="cuda")
    s_main = C.c_void_p(0)
    row = lambda i: C.c_void_p(t.data_ptr() + 4 * 1024 * i)
    ops = [("fill0", L.rd_fill, (row(0), C.c_int64(1024), C.c_float(1.5), s_main)),
           ("fill1", L.rd_fill, (row(1), C.c_int64(1024), C.c_float(-2.25), s_main)),
           ("bad", L.rd_fill, (C.c_void_p(0), C.c_int64(1024), C.c_float(9.0), s_main)),          # null pointer -> RD_EINVAL
           ("fill3", L.rd_fill, (row(3), C.c_int64(1024), C.c_float(7.0), s_main))]
    tb = OpTable(L, ops, [s_main])
    side = torch.cuda.Stream()
    s_main.value = side.cuda_stream                     # the slot's value at RUN time is what counts
    tb.run(1, 2)
    side.synchronize()
    assert t[0].abs().max().item() == 0.0 and bool((t[1] == -2.25).all()) and t[3].abs().max().item() == 0.0
    with pytest.raises(RadarDepthHipError, match="bad"):
        tb.run(0, 4)
    side.synchronize()
    assert bool((t[0] == 1.5).all()) and t[3].abs().max().item() == 0.0          # ops behind the failing one were not issued
    tb.close()
    # bare numbers are marshalled through the compiled prototypes: the same bits as explicit wrappers (1027: not a multiple of a block)
    n, got = 1027, []
    torch.manual_seed(0)
    p0, g0 = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    for wrap in (False, True):
        i64, f32 = (C.c_int64, C.c_float) if wrap else (int, float)
        p, g, mom, filled = p0.clone(), g0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n + 5, device="cuda")
        tb = OpTable(L, [("fill", L.rd_fill, (ptr(filled), i64(n), f32(2.5), s_main)),
                         ("sgd", L.rd_sgd_step, (ptr(p), ptr(g), ptr(mom), i64(n), f32(0.01), f32(0.9), f32(1e-4), f32(0.5), 1, s_main))],
                     [s_main])
        tb.run()
        side.synchronize()
        tb.close()
        got.append((filled, p, g, mom))
    assert bool((got[0][0][:n] == 2.5).all()) and got[0][0][n:].abs().max().item() == 0.0 and not torch.equal(got[0][1], p0)
    for a, b in zip(*got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("storage,operands", [("fp32", None), ("bf16", None)])
def test_batched_weight_pack_matches_the_single_tensor_packs(storage, operands):
    """rd_pack_weights_batched's unit-per-thread form for bf16 / three-piece operands (one thread = eight reduction rows x all taps of
    one column) against rd_pack_weights_bf16 per tensor and the piece definition w = p0 + p1 + p2: every packed buffer of the plan,
    forward and transposed (dgrad) operands, concatenated jobs sharing one buffer included -- bit-exact."""
    from radar_depth_amd import ops
    from radar_depth_amd.main import HipTrainStep
    from radar_depth_amd.synthetic import make_batch
    b, h, w = 2, 97, 161
    m = build(h, w)
    ts = HipTrainStep(m, b, h, w, lr=0.0, momentum=0.0, weight_decay=0.0, storage=storage, operands=operands)
    x, t = make_batch(b, h, w, 900, ref_pixels=h * w)
    ts.step(x.cuda(), t.cuda())                                    # (lr = 0: the weights the pack read are the weights still there)
    torch.cuda.synchronize()
    by_dst, seen = {}, 0
    for (src, dst, o, i, tt, ldc, off, rows, tr, scale, quad) in ts.plan.pack_jobs:
        if quad < 2 or scale is not None:
            continue
        k, w4 = dst.data_ptr(), src.detach().reshape(o, i, -1, 1)
        exp = ops.pack_weights_split(w4, bool(tr), ldc, off, rows) if quad == 3 else ops.pack_weights_bf16(w4, bool(tr), ldc, off, rows)[None]
        if k not in by_dst:
            by_dst[k] = [dst, torch.zeros_like(exp)]
        by_dst[k][1] += exp                                         # (disjoint regions: adding zeros is exact)
        seen += 1
    assert seen > 20
    for dst, exp in by_dst.values():
        assert torch.equal(dst.reshape(-1)[:exp.numel()].view(torch.int16), exp.reshape(-1).view(torch.int16))

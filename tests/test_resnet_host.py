"""Host-side checks of the early-fusion ResNet (--arch resnet18 / resnet34): the reference's command-line defaults build a model, the
state_dict surface and the initialisers against the reference-generated fixture (tests/golden/resnet_surface.npz), the local
ImageNet weight file, the scope errors, and the structure of dry-run plans (no GPU)."""
import collections
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _surface():
    return np.load(os.path.join(GOLD, "resnet_surface.npz"))


def _shapes(sd):
    return [list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()]


def test_reference_default_command_line_builds():
    """`--no-pretrain` and otherwise the reference's bare defaults: resnet18, rgb, deconv2."""
    from radar_depth_amd import main, utils
    from radar_depth_amd.model.models import DeConv, ResNet
    a = utils.parse_command(["--no-pretrain"])
    assert (a.arch, a.modality, a.decoder) == ("resnet18", "rgb", "deconv2")
    m = main.create_model(a, [450, 800])
    assert isinstance(m, ResNet) and isinstance(m.decoder, DeConv) and isinstance(m.decoder.layer1.deconv2, nn.ConvTranspose2d)
    assert tuple(m.conv1.weight.shape) == (64, 3, 7, 7)
    for modality, planes in (("rgbd", 4), ("d", 1)):
        m = main.create_model(utils.parse_command(["-m", modality, "--no-pretrain"]), [450, 800])
        assert isinstance(m, ResNet) and tuple(m.conv1.weight.shape) == (64, planes, 7, 7)
    m = main.create_model(utils.parse_command(["-a", "resnet34", "-m", "rgbd", "--no-pretrain"]), [450, 800])
    assert isinstance(m, ResNet) and [len(getattr(m, "layer%d" % i)) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]


def test_state_dict_matches_reference():
    from radar_depth_amd.model.models import ResNet
    want = _surface()
    tags = sorted({k.rsplit("/", 1)[0] for k in want.files if k.endswith("/names") and not k.startswith("init/")})
    assert len(tags) == 12
    for tag in tags:
        layers, cin, dec = tag.split("/")
        sd = ResNet(int(layers), dec, [450, 800], int(cin), False).state_dict()
        assert list(sd) == list(want[tag + "/names"]), tag
        assert _shapes(sd) == want[tag + "/shapes"].tolist(), tag
        if layers == "18":
            assert len(sd) == (199 if dec == "upproj" else 151)


def test_initialiser_moments_match_reference():
    """Per-tensor moments of a freshly constructed ResNet(18, "deconv2", ..., 4, False): the encoder as torchvision constructs it
    (Kaiming-normal fan_out), the four-plane stem and everything behind the encoder through weights_init."""
    from radar_depth_amd.model.models import ResNet
    want = _surface()
    names, rows = list(want["init/names"]), want["init/rows"]
    torch.manual_seed(20240917)
    m = ResNet(18, "deconv2", [450, 800], 4, False)
    sd = {k: v for k, v in m.state_dict().items() if not (v.dim() == 0 and not v.is_floating_point())}
    assert list(sd) == names
    for (k, v), (n, mean, std, amax, kurt) in zip(sd.items(), rows):
        x = v.double().flatten()
        assert x.numel() == n, k
        if k.endswith("weight") and v.dim() == 4:
            fan = v.shape[2] * v.shape[3] * v.shape[0]      # (Conv2d: out_channels, ConvTranspose2d: in_channels -- dim 0 of both)
            # 5 % on the standard deviation; the sample standard deviation of n normal draws scatters by 1 / sqrt(2 n) (the mean by
            # 1 / sqrt(n)) around the law's, which for the 144-element head convolution alone is more than that: three standard errors there
            tol, tol_mean = max(0.05, 3.0 / np.sqrt(2.0 * n)), max(0.05, 3.0 / np.sqrt(n))
            assert abs(x.std().item() - std) < tol * std, k
            assert abs(std - np.sqrt(2.0 / fan)) < tol * std, k
            assert abs(x.mean().item()) < tol_mean * std and abs(mean) < tol_mean * std, k
        else:
            assert np.allclose([x.mean().item(), x.std(unbiased=False).item()], [mean, std], atol=1e-12), k


@pytest.mark.parametrize("layers", [18, 34])
def test_pretrained_reads_a_local_state_dict(layers, tmp_path, monkeypatch):
    from radar_depth_amd.model.models import ResNet
    var = "RADAR_DEPTH_RESNET%d_WEIGHTS" % layers
    monkeypatch.delenv(var, raising=False)
    with pytest.raises(RuntimeError, match=var):
        ResNet(layers, "deconv2", [97, 161], 3, True)
    # a synthetic torchvision-format state_dict: every encoder tensor a recognisable constant, plus the classifier torchvision carries
    src = ResNet(layers, "deconv2", [97, 161], 3, False)
    tv = {k: torch.full_like(v, 0.25) if v.is_floating_point() else v.clone() for k, v in src.state_dict().items()
          if k.split(".")[0] in ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4")}
    tv["fc.weight"], tv["fc.bias"] = torch.zeros(1000, 512), torch.zeros(1000)
    path = tmp_path / "resnet.pth"
    torch.save(tv, str(path))
    monkeypatch.setenv(var, str(path))
    for cin in (3, 4, 1):
        m = ResNet(layers, "deconv2", [97, 161], cin, True)
        sd = m.state_dict()
        for k, v in sd.items():
            top = k.split(".")[0]
            if not v.is_floating_point():
                continue
            taken = top.startswith("layer") or (cin == 3 and top in ("conv1", "bn1"))
            assert bool((v == 0.25).all()) == taken, (cin, k)
        assert tuple(m.conv1.weight.shape) == (64, cin, 7, 7)


def test_scope_errors():
    from radar_depth_amd import main, utils
    from radar_depth_amd.engine import ResNetPlan
    from radar_depth_amd.model.models import ResNet
    for layers in (50, 101, 152):
        with pytest.raises(NotImplementedError, match="Bottleneck"):
            ResNet(layers, "deconv2", [97, 161], 3, False)
    with pytest.raises(RuntimeError, match="Only 18, 34, 50, 101, and 152"):
        ResNet(19, "deconv2", [97, 161], 3, False)
    for arch in ("resnet50", "resnet18_new", "resnet18_multistage_uncertainty"):
        with pytest.raises(NotImplementedError, match="outside the MI355X hot path"):
            main.create_model(utils.parse_command(["-a", arch, "--no-pretrain"]), [97, 161])
    m = ResNet(18, "upproj", [97, 161], 4, False)
    with pytest.raises(NotImplementedError, match="bf16"):
        ResNetPlan(m, 2, 97, 161, train=True, dry_run=True, bf16=True)
    with pytest.raises(NotImplementedError, match="bf16"):
        ResNetPlan(m, 2, 97, 161, train=True, dry_run=True, storage="bf16")
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 4, 97, 161))


CASES = [(18, 4, "upproj"), (18, 3, "deconv2"), (34, 4, "upconv")]


def _dry_plan(layers, cin, dec, split=True, train=True):
    from radar_depth_amd.engine import ResNetPlan
    from radar_depth_amd.model.models import ResNet
    torch.manual_seed(0)
    m = ResNet(layers, dec, [450, 800], cin, False)
    return m, ResNetPlan(m, 16, 450, 800, train=train, dry_run=True, split=split)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_dry_run_plan_structure(case, split):
    from radar_depth_amd.main import _param_offsets, bucket_segments
    layers, cin, dec = case
    m, plan = _dry_plan(layers, cin, dec, split=split)
    names = [n for n, _, _ in plan.bwd]
    # four segments, each ending joined; the buckets tile the whole arena exactly once
    segs = bucket_segments(plan, _param_offsets(m))
    assert len(segs) == 4 and segs[0][0] == 0 and segs[-1][1] == len(names)
    cover = sorted(sl for _, _, sls in segs for sl in sls)
    assert cover[0][0] == 0 and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    assert cover[-1][1] == m._ensure_arenas()["total"]
    for begin, end, sls in segs:
        assert names[end - 1].endswith(".wait")
    # every convolution weight except the stem's and the head's has one slab-reduce writer, every BatchNorm one backward apply
    gv = m._ensure_arenas()["gviews"]
    gptr = {gv[id(p)].data_ptr(): n for n, p in m.named_parameters()}
    writers = collections.Counter(gptr[args[2].value] for n, _, args in plan.bwd if n.endswith(".wreduce"))
    conv_w = [n for n, p in m.named_parameters() if p.dim() == 4 and n not in ("conv1.weight", "conv3.weight")]
    assert sorted(writers) == sorted(conv_w) and set(writers.values()) == {1}
    n_bn = sum(1 for n, p in m.named_parameters() if n.endswith(".bias"))
    # (one apply per two-operand join: the three down-sampling blocks, and the four UpProj modules' upper + bottom branches)
    assert sum(1 for n in names if n.endswith(".bwd_apply")) == n_bn - 3 - (4 if dec == "upproj" else 0)
    # one encoder: nothing of the late-fusion network's depth stream or fusion layer
    every = [n for n, _, _ in plan.prep + plan.fwd + plan.bwd]
    assert not [n for n in every if "_depth" in n or "fusion" in n]
    # the number of blocks per stage comes from the module
    assert [len(s) for s in plan.stages] == ([2, 2, 2, 2] if layers == 18 else [3, 4, 6, 3])
    L = plan.L
    stem = [(n, fn) for n, fn, _ in plan.fwd if n == "conv1"]
    stem_b = [(n, fn) for n, fn, _ in plan.bwd if n.startswith("conv1.")]
    if split:
        assert [fn.__name__ for _, fn in stem] == ["rd_stem_fwd_split"]
        assert ("conv1.bn.bn1.bwd_apply", "rd_stem_wgrad_split_bn_t") in [(n, fn.__name__) for n, fn in stem_b]
        assert not [n for n, _ in stem_b if n == "conv1.wgrad"]
    else:
        assert [fn.__name__ for _, fn in stem] == ["rd_stem_fwd_t"]
        assert ("conv1.wgrad", "rd_stem_wgrad_t") in [(n, fn.__name__) for n, fn in stem_b]
    assert plan.x_in.shape == (16, cin, 450, 800) and len(plan.c_stem["pl"]) == max(3, cin)
    assert L.rd_stem_wgrad_split_supported(cin, 64) == 1


@pytest.mark.parametrize("case", CASES)
def test_dry_run_eval_plan(case):
    layers, cin, dec = case
    m, ev = _dry_plan(layers, cin, dec, split=False, train=False)
    assert ev.bwd == [] and not hasattr(ev, "bwd_segments")
    assert [n for n, _, _ in ev.fwd][-2:] == ["conv3", "bilinear"]
    n_conv = sum(1 for n, p in m.named_parameters() if p.dim() == 4 and n not in ("conv1.weight", "conv3.weight"))
    # (an UpProj module's two 5x5 convolutions are one launch)
    assert sum(1 for k in ev.meta) == n_conv - (4 if dec == "upproj" else 0)


def test_bind_input_points_the_stem_at_a_caller_batch():
    m, plan = _dry_plan(18, 4, "deconv2")
    pl, st = plan.c_stem["pl"], plan.c_stem["st"]
    hw = 450 * 800
    own = plan.x_in.data_ptr()
    assert [pl[c] for c in range(4)] == [own + 4 * hw * c for c in range(4)] and [st[c] for c in range(4)] == [4 * hw] * 4
    plan.bind_input(1 << 20, 4)
    assert [pl[c] for c in range(4)] == [(1 << 20) + 4 * hw * c for c in range(4)]
    plan.bind_own_input()
    assert pl[0] == own

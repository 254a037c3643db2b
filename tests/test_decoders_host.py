"""Host-side checks of the deconv2 / deconv3 / upconv decoders: the reference's surface (state_dict names and shapes, the
--decoder dispatch and its errors, the initialisers), the transposed-convolution descriptors against F.conv_transpose2d and
autograd in float64, and the structure of dry-run plans (no GPU)."""
import collections
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from desc_emulator import pack_dgrad, pack_fwd, run_desc, run_wgrad

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECODERS = ("deconv2", "deconv3", "upconv")


def _surface():
    return np.load(os.path.join(GOLD, "decoders_surface.npz"))


def _shapes(sd):
    return [list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()]


@pytest.mark.parametrize("dec", DECODERS)
def test_state_dict_matches_reference(dec):
    from radar_depth_amd import main, utils
    want = _surface()
    a = utils.parse_command(["-a", "resnet18_latefusion", "-d", dec, "-m", "rgbd", "--no-pretrain"])
    m = main.create_model(a, [450, 800])
    sd = m.state_dict()
    assert list(sd) == list(want["%s/lf/names" % dec])
    assert _shapes(sd) == want["%s/lf/shapes" % dec].tolist()
    a = utils.parse_command(["-a", "resnet18_multistage_uncertainty_fixs", "-d", dec, "-m", "rgbd", "--no-pretrain"])
    m, _ = main.create_model(a, [450, 800])
    sd = m.state_dict()
    assert list(sd) == list(want["%s/ms/names" % dec])
    assert _shapes(sd) == want["%s/ms/shapes" % dec].tolist()


def test_reference_default_decoder_builds():
    """The reference's --decoder default is deconv2: a command line without -d builds a model."""
    from radar_depth_amd import main, utils
    from radar_depth_amd.model.models import DeConv
    a = utils.parse_command(["-a", "resnet18_latefusion", "-m", "rgbd", "--no-pretrain"])
    assert a.decoder == "deconv2"
    m = main.create_model(a, [450, 800])
    assert isinstance(m.decoder, DeConv) and isinstance(m.decoder.layer1.deconv2, nn.ConvTranspose2d)


def test_decoder_dispatch_errors():
    from radar_depth_amd.engine import LateFusionPlan
    from radar_depth_amd.model.models import DeConv, ResNet_latefusion, UpConv, choose_decoder
    assert isinstance(choose_decoder("deconv3", 256), DeConv) and isinstance(choose_decoder("upconv", 256), UpConv)
    with pytest.raises(NotImplementedError, match="deconv2 and deconv3"):
        choose_decoder("deconv4", 256)
    with pytest.raises(NotImplementedError, match="deconv2 and deconv3"):
        choose_decoder("deconv9", 256)
    for bad in ("deconv9x", "deconv1", "deconv0"):      # (the reference's assertions: length 7, DeConv's kernel_size >= 2)
        with pytest.raises(AssertionError):
            choose_decoder(bad, 256)
    with pytest.raises(AssertionError):
        choose_decoder("bogus", 256)
    for dec in DECODERS:
        m = ResNet_latefusion(18, dec, [97, 161], 4, False)
        with pytest.raises(NotImplementedError, match="upproj decoder only"):
            LateFusionPlan(m, 2, 97, 161, train=True, dry_run=True, storage="bf16")
        with pytest.raises(NotImplementedError, match="upproj decoder only"):
            LateFusionPlan(m, 2, 97, 161, train=True, dry_run=True, bf16=True)


def test_plan_only_transposed_conv():
    from radar_depth_amd.model.models import DeConv
    d = DeConv(64, 3)
    ct = d.layer2.deconv3
    assert isinstance(ct, nn.ConvTranspose2d) and tuple(ct.weight.shape) == (32, 16, 3, 3)
    assert (ct.stride, ct.padding, ct.output_padding) == ((2, 2), (1, 1), (1, 1))
    with pytest.raises(RuntimeError, match="parameter container"):
        ct(torch.zeros(1, 32, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):
        d(torch.zeros(1, 64, 4, 4))


@pytest.mark.parametrize("dec", DECODERS)
def test_initialiser_moments_match_reference(dec):
    """Per-tensor moments of a freshly constructed decoder (decoder.apply(weights_init)) against the reference's: the ConvTranspose2d
    branch draws N(0, sqrt(2 / (kh kw in_channels)))."""
    from radar_depth_amd.model.models import choose_decoder, weights_init
    want = _surface()
    names, rows = list(want["%s/init/names" % dec]), want["%s/init/rows" % dec]
    torch.manual_seed(20240917)
    d = choose_decoder(dec, 256)
    d.apply(weights_init)
    sd = {k: v for k, v in d.state_dict().items() if not (v.dim() == 0 and not v.is_floating_point())}
    assert list(sd) == names
    for (k, v), (n, mean, std, amax, kurt) in zip(sd.items(), rows):
        x = v.double().flatten()
        assert x.numel() == n, k
        if k.endswith("weight") and v.dim() == 4:
            fan = v.shape[2] * v.shape[3] * v.shape[0]      # (Conv2d: out_channels, ConvTranspose2d: in_channels -- dim 0 of both)
            assert abs(x.std().item() - std) < 0.05 * std, k
            assert abs(std - np.sqrt(2.0 / fan)) < 0.05 * std, k
            assert abs(x.mean().item()) < 0.05 * std and abs(mean) < 0.05 * std, k
        else:
            assert np.allclose([x.mean().item(), x.std(unbiased=False).item()], [mean, std], atol=1e-12), k


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("h,w", [(3, 5), (4, 4), (5, 2), (1, 1)])
@pytest.mark.parametrize("cin,cout", [(6, 5), (16, 8), (3, 7)])
def test_deconv_descriptors(k, h, w, cin, cout):
    """deconv_fwd / deconv_dgrad / deconv_wgrad through the descriptor emulator against F.conv_transpose2d and autograd in float64."""
    from radar_depth_amd import convdesc as cd
    g = torch.Generator().manual_seed(100 * k + 10 * h + w + cin)
    N = 2
    x = torch.randn(N, cin, h, w, dtype=torch.float64, generator=g).requires_grad_(True)
    wt = torch.randn(cin, cout, k, k, dtype=torch.float64, generator=g).requires_grad_(True)
    y = F.conv_transpose2d(x, wt, stride=2, padding=(k - 1) // 2, output_padding=k % 2)
    assert y.shape == (N, cout, 2 * h, 2 * w)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(gy)
    d = cd.deconv_fwd(N, h, w, cin, cout, k)
    assert (d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout, d.out_stride, d.n_phases) == (h, w, cin, 2 * h, 2 * w, cout, 2, 4)
    got = run_desc(d, x.detach().permute(0, 2, 3, 1), pack_dgrad(wt.detach()))       # (transposed operand: [slab][cin][cout])
    assert not torch.isnan(got).any()
    assert (got - y.detach().permute(0, 2, 3, 1)).abs().max().item() < 1e-12
    dd = cd.deconv_dgrad(N, h, w, cin, cout, k)
    assert (dd.in_stride, dd.n_phases, dd.phase[0].n_taps) == (2, 1, k * k)
    gx = run_desc(dd, gy.permute(0, 2, 3, 1), pack_fwd(wt.detach()))
    assert (gx - x.grad.permute(0, 2, 3, 1)).abs().max().item() < 1e-12
    dw = cd.deconv_wgrad(N, h, w, cin, cout, k)
    slabs = run_wgrad(dw, gy.permute(0, 2, 3, 1), x.detach().permute(0, 2, 3, 1), k * k)      # [k*k][cout][cin]
    gw = slabs.permute(2, 1, 0).reshape(cin, cout, k, k)                                        # the OIHW reduce of an [cin, cout] weight
    assert (gw - wt.grad).abs().max().item() < 1e-12
    taps = sorted(d.phase[i].n_taps for i in range(d.n_phases))
    assert taps == ([1, 1, 1, 1] if k == 2 else [1, 2, 2, 4])


def _dry_plan(dec, split=True, train=True):
    from radar_depth_amd.engine import LateFusionPlan
    from radar_depth_amd.model.models import ResNet_latefusion
    torch.manual_seed(0)
    m = ResNet_latefusion(18, dec, [450, 800], 4, False)
    return m, LateFusionPlan(m, 16, 450, 800, train=train, dry_run=True, split=split)


@pytest.mark.parametrize("dec", DECODERS)
def test_dry_run_plan_structure(dec):
    from radar_depth_amd.main import _param_offsets, bucket_segments
    m, plan = _dry_plan(dec)
    names = [n for n, _, _ in plan.bwd]
    # buckets tile the whole arena exactly once, and every segment ends with the side streams joined
    segs = bucket_segments(plan, _param_offsets(m))
    assert len(segs) == 4 and segs[0][0] == 0 and segs[-1][1] == len(names)
    cover = sorted(sl for _, _, sls in segs for sl in sls)
    assert cover[0][0] == 0 and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    assert cover[-1][1] == m._ensure_arenas()["total"]
    for begin, end, sls in segs:
        assert names[end - 1].endswith(".wait")
    # every convolution weight has exactly one gradient writer (its slab reduce), every BatchNorm exactly one backward apply
    gv = m._ensure_arenas()["gviews"]
    gptr = {gv[id(p)].data_ptr(): n for n, p in m.named_parameters()}
    writers = collections.Counter(gptr[args[2].value] for n, _, args in plan.bwd if n.endswith(".wreduce"))
    conv_w = [n for n, p in m.named_parameters() if p.dim() == 4 and n not in ("conv1.weight", "conv1_depth.weight", "conv3.weight")]
    assert sorted(writers) == sorted(conv_w) and set(writers.values()) == {1}
    n_bn = sum(1 for n, p in m.named_parameters() if n.endswith(".bias"))
    assert sum(1 for n in names if n.endswith(".bwd_apply")) == n_bn - 6      # (the six two-operand joins of the down-sampling blocks)
    dec_ops = [n for n in names if n.startswith("decoder.")]
    assert dec_ops and all(n.split(".")[0] in plan.bwd_segments[0][2] for n in dec_ops)
    # kernel families of the decoder layers: split kernels wherever both sides have >= 32 channels, the fp32 gconv on layer 4 only
    conv = "deconv%s" % dec[-1] if dec.startswith("deconv") else "conv"
    for i in (1, 2, 3, 4):
        base = "decoder.layer%d.%s" % (i, conv)
        fams = [plan.meta[base][0], plan.meta[base + ".dgrad"][0]]
        if i == 4:
            assert fams[0] == "gconv", (base, fams)
            assert plan.meta[base][1].Cout == 16
        elif dec == "deconv2":
            # the input gradient (one 4-tap phase at input stride 2) on the few-tap kernel, where its gate measured it ahead
            assert fams[0].startswith("gconv_split") and fams[1] == "gemm_taps_split", (base, fams)
        else:
            assert all(f.startswith("gconv_split") for f in fams), (base, fams)
    assert all(plan.meta[k][0] in ("gconv", "gconv_split", "gconv_split_pre", "gemm_taps_split") for k in plan.meta if k.startswith("decoder.")
               and not k.endswith(".wgrad"))


@pytest.mark.parametrize("dec", DECODERS)
def test_dry_run_fp32_and_eval_plans(dec):
    """The plain fp32-MFMA plan keeps every decoder layer on gconv; the eval plan folds BatchNorm into one launch per layer (a
    transposed convolution's scale by column of its weight)."""
    m, plan = _dry_plan(dec, split=False)
    assert all(plan.meta[k][0] in ("gconv", "gconv_bnb", "wgrad") for k in plan.meta if k.startswith("decoder."))
    m, ev = _dry_plan(dec, split=False, train=False)
    layers = [k for k in ev.meta if k.startswith("decoder.")]
    assert len(layers) == 4 and all(ev.meta[k][0] == "gconv" for k in layers)
    from radar_depth_amd.engine import _ColScale
    col = [j for j in ev.pack_jobs if isinstance(j[9], _ColScale)]
    assert len(col) == (4 if dec.startswith("deconv") else 0)
    for j in col:
        src, o, i, tr = j[0], j[2], j[3], j[8]
        assert tr == 1 and (o, i) == tuple(src.shape[:2]) and j[9].t.numel() == i


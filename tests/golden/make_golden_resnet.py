#!/usr/bin/env python3
"""Generate the early-fusion ResNet golden vectors (--arch resnet18 / resnet34) in this directory from the REAL reference.

Runs only in the authoring container, like make_golden.py, whose shims it reuses (torchvision stand-in, `Tensor.cuda`
neutralised); the torchvision.models.resnet34 stand-in is added here, built from the shim's BasicBlock.  Usage:

    python tests/golden/make_golden_resnet.py      # writes tests/golden/resnet_*.npz

  resnet_surface.npz       state_dict names / shapes of ResNet(layers, decoder, [450, 800], in_channels, False) for layers 18 / 34,
                           in_channels 1 / 3 / 4, decoders deconv2 / upproj, and make_golden.init_stats moments of a freshly
                           constructed ResNet(18, "deconv2", [450, 800], 4, False) under a fixed seed
  resnet_net_<case>.npz    one float64 step of the reference's loop body (main.py:440-445) at 97x161, b = 2, and the eval forward on the
                           same batch, the input sliced to the modality: rgbd_upproj, rgb_deconv2, d_deconv3 (layers = 18),
                           rgbd34_upconv (layers = 34)
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from radar_depth_amd.synthetic import make_batch, procedural_fill_  # noqa: E402

SURFACE_LAYERS, SURFACE_CIN, SURFACE_DECODERS = (18, 34), (1, 3, 4), ("deconv2", "upproj")
# case -> (layers, decoder, channel slice of the [N,4,H,W] batch)
CASES = {"rgbd_upproj": (18, "upproj", (0, 4)), "rgb_deconv2": (18, "deconv2", (0, 3)), "d_deconv3": (18, "deconv3", (3, 4)),
         "rgbd34_upconv": (34, "upconv", (0, 4))}
FLOOR = 1e-6          # the gradient-norm bar of the tests is 1e-2 c + FLOOR max: no parameter may be excused by the floor


def _install_resnet34():
    """torchvision.models.resnet34 with the torchvision-0.4.2 topology ([3, 4, 6, 3] BasicBlocks) and initialisation."""
    import torchvision
    tvr = torchvision.models.resnet

    class TVResNet34(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
            self.bn1 = nn.BatchNorm2d(64)
            self.relu = nn.ReLU(inplace=True)
            self.maxpool = nn.MaxPool2d(3, 2, 1)
            inpl = 64
            for i, (planes, stride, blocks) in enumerate(((64, 1, 3), (128, 2, 4), (256, 2, 6), (512, 2, 3)), 1):
                down = None
                if stride != 1 or inpl != planes:
                    down = nn.Sequential(tvr.conv1x1(inpl, planes, stride), nn.BatchNorm2d(planes))
                seq = [tvr.BasicBlock(inpl, planes, stride, down)] + [tvr.BasicBlock(planes, planes) for _ in range(1, blocks)]
                setattr(self, "layer%d" % i, nn.Sequential(*seq))
                inpl = planes
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                elif isinstance(m, nn.BatchNorm2d):
                    nn.init.constant_(m.weight, 1)
                    nn.init.constant_(m.bias, 0)

    torchvision.models.resnet34 = lambda pretrained=False, **kw: TVResNet34()


def surface(models):
    out = {}
    for layers in SURFACE_LAYERS:
        for cin in SURFACE_CIN:
            for dec in SURFACE_DECODERS:
                sd = models.ResNet(layers, dec, [450, 800], cin, False).state_dict()
                tag = "%d/%d/%s" % (layers, cin, dec)
                out[tag + "/names"] = np.array(list(sd.keys()))
                out[tag + "/shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    torch.manual_seed(20240917)
    st = mg.init_stats(models.ResNet(18, "deconv2", [450, 800], 4, False))
    out["init/names"], out["init/rows"] = st["names"], st["rows"]
    return out


def net_case(models, crit_mod, layers, dec, chans, batch=2, h=97, w=161, seed=4321):
    """make_golden_decoders.net_case for the early-fusion network: one float64 step and the eval forward."""
    dtype = torch.float64
    torch.manual_seed(0)
    model = models.ResNet(layers, dec, [h, w], chans[1] - chans[0], False)
    procedural_fill_(model)
    model.to(dtype)
    for m in model.modules():
        for k, v in list(vars(m).items()):
            if isinstance(v, torch.Tensor) and v.is_floating_point():
                setattr(m, k, v.to(dtype))          # (Unpool.weights is a plain attribute)
    x, t = make_batch(batch, h, w, seed, ref_pixels=h * w)
    x, t = x[:, chans[0]:chans[1]].contiguous().to(dtype), t.to(dtype)
    out = {}
    model.eval()
    with torch.no_grad():
        out["eval_out"] = mg._np(model(x)).astype(np.float32)
    model.train()
    opt = torch.optim.SGD(model.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    y = model(x)
    loss = crit_mod.MaskedL1Loss()(y, t)
    opt.zero_grad()
    loss.backward()
    out["train_out"] = mg._np(y).astype(np.float32)
    out["loss"] = np.array([loss.item()])
    out["param_names"] = np.array([n for n, _ in model.named_parameters()])
    out["grad_norms"] = np.array([p.grad.norm().item() for _, p in model.named_parameters()])
    assert out["grad_norms"].min() > 100 * FLOOR * out["grad_norms"].max(), "a gradient norm sits near the tests' floor"
    opt.step()
    out["param_norms1"] = np.array([p.norm().item() for _, p in model.named_parameters()])
    out["bn1_running_mean"] = mg._np(model.bn1.running_mean)
    out["bn1_running_var"] = mg._np(model.bn1.running_var)
    out["valid_fraction"] = np.array([(t > 0).double().mean().item()])
    return out


def main():
    mg._install_shims()
    _install_resnet34()
    from model import models
    from evaluation import criteria_new as crit_mod
    torch.set_num_threads(8)
    np.savez_compressed(os.path.join(HERE, "resnet_surface.npz"), **surface(models))
    for case, (layers, dec, chans) in CASES.items():
        out = net_case(models, crit_mod, layers, dec, chans)
        np.savez_compressed(os.path.join(HERE, "resnet_net_%s.npz" % case), **out)
        print(case, "loss %.4f" % out["loss"][0], "grad norms %.4g .. %.4g" % (out["grad_norms"].min(), out["grad_norms"].max()),
              "valid %.3f" % out["valid_fraction"][0])
    for f in sorted(os.listdir(HERE)):
        if f.startswith("resnet_"):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()

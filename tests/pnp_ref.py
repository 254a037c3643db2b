"""Host restatement of PnP-Depth refinement for the tests: the reference's two halves (model/models.py:669-707) composed from
the sub-modules of oracle.models.ResNet_latefusion, the loop around them, and the inputs of the fixtures tests/golden/pnp_*.npz
(tests/golden/make_golden_pnp.py writes those from the real reference with the same constants)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RADAR_POINTS = 2400.0            # (the seed of a case's inputs is stored in its fixture: make_golden_pnp.py chooses it)
H, W = 97, 161
ZERO_H, ZERO_W = 225, 400
# case -> (class, decoder, planes of the [1,4,H,W] batch the network reads, sparse passed explicitly)
CASES = {"lf_upproj": ("ResNet_latefusion", "upproj", (0, 4), False), "lf_deconv2": ("ResNet_latefusion", "deconv2", (0, 4), False),
         "lf_deconv3": ("ResNet_latefusion", "deconv3", (0, 4), False), "lf_upconv": ("ResNet_latefusion", "upconv", (0, 4), False),
         "rn_upproj_rgbd": ("ResNet_pnp", "upproj", (0, 4), False), "rn_deconv2_rgb": ("ResNet_pnp", "deconv2", (0, 3), True)}


def golden(case):
    return np.load(os.path.join(GOLDEN, "pnp_%s.npz" % case))


def case_inputs(case):
    """-> (x [1,C,H,W], sparse [1,1,H,W]) fp32 CPU tensors of a fixture case ("zero": the one-valid-pixel frame at 225x400)."""
    from radar_depth_amd.synthetic import make_batch
    seed = int(golden(case)["seed"][0])
    if case == "zero":
        x, _ = make_batch(1, ZERO_H, ZERO_W, seed, radar_points=RADAR_POINTS)
        x[:, 3] = 0.0
        x[0, 3, 0, 0] = float(golden("zero")["depth"][0])
        return x, x[:, 3:4].contiguous()
    chans = CASES[case][2]
    x4, _ = make_batch(1, H, W, seed, radar_points=RADAR_POINTS)
    return x4[:, chans[0]:chans[1]].contiguous(), x4[:, 3:4].contiguous()


def front(model, x):
    """pnp_forward_front of the oracle's ResNet_latefusion: both encoders, the fusion layer, conv2, bn2."""
    rgb, d = model._split(x)
    rgb = model.maxpool(model.relu(model.bn1(model.conv1(rgb))))
    rgb = model.layer4(model.layer3(model.layer2(model.layer1(rgb))))
    d = model.maxpool_depth(model.relu_depth(model.bn1_depth(model.conv1_depth(d))))
    d = model.layer4_depth(model.layer3_depth(model.layer2_depth(model.layer1_depth(d))))
    f = model.bn_fusion(model.conv_fusion(torch.cat((rgb, d), dim=1)))
    return model.bn2(model.conv2(f))


def rear(model, z):
    """pnp_forward_rear: decoder, conv3, bilinear resize."""
    return model.bilinear(model.conv3(model.decoder(z)))


def rear_grad(model, criterion, z, sparse):
    """-> (pred, d criterion(pred, sparse) / d z, loss) of one rear pass."""
    z = z.detach().clone().requires_grad_(True)
    pred = rear(model, z)
    loss = criterion(pred, sparse)
    g, = torch.autograd.grad(loss, z)
    return pred.detach(), g, loss.detach()


def update(z, g, alpha):
    """z - alpha * sign(g) on numpy arrays, in z's precision (sign(+-0) = 0, sign(NaN) = NaN)."""
    return z - z.dtype.type(alpha) * np.sign(g)


def loop(model, criterion, x, sparse, iters, alpha):
    """The whole refinement -> (final prediction, [(z_k, pred_k, g_k, loss_k)]); the last pass takes no gradient (g, loss: None)."""
    with torch.no_grad():
        z = front(model, x)
        steps = []
        for k in range(iters - 1):
            with torch.enable_grad():
                pred, g, loss = rear_grad(model, criterion, z, sparse)
            steps.append((z, pred, g, loss))
            z = z - alpha * torch.sign(g)
        steps.append((z, rear(model, z), None, None))
    return steps[-1][1], steps

"""Host-side checks of PnP-Depth refinement (no GPU): the reference-generated fixtures tests/golden/pnp_*.npz are self-consistent, the
oracle's rear half reproduces them in float64, ResNet_pnp's state_dict surface is the reference's, the two kernels' entry points refuse
bad arguments with their own codes before anything is launched, and a pnp plan's op lists have the structure engine.py documents."""
import ctypes as C

import numpy as np
import pytest
import torch

import pnp_ref


@pytest.mark.parametrize("case", sorted(pnp_ref.CASES))
def test_fixture_is_self_consistent(case):
    """z_{k+1} == z_k - alpha * sign(g_k) exactly, in float64; losses fall; enough valid pixels."""
    gd = pnp_ref.golden(case)
    alpha, iters = float(gd["alpha"][0]), int(gd["iters"][0])
    assert iters == 3 and gd["n_valid"][0] >= 30
    for k in range(iters):
        assert gd["z_%d" % k].dtype == np.float64 and gd["g_%d" % k].dtype == np.float64
        assert gd["z_%d" % k].shape == gd["g_%d" % k].shape == (1, 256, 4, 6)
        assert gd["pred_%d" % k].shape == (1, 1, pnp_ref.H, pnp_ref.W)
        if k + 1 < iters:
            assert np.array_equal(gd["z_%d" % (k + 1)], pnp_ref.update(gd["z_%d" % k], gd["g_%d" % k], alpha))
            assert gd["loss_%d" % (k + 1)][0] < gd["loss_%d" % k][0]
    assert np.array_equal(gd["final"], gd["pred_%d" % (iters - 1)].astype(np.float32))
    assert 0 < gd["d32"][0] < 1e-4
    x, sparse = pnp_ref.case_inputs(case)
    assert int((sparse > 0).sum()) == gd["n_valid"][0] and x.shape[1] == pnp_ref.CASES[case][2][1] - pnp_ref.CASES[case][2][0]


def test_zero_region_fixture():
    """One valid pixel in the top-left corner: g_0 is exactly zero outside the corner of the latent its receptive field reaches."""
    g = pnp_ref.golden("zero")["g_0"]
    assert g.shape == (1, 256, 8, 13)
    nz = (g != 0).any(axis=(0, 1))
    rows, cols = np.nonzero(nz.any(axis=1))[0], np.nonzero(nz.any(axis=0))[0]
    r, c = rows.max() + 1, cols.max() + 1
    assert 0 < r <= 4 and 0 < c <= 4, (r, c)
    assert (g[:, :, :r, :c] != 0).all()                        # every exact zero lies outside the corner
    assert (g == 0).sum() == g.size - 256 * r * c > 0
    x, sparse = pnp_ref.case_inputs("zero")
    assert int((sparse > 0).sum()) == 1 and sparse[0, 0, 0, 0] > 0


def test_oracle_rear_reproduces_fixture():
    """ResNet_latefusion / upproj: the oracle's eval-mode halves, composed from its sub-modules, give the fixture's z_0, pred_0 and g_0
    within 1e-10 relative in float64."""
    from oracle.criteria import MaskedL1Loss
    from oracle.models import ResNet_latefusion
    from radar_depth_amd.synthetic import procedural_fill_
    gd = pnp_ref.golden("lf_upproj")
    m = ResNet_latefusion(18, "upproj", [pnp_ref.H, pnp_ref.W], 4, False)
    procedural_fill_(m)
    m.double().eval()
    x, sparse = pnp_ref.case_inputs("lf_upproj")
    x, sparse = x.double(), sparse.double()
    with torch.no_grad():
        z0 = pnp_ref.front(m, x).numpy()
    assert np.abs(z0 - gd["z_0"]).max() <= 1e-10 * np.abs(gd["z_0"]).max()
    pred, g, loss = pnp_ref.rear_grad(m, MaskedL1Loss(), torch.from_numpy(gd["z_0"]), sparse)
    assert gd["pred_0"].dtype == np.float64
    assert np.abs(pred.numpy() - gd["pred_0"]).max() <= 1e-10 * np.abs(gd["pred_0"]).max()
    assert np.abs(g.numpy() - gd["g_0"]).max() <= 1e-10 * np.abs(gd["g_0"]).max()
    assert abs(loss.item() - gd["loss_0"][0]) <= 1e-10 * gd["loss_0"][0]
    assert all(p.grad is None for p in m.parameters())
    # and the whole loop: the final prediction (stored as float32)
    final, steps = pnp_ref.loop(m, MaskedL1Loss(), x, sparse, int(gd["iters"][0]), float(gd["alpha"][0]))
    assert np.array_equal(steps[2][0].numpy(), gd["z_2"])
    assert np.abs(final.numpy() - gd["final"]).max() <= 1e-6 * np.abs(gd["final"]).max()


@pytest.mark.parametrize("case", ["rn_upproj_rgbd", "rn_deconv2_rgb"])
def test_resnet_pnp_state_dict_matches_reference(case):
    from radar_depth_amd.model.models import ResNet, ResNet_pnp
    gd = pnp_ref.golden(case)
    _, dec, chans, _ = pnp_ref.CASES[case]
    m = ResNet_pnp(18, dec, [pnp_ref.H, pnp_ref.W], chans[1] - chans[0], False)
    sd = m.state_dict()
    assert list(sd) == list(gd["sd_names"])
    assert [list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()] == gd["sd_shapes"].tolist()
    assert isinstance(m, ResNet) and ResNet_pnp.forward is ResNet.forward          # shared, not copied
    assert callable(m.pnp_forward_front) and callable(m.pnp_forward_rear) and not hasattr(ResNet, "pnp_forward_front")
    with pytest.raises(NotImplementedError):
        ResNet_pnp(50, dec, [450, 800], 3, False)
    with pytest.raises(NotImplementedError):
        ResNet_pnp(18, dec, [450, 800], 2, False)


def test_halves_refuse_training_mode_and_cpu():
    from radar_depth_amd.model.models import ResNet_latefusion, ResNet_pnp
    for m in (ResNet_latefusion(18, "upproj", [97, 161], 4, False), ResNet_pnp(18, "deconv2", [97, 161], 3, False)):
        m.train()
        with pytest.raises(RuntimeError, match="eval mode"):
            m.pnp_forward_front(torch.zeros(1, 4, 97, 161))
        with pytest.raises(RuntimeError, match="eval mode"):
            m.pnp_forward_rear(torch.zeros(1, 256, 4, 6))
        m.eval()
        with pytest.raises(RuntimeError, match="MI355X only"):
            m.pnp_forward_front(torch.zeros(1, 4, 97, 161))
        with pytest.raises(RuntimeError, match="MI355X only"):
            m.pnp_forward_rear(torch.zeros(1, 256, 4, 6))


@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_kernel_entry_points_refuse_bad_arguments(L):
    """Every RD_EPNP_* code, reached on the host: the checks run before anything is launched (the pointers are never read)."""
    from radar_depth_amd import _lib
    buf = np.zeros(4096, dtype=np.float32)
    base = buf.ctypes.data
    p = lambda off=0: C.c_void_p(base + 4 * off)
    ok = dict(dtype=0, dy=p(0), lddy=8, y=p(1024), ldy=8, out=p(2048), ldo=8, M=4, C=8, act=1)

    def gate(**kw):
        a = dict(ok, **kw)
        return L.rd_act_gate_t(a["dtype"], a["dy"], a["lddy"], a["y"], a["ldy"], a["out"], a["ldo"], a["M"], a["C"], a["act"], None)
    for name in ("dy", "y", "out"):
        assert gate(**{name: None}) == _lib.RD_EPNP_NULL
    assert gate(M=0) == gate(M=-3) == gate(C=0) == _lib.RD_EPNP_RANGE
    for name in ("lddy", "ldy", "ldo"):
        assert gate(**{name: 7}) == _lib.RD_EPNP_STRIDE
    assert gate(act=0) == gate(act=2) == gate(act=7) == _lib.RD_EPNP_ACT
    assert b"ReLU" in L.rd_last_error()
    assert gate(dtype=1) == gate(dtype=5) == _lib.RD_EPNP_DTYPE
    assert gate(out=p(1024)) == gate(out=p(1024 + 3)) == gate(out=p(1024 - 8)) == _lib.RD_EPNP_OVERLAP          # out on / across y
    assert gate(out=p(4)) == gate(out=p(0), ldo=16, lddy=8) == _lib.RD_EPNP_OVERLAP                              # out across dy without being dy
    assert b"overlaps" in L.rd_last_error()
    # two column windows of one tensor (an UpProj module's halves) do not overlap: the call gets as far as the activation check,
    # which comes behind the overlap checks (nothing here may pass every check: these are host pointers); shifted into each other they do
    assert gate(y=p(1024), ldy=32, C=16, out=p(1024 + 16), ldo=32, lddy=16, act=0) == _lib.RD_EPNP_ACT
    assert gate(y=p(1024), ldy=32, C=16, out=p(1024 + 8), ldo=32, lddy=16, act=0) == _lib.RD_EPNP_OVERLAP
    assert gate(dy=p(2048), act=0) == _lib.RD_EPNP_ACT                                                           # in place: out is dy

    def upd(z=p(0), ldz=8, g=p(1024), ldg=8, M=4, Cc=8, alpha=p(4000)):
        return L.rd_pnp_update(z, ldz, g, ldg, M, Cc, alpha, None)
    assert upd(z=None) == upd(g=None) == upd(alpha=None) == _lib.RD_EPNP_NULL
    assert upd(M=0) == upd(Cc=-1) == _lib.RD_EPNP_RANGE
    assert upd(ldz=7) == upd(ldg=3) == _lib.RD_EPNP_STRIDE
    assert upd(g=p(0)) == upd(g=p(5)) == _lib.RD_EPNP_OVERLAP
    codes = [_lib.RD_EPNP_NULL, _lib.RD_EPNP_RANGE, _lib.RD_EPNP_STRIDE, _lib.RD_EPNP_ACT, _lib.RD_EPNP_DTYPE, _lib.RD_EPNP_OVERLAP]
    assert codes == [-43, -44, -45, -46, -47, -48]
    assert L.rd_optable_entry_args(b"rd_act_gate_t") == 11 and L.rd_optable_entry_args(b"rd_pnp_update") == 8


DECODERS = ("upproj", "deconv2", "deconv3", "upconv")


@pytest.mark.parametrize("dec", DECODERS)
def test_dry_run_pnp_plan_structure(dec):
    """A pnp plan's forward op list is the plain eval plan's (split point remembered, nothing added), pnp_bwd holds bilinear.bwd,
    conv3.dgrad and per decoder layer in reverse its gates and input gradients, all on the main stream; the pack table gains one
    folded input-gradient operand per rear convolution."""
    from radar_depth_amd.engine import LateFusionPlan, ResNetPlan
    from radar_depth_amd.model.models import ResNet_latefusion, ResNet_pnp
    for net, Plan in ((ResNet_latefusion(18, dec, [97, 161], 4, False), LateFusionPlan), (ResNet_pnp(18, dec, [97, 161], 4, False), ResNetPlan)):
        net.eval()
        plain = Plan(net, 1, 97, 161, train=False, dry_run=True)
        p = Plan(net, 1, 97, 161, train=False, dry_run=True, pnp=True)
        assert [(n, f.__name__) for n, f, _ in p.fwd] == [(n, f.__name__) for n, f, _ in plain.fwd]
        assert [n for n, _, _ in p.prep] == [n for n, _, _ in plain.prep] and plain.pnp_bwd == [] and not hasattr(plain, "rear_begin")
        assert p.fwd[p.rear_begin - 1][0] == "conv2" and p.fwd[p.rear_begin][0].startswith("decoder.layer1")
        assert p.taps["bn2"] is p.pnp_z and tuple(p.pnp_z.t.shape) == tuple(p.pnp_g.t.shape) == (1, 4, 6, 256)
        names = [n for n, _, _ in p.pnp_bwd]
        want = ["bilinear.bwd", "conv3.dgrad"]
        for i in (4, 3, 2, 1):
            ln = "decoder.layer%d" % i
            if dec == "upproj":
                want += [ln + ".relu.gate", ln + ".upper_branch.conv2.dgrad", ln + ".upper_branch.relu.gate", ln + ".conv5x5.dgrad"]
            else:
                want += [ln + ".relu.gate", ln + (".conv" if dec == "upconv" else "." + dec) + ".dgrad"]
        assert names == want
        for name, fn, args in p.pnp_bwd:
            assert args[-1] is p.streams[0], name                      # one stream: the captured loop has no parallel branches
            assert fn.__name__ not in ("rd_event_record", "rd_stream_wait_event")
            if name.endswith(".dgrad") and name != "conv3.dgrad":
                assert fn.__name__ == "rd_gconv_ws" and p.meta[name][0] == "gconv"
        # (an UpProj module: two parts of the joint 5x5 convolution and the 3x3; the other layers: one convolution)
        assert len(p.pack_jobs) == len(plain.pack_jobs) + (12 if dec == "upproj" else 4)
        # the folded gradient operands carry the same scale slices as the forward operands of their convolutions
        fwd_scaled = sorted(j[9].data_ptr() for j in plain.pack_jobs if j[9] is not None)
        assert len([j for j in p.pack_jobs if j[9] is not None]) == len(fwd_scaled) + (12 if dec == "upproj" else 4)
        # the last input gradient writes the plan-owned g
        assert p.pnp_bwd[-1][2][3].value == p.pnp_g.t.data_ptr()


def test_pnp_plan_refusals():
    from radar_depth_amd.engine import LateFusionPlan
    from radar_depth_amd.model.models import ResNet_latefusion
    net = ResNet_latefusion(18, "upproj", [97, 161], 4, False).eval()
    with pytest.raises(NotImplementedError, match="bf16"):
        LateFusionPlan(net, 1, 97, 161, train=False, dry_run=True, bf16=True, pnp=True)
    with pytest.raises(NotImplementedError, match="bf16"):
        LateFusionPlan(net, 1, 97, 161, train=False, dry_run=True, storage="bf16", pnp=True)
    with pytest.raises(ValueError, match="eval-mode"):
        LateFusionPlan(net, 1, 97, 161, train=True, dry_run=True, pnp=True)

"""PnP-Depth refinement on the GPU: the two kernels of csrc/pnp.hip against numpy, the eval-mode backward of the rear half and the
whole loop (main.HipPnPInference, model.pnp_forward_front / pnp_forward_rear) against the reference's own float64 run in
tests/golden/pnp_*.npz (tests/golden/make_golden_pnp.py).

Bars: 1e-3 relative in max norm, the project's fp32 parity bar, for the prediction, the latent and the gradient alike (the gradient
relative to max |g_k|); the sign of the gradient wherever |g_k| exceeds that bar; teacher-forced losses within 1e-5 relative (a
float64 sum of about a hundred fp32 terms against a float64 mean); the losses of the free-running loop within 1e-4 (there the latent is
the fp32 trajectory's own, within the bar of the reference's, and the loss moves with it); the kernels, the update and the three ways
to run the loop bit for bit.  Measured values: README, "PnP-Depth refinement"."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAR = 1e-3
GUARD = 64              # floats in front of and behind every buffer (keeps the 16-byte alignment of the data)
SENTINEL = 777.0


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


# ------------------------------------------------------------------------------------------------ kernels
# (M, C, ld, channel offset): one element; the scalar path on odd bases; an UpProj half; more than one block per CU's worth of rows
SHAPES = [(1, 1, 1, 0), (7, 5, 9, 1), (193, 16, 32, 16), (4099, 128, 128, 0)]
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, np.inf, -np.inf, np.nan, 3.0, -2.0], dtype=np.float32)


def _guarded(rows, ld, fill):
    """A [rows, ld] fp32 device matrix inside a flat buffer with GUARD sentinel floats on either side -> (flat, matrix view)."""
    flat = torch.full((2 * GUARD + rows * ld,), SENTINEL, device=DEV)
    m = flat[GUARD:GUARD + rows * ld].view(rows, ld)
    m.copy_(torch.from_numpy(fill))
    return flat, m


def _guards_ok(flat):
    f = flat.cpu().numpy()
    return bool((f[:GUARD] == SENTINEL).all() and (f[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize("M,Cc,ld,c0", SHAPES)
@pytest.mark.parametrize("inplace", [False, True])
def test_act_gate_matches_numpy(M, Cc, ld, c0, inplace):
    rng = np.random.default_rng(M * 131 + Cc)
    dy = rng.standard_normal((M, ld)).astype(np.float32)
    y = rng.standard_normal((M, ld)).astype(np.float32)
    y[rng.random((M, ld)) < 0.2] = 0.0
    y.flat[::7] = -0.0
    fdy, mdy = _guarded(M, ld, dy)
    fy, my = _guarded(M, ld, y)
    fo, mo = (fdy, mdy) if inplace else _guarded(M, ld, np.full((M, ld), SENTINEL, dtype=np.float32))
    rc = _L().rd_act_gate_t(0, _p(mdy, c0), ld, _p(my, c0), ld, _p(mo, c0), ld, M, Cc, 1, _st())
    assert rc == 0, _L().rd_last_error()
    torch.cuda.synchronize()
    want = dy.copy() if inplace else np.full((M, ld), SENTINEL, dtype=np.float32)
    want[:, c0:c0 + Cc] = np.where(y[:, c0:c0 + Cc] > 0, dy[:, c0:c0 + Cc], np.float32(0))
    assert np.array_equal(mo.cpu().numpy(), want)                          # the slice, and every channel beside it untouched
    assert _guards_ok(fo) and _guards_ok(fy) and _guards_ok(fdy)
    assert np.array_equal(my.cpu().numpy(), y) and (inplace or np.array_equal(mdy.cpu().numpy(), dy))


@pytest.mark.parametrize("M,Cc,ld,c0", SHAPES)
def test_pnp_update_matches_numpy(M, Cc, ld, c0):
    """z - alpha * sign(g) in one fp32 rounding, on +-0, denormals, +-inf and NaN; alpha read on the device at run time."""
    rng = np.random.default_rng(M * 17 + Cc)
    z = rng.standard_normal((M, ld)).astype(np.float32)
    g = rng.standard_normal((M, ld)).astype(np.float32)
    n = M * Cc
    gs = g[:, c0:c0 + Cc].reshape(-1).copy()
    gs[:min(n, len(SPECIALS))] = SPECIALS[:min(n, len(SPECIALS))] if n > 1 else SPECIALS[1:2]
    g[:, c0:c0 + Cc] = gs.reshape(M, Cc)
    fz, mz = _guarded(M, ld, z)
    fg, mg = _guarded(M, ld, g)
    alpha = torch.full((1,), 0.01, device=DEV)
    want = z.copy()
    for a in (0.01, 0.37):                                 # the second call reads the value written between the two
        alpha.fill_(a)
        rc = _L().rd_pnp_update(_p(mz, c0), ld, _p(mg, c0), ld, M, Cc, _p(alpha), _st())
        assert rc == 0, _L().rd_last_error()
        torch.cuda.synchronize()
        with np.errstate(invalid="ignore"):
            want[:, c0:c0 + Cc] = want[:, c0:c0 + Cc] - np.float32(a) * np.sign(g[:, c0:c0 + Cc])
        got = mz.cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True)
    if n >= len(SPECIALS):
        zs, z_in = mz.cpu().numpy()[:, c0:c0 + Cc].reshape(-1), z[:, c0:c0 + Cc].reshape(-1)
        assert np.isnan(zs[6]) and not np.isnan(np.delete(zs, 6)).any()                  # NaN in g gives NaN, and only there
        assert zs[0] == z_in[0] and zs[1] == z_in[1]                                     # sign(+-0) = 0
        for i in (2, 4):                                                                 # a denormal counts like +inf: sign +1
            assert zs[i] == np.float32(np.float32(z_in[i] - np.float32(0.01)) - np.float32(0.37))
    assert _guards_ok(fz) and _guards_ok(fg) and np.array_equal(mg.cpu().numpy(), g, equal_nan=True)


# ------------------------------------------------------------------------------------------------ models, objects and inputs (built once)
_CACHE = {}


def _model(case, h=P.H, w=P.W):
    key = ("model", case, h, w)
    if key not in _CACHE:
        from radar_depth_amd.model import models
        from radar_depth_amd.synthetic import procedural_fill_
        cls, dec, chans, _ = P.CASES["lf_upproj" if case == "zero" else case]
        m = getattr(models, cls)(18, dec, [h, w], chans[1] - chans[0], False)
        procedural_fill_(m)
        _CACHE[key] = m.to(DEV).eval()
    return _CACHE[key]


def _inputs(case):
    key = ("inputs", case)
    if key not in _CACHE:
        x, sparse = P.case_inputs(case)
        _CACHE[key] = (x.to(DEV), sparse.to(DEV))
    return _CACHE[key]


def _pnp(case, **kw):
    """A HipPnPInference of a fixture case (iters and alpha from the fixture unless given)."""
    from radar_depth_amd.main import HipPnPInference
    key = ("pnp", case) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        h, w = (P.ZERO_H, P.ZERO_W) if case == "zero" else (P.H, P.W)
        gd = P.golden("lf_upproj")
        args = dict(iters=int(gd["iters"][0]), alpha=float(gd["alpha"][0]))
        args.update(kw)
        _CACHE[key] = HipPnPInference(_model(case, h, w), 1, h, w, **args)
    return _CACHE[key]


def _explicit(case):
    """The sparse plane to pass: None where the network reads it itself (four planes), the plane where it does not (rgb)."""
    return _inputs(case)[1] if P.CASES[case][3] else None


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ teacher-forced iterations
@pytest.mark.parametrize("case", sorted(P.CASES))
def test_teacher_forced_iterations(case):
    gd = P.golden(case)
    pnp = _pnp(case)
    x, _ = _inputs(case)
    z0 = _np(pnp.front(x, _explicit(case)))
    assert z0.shape == gd["z_0"].shape
    print("%s front: z rel err %.3g" % (case, _rel(z0, gd["z_0"])))
    assert _rel(z0, gd["z_0"]) <= BAR
    for k in range(int(gd["iters"][0])):
        zk, gk = gd["z_%d" % k], gd["g_%d" % k]
        pnp.z.copy_(torch.from_numpy(zk).float())
        pred = _np(pnp.rear())
        g = _np(pnp.grad())
        loss = float(pnp.last_loss.item())
        gmax = np.abs(gk).max()
        print("%s k=%d: pred rel err %.3g, g rel err %.3g, loss %.7g (reference %.7g)" % (case, k, _rel(pred, gd["pred_%d" % k]),
                                                                                          _rel(g, gk), loss, gd["loss_%d" % k][0]))
        assert _rel(pred, gd["pred_%d" % k].astype(np.float64)) <= BAR
        assert _rel(g, gk) <= BAR
        big = np.abs(gk) > BAR * gmax
        assert big.any() and np.array_equal(np.sign(g)[big], np.sign(gk)[big])
        assert abs(loss - gd["loss_%d" % k][0]) <= 1e-5 * gd["loss_%d" % k][0]
        if k < len(pnp.losses):
            assert float(pnp.losses[k].item()) == loss
        # the update: one fp32 rounding of z - alpha * sign(g), formed in numpy from the readbacks
        zb = _np(pnp.z).copy()
        za = _np(pnp.update())
        assert np.array_equal(za, zb - np.float32(pnp.alpha) * np.sign(g))
    assert all(q.grad is None for q in _model(case).parameters())


def test_exact_zeros_outside_the_receptive_field():
    """One valid pixel in the corner: g is exactly zero wherever the reference's is, with every gradient buffer of the backward
    poisoned beforehand -- a stale buffer, a missing zero fill or a gate read from the wrong slice cannot hide."""
    gd = P.golden("zero")
    pnp = _pnp("zero")
    x, sparse = _inputs("zero")
    pnp.front(x)
    pnp.rear()
    for name, a in pnp.plan.taps.items():
        if name.startswith("pnp_grad"):
            a.t.fill_(float("nan"))
    pnp.plan.dpred.fill_(float("nan"))
    pnp.plan.pnp_ddm.fill_(float("nan"))
    g = _np(pnp.grad())
    zero = gd["g_0"] == 0
    assert zero.sum() > 0.9 * zero.size
    assert (g[zero] == 0).all() and np.isfinite(g).all()
    print("zero case: g rel err %.3g" % _rel(g, gd["g_0"]))
    assert _rel(g, gd["g_0"]) <= BAR
    assert abs(float(pnp.last_loss.item()) - gd["loss_0"][0]) <= 1e-5 * gd["loss_0"][0]


# ------------------------------------------------------------------------------------------------ the loop
@pytest.mark.parametrize("case", sorted(P.CASES))
def test_loop_three_ways_bit_identical(case):
    gd = P.golden(case)
    iters = int(gd["iters"][0])
    x, _ = _inputs(case)
    sp = _explicit(case)
    graph = _pnp(case)
    for _ in range(3):
        r_graph = graph(x, sp).clone()
    assert graph.graph is not None
    l_graph = graph.losses.clone()
    plain = _pnp(case, use_graph=False)
    r_plain = plain(x, sp).clone()
    assert plain.graph is None
    hand = _pnp(case, use_graph=False)
    hand.front(x, sp)
    for k in range(iters):
        r_hand = hand.rear()
        if k < iters - 1:
            hand.grad()
            hand.update()
    assert torch.equal(r_graph, r_plain) and torch.equal(r_graph, r_hand)
    assert torch.equal(l_graph, plain.losses) and l_graph.shape == (iters - 1,)
    bar = max(BAR, 4 * float(gd["d32"][0]))
    print("%s loop: final rel err %.3g (bar %.3g), losses %s" % (case, _rel(_np(r_graph), gd["final"].astype(np.float64)), bar, _np(l_graph)))
    assert _rel(_np(r_graph), gd["final"].astype(np.float64)) <= bar
    for k in range(iters - 1):
        assert abs(float(l_graph[k].item()) - gd["loss_%d" % k][0]) <= 1e-4 * gd["loss_%d" % k][0]


@pytest.mark.parametrize("case", ["lf_upproj", "rn_deconv2_rgb"])
def test_one_iteration_is_the_plain_prediction(case):
    from radar_depth_amd.main import HipInference
    x, _ = _inputs(case)
    one = _pnp(case, iters=1)
    assert one.losses.shape == (0,)
    got = [one(x, _explicit(case)).clone() for _ in range(2)][-1]
    inf = HipInference(_model(case), 1, P.H, P.W)
    want = [inf(x).clone() for _ in range(2)][-1]
    assert torch.equal(got, want)
    assert _rel(_np(got), P.golden(case)["pred_0"].astype(np.float64)) <= BAR


# ------------------------------------------------------------------------------------------------ the drop-in route
def test_drop_in_route_matches_the_object():
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    case = "lf_upproj"
    model, (x, sparse), pnp = _model(case), _inputs(case), _pnp(case)
    pnp.front(x)
    pred_obj = pnp.rear().clone()
    g_obj = pnp.grad().clone()
    z = model.pnp_forward_front(x)
    assert torch.equal(z, pnp.z) and z.is_contiguous()
    z.requires_grad_()
    pred = model.pnp_forward_rear(z)
    assert torch.equal(pred, pred_obj) and pred.requires_grad
    loss = MaskedL1Loss()(pred, sparse)
    g, = torch.autograd.grad(loss, z, retain_graph=True)
    assert torch.equal(g, g_obj)
    assert all(q.grad is None for q in model.parameters())
    # torch's own arithmetic as the criterion: the same gradient up to the rounding of 1 / count
    mask = sparse > 0
    g_t, = torch.autograd.grad((sparse - pred)[mask].abs().mean(), z)
    assert _rel(_np(g_t), _np(g_obj).astype(np.float64)) <= 1e-5
    # a gradient taken after another rear pass of the same plan would read that pass's activations: refused
    pred2 = model.pnp_forward_rear(z)
    model.pnp_forward_rear(z.detach())
    with pytest.raises(RuntimeError, match="another forward"):
        torch.autograd.grad(pred2.sum(), z)
    with torch.no_grad():
        assert not model.pnp_forward_rear(z).requires_grad
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            model.pnp_forward_front(x)
        with pytest.raises(RuntimeError, match="eval mode"):
            model.pnp_forward_rear(z)
    finally:
        model.eval()


def test_drop_in_route_batch_of_two():
    """The loss is the mean over the valid pixels of the whole batch (the reference's criterion): the same frame twice gives the same
    g rows, each half the b = 1 value."""
    from radar_depth_amd.evaluation.criteria_new import MaskedL1Loss
    case = "lf_upproj"
    model, (x, sparse) = _model(case), _inputs(case)

    def grad_of(xb, sb):
        z = model.pnp_forward_front(xb).requires_grad_()
        g, = torch.autograd.grad(MaskedL1Loss()(model.pnp_forward_rear(z), sb), z)
        return _np(g).astype(np.float64)
    g1 = grad_of(x, sparse)
    g2 = grad_of(torch.cat([x, x]), torch.cat([sparse, sparse]))
    assert g2.shape == (2,) + g1.shape[1:] and np.array_equal(g2[0], g2[1])
    assert np.abs(g2[0] - 0.5 * g1[0]).max() <= 1e-6 * np.abs(0.5 * g1[0]).max()


# ------------------------------------------------------------------------------------------------ no valid pixel
def test_empty_sparse_plane():
    case = "lf_upproj"
    x, sparse = _inputs(case)
    pnp = _pnp(case, use_graph=False)
    z0 = pnp.front(x).clone()
    plain = pnp.rear().clone()
    got = pnp(x, torch.zeros_like(sparse)).clone()
    assert torch.equal(pnp.z, z0)
    assert torch.equal(got, plain)
    assert bool(torch.isnan(pnp.losses).all()) and pnp.losses.numel() == 2
    assert bool((pnp.g == 0).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from radar_depth_amd.main import HipPnPInference
    from radar_depth_amd.model.multistage_model import ResNet_multistage
    model = _model("lf_upproj")
    with pytest.raises(NotImplementedError, match="bf16"):
        model._plan(1, P.H, P.W, False, bf16=True, pnp=True)
    with pytest.raises(NotImplementedError, match="bf16"):
        model._plan(1, P.H, P.W, False, bf16=True, storage="bf16", pnp=True)
    with pytest.raises(NotImplementedError, match="bf16"):
        _model("rn_upproj_rgbd")._plan(1, P.H, P.W, False, bf16=True, pnp=True)
    rgb = _pnp("rn_deconv2_rgb")
    x, sparse = _inputs("rn_deconv2_rgb")
    with pytest.raises(ValueError, match="sparse"):
        rgb(x)
    with pytest.raises(ValueError, match="sparse"):
        rgb.front(x)
    with pytest.raises(NotImplementedError, match="ResNet_multistage"):
        HipPnPInference(ResNet_multistage(18, "upproj", [P.H, P.W], False), 1, P.H, P.W)
    with pytest.raises(ValueError, match="criterion"):
        HipPnPInference(model, 1, P.H, P.W, criterion="berhu")
    with pytest.raises(ValueError, match="iters"):
        HipPnPInference(model, 1, P.H, P.W, iters=0)

"""GPU parity of the stem kernels at the early-fusion shapes: four input planes -> 64 channels (modality rgbd) and one plane -> 64
channels (modality d), through the C ABI with four-entry plane tables.  The bodies and the bars are those of tests/test_gpu_stem.py."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [
    (2, 4, 64, 97, 161),      # RGB-D stem, ragged tiles in both directions
    (16, 4, 64, 450, 800),    # the geometry users run
    (1, 4, 64, 15, 63),       # a single ragged tile row
    (3, 4, 64, 9, 11),        # tiles smaller than the kernels' blocks
    (2, 1, 64, 97, 161),      # modality d: one plane, 64 channels
]


def _tables(x, cin, h, w, first=1):
    """Plane pointers / image strides of planes first .. first + cin - 1 of the wider NCHW tensor x, as four-entry arrays."""
    hw, ctot = h * w, x.shape[1]
    planes = (C.c_void_p * 4)(*[x.data_ptr() + 4 * hw * (first + c) if c < cin else None for c in range(4)])
    strides = (C.c_int64 * 4)(*[ctot * hw if c < cin else 0 for c in range(4)])
    return planes, strides


@pytest.mark.parametrize("cfg", SHAPES)
def test_stem4_forward(cfg):
    """rd_stem_fwd (fp32 MFMA) against torch CPU fp32 conv2d, incl. the BatchNorm partial sums."""
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    L = lib()
    n, cin, cout, h, w = cfg
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, cin + 1, h, w, generator=g)          # the stem reads planes 1.. of a wider NCHW tensor (strided images)
    wt = torch.randn(cout, cin, 7, 7, generator=g) * 0.1
    y = F.conv2d(x[:, 1:], wt, stride=2, padding=3)
    xg = x.cuda()
    planes, strides = _tables(xg, cin, h, w)
    wp = wt.permute(2, 3, 1, 0).reshape(49, cin, cout).contiguous().cuda()
    ho, wo = y.shape[2], y.shape[3]
    out = torch.full((n, ho, wo, cout), float("nan"), device="cuda")
    tiles = L.rd_stem_stat_tiles(n, h, w)
    stat = torch.zeros(tiles, 2, cout, device="cuda")
    check(L.rd_stem_fwd(planes, strides, cin, n, h, w, ptr(wp), cout, ptr(out), ptr(stat), current_stream()), "rd_stem_fwd")
    torch.cuda.synchronize()
    got = out.permute(0, 3, 1, 2).cpu()
    assert not torch.isnan(got).any()
    err = ((got - y).abs().max() / y.abs().max()).item()
    print("stem4 forward %s: %.2e of the output's max" % (cfg, err))
    assert err < 2e-5, cfg
    s_ = stat.sum(0).cpu().double()
    ref_s, ref_q = y.double().sum((0, 2, 3)), (y.double() ** 2).sum((0, 2, 3))
    assert ((s_[0] - ref_s).abs().max() / ref_q.sqrt().max()).item() < 1e-4
    assert ((s_[1] - ref_q).abs().max() / ref_q.max()).item() < 1e-4


@pytest.mark.parametrize("cfg", SHAPES)
def test_stem4_forward_split(cfg):
    """rd_stem_fwd_split against an fp64 convolution, inputs spanning 2^-20 .. 2^20 in magnitude: within twice the fp32-MFMA kernel's
    error on the same input (+ 1e-7) and within 2e-5; statistics within 1e-5 of the fp32 kernel's.  (Three planes were observed at
    2e-6; with 196 products per output the figure is printed, not required.)"""
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    L = lib()
    n, cin, cout, h, w = cfg
    g = torch.Generator().manual_seed(6)
    x = torch.randn(n, cin + 1, h, w, generator=g)
    x[:, 1:, : h // 3] *= 2.0 ** 20                         # dynamic range: the pieces of large and of tiny values
    x[:, 1:, 2 * h // 3:] *= 2.0 ** -20
    wt = torch.randn(cout, cin, 7, 7, generator=g) * 0.1
    xg, wg = x.cuda(), wt.cuda()
    y = F.conv2d(xg[:, 1:].double(), wg.double(), stride=2, padding=3)
    planes, strides = _tables(xg, cin, h, w)
    wp = wt.permute(2, 3, 1, 0).reshape(49, cin, cout).contiguous().cuda()
    ho, wo = y.shape[2], y.shape[3]
    tiles = L.rd_stem_stat_tiles(n, h, w)
    res = {}
    for name, fn in (("split", L.rd_stem_fwd_split), ("fp32", L.rd_stem_fwd)):
        out = torch.full((n, ho, wo, cout), float("nan"), device="cuda")
        stat = torch.zeros(tiles, 2, cout, device="cuda")
        check(fn(planes, strides, cin, n, h, w, ptr(wp), cout, ptr(out), ptr(stat), current_stream()), name)
        torch.cuda.synchronize()
        got = out.permute(0, 3, 1, 2).double()
        assert not torch.isnan(got).any()
        # per third of the image (each has its own magnitude): error relative to that third's largest output
        errs = []
        for lo, hi in ((0, ho // 3 - 2), (ho // 3 + 2, 2 * ho // 3 - 2), (2 * ho // 3 + 2, ho)):
            if hi > lo:
                errs.append(((got[:, :, lo:hi] - y[:, :, lo:hi]).abs().max() / y[:, :, lo:hi].abs().max()).item())
        if not errs:      # (an output of a few rows: every row mixes the thirds' magnitudes -- relative to the whole output's largest value)
            errs.append(((got - y).abs().max() / y.abs().max()).item())
        res[name] = (max(errs), stat)
    print("stem4 forward split %s: split %.2e, fp32-MFMA %.2e of the output's max" % (cfg, res["split"][0], res["fp32"][0]))
    assert res["split"][0] < 2.0 * res["fp32"][0] + 1e-7, (cfg, res["split"][0], res["fp32"][0])
    assert res["split"][0] < 2e-5, (cfg, res["split"][0])
    s_, f_ = res["split"][1].sum(0).double(), res["fp32"][1].sum(0).double()
    assert ((s_ - f_).abs().max() / f_.abs().max()).item() < 1e-5


def test_stem4_wgrad_split_supported():
    from radar_depth_amd._lib import lib
    L = lib()
    assert L.rd_stem_wgrad_split_supported(4, 64) == 1
    assert L.rd_stem_wgrad_split_supported(1, 64) == 1
    assert L.rd_stem_wgrad_split_supported(5, 64) == 0
    assert L.rd_stem_wgrad_split_supported(3, 64) == 1 and L.rd_stem_wgrad_split_supported(1, 16) == 1      # (as before)


@pytest.mark.parametrize("cfg", SHAPES)
def test_stem4_wgrad(cfg):
    """rd_stem_wgrad_t (fp32 MFMA) and rd_stem_wgrad_split_t (three-piece operands on the bf16 matrix cores) on an fp32 output gradient
    against the fp64 weight gradient; every element written (NaN-filled target and workspace)."""
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    L = lib()
    n, cin, cout, h, w = cfg
    assert L.rd_stem_wgrad_split_supported(cin, cout) == 1
    gen = torch.Generator().manual_seed(17)
    mag = torch.exp2(torch.randint(-12, 13, (n, cin + 1, 1, 1), generator=gen).float())
    x = (torch.randn(n, cin + 1, h, w, generator=gen) * mag).cuda()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dout = (torch.randn(n, ho, wo, cout, generator=gen) * torch.exp2(torch.randint(-6, 7, (1, 1, 1, cout), generator=gen).float())).cuda()
    planes, strides = _tables(x, cin, h, w)
    nws = int(L.rd_stem_wgrad_workspace_floats(n, h, w, cin, cout))
    want = torch.nn.grad.conv2d_weight(x[:, 1:].double(), (cout, cin, 7, 7), dout.double().permute(0, 3, 1, 2).contiguous(), stride=2, padding=3).cpu()
    err = {}
    for name, fn in (("fp32", L.rd_stem_wgrad_t), ("split", L.rd_stem_wgrad_split_t)):
        ws = torch.full((nws,), float("nan"), device="cuda")
        gw = torch.full((cout, cin, 7, 7), float("nan"), device="cuda")
        check(fn(0, planes, strides, cin, n, h, w, ptr(dout), cout, ptr(gw), ptr(ws), current_stream()), name)
        torch.cuda.synchronize()
        got = gw.cpu().double()
        assert not torch.isnan(got).any(), (cfg, name)
        err[name] = ((got - want).abs().max() / want.abs().max()).item()
    print("stem4 wgrad %s: fp32-MFMA %.2e, split %.2e of the gradient's max" % (cfg, err["fp32"], err["split"]))
    assert err["split"] < 1.5 * err["fp32"] + 2e-7, (cfg, err)
    assert err["split"] < 2e-5, (cfg, err)


@pytest.mark.parametrize("cfg", SHAPES)
def test_stem4_wgrad_split_bn_same_bits_as_two_passes(cfg):
    """rd_stem_wgrad_split_bn_t against rd_bn_bwd_apply_t + rd_stem_wgrad_split_t on the same tensors: bit-identical weight gradient,
    dgamma, dbeta."""
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    L = lib()
    n, cin, cout, h, w = cfg
    gen = torch.Generator().manual_seed(11)
    x_in = torch.randn(n, cin, h, w, generator=gen).cuda()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    m = n * ho * wo
    raw = (torch.randn(n, ho, wo, cout, generator=gen) * 1.5 + 0.3).cuda()
    g = (torch.randn(n, ho, wo, cout, generator=gen) * (torch.rand(n, ho, wo, cout, generator=gen) < 0.3)).cuda()   # pooled gradients are sparse
    gamma = (torch.rand(cout, generator=gen) + 0.5).cuda()
    mean = raw.mean((0, 1, 2))
    invstd = 1.0 / torch.sqrt(raw.var((0, 1, 2), unbiased=False) + 1e-5)
    tiles = L.rd_bn_bwd_tiles(C.c_int64(m), cout)
    red = torch.zeros(tiles, 3, cout, device="cuda")
    check(L.rd_bn_bwd_reduce_t(0, ptr(g), cout, None, 0, ptr(raw), cout, ptr(mean), None, 0, None, None, 0, C.c_int64(m), cout, 0, ptr(red),
                               current_stream()), "rd_bn_bwd_reduce_t")
    planes, strides = _tables(x_in, cin, h, w, first=0)
    nws = L.rd_stem_wgrad_workspace_floats(n, h, w, cin, cout)
    res = []
    for fused in (0, 1):
        ws = torch.full((int(nws),), float("nan"), device="cuda")
        dg, db = torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")
        coef = torch.zeros(3 * cout, device="cuda")
        gw = torch.full((cout, cin, 7, 7), float("nan"), device="cuda")
        if fused:
            check(L.rd_stem_wgrad_split_bn_t(0, planes, strides, cin, n, h, w, ptr(g), ptr(raw), ptr(red), tiles, ptr(gamma), ptr(mean), ptr(invstd),
                                             ptr(dg), ptr(db), ptr(coef), cout, ptr(gw), ptr(ws), current_stream()), "rd_stem_wgrad_split_bn_t")
        else:
            dx = torch.empty_like(raw)
            check(L.rd_bn_bwd_apply_t(0, ptr(g), cout, ptr(raw), cout, ptr(red), tiles, 1, ptr(gamma), ptr(mean), ptr(invstd), ptr(dg), ptr(db),
                                      ptr(coef), ptr(dx), cout, C.c_int64(m), cout, current_stream()), "rd_bn_bwd_apply_t")
            check(L.rd_stem_wgrad_split_t(0, planes, strides, cin, n, h, w, ptr(dx), cout, ptr(gw), ptr(ws), current_stream()), "rd_stem_wgrad_split_t")
        torch.cuda.synchronize()
        res.append((gw.cpu(), dg.cpu(), db.cpu()))
    for a_, b_ in zip(res[0], res[1]):
        assert not torch.isnan(b_).any()
        assert torch.equal(a_, b_), cfg


def test_stem_five_planes_is_an_error():
    """Cin = 5 returns an error code from every entry point and launches nothing (the NaN-filled targets stay untouched)."""
    from radar_depth_amd._lib import current_stream, lib, ptr
    L = lib()
    n, cin, cout, h, w = 1, 5, 64, 15, 63
    x = torch.randn(n, cin, h, w).cuda()
    hw = h * w
    planes = (C.c_void_p * 5)(*[x.data_ptr() + 4 * hw * c for c in range(5)])
    strides = (C.c_int64 * 5)(*[cin * hw] * 5)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    wp = torch.zeros(49, cin, cout, device="cuda")
    out = torch.full((n, ho, wo, cout), float("nan"), device="cuda")
    dout = torch.zeros(n, ho, wo, cout, device="cuda")
    gw = torch.full((cout, cin, 7, 7), float("nan"), device="cuda")
    ws = torch.zeros(int(L.rd_stem_wgrad_workspace_floats(n, h, w, cin, cout)), device="cuda")
    assert L.rd_stem_fwd(planes, strides, cin, n, h, w, ptr(wp), cout, ptr(out), None, current_stream()) != 0
    assert L.rd_stem_fwd_split(planes, strides, cin, n, h, w, ptr(wp), cout, ptr(out), None, current_stream()) != 0
    assert L.rd_stem_wgrad_t(0, planes, strides, cin, n, h, w, ptr(dout), cout, ptr(gw), ptr(ws), current_stream()) != 0
    assert L.rd_stem_wgrad_split_t(0, planes, strides, cin, n, h, w, ptr(dout), cout, ptr(gw), ptr(ws), current_stream()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(gw).all()

"""The producers of pre-split piece planes, EXACTLY.  The headline plan (operands="split", RD_SPLIT_PRE=1) feeds its convolutions and
weight gradients with three bf16 planes [piece][C/16][M][16] written by store_pieces4 (csrc/common.h) from the epilogues of
rd_bn_act_p, rd_bn_bwd_apply_p, rd_bn_bwd_apply_x_p, rd_bn_bwd_apply_x2_p and rd_bnact_maxpool_fwd_p, or by rd_split_pieces; the
consumers only copy them.  "The split is exact" therefore rests on these planes, bit for bit.  No tolerance appears in this file:
every assertion is torch.equal (on values or on bit patterns) or an integer comparison.

For every launch (y = the fp32 tensor the same launch wrote):
  1. the float64 sum of the three planes equals y.double();
  2. piece 0 = bf16(y), piece 1 = bf16(y - p0), piece 2 = bf16(y - p0 - p1), round to nearest even (torch's conversion);
  3. the planes are bit-identical to rd_split_pieces applied to y;
  4. y is bit-identical to what the plain entry point (no planes) writes;
  5. nothing but the written channel blocks changed: the planes live in one canary-filled buffer with slack rows behind each.
The reference conversions run in torch (on the CPU for small cases, with torch's device kernels for the large ones: a conversion, an
exact fp32 subtraction and an exact float64 sum have one right answer)."""
import ctypes as C
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 0x5A5B          # bit pattern of the untouched bf16 elements
SLACK_ROWS = 4           # 16-element rows behind every plane, inside the same buffer
EINVAL = -1


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _ok(rc, what):
    from radar_depth_amd._lib import check
    check(rc, what)


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _p(t, byte_off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + byte_off)


class Planes:
    """Three piece planes of an [m][ctot] tensor in ONE int16 buffer: plane k at k * stride, stride = ctot * m + slack."""

    def __init__(self, ctot, m, slack_rows=SLACK_ROWS):
        self.ctot, self.m = ctot, m
        self.stride = ctot * m + slack_rows * 16
        self.raw = torch.full((3 * self.stride,), CANARY, dtype=torch.int16, device=DEV)

    def ptr(self, c0=0, byte_off=0):
        """Pointer for a producer of channels [c0, ...): the plane base advanced by (c0 / 16) * m * 16 elements (engine._pc_bind)."""
        return C.c_void_p(self.raw.data_ptr() + (c0 // 16) * self.m * 16 * 2 + byte_off)

    def pe(self):
        return C.c_int64(self.stride)

    def blocks(self):
        """int16 bit patterns [3][ctot/16][m][16]"""
        return torch.stack([self.raw[k * self.stride: k * self.stride + self.ctot * self.m].view(self.ctot // 16, self.m, 16) for k in range(3)])

    def slack(self):
        return torch.stack([self.raw[k * self.stride + self.ctot * self.m: (k + 1) * self.stride] for k in range(3)])

    def values(self, c0, c):
        """bf16 [3][m][c]: channels [c0, c0 + c) reassembled from their 16-channel blocks"""
        b = self.blocks()[:, c0 // 16: (c0 + c) // 16].view(torch.bfloat16)
        return b.permute(0, 2, 1, 3).reshape(3, self.m, c)

    def as_tensor(self):
        assert self.stride == self.ctot * self.m
        return self.raw.view(torch.bfloat16).view(3, self.ctot // 16, self.m, 16)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _split_pieces_into(pl, x, ldx, c0, c, byte_off_x=0):
    _ok(_L().rd_split_pieces(_p(x, byte_off_x), ldx, C.c_int64(pl.m), c, pl.ptr(c0), pl.pe(), _st()), "rd_split_pieces")


def _check_pieces(pl, c0, y, y_plain=None, only=None, whole_buffer=True):
    """Checks 1-5 for channels [c0, c0 + c) of pl against y [m][c] (fp32, what the launch wrote).  only: bool mask [m][c] of the entries
    that checks 1-3 cover (the non-finite case).  whole_buffer: nothing else of the buffer may differ from the canary."""
    torch.cuda.synchronize()
    m, c = y.shape
    y = y.contiguous()
    got = pl.values(c0, c)
    if y.numel() <= (1 << 22):          # small: torch's CPU kernels are the reference
        y_, got_ = y.cpu(), got.cpu()
    else:
        y_, got_ = y, got
    fin = torch.isfinite(y_)
    sel = fin if only is None else only.to(y_.device)
    if only is None:
        assert bool(fin.all())
        assert bool(((y_ == 0) | (y_.abs() >= 2.0 ** -100)).all()), "test input outside the range the exactness claim is made for"
    # 1. exact sum
    s = got_[0].double() + got_[1].double() + got_[2].double()
    assert torch.equal(s[sel], y_.double()[sel]), "p0 + p1 + p2 != y"
    # 2. piece values, round to nearest even
    p0 = y_.to(torch.bfloat16)
    r1 = y_ - p0.float()
    p1 = r1.to(torch.bfloat16)
    p2 = (r1 - p1.float()).to(torch.bfloat16)
    for k, want in enumerate((p0, p1, p2)):
        assert torch.equal(_bits(got_[k])[sel], _bits(want)[sel]), "piece %d is not bf16_rne of the running remainder" % k
    # 3. same bits as the stand-alone producer on the same y
    ref = Planes(c, m)
    _split_pieces_into(ref, y, c, 0, c)
    torch.cuda.synchronize()
    a, b = pl.blocks()[:, c0 // 16: (c0 + c) // 16], ref.blocks()
    if only is None:
        assert torch.equal(a, b), "planes differ from rd_split_pieces(y)"
    else:
        mk = only.to(DEV).view(m, c // 16, 16).permute(1, 0, 2).expand(3, -1, -1, -1)
        assert torch.equal(a[mk], b[mk])
    assert bool((ref.slack() == CANARY).all())
    # 4. the fp32 output does not depend on the planes being written
    if y_plain is not None:
        assert torch.equal(_bits(y), _bits(y_plain)), "the fp32 output changed with the piece planes"
    # 5. no stray writes
    assert bool((pl.slack() == CANARY).all()), "a producer wrote behind a plane"
    if whole_buffer:
        blk = pl.blocks()
        assert bool((blk[:, : c0 // 16] == CANARY).all()) and bool((blk[:, (c0 + c) // 16:] == CANARY).all()), "a producer wrote a block it does not own"


def _values(shape, g):
    """Every magnitude 2^-30 .. 2^30 per element, exact +0.0 / -0.0 and bf16-representable values sprinkled in."""
    v = torch.randn(shape, generator=g, device=DEV) * torch.exp2(torch.randint(-30, 31, shape, generator=g, device=DEV).float())
    f = v.view(-1)
    f[::97] = 0.0
    f[5::193] = -0.0
    f[7::389] = f[7::389].to(torch.bfloat16).float()
    return v


def _coef(c, g):
    """Per-channel scale / shift; the first four channels of every block pass x through times a power of two (shift exactly 0), so
    that y keeps the zeros, the signed zero and the bf16-representable values of x."""
    sc = torch.rand(c, generator=g, device=DEV) + 0.5
    sh = torch.randn(c, generator=g, device=DEV) * 0.1
    ch = torch.arange(c, device=DEV)
    thru = ch % 16 < 4
    sc[thru] = torch.exp2(((ch[thru] // 16) % 5 - 2).float())
    sh[thru] = 0.0
    return sc, sh


def _bn_act(x1, ldx1, s1, t1, x2, ldx2, s2, t2, y, ldy, m, c, act, pc=None, pe=None, y_off=0, c_arg=None):
    """rd_bn_act (pc is None) or rd_bn_act_p; returns the status code."""
    L = _L()
    a = (_p(x1), ldx1, _p(s1), _p(t1), _p(x2), ldx2, _p(s2), _p(t2), _p(y, y_off), ldy, C.c_int64(m), c if c_arg is None else c_arg, act)
    if pc is None:
        return L.rd_bn_act(*a, _st())
    return L.rd_bn_act_p(*a, pc, pe, _st())


BN_ACT_SHAPES = [(1, 16), (1, 640), (1, 48), (3, 32), (3, 512), (3, 48), (255, 48), (255, 128), (255, 640), (256, 16), (256, 64), (256, 512),
                 (257, 48), (257, 32), (257, 128), (22600, 64), (22600, 640), (22600, 48), (22600, 512), (361600, 16), (361600, 64),
                 (361600, 48)]
# act in {none, ReLU, leaky} x second operand in {none, identity, BatchNorm}: all nine over the first nine shapes, then again
BN_ACT_CASES = [(m, c, i % 3, (None, "id", "bn")[(i // 3) % 3]) for i, (m, c) in enumerate(BN_ACT_SHAPES)]


@pytest.mark.parametrize("m,c,act,res", BN_ACT_CASES)
def test_bn_act_p(m, c, act, res):
    g = torch.Generator(device=DEV).manual_seed(1000 + m + c)
    x1 = _values((m, c), g)
    s1, t1 = _coef(c, g)
    x2 = _values((m, c), g) if res else None
    s2, t2 = _coef(c, g) if res == "bn" else (None, None)
    y0 = torch.full((m, c), float("nan"), device=DEV)
    y = torch.full((m, c), float("nan"), device=DEV)
    pl = Planes(c, m)
    _ok(_bn_act(x1, c, s1, t1, x2, c if res else 0, s2, t2, y0, c, m, c, act), "rd_bn_act")
    _ok(_bn_act(x1, c, s1, t1, x2, c if res else 0, s2, t2, y, c, m, c, act, pl.ptr(), pl.pe()), "rd_bn_act_p")
    _check_pieces(pl, 0, y, y0)


def test_bn_act_p_non_finite():
    """A few inf / NaN inputs: piece 0 is bf16(y) there, the plane sum is non-finite at exactly those entries, every other entry keeps
    checks 1-3."""
    m, c = 257, 48
    g = torch.Generator(device=DEV).manual_seed(77)
    x1 = _values((m, c), g)
    s1, t1 = _coef(c, g)
    bad = [(0, 0, float("inf")), (3, 17, float("-inf")), (100, 47, float("nan")), (256, 32, float("inf")), (255, 5, float("nan"))]
    for r, k, v in bad:
        x1[r, k] = v
    y0, y = torch.empty(m, c, device=DEV), torch.empty(m, c, device=DEV)
    pl = Planes(c, m)
    _ok(_bn_act(x1, c, s1, t1, None, 0, None, None, y0, c, m, c, 0), "rd_bn_act")
    _ok(_bn_act(x1, c, s1, t1, None, 0, None, None, y, c, m, c, 0, pl.ptr(), pl.pe()), "rd_bn_act_p")
    torch.cuda.synchronize()
    yc = y.cpu()
    fin = torch.isfinite(yc)
    assert int((~fin).sum()) == len(bad) and all(not fin[r, k] for r, k, _ in bad)
    got = pl.values(0, c).cpu()
    want0 = yc.to(torch.bfloat16)
    assert torch.equal(torch.isnan(got[0]), torch.isnan(want0))
    assert torch.equal(got[0][~torch.isnan(want0)], want0[~torch.isnan(want0)])          # +-inf and every finite entry
    s = got[0].double() + got[1].double() + got[2].double()
    assert torch.equal(torch.isfinite(s), fin)
    assert torch.equal(torch.isnan(y0.cpu()), torch.isnan(yc)) and torch.equal(y0.cpu()[fin], yc[fin])
    _check_pieces(pl, 0, y, None, only=fin)


# ------------------------------------------------------------------------------------------------ BatchNorm backward producers
def _bwd_setup(m, c, act, res, seed):
    """Inputs of the BatchNorm-backward apply passes, built as tests/test_gpu_norm.py::test_bn_forward_backward builds them: statistics
    and coefficients from rd_bn_stats / rd_bn_finalize, y from rd_bn_act; the output gradient carries 2^-20 .. 2^20 per element."""
    from radar_depth_amd import ops
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(seed)
    S = types.SimpleNamespace(m=m, c=c, act=act, res=res)
    S.x1 = torch.randn(m, c, generator=g, device=DEV) * 2 + 0.5
    S.x2 = torch.randn(m, c, generator=g, device=DEV) if res else None
    S.gam1, S.bet1 = torch.rand(c, generator=g, device=DEV) + 0.5, torch.randn(c, generator=g, device=DEV) * 0.1
    S.gam2, S.bet2 = torch.rand(c, generator=g, device=DEV) + 0.5, torch.randn(c, generator=g, device=DEV) * 0.1

    def coeffs(x, gm, bt):
        part, tiles = ops.bn_stats(x, c)
        out = [torch.empty(c, device=DEV) for _ in range(4)]
        _ok(L.rd_bn_finalize(_p(part), tiles, c, 0, c, C.c_int64(m), _p(gm), _p(bt), C.c_float(1e-5), C.c_float(0.1), None, None, None,
                             _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _st()), "rd_bn_finalize")
        return out

    S.mean1, S.inv1, S.sc1, S.sh1 = coeffs(S.x1, S.gam1, S.bet1)
    if res == "bn":
        S.mean2, S.inv2, S.sc2, S.sh2 = coeffs(S.x2, S.gam2, S.bet2)
    else:
        S.mean2 = S.inv2 = S.sc2 = S.sh2 = None
    S.y = torch.empty(m, c, device=DEV)
    _ok(_bn_act(S.x1, c, S.sc1, S.sh1, S.x2, c if res else 0, S.sc2, S.sh2, S.y, c, m, c, act), "rd_bn_act")
    S.dy = torch.randn(m, c, generator=g, device=DEV) * torch.exp2(torch.randint(-20, 21, (m, c), generator=g, device=DEV).float())
    S.dy.view(-1)[::97] = 0.0
    S.tiles = L.rd_bn_bwd_tiles(C.c_int64(m), c)
    assert S.tiles > 0
    S.red = torch.zeros(S.tiles, 3, c, device=DEV)
    return S


def _outs(c, m):
    return (torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.empty(3 * c, device=DEV), torch.full((m, c), float("nan"), device=DEV))


def _apply(S, which, gt, red, dx, dg, db, coef, pc=None, pe=None, c_arg=None):
    L = _L()
    x, gm, mean, inv = (S.x1, S.gam1, S.mean1, S.inv1) if which == 1 else (S.x2, S.gam2, S.mean2, S.inv2)
    c = S.c if c_arg is None else c_arg
    a = (_p(gt), S.c, _p(x), S.c, _p(red), S.tiles, which, _p(gm), _p(mean), _p(inv), _p(dg), _p(db), _p(coef), _p(dx), S.c, C.c_int64(S.m), c)
    return L.rd_bn_bwd_apply(*a, _st()) if pc is None else L.rd_bn_bwd_apply_p(*a, pc, pe, _st())


def _reduce(S, gt):
    bn2 = S.res == "bn"
    _ok(_L().rd_bn_bwd_reduce(_p(S.dy), S.c, _p(S.y), S.c, _p(S.x1), S.c, _p(S.mean1), _p(S.x2) if bn2 else None, S.c if bn2 else 0,
                              _p(S.mean2) if bn2 else None, _p(gt), S.c, C.c_int64(S.m), S.c, S.act, _p(S.red), _st()), "rd_bn_bwd_reduce")


@pytest.mark.parametrize("m,c,act,res,which", [(3, 32, 1, "bn", 1), (3, 32, 1, "bn", 2), (257, 48, 2, "bn", 2), (257, 48, 0, None, 1),
                                               (22600, 64, 1, "bn", 1), (22600, 64, 1, "bn", 2), (77, 640, 1, "bn", 2), (77, 640, 0, None, 1),
                                               (256, 128, 1, "id", 1)])
def test_bn_bwd_apply_p(m, c, act, res, which):
    S = _bwd_setup(m, c, act, res, 2000 + m + c)
    gt = torch.empty(m, c, device=DEV)
    _reduce(S, gt)
    dg0, db0, coef0, dx0 = _outs(c, m)
    dg, db, coef, dx = _outs(c, m)
    pl = Planes(c, m)
    _ok(_apply(S, which, gt, S.red, dx0, dg0, db0, coef0), "rd_bn_bwd_apply")
    _ok(_apply(S, which, gt, S.red, dx, dg, db, coef, pl.ptr(), pl.pe()), "rd_bn_bwd_apply_p")
    _check_pieces(pl, 0, dx, dx0)
    assert torch.equal(_bits(dg), _bits(dg0)) and torch.equal(_bits(db), _bits(db0)) and torch.equal(_bits(coef), _bits(coef0))


def _apply_x(S, red, dx, dg, db, coef, pc=None, pe=None, c_arg=None):
    L = _L()
    c = S.c if c_arg is None else c_arg
    a = (_p(S.dy), S.c, _p(S.x1), S.c, _p(red), S.tiles, _p(S.gam1), _p(S.mean1), _p(S.inv1), _p(S.sc1), _p(S.sh1), S.act, _p(dg), _p(db),
         _p(coef), _p(dx), S.c, C.c_int64(S.m), c)
    return L.rd_bn_bwd_apply_x(*a, _st()) if pc is None else L.rd_bn_bwd_apply_x_p(*a, pc, pe, _st())


def _reduce_x(S):
    _ok(_L().rd_bn_bwd_reduce_x(_p(S.dy), S.c, _p(S.x1), S.c, _p(S.mean1), _p(S.sc1), _p(S.sh1), None, 0, C.c_int64(S.m), S.c, S.act,
                                _p(S.red), _st()), "rd_bn_bwd_reduce_x")


@pytest.mark.parametrize("m,c,act", [(3, 32, 1), (257, 48, 2), (22600, 64, 1), (77, 640, 2), (1, 16, 1)])
def test_bn_bwd_apply_x_p(m, c, act):
    S = _bwd_setup(m, c, act, None, 3000 + m + c)
    _reduce_x(S)
    dg0, db0, coef0, dx0 = _outs(c, m)
    dg, db, coef, dx = _outs(c, m)
    pl = Planes(c, m)
    _ok(_apply_x(S, S.red, dx0, dg0, db0, coef0), "rd_bn_bwd_apply_x")
    _ok(_apply_x(S, S.red, dx, dg, db, coef, pl.ptr(), pl.pe()), "rd_bn_bwd_apply_x_p")
    _check_pieces(pl, 0, dx, dx0)
    assert torch.equal(_bits(dg), _bits(dg0)) and torch.equal(_bits(db), _bits(db0))


def _apply_x2(S, red, o1, o2, coef6, pcs=None, c_arg=None):
    """o1 / o2 = (dgamma, dbeta, _, dx) of each operand; pcs = ((ptr1, pe1), (ptr2, pe2)) with None pointers allowed, or None = plain."""
    L = _L()
    c = S.c if c_arg is None else c_arg
    a = (_p(S.dy), S.c, _p(S.x1), S.c, _p(S.x2), S.c, _p(red), S.tiles, _p(S.gam1), _p(S.mean1), _p(S.inv1), _p(S.sc1), _p(S.sh1), _p(S.gam2),
         _p(S.mean2), _p(S.inv2), _p(S.sc2), _p(S.sh2), S.act, _p(o1[0]), _p(o1[1]), _p(o2[0]), _p(o2[1]), _p(coef6), _p(o1[3]), S.c, _p(o2[3]),
         S.c, C.c_int64(S.m), c)
    if pcs is None:
        return L.rd_bn_bwd_apply_x2(*a, _st())
    (p1, e1), (p2, e2) = pcs
    return L.rd_bn_bwd_apply_x2_p(*a, p1, e1, p2, e2, _st())


def _reduce_x2(S):
    _ok(_L().rd_bn_bwd_reduce_x2(_p(S.dy), S.c, _p(S.x1), S.c, _p(S.mean1), _p(S.sc1), _p(S.sh1), _p(S.x2), S.c, _p(S.mean2), _p(S.sc2),
                                 _p(S.sh2), C.c_int64(S.m), S.c, S.act, _p(S.red), _st()), "rd_bn_bwd_reduce_x2")


@pytest.mark.parametrize("mode", ["both", "first", "second"])
@pytest.mark.parametrize("m,c,act", [(3, 32, 1), (257, 48, 2), (22600, 64, 1), (77, 640, 1)])
def test_bn_bwd_apply_x2_p(m, c, act, mode):
    S = _bwd_setup(m, c, act, "bn", 4000 + m + c)
    _reduce_x2(S)
    a0, b0, a, b = _outs(c, m), _outs(c, m), _outs(c, m), _outs(c, m)
    coef6_0, coef6 = torch.empty(6 * c, device=DEV), torch.empty(6 * c, device=DEV)
    pl1, pl2 = Planes(c, m), Planes(c, m)
    null = (C.c_void_p(0), C.c_int64(0))
    pcs = ((pl1.ptr(), pl1.pe()) if mode != "second" else null, (pl2.ptr(), pl2.pe()) if mode != "first" else null)
    _ok(_apply_x2(S, S.red, a0, b0, coef6_0), "rd_bn_bwd_apply_x2")
    _ok(_apply_x2(S, S.red, a, b, coef6, pcs), "rd_bn_bwd_apply_x2_p")
    torch.cuda.synchronize()
    assert torch.equal(_bits(a[3]), _bits(a0[3])) and torch.equal(_bits(b[3]), _bits(b0[3]))
    if mode != "second":
        _check_pieces(pl1, 0, a[3], a0[3])
    else:
        assert bool((pl1.raw == CANARY).all())
    if mode != "first":
        _check_pieces(pl2, 0, b[3], b0[3])
    else:
        assert bool((pl2.raw == CANARY).all())


# ------------------------------------------------------------------------------------------------ the stem's BatchNorm + act + max-pool
def _maxpool(x, sc, sh, act, n, h, w, c, y, idx, pc=None, pe=None, c_arg=None):
    L = _L()
    a = (_p(x), _p(sc), _p(sh), act, n, h, w, c if c_arg is None else c_arg, _p(y), c, _p(idx))
    return L.rd_bnact_maxpool_fwd(*a, _st()) if pc is None else L.rd_bnact_maxpool_fwd_p(*a, pc, pe, _st())


@pytest.mark.parametrize("n,h,w,c,act", [(2, 49, 81, 64, 1), (2, 50, 80, 16, 2), (1, 7, 9, 16, 2), (3, 8, 9, 16, 1), (1, 9, 8, 64, 2), (2, 1, 5, 16, 1),
                                         (16, 225, 400, 64, 1)])
def test_bnact_maxpool_fwd_p(n, h, w, c, act):
    """The planes are indexed by OUTPUT pixels N * Ho * Wo; the argmax bytes must not depend on the planes either."""
    g = torch.Generator(device=DEV).manual_seed(5000 + h + w)
    x = _values((n, h, w, c), g)
    sc, sh = _coef(c, g)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    m = n * ho * wo
    y0, y = torch.full((m, c), float("nan"), device=DEV), torch.full((m, c), float("nan"), device=DEV)
    i0, i1 = torch.full((m, c), 255, dtype=torch.uint8, device=DEV), torch.full((m, c), 255, dtype=torch.uint8, device=DEV)
    pl = Planes(c, m)
    _ok(_maxpool(x, sc, sh, act, n, h, w, c, y0, i0), "rd_bnact_maxpool_fwd")
    _ok(_maxpool(x, sc, sh, act, n, h, w, c, y, i1, pl.ptr(), pl.pe()), "rd_bnact_maxpool_fwd_p")
    _check_pieces(pl, 0, y, y0)
    assert torch.equal(i0, i1) and int(i1.max()) <= 8


# ------------------------------------------------------------------------------------------------ rd_split_pieces on a slice; slices as bound
@pytest.mark.parametrize("m,ctot,c0,c", [(231, 96, 16, 48), (1, 64, 48, 16), (4097, 640, 512, 128)])
def test_split_pieces_of_a_channel_slice(m, ctot, c0, c):
    """ldx > C: channels [c0, c0 + c) of a wider tensor into planes of their own."""
    g = torch.Generator(device=DEV).manual_seed(6000 + m)
    x = _values((m, ctot), g)
    pl = Planes(c, m)
    _split_pieces_into(pl, x, ctot, 0, c, byte_off_x=4 * c0)
    _check_pieces(pl, 0, x[:, c0: c0 + c].contiguous())


@pytest.mark.parametrize("b_is", ["bn_act_p", "split_pieces"])
@pytest.mark.parametrize("m,ctot,ca", [(750, 640, 512), (257, 64, 16), (22600, 64, 48)])
def test_channel_slices_as_the_plan_binds_them(m, ctot, ca, b_is):
    """A tensor of ctot channels whose planes have stride ctot * m (engine._pc_bind).  Producer A writes channels [0, ca) with
    ldy = ctot and the pointer at the plane base; producer B writes [ca, ctot) with its pointer advanced by (ca / 16) * m * 16 elements.
    After A alone B's blocks still hold the canary; after both the planes are rd_split_pieces of the whole tensor."""
    g = torch.Generator(device=DEV).manual_seed(7000 + m + ca)
    cb = ctot - ca
    xa, xb = _values((m, ca), g), _values((m, cb), g)
    (sa, ta), (sb, tb) = _coef(ca, g), _coef(cb, g)
    y = torch.full((m, ctot), float("nan"), device=DEV)
    pl = Planes(ctot, m)
    _ok(_bn_act(xa, ca, sa, ta, None, 0, None, None, y, ctot, m, ca, 1, pl.ptr(0), pl.pe()), "A: rd_bn_act_p")
    torch.cuda.synchronize()
    assert bool((pl.blocks()[:, ca // 16:] == CANARY).all()), "producer A wrote into B's channel blocks"
    assert bool(torch.isnan(y[:, ca:]).all())
    _check_pieces(pl, 0, y[:, :ca].contiguous())
    if b_is == "bn_act_p":
        _ok(_bn_act(xb, cb, sb, tb, None, 0, None, None, y, ctot, m, cb, 2, pl.ptr(ca), pl.pe(), y_off=4 * ca), "B: rd_bn_act_p")
    else:
        y[:, ca:] = xb
        _split_pieces_into(pl, y, ctot, ca, cb, byte_off_x=4 * ca)
    _check_pieces(pl, ca, y[:, ca:].contiguous(), whole_buffer=False)
    _check_pieces(pl, 0, y[:, :ca].contiguous(), whole_buffer=False)          # B left A's blocks alone
    whole = Planes(ctot, m)
    _split_pieces_into(whole, y, ctot, 0, ctot)
    torch.cuda.synchronize()
    assert torch.equal(pl.raw, whole.raw), "the two slices together are not rd_split_pieces of the whole tensor"
    _check_pieces(whole, 0, y)


# ------------------------------------------------------------------------------------------------ consumers
def test_consumers_see_the_same_operands():
    """rd_gconv_split_pre and rd_wgrad_split_pre fed with producer-written planes give bit-identical results to the same launches fed
    by ops.split_pieces(y)."""
    from radar_depth_amd import convdesc as cd, ops
    n, h, w, ci, co = 2, 113, 200, 64, 64          # layer1 of the network at the benchmark geometry
    m = n * h * w
    g = torch.Generator(device=DEV).manual_seed(8000)
    d = cd.conv_fwd(n, h, w, ci, co, 3, 1, 1)
    assert ops.gconv_split_pre_supported(d) and ops.wgrad_split_pre_supported(d)          # (a layer the default plan routes there)
    planes, ys = [], []
    for cc, act in ((ci, 1), (co, 0)):          # the activation (ReLU'd BatchNorm) and an output gradient
        x = torch.randn(m, cc, generator=g, device=DEV)
        sc, sh = torch.rand(cc, generator=g, device=DEV) + 0.5, torch.randn(cc, generator=g, device=DEV) * 0.1
        y = torch.empty(m, cc, device=DEV)
        pl = Planes(cc, m, slack_rows=0)
        _ok(_bn_act(x, cc, sc, sh, None, 0, None, None, y, cc, m, cc, act, pl.ptr(), pl.pe()), "rd_bn_act_p")
        planes.append(pl.as_tensor())
        ys.append(y.view(n, h, w, cc))
    wt = torch.randn(co, ci, 3, 3, generator=g, device=DEV) * (2.0 / (9 * ci)) ** 0.5
    wp = ops.pack_weights_split(wt)
    res = []
    for xp, gp in ((planes[0], planes[1]), (ops.split_pieces(ys[0]), ops.split_pieces(ys[1]))):
        out = torch.full((n, d.Ho, d.Wo, co), float("nan"), device=DEV)
        ops.gconv_split_pre(d, xp, wp, out)
        slabs = torch.full((ops.wgrad_split_workspace_floats(d),), float("nan"), device=DEV)
        ops.wgrad_split_pre(d, xp, gp, slabs)
        grad = torch.full((co, ci, 3, 3), float("nan"), device=DEV)
        ops.wgrad_split_reduce(d, slabs, grad)
        torch.cuda.synchronize()
        res.append((out, grad))
    assert not torch.isnan(res[0][0]).any() and not torch.isnan(res[0][1]).any()
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))


# ------------------------------------------------------------------------------------------------ argument checks
def _producer_launchers(m, c):
    """name -> f(pieces pointer, piece_elems, c_arg): one launch of each producer at [m][c] (the stem: m pooled pixels).  Every buffer,
    the canary buffer included, is sized for max(c, 32) channels, so that no launch could leave its buffers even if a check were
    missing; c_arg replaces the channel count the entry point is told (the rows keep their stride c)."""
    S = _bwd_setup(m, c, 1, "bn", 9000)
    gt = torch.empty(m, c, device=DEV)
    _reduce(S, gt)
    S1 = _bwd_setup(m, c, 1, None, 9001)
    _reduce_x(S1)
    S2 = _bwd_setup(m, c, 1, "bn", 9002)
    _reduce_x2(S2)
    o = [_outs(c, m) for _ in range(4)]
    coef6 = torch.empty(6 * c, device=DEV)
    y = torch.empty(m, c, device=DEV)
    n, h, w = 1, 2 * m, 1          # pooled: m x 1 pixels
    xs = torch.randn(n, h, w, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9003))
    idx = torch.empty(m, c, dtype=torch.uint8, device=DEV)
    keep = [S, S1, S2, gt, o, coef6, y, xs, idx]
    null = (C.c_void_p(0), C.c_int64(0))
    return keep, {
        "rd_bn_act_p": lambda p, e, ca: _bn_act(S.x1, c, S.sc1, S.sh1, None, 0, None, None, y, c, m, c, 1, p, e, c_arg=ca),
        "rd_bn_bwd_apply_p": lambda p, e, ca: _apply(S, 1, gt, S.red, o[0][3], o[0][0], o[0][1], o[0][2], p, e, c_arg=ca),
        "rd_bn_bwd_apply_x_p": lambda p, e, ca: _apply_x(S1, S1.red, o[1][3], o[1][0], o[1][1], o[1][2], p, e, c_arg=ca),
        "rd_bn_bwd_apply_x2_p(1)": lambda p, e, ca: _apply_x2(S2, S2.red, o[2], o[3], coef6, ((p, e), null), c_arg=ca),
        "rd_bn_bwd_apply_x2_p(2)": lambda p, e, ca: _apply_x2(S2, S2.red, o[2], o[3], coef6, (null, (p, e)), c_arg=ca),
        "rd_bnact_maxpool_fwd_p": lambda p, e, ca: _maxpool(xs, S.sc1, S.sh1, 1, n, h, w, c, y, idx, p, e, c_arg=ca),
        "rd_split_pieces": lambda p, e, ca: _L().rd_split_pieces(_p(S.x1), c, C.c_int64(m), c if ca is None else ca, p, e, _st()),
    }


def test_producers_reject_bad_plane_arguments():
    """C % 16 != 0, a plane pointer that is not 16-byte aligned, piece_elems < C * M and piece_elems % 8 != 0 are RD_EINVAL from every
    producer, before anything is launched (the canary buffer stays untouched).  A good call through the same closure succeeds."""
    m, c = 37, 32
    keep, launchers = _producer_launchers(m, c)
    for name, f in launchers.items():
        pl = Planes(c, m)
        bad = {
            "C % 16 != 0": (pl.ptr(), pl.pe(), 24),
            "misaligned pointer": (pl.ptr(byte_off=8), C.c_int64(c * m), None),
            "piece_elems < C * M": (pl.ptr(), C.c_int64(c * m - 16), None),
            "piece_elems % 8 != 0": (pl.ptr(), C.c_int64(c * m + 4), None),
        }
        for what, (p, e, ca) in bad.items():
            rc = f(p, e, ca)
            torch.cuda.synchronize()
            assert rc == EINVAL, (name, what, rc)
            assert bool((pl.raw == CANARY).all()), (name, what, "wrote planes although it rejected the call")
        assert f(pl.ptr(), pl.pe(), None) == 0, name
        torch.cuda.synchronize()
        assert bool((pl.blocks() != CANARY).any()) and bool((pl.slack() == CANARY).all()), name
    del keep

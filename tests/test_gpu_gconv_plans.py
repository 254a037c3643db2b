"""The fp32 convolution (csrc/gconv.hip: rd_gconv_ws, rd_gconv_fused, rd_gconv_bnbwd) under EVERY plan its tuner can pin -- five
register tiles, both patch chunks, plain / pipelined / half-depth loop, split-K 1 / 2 / 4 with the combine kernel -- and the
inference epilogue of the other convolution families, against a float64 reference on exactly representable data
(tests/gconv_plan_cases.py): whatever plan runs, the result must equal the reference BIT FOR BIT, so one dropped, doubled or
misplaced tap, row, column, chunk, slab or slice, or an activation boundary off by one channel, fails.

Per case, for every candidate of rd_gconv_tune_candidates(d, allow_split = 1), pinned and verified through rd_gconv_plan_info:
  1. rd_gconv_fused on the quarter grid: bias + addend + ReLU on all columns; bias alone; LeakyReLU(0.2) on a column count that is
     no multiple of 32, and on one that is no multiple of 4; ReLU on Cout / 2 columns for the UpProj case.  Output NaN-filled before
     the launch; channel-slice cases carry a sentinel outside the slice (and NaN around the input / addend slices).
  2. rd_gconv_ws with addend and statistics on the unit grid: output bit-exact, statistics rows summed in float64 equal to sum y and
     sum y^2 exactly (NaN-filled rows: every row must be written).
  3. rd_gconv_bnbwd (c3, c3r, c3w; candidates that do not split): dx bit-equal to the plain launch, slots 0 / 1 exact, slot 2 untouched.
  4. ordinary randn values (c3, up, dgs2) at the kernel's existing bar: 2e-5 of the output's largest magnitude against float64.
The split-K workspace is NaN-filled before every launch.  Nothing is committed: every case returns its descriptor to the heuristic."""
import ctypes as C

import pytest
import torch

import gconv_plan_cases as G

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
NAN = float("nan")


def _lib():
    from radar_depth_amd._lib import lib
    return lib()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sliced(t, ld, off, fill):
    """float64 CPU [..., C] -> (float32 CUDA buffer [..., ld or C] with `fill` outside the slice, NHWC view of the slice, flat tensor that
    starts at the slice's first element)."""
    c = t.shape[-1]
    if not ld:
        buf = t.float().cuda().contiguous()
        return buf, buf, buf.view(-1)
    buf = torch.full(tuple(t.shape[:-1]) + (ld,), fill, dtype=torch.float32)
    buf[..., off:off + c] = t.float()
    buf = buf.cuda()
    return buf, buf[..., off:off + c], buf.view(-1)[off:]


class Out:
    """Output buffer of a case: NaN inside the slice and a sentinel outside before every launch; one comparison against `expect`
    (reference inside, sentinel outside) then shows a wrong value, a value left NaN and a write outside the slice alike."""

    def __init__(self, case, d):
        self.c, self.off = d.Cout, case.out_off
        shape = (d.N, d.Ho, d.Wo, d.ldo)
        self.tmpl = torch.full(shape, SENTINEL, device="cuda")
        self.tmpl[..., self.off:self.off + self.c] = NAN
        self.buf = self.tmpl.clone()
        self.flat = self.buf.view(-1)[self.off:]
        self.view = self.buf[..., self.off:self.off + self.c]

    def reset(self):
        self.buf.copy_(self.tmpl)

    def expect(self, ref32):
        e = self.tmpl.clone()
        e[..., self.off:self.off + self.c] = ref32.cuda()
        return e

    def mismatch(self, expect):
        """None when the buffer equals expect (values: -0 == 0; NaN never equal), else a short description."""
        bad = ~(self.buf == expect)
        n = int(bad.sum())
        if n == 0:
            return None
        i = bad.nonzero()[0].tolist()
        return "%d elements differ, first at %s: got %r want %r" % (n, i, float(self.buf[tuple(i)]), float(expect[tuple(i)]))


_DATA = {}


def _data(case, grid):
    """Reference data of a case, computed once and shared (never modified)."""
    key = (case.name, grid)
    if key not in _DATA:
        d = case.desc()
        data = G.make_data(case, grid)
        y = G.conv_ref(d, data["x"], data["w"])
        assert G.covers_output(d) and not torch.isnan(y).any()
        G.check_budget(case, grid, data, y)
        data["y"] = y
        _DATA[key] = data
    return _DATA[key]


def _variants(case, d):
    """(name, bias?, addend?, act, act_cols) of the inference epilogue."""
    co = d.Cout
    a = co // 2 if (co // 2) % 32 else co // 2 + 4          # a multiple of 4, not of 32 (c3r: 20)
    b = a - 2                                               # no multiple of 4           (c3r: 18)
    assert a % 32 != 0 and a % 4 == 0 and b % 4 != 0 and 0 < b < a < co
    v = [("relu_all", True, True, G.ACT_RELU, co), ("bias_only", True, False, G.ACT_NONE, 0),
         ("leaky_%d" % a, True, True, G.ACT_LEAKY02, a), ("leaky_%d_nobias" % b, False, True, G.ACT_LEAKY02, b)]
    if case.kind == "up":
        v.append(("relu_half", True, False, G.ACT_RELU, co // 2))
    return v


class Fused:
    """Device operands and per-variant expectations of the inference form on the quarter grid."""

    def __init__(self, case):
        self.case, self.d = case, case.desc()
        d = self.d
        data = _data(case, "quarter")
        self.w32 = data["w"].float()
        self.xbuf, self.xview, self.x = _sliced(data["x"], case.ldi, case.in_off, NAN)
        self.abuf, self.aview, self.add = _sliced(data["addend"], case.ld_add_, case.add_off, NAN)
        self.bias = data["bias"].float().cuda()
        self.out = Out(case, d)
        self.variants = []
        for name, hb, ha, act, cols in _variants(case, d):
            ref = G.epilogue_ref(data["y"], data["bias"] if hb else None, data["addend"] if ha else None, act, cols)
            self.variants.append((name, self.bias if hb else None, self.add if ha else None, act, cols, self.out.expect(ref)))

    def run(self, launch, tag, failures):
        """launch(bias, act, act_cols, addend, ld_add) -> rc, for every variant."""
        for name, bias, add, act, cols, expect in self.variants:
            self.out.reset()
            rc = launch(bias, act, cols, add, self.case.ld_add if add is not None else 0)
            assert rc == 0, (self.case.name, tag, name, rc)
            bad = self.out.mismatch(expect)
            if bad:
                failures.append("%s %s %s: %s" % (self.case.name, tag, name, bad))


def _ws(L, d, cache):
    n = int(L.rd_gconv_workspace_floats(C.byref(d)))
    assert n >= 0
    if n == 0:
        return None
    if n not in cache:
        cache[n] = torch.empty(n, device="cuda")
    cache[n].fill_(NAN)
    return cache[n]


def _stat_ok(stat, want):
    """Rows summed in float64 on the device == the reference sums (a NaN row fails)."""
    return bool((stat.double().sum(0) == want).all())


@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_every_plan_is_bit_exact(case):
    L = _lib()
    d = case.desc()
    dref = C.byref(d)
    # state 2 = somebody planned this descriptor without the tuner and it cannot be pinned any more: change the case's shape
    # (1: tests/test_gconv_plans_host.py pinned it earlier in this process and returned it to the heuristic -- still replaceable)
    assert case.name == "c16" or L.rd_gconv_plan_state(dref, 1) != 2, "%s is already planned and in use in this process: change the case's shape" % case.name
    cands = G.candidates(L, d)
    if case.name == "c16":
        assert cands == []
    else:
        assert len(cands) > 1
    fused = Fused(case)
    wq = G.pack_quad(fused.w32, 4).cuda()
    # training form, unit grid
    ud = _data(case, "unit")
    _, _, ux = _sliced(ud["x"], case.ldi, case.in_off, NAN)
    _, _, uadd = _sliced(ud["addend"], case.ld_add_, case.add_off, NAN)
    uwq = G.pack_quad(ud["w"].float(), 4).cuda()
    uy = ud["y"] + ud["addend"]
    uout = Out(case, d)
    u_expect = uout.expect(uy.float())
    u_plain = uout.expect(ud["y"].float())
    u_sums = torch.stack((uy.sum((0, 1, 2)), (uy * uy).sum((0, 1, 2)))).cuda()
    do_bnb = case.name in ("c3", "c3r", "c3w")
    if do_bnb:
        _, _, bnx = _sliced(ud["bn_x"], d.Cout + 8, 4, NAN)
        mean, scale, shift = (ud[k].float().cuda() for k in ("mean", "scale", "shift"))
        b0, b1 = G.bnbwd_ref(ud["y"], ud["bn_x"], ud["mean"], ud["scale"], ud["shift"], G.ACT_RELU)
        b_sums = torch.stack((b0, b1)).cuda()
    do_randn = case.name in ("c3", "up", "dgs2")
    if do_randn:
        rd = G.make_randn(case)
        _, _, rx = _sliced(rd["x"], case.ldi, case.in_off, NAN)
        rwq = G.pack_quad(rd["w"].float(), 4).cuda()
        ry = G.conv_ref(d, rd["x"], rd["w"]).cuda()
        rmax = float(ry.abs().max())
        rout = Out(case, d)
    wsc, failures, n_bnb, worst = {}, [], 0, 0.0
    try:
        for cand in (cands or [None]):
            if cand is not None:
                info = G.pin(L, d, cand)
                assert (info[4] // 100) % 100 == cand[7]
                assert (int(L.rd_gconv_workspace_floats(dref)) > 0) == (cand[7] > 1)
            tag = str(cand)
            # 1. inference form
            ws = _ws(L, d, wsc)
            fused.run(lambda bias, act, cols, add, ld_add: L.rd_gconv_fused(dref, _p(fused.x), _p(wq), _p(fused.out.flat), _p(bias), act, cols,
                                                                             _p(add), ld_add, _p(ws), _stream()), tag, failures)
            # 2. training form: addend + statistics
            tiles = L.rd_gconv_stat_tiles_ws(dref)
            assert tiles > 0
            stat = torch.full((tiles, 2, d.Cout), NAN, device="cuda")
            ws = _ws(L, d, wsc)
            uout.reset()
            assert L.rd_gconv_ws(dref, _p(ux), _p(uwq), _p(uout.flat), _p(uadd), case.ld_add, _p(stat), _p(ws), _stream()) == 0
            bad = uout.mismatch(u_expect)
            if bad:
                failures.append("%s %s training form: %s" % (case.name, tag, bad))
            if not _stat_ok(stat, u_sums):
                failures.append("%s %s statistics: got %s want %s" % (case.name, tag, stat.double().sum(0)[:, :4].tolist(), u_sums[:, :4].tolist()))
            # 3. BatchNorm-backward form
            if do_bnb and (cand is None or cand[7] == 1):
                assert L.rd_gconv_bnbwd_supported(dref) == 1
                n_bnb += 1
                uout.reset()
                assert L.rd_gconv_ws(dref, _p(ux), _p(uwq), _p(uout.flat), None, 0, None, None, _stream()) == 0
                plain = uout.buf.clone()
                red = torch.full((tiles, 3, d.Cout), NAN, device="cuda")
                uout.reset()
                assert L.rd_gconv_bnbwd(dref, _p(ux), _p(uwq), _p(uout.flat), _p(bnx), d.Cout + 8, _p(mean), _p(scale), _p(shift), G.ACT_RELU,
                                        _p(red), None, _stream()) == 0
                bad = uout.mismatch(u_plain)
                if bad or not bool((uout.buf == plain).all()):
                    failures.append("%s %s bnbwd dx: %s" % (case.name, tag, bad or "differs from the plain launch"))
                if not _stat_ok(red[:, :2], b_sums):
                    failures.append("%s %s bnbwd sums: got %s want %s" % (case.name, tag, red[:, :2].double().sum(0)[:, :4].tolist(), b_sums[:, :4].tolist()))
                if not bool(torch.isnan(red[:, 2]).all()):
                    failures.append("%s %s bnbwd wrote slot 2" % (case.name, tag))
            # 4. ordinary values
            if do_randn:
                ws = _ws(L, d, wsc)
                rout.reset()
                assert L.rd_gconv_ws(dref, _p(rx), _p(rwq), _p(rout.flat), None, 0, None, _p(ws), _stream()) == 0
                err = float((rout.view.double() - ry).abs().max()) / rmax
                worst = max(worst, err) if err == err else NAN
                if not err < 2e-5:
                    failures.append("%s %s randn: %g of the largest magnitude" % (case.name, tag, err))
    finally:
        if cands:
            L.rd_gconv_tune_pin(dref, 1, None)
    torch.cuda.synchronize()
    print("%s: %d candidates x %d epilogue variants%s%s" % (case.name, len(cands) or 1, len(fused.variants),
                                                           ", %d with BatchNorm-backward sums" % n_bnb if do_bnb else "",
                                                           ", randn worst %.2e" % worst if do_randn else ""))
    assert not failures, "%d failures, first: %s" % (len(failures), failures[:6])
    if cands:
        assert L.rd_gconv_plan_state(dref, 1) == 1, "nothing may be committed"


# ------------------------------------------------------------------------------------------------ the other families' inference epilogue
@pytest.fixture
def plan_every_shape():
    """The split planners accept every shape their kernels can run (a per-process switch of the library, restored afterwards)."""
    L = _lib()
    prev = L.rd_gconv_split_plan_all(1)
    yield
    L.rd_gconv_split_plan_all(1 if prev == 1 else 0)


@pytest.mark.parametrize("name", ["c3", "c3s", "c1s2", "up"])
def test_split_and_bf16_families_inference_epilogue(name, plan_every_shape):
    """rd_gconv_split, rd_gconv_split_pre (activation split by rd_split_pieces) and rd_gconv_bf16 on their own plans.  Quarter-grid values
    are bf16 numbers, so the second and third pieces are zero, every bf16 product is exact and fp32 accumulation is exact: bit for bit."""
    from radar_depth_amd import ops
    case = G.BY_NAME[name]
    f = Fused(case)
    d = f.d
    assert bool((f.w32.to(torch.bfloat16).float() == f.w32).all())
    assert ops.gconv_split_supported(d) and ops.gconv_split_pre_supported(d), name
    wsp = G.split_operand(f.w32).cuda()
    assert not bool(wsp[1:].float().any()), "quarter-grid weights have no lower pieces"
    wbf = G.pack_quad(f.w32, 8).to(torch.bfloat16).cuda()
    pieces = ops.split_pieces(f.xview)
    assert not bool(pieces[1:].float().any())
    failures = []

    def rc_of(fn):
        def launch(bias, act, cols, add, ld_add):
            fn(bias, act, cols, add, ld_add)
            return 0
        return launch
    f.run(rc_of(lambda b, a, c, ad, ld: ops.gconv_split(d, f.x, wsp, f.out.flat, bias=b, act=a, act_cols=c, addend=ad, ld_add=ld)), "split", failures)
    f.run(rc_of(lambda b, a, c, ad, ld: ops.gconv_split_pre(d, pieces, wsp, f.out.flat, bias=b, act=a, act_cols=c, addend=ad, ld_add=ld)),
          "split_pre", failures)
    f.run(rc_of(lambda b, a, c, ad, ld: ops.gconv_bf16(d, f.x, wbf, f.out.flat, bias=b, act=a, act_cols=c, addend=ad, ld_add=ld)), "bf16", failures)
    torch.cuda.synchronize()
    print("%s: 3 families x %d epilogue variants" % (name, len(f.variants)))
    assert not failures, failures[:6]


@pytest.mark.parametrize("name", ["dc3", "dc2", "c1s2"])
def test_gemm_taps_split_inference_epilogue(name, plan_every_shape):
    """rd_gemm_taps_split (phases of 1..4 taps as a channel-grouped GEMM): the same epilogue, bit for bit for the same reason."""
    from radar_depth_amd import ops
    case = G.BY_NAME[name]
    f = Fused(case)
    d = f.d
    assert ops.gemm_taps_split_supported(d), name
    wsp = G.split_operand(f.w32).cuda()
    failures = []

    def launch(bias, act, cols, add, ld_add):
        ops.gemm_taps_split(d, f.x, wsp, f.out.flat, bias=bias, act=act, act_cols=cols, addend=add, ld_add=ld_add)
        return 0
    f.run(launch, "gemm_taps_split", failures)
    torch.cuda.synchronize()
    print("%s: %d epilogue variants" % (name, len(f.variants)))
    assert not failures, failures[:6]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("case", [G.BY_NAME["c3"], G.BY_NAME["c3w"], G.WINO_EXTRA], ids=repr)
def test_wino_is_bit_exact(case, flip):
    """rd_wino_conv3x3 with addend and statistics, forward operand and `flip` (input-gradient) operand.  The transforms stay exact on
    both grids: U = G g G^T has entries in multiples of 1/16 with at most 6 significant bits (bf16 numbers: no lower pieces), the input
    transform adds four grid values (|V| <= 8 in multiples of 1/4, bf16 numbers too), products are multiples of 1/64 whose sums over 64
    channels stay below 2^11, and the output transform adds four of those.  Output: quarter grid; statistics: unit grid (their budget)."""
    from radar_depth_amd import convdesc as cd, ops
    n, h, w_, ci, co = case.N, case.H, case.W, case.Cin, case.Cout
    assert ci == co and ops.wino_supported(h, w_, ci, co)
    d = cd.conv_dgrad(n, h, w_, ci, co, 3, 1, 1)[0] if flip else case.desc()
    tiles = ops.wino_stat_tiles(n, h, w_)
    for grid in ("quarter", "unit"):
        data = _data(case, grid)
        # the logical operand [9][rows][cols] read as the forward operand of W (rows = I) or as the transposed operand of W (rows = O)
        wl = data["w"].float()
        w_oihw = (wl.reshape(3, 3, co, ci).permute(2, 3, 0, 1) if flip else wl.reshape(3, 3, ci, co).permute(3, 2, 0, 1)).contiguous()
        y = G.conv_ref(d, data["x"], data["w"]) if flip else data["y"]
        G.check_budget(case, grid, data, y, d)
        z = y + data["addend"]
        u = ops.wino_pack(w_oihw.cuda(), flip=bool(flip))
        x = data["x"].float().cuda()
        add = data["addend"].float().cuda()
        out = torch.full((n, h, w_, co), NAN, device="cuda")
        stat = torch.full((tiles, 2, co), NAN, device="cuda")
        ops.wino_conv3x3(x, u, out, addend=add, stat=stat)
        torch.cuda.synchronize()
        assert z.float().double().equal(z)
        bad = ~(out == z.float().cuda())
        assert not bool(bad.any()), (case.name, flip, grid, int(bad.sum()), bad.nonzero()[0].tolist())
        if grid == "unit":
            sums = torch.stack((z.sum((0, 1, 2)), (z * z).sum((0, 1, 2)))).cuda()
            assert _stat_ok(stat, sums), (case.name, flip, stat.double().sum(0)[:, :4].tolist(), sums[:, :4].tolist())
        out.fill_(NAN)
        ops.wino_conv3x3(x, u, out)
        assert bool((out == y.float().cuda()).all()), (case.name, flip, grid, "no addend")
    print("%s flip=%d: 2 grids, addend + statistics" % (case.name, flip))

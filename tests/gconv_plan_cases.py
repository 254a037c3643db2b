"""Shared cases, exactly representable data and the float64 reference of the plan tests of the fp32 convolution (csrc/gconv.hip):
tests/test_gconv_plans_host.py (no GPU) and tests/test_gpu_gconv_plans.py.  Importable without a GPU.

The cases are small on purpose: every one has ragged tiles under at least one register tile of the planner, and together their
candidate sets (rd_gconv_tune_candidates) cover every register tile, patch chunk, split and loop form a tuned or autotuned
process can pin.

Exact data.  On the QUARTER grid inputs, addends and biases are multiples of 1/4 in [-2, 2] and weights multiples of 1/4 in [-1, 1]:
every product is a multiple of 1/16, and as long as the sum of the products' magnitudes of one output element (plus |bias| +
|addend|) stays below 2^24 quanta of 1/16, every partial sum in any order -- any tile, chunk, slab, tap order, split-K slice -- is an
integer number of quanta below 2^24 and fp32 FMA accumulation is exact: the kernel must equal the float64 evaluation bit for bit.
On the UNIT grid (inputs and addends in {-1, 0, 1}, weights in {-1, 0, 1} with about 3/4 zeros) outputs are small integers, so the
per-tile BatchNorm sums are exact too as long as, per channel, sum |y| and sum y^2 over the WHOLE tensor stay below 2^24 (every
partial sum of either is bounded by the total); the BatchNorm-backward sums use means in multiples of 1/4, scales +-1 and integer
shifts, so g (x - mean) is a multiple of 1/4 with |x - mean| <= 2: 8 sum |y| < 2^24 bounds them.  check_budget() ASSERTS these
bounds on the float64 reference, so a test cannot pass on data that is not exact."""
import ctypes as C

import torch
import torch.nn.functional as F

from radar_depth_amd import convdesc as cd

LIMIT = float(2 ** 24)
ACT_NONE, ACT_RELU, ACT_LEAKY02 = 0, 1, 2


class Case:
    """kind: conv (k, s) | up | updg | deconv (k) | dgrad (k, s).  Cin -> Cout are the LAYER's channels; the descriptor's own
    (d.Cin = reduction channels, d.Cout = output channels) are swapped for the two input-gradient kinds."""

    def __init__(self, name, kind, N, H, W, Cin, Cout, k=0, s=1, ldi=None, ldo=None, ld_add=None, split_ok=True, note=""):
        self.name, self.kind, self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.s = name, kind, N, H, W, Cin, Cout, k, s
        self.ldi, self.ldo, self.ld_add_, self.split_ok, self.note = ldi, ldo, ld_add, split_ok, note

    def desc(self):
        N, H, W, ci, co, k, s = self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.s
        if self.kind == "conv":
            return cd.conv_fwd(N, H, W, ci, co, k, s, k // 2, ldi=self.ldi, ldo=self.ldo)
        if self.kind == "up":
            return cd.upproj_fwd(N, H, W, ci, co)
        if self.kind == "updg":
            return cd.upproj_dgrad(N, H, W, ci, co)
        if self.kind == "deconv":
            return cd.deconv_fwd(N, H, W, ci, co, k)
        assert self.kind == "dgrad"
        d, zero_fill = cd.conv_dgrad(N, H, W, ci, co, k, s, k // 2)
        assert not zero_fill
        return d

    @property
    def ld_add(self):
        return self.ld_add_ or self.desc().Cout

    # channel offsets of the slices inside their wider buffers (multiples of four floats: the kernels' 16-byte accesses)
    @property
    def in_off(self):
        return 8 if self.ldi else 0

    @property
    def out_off(self):
        return 4 if self.ldo else 0

    @property
    def add_off(self):
        return 4 if self.ld_add_ else 0

    def __repr__(self):
        return self.name


CASES = [
    Case("c3", "conv", 2, 9, 37, 64, 64, k=3, note="dense; split-K 1/2/4"),
    Case("c3r", "conv", 1, 11, 13, 48, 40, k=3, note="Cout not a multiple of 32; 16-channel chunks only"),
    Case("c3w", "conv", 1, 3, 150, 64, 64, k=3, note="several column tiles on every register tile"),
    Case("c3s", "conv", 2, 9, 37, 64, 64, k=3, ldi=80, ldo=72, ld_add=68, split_ok=False, note="channel slices of wider buffers"),
    # (not 2x13x21: that is layer3_depth.0.conv1 of the 2x97x161 models, which other tests plan -- and commit -- first)
    Case("c3s2", "conv", 2, 13, 19, 32, 64, k=3, s=2, note="input-parity groups, odd sizes"),
    Case("c1s2", "conv", 2, 13, 21, 64, 128, k=1, s=2, note="downsample"),
    Case("c1", "conv", 3, 5, 7, 160, 64, k=1, note="fusion 1x1"),
    Case("up", "up", 1, 5, 6, 32, 32, note="4 phases of 9/6/6/4 taps, two branches of 16"),
    Case("updg", "updg", 1, 5, 6, 32, 32, note="25 taps: the CKW = 4 instantiations"),
    Case("dc3", "deconv", 1, 5, 7, 64, 32, k=3, note="4 phases, out_stride 2"),
    Case("dc2", "deconv", 1, 5, 7, 64, 32, k=2, note="4 phases, out_stride 2"),
    Case("dgs2", "dgrad", 1, 13, 21, 32, 64, k=3, s=2, note="4 phases of 4/2/2/1 taps"),
    Case("c16", "conv", 1, 7, 9, 16, 16, k=3, note="conv16-eligible: no candidates; the fused form is the re-plan"),
]
BY_NAME = {c.name: c for c in CASES}
WINO_EXTRA = Case("w57", "conv", 1, 5, 7, 64, 64, k=3, note="Winograd: one partial 2x2 output tile per edge")


def n_slabs(d):
    return max(d.phase[i].widx[t] for i in range(d.n_phases) for t in range(d.phase[i].n_taps)) + 1


def covers_output(d):
    return sum(d.phase[i].lh * d.phase[i].lw for i in range(d.n_phases)) == d.Ho * d.Wo if d.n_phases > 1 else d.out_stride == 1


# ------------------------------------------------------------------------------------------------ data
def _grid(g, shape, lo, hi, step):
    return torch.randint(lo, hi + 1, shape, generator=g).double() * step


def make_data(case, grid, seed=0):
    """-> dict of float64 CPU tensors: x [N,Hi,Wi,Cin], w [slabs,Cin,Cout] (the LOGICAL operand), addend [N,Ho,Wo,Cout], bias [Cout],
    and for the unit grid the BatchNorm-backward operands bn_x [N,Ho,Wo,Cout], mean, scale, shift [Cout]."""
    d = case.desc()
    g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, case.name)))
    out = {}
    if grid == "quarter":
        out["x"] = _grid(g, (d.N, d.Hi, d.Wi, d.Cin), -8, 8, 0.25)
        out["w"] = _grid(g, (n_slabs(d), d.Cin, d.Cout), -4, 4, 0.25)
        out["addend"] = _grid(g, (d.N, d.Ho, d.Wo, d.Cout), -8, 8, 0.25)
        out["bias"] = _grid(g, (d.Cout,), -8, 8, 0.25)
    else:
        assert grid == "unit"
        out["x"] = _grid(g, (d.N, d.Hi, d.Wi, d.Cin), -1, 1, 1.0)
        w = _grid(g, (n_slabs(d), d.Cin, d.Cout), -1, 1, 1.0)
        out["w"] = w * (torch.rand(w.shape, generator=g) < 0.375).double()          # 2/3 * 3/8 = 1/4 of the weights non-zero
        out["addend"] = _grid(g, (d.N, d.Ho, d.Wo, d.Cout), -1, 1, 1.0)
        out["bias"] = torch.zeros(d.Cout, dtype=torch.float64)
        out["bn_x"] = _grid(g, (d.N, d.Ho, d.Wo, d.Cout), -1, 1, 1.0)
        out["mean"] = _grid(g, (d.Cout,), -4, 4, 0.25)
        out["scale"] = _grid(g, (d.Cout,), 0, 1, 2.0) - 1.0
        out["shift"] = _grid(g, (d.Cout,), -1, 1, 1.0)
    return out


def make_randn(case, seed=0):
    """Ordinary values (full mantissas): float32-representable float64 tensors x, w."""
    d = case.desc()
    g = torch.Generator().manual_seed(77 + 1000 * seed + sum(map(ord, case.name)))
    taps = max(d.phase[i].n_taps for i in range(d.n_phases))
    x = torch.randn(d.N, d.Hi, d.Wi, d.Cin, generator=g)
    w = torch.randn(n_slabs(d), d.Cin, d.Cout, generator=g) * (2.0 / (taps * d.Cin)) ** 0.5
    return {"x": x.double(), "w": w.double()}


# ------------------------------------------------------------------------------------------------ reference
def conv_ref(d, x, w):
    """float64 convolution of the descriptor on the logical operand; pixels no phase writes are NaN."""
    from desc_emulator import run_desc
    assert x.dtype == torch.float64 and w.dtype == torch.float64
    return run_desc(d, x, w)


_F02 = torch.tensor(0.2, dtype=torch.float32)


def epilogue_ref(y, bias=None, addend=None, act=ACT_NONE, act_cols=0):
    """out = act_{co < act_cols}(y + bias + addend), in the device's order: bias, addend, activation.  y, bias, addend float64; the
    sum must be a float32 number (asserted); LeakyReLU is the device's single float32 multiply by 0.2f.  -> float32."""
    z = y.clone()
    if bias is not None:
        z = z + bias
    if addend is not None:
        z = z + addend
    z32 = z.float()
    ok = torch.isnan(z) | (z32.double() == z)
    assert bool(ok.all()), "the pre-activation is not a float32 number: the data is not exact"
    if act == ACT_NONE or act_cols <= 0:
        return z32
    if act == ACT_RELU:
        a = torch.where(z32 > 0, z32, torch.zeros_like(z32))
    else:
        assert act == ACT_LEAKY02
        a = torch.where(z32 > 0, z32, _F02 * z32)
    col = torch.arange(z32.shape[-1]) < act_cols
    return torch.where(col, a, z32)


def bnbwd_ref(y, bn_x, mean, scale, shift, act=ACT_RELU):
    """-> (sum g, sum g (x - mean)) per channel in float64, g = y act'(scale x + shift) (the derivative at 0 is that of the negative side)."""
    z = scale * bn_x + shift
    slope = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.0 if act == ACT_RELU else 0.2))
    g = y * slope
    return g.sum((0, 1, 2)), (g * (bn_x - mean)).sum((0, 1, 2))


def check_budget(case, grid, data, y=None, d=None):
    """Assert on the float64 reference that fp32 accumulation of this case's data is exact (module docstring).  -> dict of the
    figures, in quanta.  d: another descriptor run on the case's data (default: the case's own)."""
    d = d or case.desc()
    y = conv_ref(d, data["x"], data["w"]) if y is None else y
    live = ~torch.isnan(y)
    if grid == "quarter":
        mag = conv_ref(d, data["x"].abs(), data["w"].abs())
        mag = torch.where(live, mag, torch.zeros_like(mag)) + data["bias"].abs() + data["addend"].abs()
        q = float(mag.max()) * 16
        assert q < LIMIT, (case.name, q)
        for t in (data["x"], data["addend"], data["bias"], data["w"]):
            assert bool((t * 4 == (t * 4).round()).all())
        assert float(data["x"].abs().max()) <= 2 and float(data["w"].abs().max()) <= 1
        return {"element_quanta": q}
    z = torch.where(live, y, torch.zeros_like(y)) + data["addend"]
    assert bool((z == z.round()).all())
    s1 = float(z.abs().sum((0, 1, 2)).max())
    s2 = float((z * z).sum((0, 1, 2)).max())
    y0 = torch.where(live, y, torch.zeros_like(y))
    sb = 8 * float(y0.abs().sum((0, 1, 2)).max())
    assert s1 < LIMIT and s2 < LIMIT and sb < LIMIT, (case.name, s1, s2, sb)
    assert bool(((data["mean"] * 4) == (data["mean"] * 4).round()).all()) and bool((data["scale"].abs() == 1).all())
    return {"sum_abs": s1, "sum_sq": s2, "bnbwd_quarter_quanta": sb}


# ------------------------------------------------------------------------------------------------ the same cases through torch.nn.functional
def torch_ref(case, x, w):
    """The case's operation by torch.nn.functional in float64 from the logical operand (x NHWC, w [slabs][d.Cin][d.Cout]) -> NHWC."""
    k, s = case.k, case.s
    xn = x.permute(0, 3, 1, 2)
    if case.kind == "conv":
        wo = w.reshape(k, k, w.shape[1], w.shape[2]).permute(3, 2, 0, 1)                    # OIHW
        y = F.conv2d(xn, wo, stride=s, padding=k // 2)
    elif case.kind == "up":
        wo = w.reshape(5, 5, w.shape[1], w.shape[2]).permute(3, 2, 0, 1)
        u = torch.zeros(xn.shape[0], xn.shape[1], 2 * xn.shape[2], 2 * xn.shape[3], dtype=x.dtype)
        u[:, :, ::2, ::2] = xn
        y = F.conv2d(u, wo, padding=2)
    elif case.kind == "updg":
        wf = w.reshape(5, 5, w.shape[1], w.shape[2]).permute(2, 3, 0, 1)                    # forward OIHW: O = dy channels = d.Cin
        y = F.conv_transpose2d(xn, wf, padding=2)[:, :, ::2, ::2]                           # gradient w.r.t. the unpooled tensor, at the kept pixels
    elif case.kind == "deconv":
        wt = w.reshape(k, k, w.shape[1], w.shape[2]).permute(2, 3, 0, 1)                    # ConvTranspose2d weight [Cin][Cout][k][k]
        y = F.conv_transpose2d(xn, wt, stride=2, padding=(k - 1) // 2, output_padding=k % 2)
    else:
        wf = w.reshape(k, k, w.shape[1], w.shape[2]).permute(2, 3, 0, 1)                    # forward OIHW [O = dy channels][I]
        ho, wo_ = xn.shape[2], xn.shape[3]
        op = (case.H - ((ho - 1) * s - 2 * (k // 2) + k), case.W - ((wo_ - 1) * s - 2 * (k // 2) + k))
        y = F.conv_transpose2d(xn, wf, stride=s, padding=k // 2, output_padding=op)
    return y.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ device operands
def pack_quad(w, k):
    """logical [slabs][R][C] -> the packed operand [slabs][R/k][C][k] (rows interleaved by k: 4 for fp32, 8 for bf16), flat."""
    s, r, c = w.shape
    assert r % k == 0
    return w.reshape(s, r // k, k, c).permute(0, 1, 3, 2).contiguous().reshape(-1)


def split_operand(w):
    """logical float32 operand -> three bf16 piece planes [3][...] of the bf16 layout (w = p0 + p1 + p2 exactly)."""
    p0 = w.to(torch.bfloat16).float()
    r = w - p0
    p1 = r.to(torch.bfloat16).float()
    p2 = (r - p1).to(torch.bfloat16).float()
    assert bool((p0 + p1 + p2 == w).all())
    return torch.stack([pack_quad(p, 8).to(torch.bfloat16) for p in (p0, p1, p2)]).contiguous()


# ------------------------------------------------------------------------------------------------ candidates and pins
def candidates(L, d, allow_split=1, cap=128):
    buf = (C.c_int32 * (9 * cap))()
    n = L.rd_gconv_tune_candidates(C.byref(d), allow_split, buf, cap)
    assert 0 <= n < cap, "candidate list truncated or refused: %d" % n
    return [tuple(buf[9 * i:9 * i + 9]) for i in range(n)]


def plan_info(L, d):
    info = (C.c_int32 * 10)()
    assert L.rd_gconv_plan_info(C.byref(d), info) == 0
    return tuple(info)


def info_point(info):
    """rd_gconv_plan_info -> (MT, NT, WM, WN, CKP, TH, TW, ksplit, pipelined 0 / 1): the candidate tuple, with both pipelined forms as 1."""
    return (info[0], info[1], info[2], info[3], info[5], info[6], info[7], (info[4] // 100) % 100, (info[4] // 10000) % 100)


def pin(L, d, cand, allow_split=1):
    """Pin a candidate (None: back to the heuristic) and check that the plan in effect is the pinned point -- otherwise a launch could
    silently run the heuristic plan.  rd_gconv_plan_info reports both pipelined loop forms alike; the half-depth form (2) is told
    from the full-depth form of the same point by its smaller LDS footprint."""
    if cand is None:
        assert L.rd_gconv_tune_pin(C.byref(d), allow_split, None) == 0
        return None
    if cand[8] == 2:
        twin = cand[:8] + (1,)
        assert L.rd_gconv_tune_pin(C.byref(d), allow_split, (C.c_int32 * 9)(*twin)) == 0, ("full-depth twin refused", twin)
        lds_full = plan_info(L, d)[8]
    assert L.rd_gconv_tune_pin(C.byref(d), allow_split, (C.c_int32 * 9)(*cand)) == 0, ("pin refused", cand, L.rd_last_error().decode())
    info = plan_info(L, d)
    assert info_point(info) == cand[:8] + (min(cand[8], 1),), (cand, info)
    if cand[8] == 2:
        assert info[8] < lds_full, ("half-depth weight slabs must need less LDS", cand, info[8], lds_full)
    return info

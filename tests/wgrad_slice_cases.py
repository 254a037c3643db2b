"""Cases and helpers of tests/test_gpu_wgrad_slices.py (plain data, no fixtures): weight-gradient launches whose operands are channel
slices of wider NHWC buffers -- x at channel offset cx of a [N,Hi,Wi,ldi] buffer, dy at cy of [N,Ho,Wo,ldo], every other channel NaN.
tests/test_plan_host.py reads the same lists to tie them to what the execution plans bind.

A case is (id, kind, N, Cin, cx, ldi, Cout, cy, ldo, H, W, k, stride); Cin / Cout / ldi / ldo are the DESCRIPTOR's (for kind "deconv" the
descriptor's input is the transposed convolution's output gradient, convdesc.deconv_wgrad).  Offsets are multiples of 4 floats (8 for the
bf16 family, whose strides are multiples of 8 as well) so that a slice base stays 16-byte aligned."""
import collections
import functools

import torch

Case = collections.namedtuple("Case", "id kind n cin cx ldi cout cy ldo h w k s")


def make_case(kind, n, ci, co, h, w, k=3, s=1):
    cin, cx, ldi = ci
    cout, cy, ldo = co
    name = "%s%d_s%d_%d@%dof%d_%d@%dof%d_%dx%d_n%d" % (kind, k, s, cin, cx, ldi, cout, cy, ldo, h, w, n)
    return Case(name, kind, n, cin, cx, ldi, cout, cy, ldo, h, w, k, s)


# rd_wgrad_split + rd_wgrad_split_reduce: 3x3 / stride 1 and the UpProj parity phases
SPLIT_CONV = [
    make_case("conv", 2, (72, 8, 96), (88, 36, 128), 9, 35),          # partial 64-blocks on both sides, a ragged tile column
    make_case("conv", 3, (64, 512, 640), (128, 128, 256), 17, 18),    # the binding of a 640-channel concat buffer
    make_case("conv", 1, (64, 4, 68), (64, 0, 64), 1, 1),             # a single pixel; dy dense
    make_case("conv", 2, (96, 16, 128), (160, 8, 176), 13, 33),
    make_case("conv", 2, (64, 0, 64), (64, 16, 96), 6, 20),           # x dense, dy a slice
]
SPLIT_UPPROJ = [
    make_case("upproj", 2, (64, 64, 128), (64, 0, 96), 5, 7, k=5),
    make_case("upproj", 2, (96, 16, 128), (96, 8, 112), 6, 3, k=5),
]
# rd_wgrad_split_pre: one 3x3 and one UpProj case (channel counts multiples of 16), piece planes made from the same slices
SPLIT_PRE = [SPLIT_CONV[1], SPLIT_UPPROJ[0]]

# rd_wgrad + rd_wgrad_reduce: every sub-kernel behind the entry point
WGRAD = [
    make_case("conv", 2, (64, 64, 192), (64, 8, 80), 25, 26),         # column-strip kernel, ragged last strip
    make_case("conv", 2, (64, 0, 128), (96, 32, 128), 7, 33),         # immediate-offset kernel (short image: no strip)
    make_case("conv", 3, (64, 512, 640), (128, 0, 128), 21, 27, s=2), # stride 2 out of a concat buffer; dy dense
    make_case("conv", 3, (32, 16, 64), (48, 4, 56), 9, 7),            # immediate-offset kernel on one 32-channel block (layout B)
    make_case("conv", 3, (16, 8, 32), (16, 16, 48), 37, 45),          # wgrad16.hip
    make_case("conv", 2, (192, 64, 320), (64, 4, 72), 7, 9, k=1),     # wgrad1x1.hip
    make_case("conv", 2, (96, 16, 128), (160, 8, 176), 9, 7, k=1, s=2),
    make_case("conv", 3, (16, 4, 24), (32, 0, 32), 7, 5, k=1, s=2),   # one tap below 64 channels: the generic tile
    make_case("conv", 2, (64, 0, 64), (64, 4, 72), 24, 25),           # strip kernel; x dense, dy a slice
    make_case("upproj", 2, (32, 32, 96), (32, 8, 48), 13, 9, k=5),    # four phase launches
    make_case("deconv", 2, (32, 16, 64), (64, 64, 192), 7, 9, k=2),   # deconv_wgrad(2, 7, 9, 64, 32, k): dy [2,14,18,32], x [2,7,9,64]
    make_case("deconv", 2, (32, 16, 64), (64, 64, 192), 7, 9, k=3),
]

# rd_wgrad_bf16 (fp32 tensors) and rd_wgrad_bf16_t with bf16 tensors
BF16 = [
    make_case("conv", 2, (64, 64, 192), (64, 8, 80), 23, 31),
    make_case("conv", 2, (32, 16, 64), (64, 8, 72), 30, 41, s=2),
    make_case("conv", 3, (128, 512, 640), (64, 16, 96), 9, 14, k=1),
    make_case("conv", 2, (16, 8, 32), (16, 16, 48), 20, 35),
    make_case("conv", 2, (64, 0, 64), (32, 8, 48), 9, 11),            # x dense, dy a slice
    make_case("conv", 2, (48, 8, 64), (32, 0, 32), 9, 11),            # x a slice, dy dense
    make_case("upproj", 2, (32, 32, 96), (32, 8, 48), 13, 9, k=5),
]

FAMILY_CASES = {"wgrad": WGRAD, "wgrad_split": SPLIT_CONV + SPLIT_UPPROJ, "wgrad_split_pre": SPLIT_PRE, "wgrad_bf16": BF16}


def sign_patterns(family):
    """The (ldi - Cin > 0, ldo - Cout > 0) patterns among a family's kernel-level cases; every case also runs its dense twin."""
    return {(c.ldi > c.cin, c.ldo > c.cout) for c in FAMILY_CASES[family]} | {(False, False)}


def desc(case, dense=False):
    """The case's descriptor; dense: the twin with ldi = Cin, ldo = Cout."""
    from radar_depth_amd import convdesc as cd
    ldi, ldo = (case.cin, case.cout) if dense else (case.ldi, case.ldo)
    if case.kind == "upproj":
        return cd.upproj_fwd(case.n, case.h, case.w, case.cin, case.cout, ldi=ldi, ldo=ldo)
    if case.kind == "deconv":
        return cd.deconv_wgrad(case.n, case.h, case.w, case.cout, case.cin, case.k, ld_dy=ldi, ld_x=ldo)
    return cd.conv_fwd(case.n, case.h, case.w, case.cin, case.cout, case.k, case.s, case.k // 2, ldi=ldi, ldo=ldo)


def kernel_shape(case):
    """(KH, KW) of the OIHW gradient [Cout, Cin, KH, KW] the slabs reduce into."""
    return (5, 5) if case.kind == "upproj" else (case.k, case.k)


@functools.lru_cache(maxsize=None)
def values(case):
    """The case's operand values (CPU fp32): x [N,Hi,Wi,Cin], dy [N,Ho,Wo,Cout] of the descriptor."""
    d = desc(case, dense=True)
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) for ch in case.id))
    return torch.randn(d.N, d.Hi, d.Wi, d.Cin, generator=g), torch.randn(d.N, d.Ho, d.Wo, d.Cout, generator=g)


def bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def reference(case, rounded=False):
    """float64 OIHW gradient from desc_emulator.run_wgrad on the same fp32 values (rounded: on their bf16 roundings).  Computed once
    per case and shared; callers must not modify it."""
    import desc_emulator as em
    x, dy = values(case)
    if rounded:
        x, dy = bf(x), bf(dy)
    kh, kw = kernel_shape(case)
    dw = em.run_wgrad(desc(case, dense=True), x.double(), dy.double(), kh * kw)          # [S][Cin][Cout]
    return dw.permute(2, 1, 0).reshape(case.cout, case.cin, kh, kw).contiguous()


def widen(t, c0, ld, dtype=torch.float32):
    """[N,H,W,C] values at channel offset c0 of a NaN-filled [N,H,W,ld] buffer."""
    n, h, w, c = t.shape
    assert c0 >= 0 and c0 + c <= ld
    buf = torch.full((n, h, w, ld), float("nan"), dtype=dtype)
    buf[..., c0:c0 + c] = t.to(dtype)
    return buf

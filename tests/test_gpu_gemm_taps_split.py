"""GPU parity of rd_gemm_taps_split (csrc/gemm_taps_split.hip: phases of 1..4 taps as a channel-grouped GEMM over three-piece bf16
operands) against the float64 descriptor emulator, at the 2e-5 bar of the other split-kernel tests: transposed-convolution forward and
input-gradient descriptors, the stride-2 3x3 input gradient, fuzzed phases at the image borders, N > 1, Cout not a multiple of 64,
strided ldi / ldo, and the BatchNorm partial sums of the epilogue."""
import random
import zlib

import pytest
import torch

from desc_emulator import run_desc

pytestmark = pytest.mark.gpu


def _fuzz_desc(seed):
    """1..4 phases of 1..4 random taps in [-2, 2] (many outside the image at the borders), in_stride 1 or 2, out_stride 2."""
    from radar_depth_amd import convdesc as cd
    rnd = random.Random(seed)
    n, hi, wi = rnd.randint(1, 3), rnd.randint(2, 11), rnd.randint(2, 13)
    cin, cout = rnd.choice([32, 64, 96]), rnd.choice([32, 64, 96, 160])
    ins = rnd.choice([1, 2])
    lh, lw = rnd.randint(1, 9), rnd.randint(1, 9)
    phases = []
    offs = rnd.sample([(0, 0), (0, 1), (1, 0), (1, 1)], rnd.randint(1, 4))
    slabs = 0
    for off in offs:
        taps = [(rnd.randint(-2, 2), rnd.randint(-2, 2), slabs + t) for t in range(rnd.randint(1, 4))]
        slabs += len(taps)
        phases.append(cd._phase(taps, lh, lw, off))
    return cd._desc(n, hi, wi, cin, cin, 2 * lh, 2 * lw, cout, cout, ins, 2, phases), slabs


def _case(kind):
    from radar_depth_amd import convdesc as cd
    if kind.startswith("fuzz"):
        return _fuzz_desc(int(kind[4:]))
    if kind == "deconv3_fwd":
        return cd.deconv_fwd(2, 7, 9, 64, 96, 3), 9
    if kind == "deconv3_fwd_l1":
        return cd.deconv_fwd(2, 15, 25, 256, 128, 3), 9
    if kind == "deconv2_fwd":
        return cd.deconv_fwd(3, 5, 4, 128, 64, 2), 4
    if kind == "deconv2_dgrad":
        return cd.deconv_dgrad(2, 6, 5, 64, 32, 2), 4
    if kind == "deconv3_dgrad_phase":      # (9 taps: not served)
        return cd.deconv_dgrad(2, 6, 5, 64, 32, 3), 9
    if kind == "conv3x3s2_dgrad":
        return cd.conv_dgrad(2, 13, 11, 64, 128, 3, 2, 1)[0], 9
    raise ValueError(kind)


KINDS = ["deconv3_fwd", "deconv3_fwd_l1", "deconv2_fwd", "deconv2_dgrad", "conv3x3s2_dgrad"] + ["fuzz%d" % s for s in range(12)]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_gemm_taps_split_vs_float64(kind, strided):
    from radar_depth_amd import ops
    d, slabs = _case(kind)
    assert ops.gemm_taps_split_supported(d), kind
    if strided:
        d.ldi, d.ldo = d.Cin + 32, d.Cout + 8
    g = torch.Generator().manual_seed(zlib.crc32(kind.encode()) % 1000 + strided)
    x = torch.randn(d.N, d.Hi, d.Wi, d.ldi, generator=g)
    w = torch.randn(slabs, d.Cin, d.Cout, generator=g) * (1.0 / d.Cin) ** 0.5
    want = run_desc(d, x[..., :d.Cin].double(), w.double())                     # NaN where no phase writes
    # [slab][Cin][Cout] as an "OIHW" [Cout][Cin][slabs][1] weight: the plain pack gives back [slab][Cin][Cout]
    w_split = ops.pack_weights_split(w.permute(2, 1, 0).unsqueeze(-1).contiguous().cuda())
    out = torch.full((d.N, d.Ho, d.Wo, d.ldo), float("nan"), device="cuda")
    stat = torch.zeros(ops.gemm_taps_split_stat_tiles(d), 2, d.Cout, device="cuda")
    ops.gemm_taps_split(d, x.cuda(), w_split, out, stat=stat)
    torch.cuda.synchronize()
    got = out.cpu().double()
    written = ~torch.isnan(want[..., 0])
    assert torch.equal(~torch.isnan(got[..., 0]), written), kind                 # exactly the phases' pixels are written
    assert torch.isnan(got[..., d.Cout:]).all(), kind                          # nothing beyond Cout in a strided output
    g_, w_ = got[..., :d.Cout][written], want[written]
    err = ((g_ - w_).abs().max() / w_.abs().max()).item()
    assert err < 2e-5, (kind, err)
    s = stat.sum(0).cpu().double()
    ref_s, ref_q = w_.sum(0), (w_ ** 2).sum(0)
    assert ((s[0] - ref_s).abs().max() / ref_q.sqrt().max()).item() < 1e-4, kind
    assert ((s[1] - ref_q).abs().max() / ref_q.abs().max()).item() < 1e-4, kind


def test_gemm_taps_split_rejects():
    """More than 4 taps in a phase, or channel counts off the 32-channel grid: not served (the plan keeps rd_gconv_split / rd_gconv)."""
    from radar_depth_amd import convdesc as cd, ops
    assert not ops.gemm_taps_split_supported(_case("deconv3_dgrad_phase")[0])
    assert not ops.gemm_taps_split_supported(cd.deconv_fwd(2, 7, 9, 32, 16, 3))
    assert not ops.gemm_taps_split_supported(cd.deconv_fwd(2, 7, 9, 48, 32, 3))

"""Cases of tests/test_gpu_tap_groups.py: the split convolutions (csrc/gconv_split.hip) on descriptors whose phases do not fill their
last group of three taps, through the C ABI.  run_all() runs every case under the tile choice of THIS process and returns one record per
launch; the tile-forcing knobs (RD_GCONV_SPLIT_FORCE, RD_GCONV_SP2_FORCE, RD_GCONV_SP2, RD_GCONV_SPLIT_NOPDB) are read once per
process, so the test starts this file as a script once per forced configuration:   python tests/tap_group_cases.py OUT.json

Every case is checked two ways: against a float64 evaluation of the descriptor (the reference is computed once per case and shared by
its launches), and bit for bit against the SAME convolution with every phase's tap list filled up to a multiple of three by taps that
point at an all-zero weight slab -- "the kernel skipped the step" against "the kernel multiplied by zero"."""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

MAPS = [(9, 13), (10, 14)]          # odd and even: the parity phases get different extents, and there are edge tiles
N = 2


def descriptors(cd, h, w, cin, cout):
    """(name, descriptor) with the KERNEL's channel counts: cin channels are reduced, cout are written."""
    return [
        ("dgrad_s2_k3", cd.conv_dgrad(N, h, w, cout, cin, 3, 2, 1)[0]),      # phases of 1 / 2 / 2 / 4 taps
        ("upproj_fwd", cd.upproj_fwd(N, h, w, cin, cout)),                   # 9 / 6 / 6 / 4
        ("upproj_dgrad", cd.upproj_dgrad(N, h, w, cout, cin)),               # 25: eight full groups and a single step
        ("deconv_dgrad_k2", cd.deconv_dgrad(N, h, w, cout, cin, 2)),         # one 2 x 2-tap phase
        ("conv3x3", cd.conv_fwd(N, h, w, cin, cout, 3, 1, 1)),               # control: three full groups
    ]


def n_slabs(d):
    return 1 + max(d.phase[i].widx[t] for i in range(d.n_phases) for t in range(d.phase[i].n_taps))


def zero_padded(d, zero_slab):
    """d with every phase's tap list filled up to a multiple of three: the added taps repeat the phase's first (dh, dw) and point at
    weight slab zero_slab.  None when a phase would need more taps than a descriptor holds."""
    from radar_depth_amd._lib import RD_MAX_TAPS, RdConvDesc
    p = RdConvDesc.from_buffer_copy(d)
    for i in range(p.n_phases):
        ph = p.phase[i]
        want = -(-ph.n_taps // 3) * 3
        if want > RD_MAX_TAPS:
            return None
        for t in range(ph.n_taps, want):
            ph.dh[t], ph.dw[t], ph.widx[t] = ph.dh[0], ph.dw[0], zero_slab
        ph.n_taps = want
    return p


def ref64(d, x, w):
    """float64 evaluation of the descriptor: x [N, Hi, Wi, Cin] float32, w [Cout, Cin, 1, slabs] float32 -> [N, Ho, Wo, Cout]."""
    import torch
    xd, wd = x.double(), w.double()
    out = torch.zeros(d.N, d.Ho, d.Wo, d.Cout, dtype=torch.float64)
    for i in range(d.n_phases):
        p = d.phase[i]
        oh, ow = torch.arange(p.lh), torch.arange(p.lw)
        for t in range(p.n_taps):
            ih, iw = oh * d.in_stride + p.dh[t], ow * d.in_stride + p.dw[t]
            vh, vw = (ih >= 0) & (ih < d.Hi), (iw >= 0) & (iw < d.Wi)
            sub = xd[:, ih[vh]][:, :, iw[vw]]
            rows, cols = oh[vh] * d.out_stride + p.out_off_h, ow[vw] * d.out_stride + p.out_off_w
            out[:, rows[:, None], cols[None, :]] += sub @ wd[:, :, 0, p.widx[t]].t()
    return out


def _plan(lib, d, pre):
    v = (C.c_int32 * 8)()
    f = lib.rd_gconv_split_pre_plan_info if pre else lib.rd_gconv_split_plan_info
    return list(v) if f(C.byref(d), v) == 0 else None


def _rel(got, want):
    return ((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def run_all():
    import torch
    from radar_depth_amd import convdesc as cd, ops
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    L = lib()
    prev = L.rd_gconv_split_plan_all(1)          # plan every shape the kernels can run (the library leaves the small ones to rd_gconv)
    records = []
    try:
        combos = [(False, ci, co) for ci in (64, 96) for co in (64, 96)] + [(True, ci, co) for ci in (32, 64) for co in (32, 64, 96)]
        seed = 0
        for (h, w) in MAPS:
            for (pre, cin, cout) in combos:
                for name, d in descriptors(cd, h, w, cin, cout):
                    seed += 1
                    records += _one(torch, ops, L, check, current_stream, ptr, "%s %dx%d %d->%d %s" % (name, h, w, cin, cout, "pre" if pre else "staged"),
                                    d, pre, seed)
    finally:
        L.rd_gconv_split_plan_all(1 if prev == 1 else 0)
    return records


def _one(torch, ops, L, check, current_stream, ptr, label, d, pre, seed):
    supported = (L.rd_gconv_split_pre_supported if pre else L.rd_gconv_split_supported)(C.byref(d)) == 1
    if not supported or _plan(L, d, pre) is None or (not pre and _plan(L, d, pre)[7] == 1000):       # (1000: a one-tap descriptor on gemm1_split)
        return [{"case": label, "supported": False}]
    g = torch.Generator().manual_seed(seed)
    S = n_slabs(d)
    taps = max(d.phase[i].n_taps for i in range(d.n_phases))
    x = torch.randn(d.N, d.Hi, d.Wi, d.Cin, generator=g)
    wt = torch.randn(d.Cout, d.Cin, 1, S + 1, generator=g) * (2.0 / (taps * d.Cin)) ** 0.5
    wt[:, :, :, S] = 0.0                                  # the slab the added taps of the zero-padded descriptor point at
    add = torch.randn(d.N, d.Ho, d.Wo, d.Cout, generator=g)
    want = ref64(d, x, wt)
    # BatchNorm in front of the convolution whose input gradient this launch would be: x_bn lives in a wider buffer (channel slice)
    ld = d.Cout + 8
    xb = torch.randn(d.N, d.Ho, d.Wo, ld, generator=g)
    scale = (torch.rand(d.Cout, generator=g) + 0.5) * (torch.randint(0, 2, (d.Cout,), generator=g) * 2 - 1)
    shift = torch.randn(d.Cout, generator=g) * 0.3
    mean = torch.randn(d.Cout, generator=g) * 0.2
    z = scale * xb[..., 4:4 + d.Cout] + shift
    xb[..., 4:4 + d.Cout] += torch.where(z.abs() < 1e-3, 0.25, 0.0)      # (keep act' away from its kink: fp32 and float64 then agree on it)
    bn_x = xb[..., 4:4 + d.Cout].double()
    bn_act = 1 + seed % 2                                 # ReLU / LeakyReLU(0.2)
    zz = scale.double() * bn_x + shift.double()
    assert (zz.abs() > 1e-4).all()
    slope = torch.where(zz > 0, torch.ones_like(zz), torch.full_like(zz, 0.0 if bn_act == 1 else 0.2))

    xg, wp, addg, xbg = x.cuda(), ops.pack_weights_split(wt.cuda()), add.cuda(), xb.cuda()
    xin = ops.split_pieces(xg) if pre else xg
    sg, tg, mg = scale.cuda(), shift.cuda(), mean.cuda()
    pe = C.c_int64(wp[0].numel())
    tiles = (L.rd_gconv_split_pre_stat_tiles if pre else L.rd_gconv_split_stat_tiles)(C.byref(d))

    def launch(dd, epi):
        """-> (out, stat) of one launch under NaN-poisoned LDS (a read of LDS nobody wrote shows up as NaN) into NaN-filled buffers."""
        out = torch.full((d.N, d.Ho, d.Wo, d.Cout), float("nan"), device="cuda")
        stat = torch.full((tiles, 3 if epi == "bnb" else 2, d.Cout), float("nan"), device="cuda")
        check(L.rd_debug_poison_lds(current_stream()), "rd_debug_poison_lds")
        head = (C.byref(dd), ptr(xin)) + ((C.c_int64(xin[0].numel()),) if pre else ()) + (ptr(wp), pe, ptr(out))
        if epi == "bnb":
            f = L.rd_gconv_split_pre_bnbwd if pre else L.rd_gconv_split_bnbwd
            check(f(*head, ptr(xbg.view(-1)[4:]), ld, ptr(mg), ptr(sg), ptr(tg), bn_act, ptr(stat), current_stream()), "bnbwd")
        else:
            f = L.rd_gconv_split_pre if pre else L.rd_gconv_split
            a = (ptr(addg), d.Cout) if epi == "addend" else (None, 0)
            check(f(*head, None, 0, 0, *a, ptr(stat), current_stream()), "gconv_split")
        return out, stat[:, :2]                          # (the third row of the BatchNorm-backward layout is not written by this kernel)

    plan = _plan(L, d, pre)
    dz = zero_padded(d, S) if any(d.phase[i].n_taps % 3 for i in range(d.n_phases)) else d
    if dz is None:
        padded = "inexpressible"                          # upproj_dgrad: 27 taps do not fit a descriptor's 25 slots -- check (a) only
    elif dz is d:
        padded = "no short group"
    elif (L.rd_gconv_split_pre_supported if pre else L.rd_gconv_split_supported)(C.byref(dz)) != 1:
        padded = "rejected"
    else:
        padded = "same plan" if _plan(L, dz, pre)[:7] == plan[:7] else "other plan"
    epis = ["plain", "addend"]
    if L.rd_gconv_split_bnbwd_supported(C.byref(d), 1 if pre else 0) == 1:
        epis.append("bnb")
    recs = []
    for epi in epis:
        out, stat = launch(d, epi)
        rec = {"case": label, "supported": True, "pre": pre, "epi": epi, "tile": plan[:2], "pdb": plan[7] // 100, "padded": padded}
        if padded == "same plan":
            out_z, stat_z = launch(dz, epi)
            rec["bitwise"] = bool(torch.equal(out, out_z) and torch.equal(stat, stat_z))
        o, s = out.cpu(), stat.cpu().double().sum(0)
        rec["nan"] = bool(torch.isnan(o).any() or torch.isnan(s).any())
        v = want + (add.double() if epi == "addend" else 0)
        rec["err_out"] = _rel(o, v)
        if epi == "bnb":
            gg = want * slope
            rec["err_stat"] = [_rel(s[0], gg.sum((0, 1, 2))), _rel(s[1], (gg * (bn_x - mean.double())).sum((0, 1, 2)))]
        else:
            rec["err_stat"] = [_rel(s[0], v.sum((0, 1, 2))), _rel(s[1], (v * v).sum((0, 1, 2)))]
        recs.append(rec)
    torch.cuda.synchronize()
    return recs


if __name__ == "__main__":
    with open(sys.argv[1], "w") as fh:
        json.dump(run_all(), fh)

"""The Winograd split kernel at kernel level (csrc/wino_split.hip): rd_wino_conv3x3 and rd_wino_conv3x3_bnbwd through the C ABI against
the float64 reference of tests/wino_ref.py, on the cases and at the per-element bars of tests/wino_cases.py (derived there from the
code).  tests/test_wino_host.py shows on the CPU that every named shortcut leaves these bars on these cases, that the lattice premise
holds and that every kept piece product carries one lattice class.

Every operand -- in, out, addend, bn_x -- is a channel window of a wider NaN-filled buffer with its own stride and offset and a NaN
guard behind it; the output and statistics buffers are NaN before the launch and LDS is poisoned (rd_debug_poison_lds): after the launch
everything outside the output window is still NaN, all inside is finite, the statistics rows are finite (slot 2 of the _bnbwd layout
untouched), the inputs are unchanged.  The statistics are held to float64 sums of the values the launch stored.  The lattice classes
are held bit for bit to the float64 convolution: no tolerance.

Each test prints ("FRACTION ..."; run with -s) the worst fraction of each bar.

Largest fractions observed on an MI355X when the file was added (records, not thresholds): output 0.0025 of its bar (forward), 0.0024
(input gradient with addend), 0.0020 (_bnbwd, and the cancelling addend); sum y 0.036, sum y^2 0.098, sum g 0.030, sum g (x - mean)
0.034 of theirs.  All nine lattice cases bit for bit; 20 misaligned calls refused.  A library built without the a2 b0 product fails
exactly the class A cases here and passes every per-element bar: the bars are for geometry, the lattice for the arithmetic.  No kernel
had to be changed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import norm_cases as NC
import wino_cases as WC

pytestmark = pytest.mark.gpu
F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


@pytest.mark.parametrize("c", WC.CASES, ids=WC.case_id)
def test_wino_per_element_vs_float64(c):
    """Output K_OUT(R) u S per element; statistics 34 / 35 u (sum, squares), 36 / 38 u (_bnbwd) per channel against the stored values."""
    fr = WC.run_case(c)
    print("FRACTION %-36s wgs %-3d worst %.4f  %s" % (WC.case_id(c), WC.workgroups(c), NC.worst(fr), " ".join("%s=%.4f" % kv for kv in sorted(fr.items()))))
    assert set(fr) == ({"out", "s0", "s1"} if WC.has_stat(c[0]) else {"out"})
    assert NC.worst(fr) <= 1.0, (c, {k: v for k, v in fr.items() if v > 1.0})


@pytest.mark.parametrize("c", WC.LATTICE_CASES, ids=WC.lattice_id)
def test_wino_lattice_classes_bit_for_bit(c):
    """Integer-lattice inputs on which every intermediate is exact (wino_cases.lattice_premise): the stored output IS the float64
    convolution.  Class A lives on a0 b0, a1 b0, a2 b0; B on a0 b0, a0 b1, a0 b2; C on a0 b0, a0 b1, a1 b0, a1 b1."""
    WC.lattice_premise(c)
    n_bad, first = WC.run_lattice(c)
    print("LATTICE %-24s differing elements: %d %s" % (WC.lattice_id(c), n_bad, first))
    assert n_bad == 0, (WC.lattice_id(c), n_bad, first)


def test_ops_wrappers_are_the_c_abi():
    """ops.wino_conv3x3 / ops.wino_conv3x3_bnbwd on channel slices of torch tensors: the same bits as the launches above."""
    from radar_depth_amd import ops
    c = WC.GEOMETRY[2]
    assert c[0] == "bnb_leaky"
    d, want = WC.case(c)
    st = WC.strides(c)
    out_abi, stat_abi = WC.launch(d, st)
    form, (N, H, W), red, out, _ = c

    def sl(a, key, fill=np.nan):
        ld, c0 = st[key]
        t = torch.full(a.shape[:3] + (ld,), fill, device="cuda")
        v = t[..., c0:c0 + a.shape[3]]
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return v

    x, bx = sl(d["x"], "x"), sl(d["bn_x"], "bn_x")
    y = sl(np.full((N, H, W, out), np.nan, F), "out")
    red_ = torch.full((ops.wino_stat_tiles(N, H, W), 3, out), float("nan"), device="cuda")
    u = ops.wino_pack(torch.from_numpy(d["w"]).cuda(), flip=True)
    ops.wino_conv3x3_bnbwd(x, u, y, bx, torch.from_numpy(d["mean"]).cuda(), torch.from_numpy(d["scale"]).cuda(), torch.from_numpy(d["shift"]).cuda(),
                           d["act"], red_)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.uint32), out_abi.view(np.uint32))
    assert np.array_equal(red_[:, :2].cpu().numpy().view(np.uint32), stat_abi[:, :2].view(np.uint32)) and torch.isnan(red_[:, 2]).all()


SENT = 0x7fc5a5a5          # a NaN with a payload: no kernel writes it


def test_misaligned_operands_are_refused_before_the_launch():
    """A window offset of 1 or 2 elements: `in` moves as 8-byte words (offset 1 refused), u_packed, out, addend, bn_x and the
    coefficient arrays as 16-byte words (offsets 1 and 2 refused).  RD_EINVAL from the host check -- the source is read first: every
    check stands before the launch -- and the sentinel-filled buffers stay untouched."""
    L, st = _L(), _st()
    src = open(os.path.join(REPO, "radar_depth_amd", "csrc", "wino_split.hip")).read()
    assert NC.checks_precede_launches(src, "wino_launch")
    bufs = [torch.from_numpy(np.full(1 << 18, SENT, np.uint32).view(np.int32)).cuda() for _ in range(5)]
    at = lambda b, elems=0: C.c_void_p(bufs[b].data_ptr() + 4 * elems)
    conv = [("in", at(0)), ("N", 1), ("H", 4), ("W", 4), ("Cin", 64), ("ldi", 68), ("u", at(1)), ("out", at(2)), ("Cout", 64), ("ldo", 72),
            ("addend", at(3)), ("ld_add", 76), ("stat", None), ("st", st)]
    bnb = conv[:10] + [("bn_x", at(3)), ("bn_ld", 76), ("mean", at(4)), ("scale", at(4, 64)), ("shift", at(4, 128)), ("act", 2), ("red", at(4, 256)),
                       ("st", st)]
    common = [dict(**{"in": at(0, 1)}), dict(out=at(2, 1)), dict(out=at(2, 2)), dict(u=at(1, 1)), dict(u=at(1, 2))]
    n = 0
    for name, spec, bad in (("rd_wino_conv3x3", conv, common + [dict(addend=at(3, 1)), dict(addend=at(3, 2))]),
                            ("rd_wino_conv3x3_bnbwd", bnb, common + [dict(bn_x=at(3, 1)), dict(bn_x=at(3, 2)), dict(mean=at(4, 1)), dict(mean=at(4, 2)),
                                                                     dict(scale=at(4, 65)), dict(scale=at(4, 66)), dict(shift=at(4, 129)),
                                                                     dict(shift=at(4, 130))])):
        for over in bad:
            rc = getattr(L, name)(*[over[k] if k in over else v for k, v in spec])
            shown = {k: getattr(v, "value", v) for k, v in over.items()}
            assert rc == -1, "%s(%r) returned %d: %s" % (name, shown, rc, L.rd_last_error())
            assert b"aligned" in L.rd_last_error() and b"rd_wino_conv3x3" in L.rd_last_error(), (name, shown, L.rd_last_error())
            n += 1
    torch.cuda.synchronize()
    for b in bufs:
        assert (b.cpu().numpy().view(np.uint32) == SENT).all(), "a refused call wrote"
    assert n == 20

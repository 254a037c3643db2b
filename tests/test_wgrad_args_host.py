"""No-GPU checks of the argument validation every weight-gradient entry point and query shares (csrc/common.h: RD_CHECK_WGRAD_STRIDES,
aligned16, RD_CHECK_WGRAD_COLS): a channel stride below the channel count, a tensor base that is not 16-byte aligned, and a reduction
whose columns [co_off, co_off + O) leave the descriptor's Cout are refused on the host, with a message through rd_last_error, before
anything is launched.  Every pointer handed over here is host memory and every call must return in front of its launch: the checks sit
ahead of hipLaunchKernelGGL in rd_wgrad, rd_wgrad_split, rd_wgrad_split_pre, rd_wgrad_bf16[_t] and the three reduces."""
import ctypes as C

import pytest

from wgrad_slice_cases import make_case, desc

CONV = make_case("conv", 2, (64, 8, 96), (64, 16, 96), 9, 11)                 # served by all four families
UPPROJ = make_case("upproj", 2, (64, 64, 128), (64, 0, 96), 5, 7, k=5)
FAMILIES = {    # family -> (supported, workspace, plan info + ints, launch, reduce)
    "wgrad": (None, "rd_wgrad_workspace_floats", ("rd_wgrad_plan_info", 9), "rd_wgrad", "rd_wgrad_reduce"),
    "wgrad_split": ("rd_wgrad_split_supported", "rd_wgrad_split_workspace_floats", ("rd_wgrad_split_plan_info", 4), "rd_wgrad_split",
                    "rd_wgrad_split_reduce"),
    "wgrad_split_pre": ("rd_wgrad_split_pre_supported", "rd_wgrad_split_workspace_floats", ("rd_wgrad_split_plan_info", 4), "rd_wgrad_split_pre",
                        "rd_wgrad_split_reduce"),
    "wgrad_bf16": ("rd_wgrad_bf16_supported", "rd_wgrad_bf16_workspace_floats", ("rd_wgrad_bf16_plan_info", 7), "rd_wgrad_bf16", "rd_wgrad_bf16_reduce"),
    "wgrad_bf16_t": ("rd_wgrad_bf16_supported", "rd_wgrad_bf16_workspace_floats", ("rd_wgrad_bf16_plan_info", 7), "rd_wgrad_bf16_t", "rd_wgrad_bf16_reduce"),
}


@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def host():
    """A 16-byte-aligned address inside host memory (never read: every call below fails its checks first)."""
    buf = C.create_string_buffer(4096)
    base = (C.addressof(buf) + 15) // 16 * 16
    return buf, base


def _launch(L, fam, d, x, dy, slabs):
    vp = C.c_void_p
    f = getattr(L, FAMILIES[fam][3])
    if fam == "wgrad_split_pre":
        return f(C.byref(d), vp(x), C.c_int64(1 << 30), vp(dy), C.c_int64(1 << 30), vp(slabs), None)
    if fam == "wgrad_bf16_t":
        return f(1, C.byref(d), vp(x), vp(dy), vp(slabs), None)
    return f(C.byref(d), vp(x), vp(dy), vp(slabs), None)


def _reduce(L, name, d, slabs, grad, o, co_off, s=9):
    k = 3 if s == 9 else 5
    return getattr(L, name)(C.byref(d), C.c_void_p(slabs), C.c_void_p(grad), o, d.Cin, k, k, co_off, 0, None)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("which", ["ldi", "ldo"])
def test_stride_below_the_channel_count_is_refused(L, host, fam, which):
    _, base = host
    sup, ws, (info, n_info), _, red = FAMILIES[fam]
    for case in (CONV, UPPROJ):
        good, d = desc(case), desc(case)
        setattr(d, which, (d.Cin if which == "ldi" else d.Cout) - 8)
        if sup:
            assert getattr(L, sup)(C.byref(good)) == 1 and getattr(L, sup)(C.byref(d)) == 0
        assert getattr(L, ws)(C.byref(good)) > 0
        assert getattr(L, ws)(C.byref(d)) < 0 and b"channel stride below the channel count" in L.rd_last_error()
        out = (C.c_int32 * n_info)()
        assert getattr(L, info)(C.byref(good), out) == 0 and getattr(L, info)(C.byref(d), out) != 0
        assert _launch(L, fam, d, base, base + 1024, base + 2048) == -1 and b"channel stride below the channel count" in L.rd_last_error()
        s = 25 if case.kind == "upproj" else 9
        assert _reduce(L, red, d, base, base + 1024, d.Cout, 0, s) == -1 and b"channel stride below the channel count" in L.rd_last_error()
        job = (C.c_byte * 256)()
        k = 5 if s == 25 else 3
        assert L.rd_wgrad_reduce_job(C.byref(d), int(fam.startswith("wgrad_bf16")), C.c_void_p(base), C.c_void_p(base + 1024), d.Cout, d.Cin, k, k, 0,
                                     0, job) == -1
        assert b"channel stride below the channel count" in L.rd_last_error()


@pytest.mark.parametrize("fam", sorted(FAMILIES))
@pytest.mark.parametrize("which", [0, 1, 2], ids=["in", "dout", "slabs"])
def test_unaligned_base_is_refused(L, host, fam, which):
    """A slice base off the 16-byte grid (a channel offset that is not a multiple of 4 floats): refused by every launch entry point, and an
    unaligned slab workspace by every reduction."""
    _, base = host
    d = desc(CONV)
    ptrs = [base, base + 1024, base + 2048]
    ptrs[which] += 4
    assert _launch(L, fam, d, *ptrs) == -1
    assert b"unaligned" in L.rd_last_error(), L.rd_last_error()
    red = FAMILIES[fam][4]
    assert _reduce(L, red, d, base + 4, base + 1024, d.Cout, 0) == -1 and b"unaligned" in L.rd_last_error()
    job = (C.c_byte * 256)()
    assert L.rd_wgrad_reduce_job(C.byref(d), int(fam.startswith("wgrad_bf16")), C.c_void_p(base + 8), C.c_void_p(base + 1024), d.Cout, d.Cin, 3, 3, 0, 0,
                                 job) == -1 and b"unaligned" in L.rd_last_error()


@pytest.mark.parametrize("red", ["rd_wgrad_reduce", "rd_wgrad_split_reduce", "rd_wgrad_bf16_reduce", "job", "job_bf16"])
def test_reduction_columns_outside_cout_are_refused(L, host, red):
    _, base = host
    d = desc(CONV)

    def call(o, co_off):
        if red.startswith("job"):
            return L.rd_wgrad_reduce_job(C.byref(d), int(red == "job_bf16"), C.c_void_p(base), C.c_void_p(base + 1024), o, d.Cin, 3, 3, co_off, 0,
                                         (C.c_byte * 256)())
        return _reduce(L, red, d, base, base + 1024, o, co_off)
    for o, co_off in ((16, -8), (d.Cout, 8), (d.Cout + 8, 0), (8, d.Cout)):
        assert call(o, co_off) == -1, (o, co_off)
        assert b"outside Cout" in L.rd_last_error(), L.rd_last_error()
    if red.startswith("job"):         # a host-only call: the accepted ranges fill a job record
        assert call(d.Cout, 0) == 0 and call(16, d.Cout - 16) == 0

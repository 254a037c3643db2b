"""CPU-only checks of what tests/test_gpu_wino_fp64.py stands on (tests/wino_ref.py, tests/wino_cases.py):

  - the float64 reference is torch's float64 conv2d / conv_transpose2d;
  - the documented arithmetic (wino_ref.emulate: float32 transform, three bf16 pieces, six kept products) stays inside every bar on
    every case, and every shortcut of wino_ref.MODES leaves a bar on the cases it can show on;
  - the lattice classes: the 2^24 premise in int64 along the kernel's data flow, the piece counts each class claims, and for each of
    the six kept terms a class whose result changes when that term is removed;
  - the cases cover what they are there for: six chunk residues, both workgroup orders off the XCD multiple, windows;
  - rd_wino_stat_tiles is the block arithmetic; the library's refusals, host side, nothing launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import norm_cases as NC
import wino_cases as WC
import wino_ref as R

F, D = np.float32, np.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _L():
    from radar_depth_amd._lib import lib
    return lib()


# ------------------------------------------------------------------------------------------------ the reference is the operation
@pytest.mark.parametrize("shape,O,I", [((2, 5, 7), 6, 10), ((3, 8, 3), 10, 6)])
def test_reference_is_torch_float64(shape, O, I):
    rng = np.random.default_rng(1)
    w = rng.standard_normal((O, I, 3, 3))
    x, dy = rng.standard_normal(shape + (I,)), rng.standard_normal(shape + (O,))
    y = TF.conv2d(torch.tensor(x).permute(0, 3, 1, 2), torch.tensor(w), padding=1).permute(0, 2, 3, 1).numpy()
    dx = TF.conv_transpose2d(torch.tensor(dy).permute(0, 3, 1, 2), torch.tensor(w), padding=1).permute(0, 2, 3, 1).numpy()
    assert np.abs(R.conv(x, w)[0] - y).max() <= 1e-13 * np.abs(y).max()
    assert np.abs(R.conv(dy, w, flip=True)[0] - dx).max() <= 1e-13 * np.abs(dx).max()
    # the Winograd identity the emulation and the magnitude stand on, in float64 (no pieces: U and V taken whole)
    u = R.PK.wino_gggt(R.eff_weights(w, False))
    p = np.zeros((shape[0], shape[1] + 3, shape[2] + 3, I))
    p[:, 1:shape[1] + 1, 1:shape[2] + 1] = x
    th, tw = (shape[1] + 1) // 2, (shape[2] + 1) // 2
    d = np.stack([np.stack([p[:, a:a + 2 * th:2, b:b + 2 * tw:2] for b in range(4)], 3) for a in range(4)], 3)
    m = np.einsum("ia,ntxabc,jb,qcij->ntxijq", R.BT, d, R.BT, u)
    yw = np.einsum("ri,ntxijq,sj->ntrxsq", R.AT, m, R.AT).reshape(shape[0], 2 * th, 2 * tw, O)[:, :shape[1], :shape[2]]
    assert np.abs(yw - y).max() <= 1e-12 * np.abs(y).max()
    assert (R.wino_magnitude(x, w) * (1 + 1e-6) >= np.abs(y)).all(), "S bounds the result"


# ------------------------------------------------------------------------------------------------ what the cases cover
def test_cases_cover_residues_orders_geometry_and_windows():
    L = _L()
    for c in WC.CASES:
        form, (N, H, W), red, out, layout = c
        st = WC.strides(c)
        assert L.rd_wino_supported(H, W, red, out, st["x"][0], st["out"][0]) == 1, c
        assert L.rd_wino_stat_tiles(N, H, W) == WC.blocks(N, H, W), c
        lds, offs = [v[0] for v in st.values()], [v[1] for v in st.values()]
        assert len(set(lds)) == 4 and len(set(offs)) == 4 and not any(v % 4 for v in lds + offs), c
    assert {c[2] // 16 % 6 for c in WC.CASES if not WC.is_flip(c[0])} == set(range(6)), "forward: every chunk-count residue mod 6"
    assert {c[2] // 16 % 6 for c in WC.CASES if WC.is_flip(c[0])} == set(range(6)), "input gradient: every chunk-count residue mod 6"
    assert {c[1] for c in WC.CASES} >= {(1, 2, 2), (2, 8, 16), (2, 7, 15), (2, 9, 17), (2, 3, 35), (3, 17, 33)}
    assert WC.blocks(2, 8, 16) == 2 and WC.blocks(2, 7, 15) == 2 and WC.blocks(2, 9, 17) == 8
    # both workgroup orders (channel-block-major from four channel blocks on) with more than one pixel block off the 8-XCD multiple
    for major in (False, True):
        assert any((c[3] // 64 >= 4) == major and WC.workgroups(c) % 8 and WC.blocks(*c[1]) > 1 for c in WC.CASES), major
    assert {c[3] for c in WC.CASES} >= {64, 128, 256}
    assert {c[0] for c in WC.CASES} == set(WC.FORMS)
    # a window at the end of its buffer's rows, for every operand
    ends = {k for lay in WC.LAYOUTS.values() for k, (e, c0) in lay.items() if e == c0}
    assert ends == {"x", "out", "addend", "bn_x"}
    assert WC.k_out(64) == 399 and WC.k_out(144) == 884
    # rd_wino_stat_tiles against the block arithmetic on a sweep
    for N in (1, 3):
        for H in range(2, 20):
            for W in (2, 15, 16, 17, 31, 32, 33, 200):
                assert L.rd_wino_stat_tiles(N, H, W) == N * -(-((H + 1) // 2) // 4) * -(-((W + 1) // 2) // 8)


# ------------------------------------------------------------------------------------------------ the documented arithmetic passes
def _missed(c, mode):
    d, want = WC.case(c)
    out, stat = WC.shortcut(c, mode)
    fr = WC.fracs(d, want, out, stat)
    return {k for k, v in fr.items() if v > 1.0}, fr


def test_documented_arithmetic_passes_every_bar(capsys):
    lines = []
    for c in WC.CASES:
        missed, fr = _missed(c, "exact")
        assert not missed, (c, fr)
        lines.append("%-36s %s" % (WC.case_id(c), " ".join("%s=%.4f" % kv for kv in sorted(fr.items()))))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# mode -> (the cases it can show on, the outputs that must then leave their bar)
_odd = lambda c: c[1][1] % 2 or c[1][2] % 2
WHERE = {
    "taps_not_rotated": (lambda c: WC.is_flip(c[0]), {"out"}),
    "channels_not_transposed": (lambda c: WC.is_flip(c[0]) and c[2] == c[3], {"out"}),      # (the tensor is square only there)
    "row_wrap": (lambda c: True, {"out"}),
    "next_image": (lambda c: c[1][0] >= 2, {"out"}),
    "masked_counted": (lambda c: WC.has_stat(c[0]) and _odd(c), {"s0", "s1"}),
    "stats_unrounded": (lambda c: c[0] == "fwd_stat_cancel", {"s0", "s1"}),                # elsewhere half an ulp per element: inside the bar
    "addend_at_out_stride": (lambda c: c[0] in ("dgrad_add", "fwd_stat_cancel"), {"out"}),
    "bn_x_at_out_stride": (lambda c: c[0].startswith("bnb"), {"s1"}),
    "no_mean": (lambda c: c[0].startswith("bnb"), {"s1"}),
    "relu_for_leaky": (lambda c: c[0] == "bnb_leaky", {"s0", "s1"}),
}


def test_every_mode_is_listed():
    assert set(WHERE) == set(R.MODES) - {"exact"}


@pytest.mark.parametrize("mode", sorted(WHERE))
def test_shortcuts_leave_the_bars(mode):
    shows, outputs = WHERE[mode]
    # (the larger maps add nothing here: one case per form and layout, the small maps)
    cases = [c for c in WC.CASES if shows(c) and np.prod(c[1]) * c[2] * c[3] <= 2 * 7 * 15 * 144 * 256]
    assert cases, mode
    for c in cases:
        missed, fr = _missed(c, mode)
        assert outputs <= missed, (mode, c, fr)


# ------------------------------------------------------------------------------------------------ the lattice classes
@pytest.mark.parametrize("c", WC.LATTICE_CASES, ids=WC.lattice_id)
def test_lattice_premise_holds(c, capsys):
    fig = WC.lattice_premise(c)
    d, want = WC.lattice_data(c)
    assert np.array_equal(R.emulate(d["x"], d["w"], d["flip"]), want), "all six terms: the documented arithmetic is exact on the class"
    with capsys.disabled():
        print("\n%-24s worst partial 2^%.1f, V %d bits, U %d bits, %.0f %% non-zero" % (WC.lattice_id(c), fig["worst_log2"], fig["v_bits"],
                                                                                      fig["u_bits"], 100 * fig["nonzero"]))


def test_every_kept_term_carries_a_class():
    """Each of the six kept terms, removed, changes at least one output of the class meant for it -- and of no class that does not
    claim it (there the term is exactly zero)."""
    assert {t for ts in WC.LATTICE.values() for t in ts} == set(R.KEPT)
    for c in WC.LATTICE_CASES:
        d, want = WC.lattice_data(c)
        for term in R.KEPT:
            changed = int((R.emulate(d["x"], d["w"], d["flip"], drop=term) != want).sum())
            assert (changed > 0) == (term in WC.LATTICE[c[0]]), (WC.lattice_id(c), term, changed)


# ------------------------------------------------------------------------------------------------ refusals, host side
def test_refusals_before_anything_is_launched():
    """rd_wino_supported and the entry points refuse H or W < 2, Cin % 16, Cin < 64, Cout % 64, a stride off the 4-element grid, an image
    of 2^31 bytes or more, a misaligned operand and, _bnbwd, a null mean / scale / shift / statistics pointer: -1 with the entry point's
    name in rd_last_error.  Every check stands before the launch (the source is read first); the buffers are the device's where there is
    one -- large enough for any launch of the geometry used -- and host memory otherwise."""
    L = _L()
    src = open(os.path.join(REPO, "radar_depth_amd", "csrc", "wino_split.hip")).read()
    assert NC.checks_precede_launches(src, "wino_launch")
    ok = (8, 8, 64, 64, 64, 64)
    assert L.rd_wino_supported(*ok) == 1
    bad_shapes = [(1, 8, 64, 64, 64, 64), (8, 1, 64, 64, 64, 64), (8, 8, 72, 64, 72, 64), (8, 8, 48, 64, 48, 64), (8, 8, 32, 64, 32, 64),
                  (8, 8, 64, 96, 64, 96), (8, 8, 64, 32, 64, 32), (8, 8, 64, 64, 66, 64), (8, 8, 64, 64, 64, 70),
                  (2048, 2048, 64, 64, 128, 64), (4096, 2048, 64, 64, 64, 64)]
    for s in bad_shapes:
        assert L.rd_wino_supported(*s) == 0 and L.rd_wino_preferred(*s) == 0, s
    assert L.rd_wino_supported(2048, 2047, 64, 64, 128, 64) == 1, "just below 2^31 bytes"
    n = 1 << 18
    if torch.cuda.is_available():
        bufs = [torch.zeros(n, device="cuda") for _ in range(5)]
        base = [b.data_ptr() for b in bufs]
    else:
        bufs = [np.zeros(n + 4, F) for _ in range(5)]
        base = [(b.ctypes.data + 15) // 16 * 16 for b in bufs]
    at = lambda i, nbytes=0: C.c_void_p(base[i] + nbytes)
    I, Uo, O, A, S = range(5)
    conv = [("in", at(I)), ("N", 1), ("H", 8), ("W", 8), ("Cin", 64), ("ldi", 64), ("u", at(Uo)), ("out", at(O)), ("Cout", 64), ("ldo", 64),
            ("addend", at(A)), ("ld_add", 64), ("stat", at(S)), ("st", None)]
    bnb = conv[:10] + [("bn_x", at(A)), ("bn_ld", 64), ("mean", at(S, 4096)), ("scale", at(S, 8192)), ("shift", at(S, 12288)), ("act", 1),
                       ("red", at(S)), ("st", None)]
    shape_bad = [dict(H=1), dict(W=1), dict(Cin=72, ldi=72), dict(Cin=48, ldi=48), dict(Cout=96, ldo=96), dict(ldi=66), dict(ldo=70), dict(N=0),
                 dict(**{"in": None}), dict(u=None), dict(out=None)]
    align_bad = [dict(**{"in": at(I, 4)}), dict(out=at(O, 4)), dict(out=at(O, 8)), dict(u=at(Uo, 8))]
    cases = [("rd_wino_conv3x3", conv, shape_bad + align_bad + [dict(ld_add=66), dict(addend=at(A, 4)), dict(addend=at(A, 8))]),
             ("rd_wino_conv3x3_bnbwd", bnb, shape_bad + align_bad + [dict(bn_ld=66), dict(bn_x=None), dict(mean=None), dict(scale=None),
                                                                     dict(shift=None), dict(red=None), dict(bn_x=at(A, 4)), dict(bn_x=at(A, 8)),
                                                                     dict(mean=at(S, 4100)), dict(scale=at(S, 8200)), dict(shift=at(S, 12296))])]
    refused = 0
    for name, spec, bad in cases:
        for over in bad:
            assert all(k in dict(spec) for k in over), (name, over)
            rc = getattr(L, name)(*[over[k] if k in over else v for k, v in spec])
            shown = {k: getattr(v, "value", v) for k, v in over.items()}
            assert rc == -1, "%s(%r) returned %d: %s" % (name, shown, rc, L.rd_last_error())
            assert b"rd_wino_conv3x3" in L.rd_last_error(), (name, shown, L.rd_last_error())
            refused += 1
    assert refused == 44


@pytest.mark.parametrize("kernel", WC.FLAT_ALL)
def test_flat_lattice_premise_and_kept_terms(kernel):
    """The classes without the transform (the other forward kernels of the split family): the premise is asserted with the data; all
    six terms give the float64 result exactly; a removed term changes exactly the classes that claim it."""
    for cls in sorted(WC.LATTICE):
        d, x, w, want = WC.flat_data(kernel, cls)
        assert np.array_equal(WC.flat_emulate(d, x, w), want, equal_nan=True)
        for term in R.KEPT:
            got = WC.flat_emulate(d, x, w, drop=term)
            changed = int(((got != want) & ~np.isnan(want)).sum())
            assert (changed > 0) == (term in WC.LATTICE[cls]), (kernel, cls, term, changed)


def test_flat_tile_kinds_are_what_the_forced_tile_file_needs():
    """tests/test_gpu_split_lattice_tiles.py: the library's own plan runs every kind on the 1x1 tile (so only the forced configurations
    reach the other forms), none of them is a one-tap descriptor on gemm1_split (plan marker 1000), and the phases have the tap counts
    the kinds are named for."""
    L = _L()
    prev = L.rd_gconv_split_plan_all(1)
    try:
        taps = {}
        for kernel in ("gconv_split_3x3", "gconv_split_pre_3x3") + WC.FLAT_TILE_KERNELS:
            d, slabs = WC.flat_desc(kernel)
            pre = "_pre_" in kernel
            info = (C.c_int32 * 8)()
            assert (L.rd_gconv_split_pre_supported if pre else L.rd_gconv_split_supported)(C.byref(d)) == 1, kernel
            assert (L.rd_gconv_split_pre_plan_info if pre else L.rd_gconv_split_plan_info)(C.byref(d), info) == 0
            assert list(info[:2]) == [1, 1] and info[7] != 1000, (kernel, list(info))
            kind = kernel[len("gconv_split_pre_" if pre else "gconv_split_"):]
            taps[kind] = [d.phase[i].n_taps for i in range(d.n_phases)]
            assert 1 + max(d.phase[i].widx[t] for i in range(d.n_phases) for t in range(d.phase[i].n_taps)) == slabs == WC.FLAT_TILE_KINDS[kind]
            assert (d.Cin, d.Cout) == ((96, 96) if kind == "3x3_partial" else (64, 64)) and d.N == 2
        assert taps == {"3x3": [9], "upproj_fwd": [9, 6, 6, 4], "dgrad_s2": [1, 2, 2, 4], "upproj_dgrad": [25], "3x3_partial": [9]}
    finally:
        L.rd_gconv_split_plan_all(1 if prev == 1 else 0)

"""No-GPU checks of tests/pack_ref.py, the numpy restatement tests/test_gpu_pack.py holds the pack kernels to, and of the argument
refusals of rd_pack_weights / rd_pack_weights_bf16:

  * bf16_rne equals torch's CPU conversion on the rounding ladder and on 10^5 normals; split3's pieces add up to x exactly in float32
    for 2^-60 <= |x| <= 2^60 and +-0 (inside that range no piece is subnormal and the definition has no special cases);
  * every physical index map is a bijection onto [0, T R ldc) and reproduces entries worked out by hand from the header's formulas;
  * G g G^T, with B^T d B and A^T m A, is the 3x3 correlation of a 4x4 tile (flip = 1: the transposed convolution's) to 1e-12;
  * every shortcut of pack_ref.MODES changes at least one element of the operands the GPU tests pack;
  * the refusals: host pointers only, every call returns before a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_cases as PC
import pack_ref as R

F = np.float32


# ------------------------------------------------------------------------------------------------ bit-level conversions
def _normals():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(100000) * np.exp2(rng.integers(-40, 40, 100000))).astype(F)
    return x[(np.abs(x) >= F(2.0) ** -R.RANGE_LOG2) & (np.abs(x) <= F(2.0) ** R.RANGE_LOG2)]


def test_ladder_holds_what_it_says():
    lad = R.rounding_ladder()
    bits = lad.view(np.uint32)
    low, kept = bits & 0xffff, (bits >> 16) & 0x7f
    for sign in (0, 1):
        s = (bits >> 31) == sign
        assert (s & (low == 0x8000) & (kept % 2 == 0)).any() and (s & (low == 0x8000) & (kept % 2 == 1)).any()      # ties, even and odd
        assert (s & (low == 0x7fff)).any() and (s & (low == 0x8001)).any()                                            # their neighbours
        assert (s & ((bits & 0x7fffff) == 0x7fffff)).any() and (s & (kept == 0x7f) & (low == 0x8000)).any()           # carries into the exponent
    assert (bits == 0).any() and (bits == 0x80000000).any()
    assert len(set(((bits >> 23) & 0xff).tolist())) >= 7


@pytest.mark.parametrize("which", ["ladder", "normals"])
def test_bf16_rne_equals_torch(which):
    x = R.rounding_ladder() if which == "ladder" else _normals()
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_rne(x), want)
    if which == "ladder":          # the two wrong roundings are told apart here
        assert not np.array_equal(R.bf16_rne(x, "truncate"), want) and not np.array_equal(R.bf16_rne(x, "half_up"), want)


@pytest.mark.parametrize("which", ["ladder", "normals"])
def test_split3_adds_up_exactly(which):
    x = R.rounding_ladder() if which == "ladder" else _normals()
    p0, p1, p2 = (R.bf16_to_f32(p) for p in R.split3(x))
    s = (p0 + p1) + p2
    assert s.dtype == F and np.array_equal(s, x)                # (-0 == +0: the sum of the pieces of -0 is +0)
    assert np.array_equal(np.signbit(p0), np.signbit(x))
    for p in (p0, p1, p2):                                      # no piece is subnormal in the stated range
        assert (np.abs(p[p != 0]) >= np.finfo(F).tiny).all()
    q0, q1, q2 = (R.bf16_to_f32(p) for p in R.split3(x, "two_pieces"))
    assert not np.array_equal((q0 + q1) + q2, x) and not q2.any()


# ------------------------------------------------------------------------------------------------ index maps
@pytest.mark.parametrize("quad,T,Rr,ldc", [(0, 49, 3, 5), (0, 1, 1, 1), (1, 9, 8, 7), (1, 2, 4, 1), (2, 9, 16, 5), (2, 1, 8, 3), (3, 4, 24, 6)])
def test_index_maps_are_bijections(quad, T, Rr, ldc):
    t, r, c = np.meshgrid(np.arange(T), np.arange(Rr), np.arange(ldc), indexing="ij")
    idx = R.phys_index(quad, T, Rr, ldc, t.ravel(), r.ravel(), c.ravel())
    assert np.array_equal(np.sort(idx), np.arange(T * Rr * ldc))
    if quad == 3:          # the three planes tile [0, 3 T R ldc)
        allp = np.concatenate([idx + p * R.plane_elems(T, Rr, ldc) for p in range(3)])
        assert np.array_equal(np.sort(allp), np.arange(3 * T * Rr * ldc))


def test_index_maps_by_hand():
    # quad 0: (slab R + row) ldc + col                       T = 49, R = 4, ldc = 64: (slab 2, row 3, col 5) -> (2 * 4 + 3) * 64 + 5
    assert R.phys_index(0, 49, 4, 64, 2, 3, 5) == 709
    # quad 1: ((slab R/4 + row/4) ldc + col) 4 + row%4       R = 8, ldc = 40: (1, 6, 17) -> ((1 * 2 + 1) * 40 + 17) * 4 + 2
    assert R.phys_index(1, 9, 8, 40, 1, 6, 17) == 550
    assert R.phys_index(1, 9, 8, 40, 0, 0, 0) == 0 and R.phys_index(1, 9, 8, 40, 0, 3, 0) == 3 and R.phys_index(1, 9, 8, 40, 0, 4, 0) == 160
    # quad 2: ((slab R/8 + row/8) ldc + col) 8 + row%8       R = 24, ldc = 14: (2, 19, 13) -> ((2 * 3 + 2) * 14 + 13) * 8 + 3
    assert R.phys_index(2, 9, 24, 14, 2, 19, 13) == 1003
    assert R.phys_index(2, 9, 24, 14, 0, 7, 0) == 7 and R.phys_index(2, 9, 24, 14, 0, 8, 0) == 112 and R.phys_index(2, 9, 24, 14, 0, 0, 1) == 8
    # quad 3: plane p of the quad 2 layout, T R ldc apart
    assert R.phys_index(3, 9, 24, 14, 2, 19, 13) == 1003 and R.plane_elems(9, 24, 14) == 3024
    # the wrong interleave for a bf16 operand lands elsewhere
    assert R.phys_index(2, 9, 24, 14, 2, 19, 13, "quad4_for_bf16") == ((2 * 6 + 4) * 14 + 13) * 4 + 3


def test_logical_operand_by_hand():
    """Forward: row = i, col = co_off + o; transposed: row = co_off + o, col = i; the fold is one float32 multiply by scale[o], or by
    scale[i] with scale_col."""
    O, I, T = 3, 4, 2
    w = np.arange(O * I * T, dtype=F).reshape(O, I, T) + 1
    s_row, s_col = np.array([2, 3, 5], dtype=F), np.array([7, 11, 13, 17], dtype=F)
    dst = np.zeros(T * I * 6, dtype=np.uint32)
    R.pack_into(dst, w, O, I, T, 6, 2, I, 0, 0, s_row, 0)
    L = dst.view(F).reshape(T, I, 6)
    assert L[1, 2, 2 + 1] == w[1, 2, 1] * 3 and L[0, 3, 2 + 2] == w[2, 3, 0] * 5 and not L[:, :, :2].any() and not L[:, :, 5:].any()
    dst = np.zeros(T * 8 * 4, dtype=np.uint32)
    R.pack_into(dst, w, O, I, T, 4, 4, 8, 1, 0, s_col, 1)
    L = dst.view(F).reshape(T, 8, 4)
    assert L[1, 4 + 1, 2] == w[1, 2, 1] * 13 and L[0, 4 + 2, 3] == w[2, 3, 0] * 17 and not L[:, :4].any() and not L[:, 7:].any()


# ------------------------------------------------------------------------------------------------ the Winograd transform
def _wino_tile(g, d):
    """A^T [(G g G^T) (.) (B^T d B)] A of one filter and one 4x4 tile, float64."""
    Bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
    At = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
    return At @ (R.wino_gggt(g) * (Bt @ d @ Bt.T)) @ At.T


def test_wino_transform_is_the_3x3_correlation():
    rng = np.random.default_rng(11)
    for _ in range(20):
        g, d = rng.standard_normal((3, 3)), rng.standard_normal((4, 4))
        want = np.array([[(g * d[y:y + 3, x:x + 3]).sum() for x in range(2)] for y in range(2)])
        assert np.abs(_wino_tile(g, d) - want).max() <= 1e-12
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
    g = rng.standard_normal((5, 3, 3))
    assert np.abs(R.wino_gggt(g) - G @ g @ G.T).max() <= 1e-15


def test_wino_flip_is_the_transposed_convolution():
    """flip = 1: the operand of dx = conv_transpose(dy, w): output channel = i, reduction channel = o, taps rotated by 180 degrees.
    Checked through wino_u's own unpacked pieces against torch's conv_transpose2d on one 2x2 output tile."""
    O, I = 16, 64
    rng = np.random.default_rng(12)
    w = (rng.standard_normal((O, I, 3, 3)) * 0.1).astype(F)
    dy = rng.standard_normal((O, 4, 4))                                             # a 4x4 patch of dy = the 2x2 tile of dx at its centre
    Bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
    At = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
    V = np.einsum("ab,obc,dc->oad", Bt, dy, Bt).reshape(O, 16)
    full = torch.nn.functional.conv_transpose2d(torch.from_numpy(dy)[None], torch.from_numpy(w.astype(np.float64)), padding=1)[0].numpy()

    def tile(mode):
        u = R.wino_u(w, 1, mode).reshape(16, 3, 2, 64, 8)                           # one cot, one chunk: [pos][piece][k half][co][k]
        U = sum(R.bf16_to_f32(u[:, p]).astype(np.float64) for p in range(3))        # the pieces add up to fp32(U): [pos][k half][co = i][k]
        U = U.transpose(0, 1, 3, 2).reshape(16, O, I)                               # -> U[pos][o][i]
        m = np.einsum("poi,op->ip", U, V).reshape(I, 4, 4)
        return np.einsum("ab,ibc,dc->iad", At, m, At)
    assert np.abs(tile("exact") - full[:, 1:3, 1:3]).max() <= 1e-6                  # (U is fp32 here: 16 products of ~0.1)
    assert np.abs(tile("wino_flip_no_rotation") - full[:, 1:3, 1:3]).max() > 1e-2
    # ... and to 1e-12 on the float64 transform itself, the channel roles and the rotation written out
    g = w.astype(np.float64).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]                # [i][o], rotated
    m = np.einsum("iop,op->ip", R.wino_gggt(g).reshape(I, O, 16), V).reshape(I, 4, 4)
    assert np.abs(np.einsum("ab,ibc,dc->iad", At, m, At) - full[:, 1:3, 1:3]).max() <= 1e-12


def test_wino_u_layout_by_hand():
    """[cot][chunk][pos 16][piece 3][k half 2][co 64][8 reduction channels]: one element looked up by its coordinates."""
    O, I, flip = PC.WINO[3]                     # 128 x 80
    w = PC.wino_weights(3)
    u = R.wino_u(w, flip).reshape(2, 5, 16, 3, 2, 64, 8)
    o, i = 64 + 37, 16 * 3 + 8 + 5              # cot 1, co 37; chunk 3, k half 1, k 5
    U = R.wino_gggt(w[o, i].astype(np.float64)).astype(F)
    for pos in (0, 6, 15):
        pcs = R.split3(U.reshape(16)[pos:pos + 1])
        assert [int(u[1, 3, pos, p, 1, 37, 5]) for p in range(3)] == [int(p[0]) for p in pcs]
    assert u.size * 2 == 2 * 5 * 98304


# ------------------------------------------------------------------------------------------------ the shortcuts are visible
def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def exact():
    return dict(single=[PC.expected(js) for js in PC.all_single_jobs()], batched=PC.expected(PC.batched_jobs()),
                wino=[PC.wino_expected(n) for n in range(len(PC.WINO))])


@pytest.mark.parametrize("mode", [m for m in R.MODES if m != "exact"])
def test_every_shortcut_changes_an_operand_the_gpu_tests_pack(exact, mode):
    single = any(_differs(PC.expected(js, mode), e) for js, e in zip(PC.all_single_jobs(), exact["single"]))
    batched = _differs(PC.expected(PC.batched_jobs(), mode), exact["batched"])
    wino = any(not np.array_equal(PC.wino_expected(n, mode), e) for n, e in enumerate(exact["wino"]))
    seen = dict(truncate=single and batched and wino, half_up=single and batched and wino, two_pieces=batched and wino,
                scale_after_round=batched, scale_by_row_when_col=batched, wino_round_twice=wino, wino_flip_no_rotation=wino, wino_p0_from_float=wino,
                quad4_for_bf16=single and batched)[mode]
    assert seen, (mode, single, batched, wino)
    if mode == "wino_p0_from_float":          # the planted tie: in every Winograd case, both forms of the kernel
        assert all(not np.array_equal(PC.wino_expected(n, mode), e) for n, e in enumerate(exact["wino"]))


def test_the_batched_table_takes_both_paths_and_every_fold():
    jobs = PC.batched_jobs()
    assert {j["quad"] for j in jobs} == {0, 1, 2, 3} and {j["transpose"] for j in jobs} == {0, 1}
    for quad in (2, 3):
        paths = {(PC.takes_unit_path(j), j["transpose"]) for j in jobs if j["quad"] == quad}
        assert (True, 1) in paths and (False, 1) in paths and (True, 0) in paths
    assert {j["fold"] for j in jobs} == {"none", "row", "col"}
    assert any(j["fold"] != "none" and j["transpose"] for j in jobs) and any(j["fold"] == "col" and not j["transpose"] for j in jobs)
    chunk = 2048
    idle = [j for j in jobs if PC.takes_unit_path(j) and R.pack_blocks(j["O"], j["I"], j["T"], chunk) > -(-(PC.rows(j) // 8 * j["ldc"]) // 256)]
    assert idle, "a job whose unit form leaves surplus blocks idle"
    exp = PC.expected(jobs)
    assert all((e[:PC.GUARD] == e[-1]).all() for e in exp.values())                          # guards
    assert any((e[PC.GUARD:-PC.GUARD] == e[-1]).any() for e in exp.values())                 # and unowned elements inside an operand


# ------------------------------------------------------------------------------------------------ refusals (host memory, no launch)
@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


@pytest.mark.parametrize("fn,k", [("rd_pack_weights", 4), ("rd_pack_weights_bf16", 8)])
def test_pack_geometry_outside_the_operand_is_refused(L, fn, k):
    """co_off < 0; forward: co_off + O > ldc; transposed: co_off + O > rows_total or I > ldc -- RD_EINVAL with a message, before the
    launch.  The valid neighbours pass the geometry check: handed a NULL destination they get as far as the pointer check behind it."""
    buf = C.create_string_buffer(4096)
    host = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)
    f = getattr(L, fn)

    def call(dst, O, I, ldc, off, rows_total, transpose):
        return f(host, dst, O, I, 3, 3, ldc, off, rows_total, transpose, None), L.rd_last_error()
    O, I = 2 * k, k
    bad = [((O, I, O, -1, I, 0), b"negative offset"), ((O, I, O + 8, -8, I, 0), b"negative offset"),
           ((O, I, O - 1, 0, I, 0), b"outside ldc"), ((O, I, O + 3, 4, I, 0), b"outside ldc"),
           ((O, I, I, -k, 2 * O, 1), b"negative offset"),
           ((O, I, I, k, O, 1), b"outside rows_total"), ((O, I, I, 1, O, 1), b"outside rows_total"),
           ((O, I, I - 1, 0, O, 1), b"outside ldc")]
    for args, msg in bad:
        rc, err = call(host, *args)
        assert rc == -1 and msg in err, (args, rc, err)
    good = [(O, I, O, 0, I, 0), (O, I, O + 3, 3, I, 0), (O, I, I, 0, O, 1), (O, I, I, k, O + k, 1), (O, I, I + 5, 0, O, 1)]
    for args in good:
        rc, err = call(None, *args)
        assert rc == -1 and b"null pointer" in err, (args, rc, err)
    rc, err = call(host, O, I + 1, O, 0, I + 1, 0)                                 # (the older refusal still comes first)
    assert rc == -1 and b"multiple of" in err

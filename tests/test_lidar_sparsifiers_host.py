"""The lidar sparsifiers (lidar_radar, uniform) without a GPU: the numpy restatement (tests/lidar_sparsifier_ref.py) against the vectors of
the reference's own dense_to_sparse / get_sparse_depth / transform_val / transform_train (tests/golden/lidar_sparsifiers.npz,
tests/golden/make_golden_lidar_sparsifiers.py), the tie rule, Philox4x32-10 against known answers, every argument check of the C ABI
(nothing is launched), and the Python surface."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_sparsifier_ref as S  # noqa: E402
from lidar_sparsifier_cases import G, LR_NAMES, PKEYS, STAGED, UN_NAMES, staged, tie_frame  # noqa: E402


# ------------------------------------------------------------------------------------------------ restatement and fixture
def test_fixture_lists_its_cases():
    assert G["lr_names"].tolist() == LR_NAMES and G["un_names"].tolist() == UN_NAMES and G["staged_names"].tolist() == [s[0] for s in STAGED]
    tied = [k for k in G.files if k.endswith("_n_tied")]
    assert len(tied) == len(LR_NAMES) + 4 and all(int(np.sum(G[k])) == 0 for k in tied)         # no frame is left out of any comparison


@pytest.mark.parametrize("name", LR_NAMES)
def test_restatement_lidar_radar_matches_reference_vectors(name):
    lidar, radar = G[name + "_lidar"], G[name + "_radar"]
    assert S.n_tied(lidar, radar) == 0 == int(G[name + "_n_tied"])
    got = S.lidar_radar_sparse(lidar, radar)
    assert got.dtype == np.float32 and np.array_equal(got, G[name + "_sparse"])
    assert np.array_equal(got != 0, S.lidar_radar_mask(lidar, radar))


@pytest.mark.parametrize("name", UN_NAMES)
def test_restatement_uniform_matches_reference_vectors(name):
    got = S.uniform_sparse(G[name + "_depth"], int(G[name + "_num_samples"]), float(G[name + "_max_depth"]), G[name + "_draws"])
    assert got.dtype == np.float32 and np.array_equal(got, G[name + "_sparse"])


@pytest.mark.parametrize("name,mode,sparsifier", STAGED)
def test_restatement_staging_matches_reference_vectors(name, mode, sparsifier):
    img, lidar, radar, p, crop, ns, md, draws, want_in, want_lb, before = staged(name)
    got = S.staged(mode, img, lidar, radar, p, crop, sparsifier, ns, md, draws)
    assert np.array_equal(got[0], want_in) and np.array_equal(got[1], want_lb) and np.array_equal(got[2], before)
    assert all((want_in[b, 3] != before[b, 0]).any() and (want_in[b, 3] != 0).any() for b in range(len(want_in)))     # the sparsifier acts
    if sparsifier == "lidar_radar":
        assert [S.n_tied(want_lb[b, 0], before[b, 0]) for b in range(len(want_lb))] == [0] * len(want_lb) == G[name + "_n_tied"].tolist()


def test_golden_cases_cover_what_they_claim():
    count = lambda n: int((G[n + "_lidar"] > 0).sum())        # noqa: E731
    assert [count(n) for n in LR_NAMES[:6]] == [0, 1, 2, 63, 64, 65] and 280 <= count("lr_l300") <= 320
    assert {G[n + "_lidar"].shape for n in LR_NAMES} == {(33, 47), (45, 80)}
    assert not G["lr_norad_radar"].any() and count("lr_norad") > 0 and not G["lr_norad_sparse"].any()
    assert not G["lr_l0_sparse"].any() and (G["lr_l0_radar"] > 0).sum() == 12
    assert (G["lr_l1_sparse"] != 0).sum() == 1 and (G["lr_l2_sparse"] != 0).sum() == 2      # fewer than two lidar pixels: all of them
    for name in ("lr_special", "lr_special2"):
        lidar, radar, sparse = G[name + "_lidar"], G[name + "_radar"], G[name + "_sparse"]
        h, w = lidar.shape
        assert ((lidar > 0) & (radar > 0)).any()                                            # a radar pixel on a lidar pixel
        assert sparse[0, 0] == lidar[0, 0] > 0 and sparse[h - 1, w - 1] == lidar[h - 1, w - 1] > 0      # both corners, and chosen
        assert (radar > 250).sum() >= 3                                                     # above any max_depth, and they count:
        assert not np.array_equal(S.lidar_radar_sparse(lidar, np.where(radar > 250, 0, radar)), sparse)
        picks = np.zeros(lidar.shape, np.int64)                                             # two radar pixels choose one lidar pixel
        for y, x in zip(*np.nonzero(radar > 0)):
            one = np.zeros_like(radar)
            one[y, x] = 1
            picks += S.lidar_radar_mask(lidar, one)
        assert picks.max() >= 2
    keep = lambda n: int((G[n + "_depth"] > 0).sum())         # noqa: E731
    assert keep("un_empty") == 0 and int(G["un_ns0_num_samples"]) == 0 and keep("un_ns0") > 0 and not G["un_ns0_sparse"].any()
    d = G["un_all_depth"]
    assert int(G["un_all_num_samples"]) >= keep("un_all") and np.array_equal(G["un_all_sparse"], np.where(d <= np.float32(80.0), d, 0))
    assert np.isinf(float(G["un_inf_max_depth"])) and np.isinf(float(G["un_empty_max_depth"]))
    assert float(G["un_md_max_depth"]) == 79.9
    d, u, s = G["un_md_depth"][0], G["un_md_draws"][0], G["un_md_sparse"][0]
    at, above, equal, below = (tuple(G["un_md_" + k]) for k in ("at", "above", "equal", "below"))
    assert d[at] == np.float32(79.9) and float(d[at]) > 79.9 and s[at] == d[at]              # kept although 79.900001... > 79.9 in double
    assert d[above] == np.nextafter(np.float32(79.9), np.float32(np.inf)) and u[above] == 0 and s[above] == 0
    n_keep = int(((d > 0) & (d <= np.float32(79.9))).sum())
    prob = 150.0 / n_keep
    assert prob == float(G["un_md_prob"]) and u[equal] == prob and d[equal] > 0 and s[equal] == 0      # strict <
    assert u[below] == np.nextafter(prob, 0.0) and s[below] == d[below] > 0


def test_training_draws_follow_the_recorded_recipe():
    """draw_train_params(1, rng=rs) followed by rs.uniform(0, 1, (1, ch, cw)) per frame (the reference worker's order) gives the stored
    parameters and draws; validation draws nothing before the sparsifier."""
    from radar_depth_amd.dataset import draw_train_params
    crop = tuple(int(v) for v in G["tr_un_crop"])
    lo, hi, rot = G["tr_un_draw"]
    for b, seed in enumerate(G["tr_un_seeds"]):
        rs = np.random.RandomState(int(seed))
        p = draw_train_params(1, crop, (lo, hi), rot, rng=rs)
        for k in PKEYS:
            assert np.array_equal(p[k][0], G["tr_un_p_" + k][b]), k
        assert np.array_equal(rs.uniform(0, 1, (1,) + crop), G["tr_un_draws"][b])
    crop = tuple(int(v) for v in G["val_un_crop"])
    for b, seed in enumerate(G["val_un_seeds"]):
        assert np.array_equal(np.random.RandomState(int(seed)).uniform(0, 1, (1,) + crop), G["val_un_draws"][b])


def test_equal_distances_go_to_the_lower_index():
    """Checked against the restatement only: the reference's argsort is not stable.  Four lidar pixels at distance 3: the two with the
    lower row-major index are chosen, however the frame was filled; in the mirrored frame the rule picks other POINTS (it is about
    indices)."""
    lidar, radar = tie_frame()
    assert S.n_tied(lidar, radar) == 1
    want = np.zeros_like(lidar)
    want[7, 10], want[10, 7] = lidar[7, 10], lidar[10, 7]
    assert np.array_equal(S.lidar_radar_sparse(lidar, radar), want)
    ys, xs = np.nonzero(lidar)
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        again = np.zeros_like(lidar)
        for k in order:
            again[ys[k], xs[k]] = lidar[ys[k], xs[k]]
        assert np.array_equal(S.lidar_radar_sparse(again, radar), want)
    flipped = S.lidar_radar_sparse(lidar[::-1, ::-1].copy(), radar[::-1, ::-1].copy())[::-1, ::-1]
    other = np.zeros_like(lidar)
    other[13, 10], other[10, 13] = lidar[13, 10], lidar[10, 13]
    assert np.array_equal(flipped, other)


# ------------------------------------------------------------------------------------------------ Philox
def test_philox_known_answers():
    hexes = lambda words: ["%08x" % int(w) for w in words]        # noqa: E731
    assert hexes(S.philox4x32_10((0, 0, 0, 0), (0, 0))) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert hexes(S.philox4x32_10((f, f, f, f), (f, f))) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert hexes(S.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # the counter layout: (pixel, frame low, frame high, 0) under (seed low, seed high), numpy's 53-bit recipe
    x = S.philox4x32_10((5, 0xFFFFFFFF, 2, 0), (0x89ABCDEF, 0x01234567))
    u = S.philox_uniform(0x0123456789ABCDEF, (2 << 32) | 0xFFFFFFFF, 6)[5]
    assert u == ((int(x[0]) >> 5) * 67108864 + (int(x[1]) >> 6)) / 9007199254740992 and 0.0 <= u < 1.0


@pytest.mark.parametrize("num_samples,density", [(100, 0.3), (1000, 0.5), (40, 0.05), (10 ** 6, 0.3)])
def test_philox_mask_keeps_a_plausible_number(num_samples, density):
    """k ~ Binomial(n_keep, p), p = min(1, num_samples / n_keep): |k - n_keep p| <= 6 sqrt(n_keep p (1 - p)), a bound that a correct
    generator misses with probability below 2e-9 per frame.  Seeds are fixed: the test is deterministic."""
    rng = np.random.RandomState(3)
    depth = (rng.uniform(1, 100, (3, 1, 45, 80)) * (rng.rand(3, 1, 45, 80) < density)).astype(np.float32)
    sparse = S.uniform_sparse_philox(depth, num_samples, np.inf, seed=20261019, offset=7)
    for b in range(3):
        n_keep, k = int((depth[b] > 0).sum()), int((sparse[b] != 0).sum())
        p = min(1.0, num_samples / n_keep)
        assert abs(k - n_keep * p) <= 6 * np.sqrt(n_keep * p * (1 - p)), (b, k, n_keep, p)
        assert np.array_equal(sparse[b][sparse[b] != 0], depth[b][sparse[b] != 0])


def test_philox_frames_and_seeds():
    n = 45 * 80
    a = S.philox_uniform(11, 0, n)
    assert np.array_equal(a, S.philox_uniform(11, 0, n))                                     # the same (seed, frame): the same numbers
    assert not np.array_equal(a, S.philox_uniform(11, 1, n)) and not np.array_equal(a, S.philox_uniform(12, 0, n))
    assert not np.array_equal(S.philox_uniform(11, 1 << 32, n), a)                           # the second counter word counts
    depth = np.full((2, 1, 45, 80), 5.0, np.float32)
    two = S.uniform_sparse_philox(depth, 900, np.inf, seed=11, offset=3)
    assert not np.array_equal(two[0], two[1])                                                # different frame numbers, different masks
    assert np.array_equal(S.uniform_sparse_philox(depth[:1], 900, np.inf, seed=11, offset=4)[0], two[1])
    assert abs(a.mean() - 0.5) < 6 / np.sqrt(12 * n) and a.min() >= 0.0 and a.max() < 1.0


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_new_symbols_are_exported(L):
    for name in ("rd_lidar_sparsify_workspace_bytes", "rd_lidar_radar_sparsify", "rd_uniform_sparsify"):
        assert hasattr(L, name), name
    assert L.rd_lidar_sparsify_workspace_bytes(16, 450, 800) >= 2 * 16 * 450 * 800 * 4
    assert L.rd_lidar_sparsify_workspace_bytes(0, 450, 800) < 0 and L.rd_lidar_sparsify_workspace_bytes(1, 1 << 15, 1 << 15) < 0


def test_abi_rejects_bad_arguments_without_gpu(L):
    """Every rejection happens before anything reaches the GPU (the pointers are host dummies that are never followed), each with a code
    of its own."""
    from radar_depth_amd import _lib as E
    buf = C.create_string_buffer(256)
    d = C.c_void_p((C.addressof(buf) + 15) & ~15)

    def lr(ls=33 * 47, rs=4 * 33 * 47, B=2, H=33, W=47, os_=4 * 33 * 47, null=None):
        a = [d, ls, d, rs, B, H, W, d, d, os_, None]
        if null is not None:
            a[null] = None
        return L.rd_lidar_radar_sparsify(*a)

    assert [lr(null=k) for k in (0, 2, 7, 8)] == [E.RD_ESPARSE_NULL] * 4 and b"null" in L.rd_last_error()
    assert [lr(B=0), lr(B=65537), lr(H=0), lr(W=0), lr(H=46341, W=1), lr(W=-3)] == [E.RD_ESPARSE_RANGE] * 6
    assert [lr(H=1 << 15, W=1 << 15), lr(H=40000, W=40000)] == [E.RD_ESPARSE_PIXELS] * 2 and b"2^30" in L.rd_last_error()
    assert [lr(ls=33 * 47 - 1), lr(rs=0), lr(os_=33 * 47 - 1), lr(ls=-1)] == [E.RD_ESPARSE_STRIDE] * 4

    def un(ds=33 * 47, B=2, H=33, W=47, ns=100, md=80.0, draws=None, os_=33 * 47, mask=None, null=None):
        a = [d, ds, B, H, W, ns, md, draws, 1, 0, d, d, os_, mask, None]
        if null is not None:
            a[null] = None
        return L.rd_uniform_sparsify(*a)

    assert [un(null=k) for k in (0, 10, 11)] == [E.RD_ESPARSE_NULL] * 3
    assert [un(B=0), un(H=0), un(W=46341, H=1)] == [E.RD_ESPARSE_RANGE] * 3
    assert un(H=1 << 15, W=1 << 15) == E.RD_ESPARSE_PIXELS
    assert [un(ds=33 * 47 - 1), un(os_=5)] == [E.RD_ESPARSE_STRIDE] * 2
    assert un(ns=-1) == E.RD_ESPARSE_SAMPLES and b"num_samples" in L.rd_last_error()
    assert un(md=float("nan")) == E.RD_ESPARSE_MAXDEPTH and b"NaN" in L.rd_last_error()

    # out against the planes that are read: 2 frames of 2x2 floats, 32 floats apart (planes of one [2,8,2,2] tensor)
    big = C.create_string_buffer(4096)
    at = lambda floats: C.c_void_p(((C.addressof(big) + 15) & ~15) + 4 * floats)        # noqa: E731

    def lr_at(lidar, radar, out, ls=32, rs=32, os_=32):
        return L.rd_lidar_radar_sparsify(at(lidar), ls, at(radar), rs, 2, 2, 2, d, at(out), os_, None)

    assert [lr_at(0, 4, 0), lr_at(0, 4, 3), lr_at(3, 8, 0), lr_at(32, 4, 0), lr_at(0, 4, 35), lr_at(0, 100, 0, ls=4, os_=4)] == [E.RD_ESPARSE_OVERLAP] * 6
    assert b"lidar plane" in L.rd_last_error()
    assert [lr_at(0, 4, 5), lr_at(0, 8, 6), lr_at(0, 36, 4), lr_at(0, 4, 4, ls=36, os_=36)] == [E.RD_ESPARSE_OVERLAP] * 4      # radar, but not that plane
    assert b"radar plane" in L.rd_last_error()
    assert L.rd_uniform_sparsify(at(0), 32, 2, 2, 2, 10, 80.0, None, 1, 0, d, at(2), 32, None, None) == E.RD_ESPARSE_OVERLAP
    assert b"depth plane" in L.rd_last_error()
    codes = {E.RD_ESPARSE_NULL, E.RD_ESPARSE_RANGE, E.RD_ESPARSE_PIXELS, E.RD_ESPARSE_STRIDE, E.RD_ESPARSE_SAMPLES, E.RD_ESPARSE_MAXDEPTH,
             E.RD_ESPARSE_OVERLAP}
    old = {-1, -2, E.RD_ERADAR_NULL, E.RD_ERADAR_RANGE, E.RD_ERADAR_NRADAR, E.RD_ERADAR_NLIDAR, E.RD_ERADAR_FEWLIDAR, E.RD_ERADAR_CROP}
    assert len(codes) == 7 and all(c < 0 for c in codes) and not codes & old
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "radar_depth_hip.h")).read()
    for name in ("NULL", "RANGE", "PIXELS", "STRIDE", "SAMPLES", "MAXDEPTH", "OVERLAP"):
        assert "#define RD_ESPARSE_%s (%d)" % (name, getattr(E, "RD_ESPARSE_" + name)) in hdr


# ------------------------------------------------------------------------------------------------ Python surface
def test_python_surface():
    from radar_depth_amd import dataset
    from radar_depth_amd.dataset import dense_to_sparse as D
    for name in ("UniformSampling", "LidarRadarSampling", "get_sparse_depth", "lidar_radar_sparse_depth", "uniform_sparse_depth"):
        assert getattr(dataset, name) is getattr(D, name), name
    u, lr = D.UniformSampling(100, 79.9, seed=5), D.LidarRadarSampling(100)
    assert (u.name, lr.name) == ("uar", "lidar_radar") and (type(u).__name__, type(lr).__name__) == ("UniformSampling", "LidarRadarSampling")
    assert repr(u) == "uar{ns=100,md=79.900000}" and repr(lr) == "lidar_radar{ns=100,md=inf}"
    assert (u.num_samples, u.max_depth, u.seed, u.offset, lr.num_samples, lr.max_depth) == (100, 79.9, 5, 0, 100, np.inf)
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()]        # noqa: E731
    empty = inspect.Parameter.empty
    assert sig(D.lidar_radar_sparse_depth) == [("lidar_depth", empty), ("radar_depth", empty), ("out", None)]
    assert sig(D.uniform_sparse_depth) == [("depth", empty), ("num_samples", empty), ("max_depth", float("inf")), ("draws", None), ("seed", None),
                                           ("offset", 0), ("out", None)]
    assert sig(D.UniformSampling.__init__)[1:] == [("num_samples", empty), ("max_depth", np.inf), ("seed", None)]
    assert sig(D.LidarRadarSampling.__init__)[1:] == [("num_samples", empty), ("max_depth", np.inf)]
    assert sig(D.UniformSampling.dense_to_sparse)[1:] == [("depth", empty), ("draws", None)]
    assert sig(D.LidarRadarSampling.dense_to_sparse)[1:] == [("lidar_depth", empty), ("radar_depth", empty)]
    assert [k for k, _ in sig(D.get_sparse_depth)] == ["sparsifier_func", "lidar_depth", "radar_depth", "out", "kw"]
    for kw in ({}, dict(draws=object(), seed=1)):
        with pytest.raises(ValueError, match="exactly one of draws"):
            D.uniform_sparse_depth(None, 10, **kw)
    with pytest.raises(ValueError, match="exactly one of draws"):
        D.UniformSampling(10).dense_to_sparse(None)                                          # no seed and no draws
    with pytest.raises(ValueError, match=r"^\[Error\] Invalid lidar sparsifier\.$"):
        D.get_sparse_depth(object(), None)
    with pytest.raises(NotImplementedError, match="scope.*lidar_radar_sparse_depth"):
        dataset.stage_val_batch(None, None, None, sparsifier="lidar_radar")

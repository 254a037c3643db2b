"""No-GPU checks of the KITTI devkit evaluation (csrc/kitti_eval.hip, radar_depth_amd/evaluation/kitti.py): the numpy restatement
tests/kitti_ref.py against the fixture that the devkit's own functions produced (tests/golden/make_golden_kitti_eval.py), the shortcut
variants that must miss it, the cases the fixture has to hold, the meter's text, the C ABI of the new entry points and their refusals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_ref as K  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "kitti_eval.npz")))


def cases(G, kind):
    return sorted(k[len(kind) + 1:-3] for k in G if k.startswith(kind + "_") and k.endswith("_in" if kind == "interp" else "_gt"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def error_bounds(gt, pred):
    """The relative bound per metric of the reference's float32 accumulation: 2 n 2^-24 for a sum of n non-negative float32 terms
    added one by one, halved under a square root, times k = (Sl2/n) / (Sl2/n - mean^2) for silog."""
    s = K.error_sums(gt, pred)
    n = s[9]
    base = 2.0 * n * EPS
    k = (s[5] / n) / (s[5] / n - (s[6] / n) ** 2)
    return np.array([base, base / 2, base, base / 2, base, base / 2, base / 2 * k, base, base]), n, k


def test_restatement_reproduces_the_filled_planes_and_images(G):
    from radar_depth_amd.evaluation.kitti import log_colormap
    assert np.array_equal(log_colormap(), G["table"])
    names = cases(G, "interp")
    assert len(names) >= 8
    for n in names:
        assert np.array_equal(bits(K.interpolate(G["interp_%s_in" % n])), bits(G["interp_%s_out" % n])), n
    names = cases(G, "img")
    assert len(names) >= 10
    for n in names:
        assert np.array_equal(K.error_image(G["img_%s_gt" % n], G["img_%s_pred" % n], G["table"]), G["img_%s_rgb" % n]), n


def test_restatement_reproduces_the_errors_within_the_accumulation_bound(G):
    names = cases(G, "err")
    assert len(names) >= 5
    worst = np.zeros(9)
    for n in names:
        gt, pred, ref = G["err_%s_gt" % n], G["err_%s_pred" % n], G["err_%s_errors" % n].astype(np.float64)
        bound, nv, k = error_bounds(gt, pred)
        assert nv <= 4000 and k <= 4 and bound.max() < 2e-3, (n, nv, k)
        got = K.errors(gt, pred)
        assert got[9] == nv == np.count_nonzero(gt >= 0)
        gap = np.abs(got[:9] - ref) / np.abs(ref)
        print(n, int(nv), "k=%.3f" % k, " ".join("%.2e" % g for g in gap))
        worst = np.maximum(worst, gap)
        assert np.all(gap <= bound), (n, gap, bound)
    print("worst gap per metric:", " ".join("%.2e" % g for g in worst))


def test_shortcut_variants_miss_the_fixture(G):
    def interp_hits(**kw):
        return [n for n in cases(G, "interp") if np.array_equal(bits(K.interpolate(G["interp_%s_in" % n], **kw)), bits(G["interp_%s_out" % n]))]

    def image_hits(**kw):
        return [n for n in cases(G, "img")
                if np.array_equal(K.error_image(G["img_%s_gt" % n], G["img_%s_pred" % n], G["table"], **kw), G["img_%s_rgb" % n])]
    everything = cases(G, "interp")
    assert interp_hits() == everything
    for n in ("holes", "sparse", "dense", "nan"):
        assert n not in interp_hits(row_fill="mean")
    assert "rows" not in interp_hits(fill_interior_rows=True) and "sparse" not in interp_hits(fill_interior_rows=True)
    assert "zero" not in interp_hits(positive_only=True)
    assert "overlap" not in image_hits(first_wins=True) and "random" not in image_hits(first_wins=True)
    assert "ladder" not in image_hits(bins_reversed=True) and "dmag0" not in image_hits(bins_reversed=True)


def test_fixture_holds_every_case(G):
    d, o = G["interp_holes_in"], G["interp_holes_out"]
    assert d[0, 0] < 0 and d[0, -1] < 0 and d[0, 3] >= 0                         # holes at the row start and end
    assert d[1, 63] >= 0 and d[1, 128] >= 0 and np.all(d[1, 64:128] < 0)         # lanes 64..127
    assert np.all(o[1, 64:128] == min(d[1, 63], d[1, 128]))
    assert d[2, 10] == d[2, 90] and np.count_nonzero(d[2] >= 0) == 2             # equal neighbours
    assert np.count_nonzero(d[3] >= 0) == 1 and np.all(o[3] == d[3, 77])         # a single valid pixel
    d, o = G["interp_rows_in"], G["interp_rows_out"]
    ok = (d >= 0).any(axis=1)
    assert list(ok) == [False, False, True, True, False, True, True, False, False]
    assert np.array_equal(o[4], d[4]) and np.array_equal(o[0], o[2]) and np.array_equal(o[8], o[6])
    d = G["interp_empty_in"]
    assert not (d >= 0).any() and np.array_equal(G["interp_empty_out"], d)       # an all-invalid frame
    d, o = G["interp_zero_in"], G["interp_zero_out"]
    assert np.count_nonzero(d == 0) >= 4 and np.all(o[0, 1:4] == 0) and np.signbit(d[1, 2])
    assert np.isnan(G["interp_nan_in"]).any() and np.isnan(G["interp_nan_out"][3]).all()
    assert np.isnan(G["err_nan_gt"]).any()
    # the n_err ladder: every bound, its float32 predecessor and successor, through both arms of the minimum
    table = G["table"]
    bounds = sorted(set(table[:, 0]) | set(table[:, 1]))
    gt, pred = G["img_ladder_gt"], G["img_ladder_pred"]
    at = gt >= 0
    ne = K.n_err(gt, pred)[at]
    with np.errstate(all="ignore"):
        d_err = np.abs(pred[at] - gt[at]).astype(np.float64)
        took_b = 20.0 * d_err / np.abs(gt[at]).astype(np.float64) < d_err / 3.0
    assert np.array_equal(ne, G["img_ladder_targets"]) and np.array_equal(took_b, G["img_ladder_arms"] == ord("b"))
    for arm in (False, True):
        have = set(ne[took_b == arm].tolist())
        for b in bounds:
            b = np.float32(b)
            want = [np.nextafter(b, np.float32(-np.inf)), b, np.nextafter(b, np.float32(np.inf))]
            if b == 0:
                want = [b] if not arm else []                # nothing below 0; arm b reaches neither 0 nor its successor
                if not arm:
                    want.append(np.nextafter(b, np.float32(1)))
            assert all(float(w) in have for w in want), (arm, b)
    gt, pred = G["img_dmag0_gt"], G["img_dmag0_pred"]
    assert np.count_nonzero((gt == 0) & (pred == 0)) == 1 and np.count_nonzero((gt == 0) & (pred > 0)) == 2        # d_mag = 0
    gt = G["img_border_only_gt"]
    assert (gt[0] >= 0).all() and (gt[-1] >= 0).all() and (gt[:, 0] >= 0).all() and (gt[:, -1] >= 0).all()
    assert not G["img_border_only_rgb"].any()                                    # a border pixel is never a centre
    gt = G["img_border_next_gt"]
    assert gt[1, 1] >= 0 and gt[1, -2] >= 0 and gt[-2, 1] >= 0 and gt[-2, -2] >= 0 and G["img_border_next_rgb"][0, 0].any()
    gt = G["img_overlap_gt"]                                                     # overlapping splats in the eight directions
    vs, us = np.nonzero(gt >= 0)
    seen = set()
    for i in range(len(vs)):
        for j in range(len(vs)):
            dv, du = vs[j] - vs[i], us[j] - us[i]
            if i != j and max(abs(dv), abs(du)) <= 2:
                seen.add((int(np.sign(dv)), int(np.sign(du)), int(max(abs(dv), abs(du)))))
    assert len(seen) == 16
    assert np.isnan(G["img_nan_gt"]).any() and np.isnan(G["img_nan_pred"]).any()
    assert not G["img_flat_rgb"].any() and G["img_three_rgb"].all(axis=2).all()


def test_encode_decode_round_trip_every_uint16():
    v = np.arange(65536, dtype=np.uint16)
    d = K.decode(v)
    assert d[0] == -1 and d.dtype == np.float32 and np.array_equal(d[1:], v[1:].astype(np.float64) / 256.0)
    assert np.array_equal(K.encode(d), v)
    odd = np.array([-1, np.nan, 0.0, 0.001, 1 / 256, 255.99, 255.99609375, 256.0, 1e6, np.inf, -0.0], dtype=np.float32)
    assert list(K.encode(odd)) == [0, 0, 1, 1, 1, 65533, 65535, 65535, 65535, 65535, 1]


def test_meter_text_and_quirks(G, tmp_path):
    import torch
    from radar_depth_amd.evaluation import kitti
    assert kitti.METRICS == K.METRICS
    for tag in ("stats", "statsbig", "statsnan"):
        rows = G[tag + "_rows"]
        mean, mn, mx = K.stats(rows)
        n = len(rows)
        # the reference adds float32 values one by one and divides in float32
        assert np.allclose(mean, G[tag + "_mean"], rtol=n * EPS, atol=0, equal_nan=True), tag
        assert np.array_equal(mn.astype(np.float32), G[tag + "_min"]) and np.array_equal(mx.astype(np.float32), G[tag + "_max"]), tag
        meter = kitti.KittiDepthMeter(device="cpu")          # (the state alone: update needs the GPU)
        state = np.stack([mean * n, mn, mx, np.full(9, float(n))], axis=1)
        meter.state.copy_(torch.from_numpy(state))
        path = str(tmp_path / (tag + ".txt"))
        meter.write_stats(path)
        text = open(path).read()
        assert text == K.format_stats(mean, mn, mx)
        lines = text.split("\n")
        assert len(lines) == 28 and lines[-1] == ""
        for i, name in enumerate(K.METRICS):
            for j, (kind, ref) in enumerate((("mean", G[tag + "_mean"]), ("min ", G[tag + "_min"]), ("max ", G[tag + "_max"]))):
                m = re.fullmatch(r"%s %s: (\S+) " % (kind, re.escape(name)), lines[3 * i + j])
                assert m, lines[3 * i + j]
                got, want = float(m.group(1)), float(ref[i])
                if np.isnan(want):
                    assert np.isnan(got)
                else:
                    # n 2^-24 relative for the reference's float32 sum, and half a unit of the sixth decimal that "%f" prints
                    assert abs(got - want) <= n * EPS * abs(want) + 0.5e-6, (tag, name, kind, got, want)
    assert np.all(G["statsbig_rows"] > 1) and np.all(G["statsbig_min"] == 1)     # the minimum of an all-large metric is 1
    assert np.all(K.stats(-np.abs(G["stats_rows"]))[2] == 0)                     # the maximum never goes below 0
    assert np.isnan(G["statsnan_mean"]).all() and np.isfinite(G["statsnan_min"]).all() and np.isfinite(G["statsnan_max"]).all()


NEW = ("rd_kitti_decode", "rd_kitti_encode", "rd_kitti_error_image", "rd_kitti_errors", "rd_kitti_interpolate", "rd_kitti_stats_update",
       "rd_kitti_workspace_bytes")


@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_header_table_and_binding_agree(L):
    hdr = open(os.path.join(REPO, "include", "radar_depth_hip.h")).read()
    table = dict(L.rd_abi_entry(i).decode().split(" ") for i in range(L.rd_abi_entries()))
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in table and hasattr(L, n), n
    assert sorted(n for n in table if n.startswith("rd_kitti_")) == sorted(NEW)
    assert {n: table[n] for n in NEW} == {
        "rd_kitti_decode": "i:plpliiip", "rd_kitti_encode": "i:plpliiip", "rd_kitti_interpolate": "i:plpliiipp",
        "rd_kitti_errors": "i:plpliiiippp", "rd_kitti_error_image": "i:plpliiiippllp", "rd_kitti_stats_update": "i:pipp",
        "rd_kitti_workspace_bytes": "l:iii"}
    from radar_depth_amd import _lib
    codes = dict(re.findall(r"#define (RD_EKITTI_\w+) \((-\d+)\)", hdr))
    assert len(codes) == 6 and sorted(int(v) for v in codes.values()) == list(range(-54, -48))
    for name, v in codes.items():
        assert getattr(_lib, name) == int(v)
    others = [int(v) for n, v in re.findall(r"#define (RD_E\w+) \((-\d+)\)", hdr) if not n.startswith("RD_EKITTI_")]
    assert min(others) == -48                                                    # the next free codes


def test_every_refusal_without_a_gpu(L):
    from radar_depth_amd import _lib as B
    p, q, odd = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p((1 << 22) + 4)
    table = (C.c_float * 50)()

    def refused(rc, code, word):
        assert rc == code, (rc, code, L.rd_last_error())
        assert word.encode() in L.rd_last_error(), L.rd_last_error()
    refused(L.rd_kitti_workspace_bytes(0, 4, 4), B.RD_EKITTI_RANGE, "kitti_workspace_bytes")
    refused(L.rd_kitti_workspace_bytes(1, 65536, 4), B.RD_EKITTI_RANGE, "kitti_workspace_bytes")
    assert L.rd_kitti_workspace_bytes(2, 450, 800) >= max(2 * 450 * 4, 2 * 256 * 80) and L.rd_kitti_workspace_bytes(1, 1, 1) == 256
    for fn in (L.rd_kitti_decode, L.rd_kitti_encode):
        refused(fn(None, 16, q, 16, 1, 4, 4, None), B.RD_EKITTI_NULL, "null")
        refused(fn(p, 16, None, 16, 1, 4, 4, None), B.RD_EKITTI_NULL, "null")
        refused(fn(p, 16, q, 16, 1, 4, 65536, None), B.RD_EKITTI_RANGE, "1..65535")
        refused(fn(p, 15, q, 16, 2, 4, 4, None), B.RD_EKITTI_STRIDE, "stride")
        refused(fn(p, 16, q, 15, 2, 4, 4, None), B.RD_EKITTI_STRIDE, "stride")
    f = L.rd_kitti_interpolate
    refused(f(p, 16, q, 16, 1, 4, 4, None, None), B.RD_EKITTI_NULL, "null")
    refused(f(None, 16, q, 16, 1, 4, 4, p, None), B.RD_EKITTI_NULL, "null")
    refused(f(p, 16, q, 16, 0, 4, 4, p, None), B.RD_EKITTI_RANGE, "1..65535")
    refused(f(p, 16, q, 16, 1, 0, 4, p, None), B.RD_EKITTI_RANGE, "1..65535")
    refused(f(p, 16, q, 15, 1, 4, 4, p, None), B.RD_EKITTI_STRIDE, "stride")
    refused(f(p, 16, q, 16, 1, 4, 4, odd, None), B.RD_EKITTI_ALIGN, "aligned")
    refused(f(p, 16, C.c_void_p((1 << 20) + 8), 16, 1, 4, 4, q, None), B.RD_EKITTI_OVERLAP, "overlaps")
    refused(f(p, 32, p, 16, 2, 4, 4, q, None), B.RD_EKITTI_OVERLAP, "overlaps")       # the same pointer with another stride
    f = L.rd_kitti_errors
    refused(f(p, 16, q, 16, 1, 4, 4, 0, p, None, None), B.RD_EKITTI_NULL, "null")
    refused(f(p, 16, None, 16, 1, 4, 4, 0, p, q, None), B.RD_EKITTI_NULL, "null")
    refused(f(p, 16, q, 16, 65536, 4, 4, 0, p, q, None), B.RD_EKITTI_RANGE, "1..65535")
    refused(f(p, 3, q, 16, 1, 4, 4, 0, p, q, None), B.RD_EKITTI_STRIDE, "stride")
    refused(f(p, 16, q, 16, 1, 4, 4, 0, odd, q, None), B.RD_EKITTI_ALIGN, "aligned")
    refused(f(p, 16, q, 16, 1, 4, 4, 0, p, odd, None), B.RD_EKITTI_ALIGN, "aligned")
    f = L.rd_kitti_error_image
    refused(f(p, 16, q, 16, 1, 4, 4, 0, None, p, 48, 12, None), B.RD_EKITTI_NULL, "null")
    refused(f(p, 16, q, 16, 1, 4, 4, 0, table, None, 48, 12, None), B.RD_EKITTI_NULL, "null")
    refused(f(p, 16, q, 16, 1, 4, -1, 0, table, p, 48, 12, None), B.RD_EKITTI_RANGE, "1..65535")
    refused(f(p, 16, q, 15, 1, 4, 4, 0, table, p, 48, 12, None), B.RD_EKITTI_STRIDE, "stride")
    refused(f(p, 16, q, 16, 1, 4, 4, 0, table, p, 48, 11, None), B.RD_EKITTI_PITCH, "pitch")
    refused(f(p, 16, q, 16, 2, 4, 4, 0, table, p, 47, 12, None), B.RD_EKITTI_PITCH, "pitch")
    f = L.rd_kitti_stats_update
    refused(f(None, 1, p, None), B.RD_EKITTI_NULL, "null")
    refused(f(p, 1, None, None), B.RD_EKITTI_NULL, "null")
    refused(f(p, 0, q, None), B.RD_EKITTI_RANGE, "1..65535")
    refused(f(odd, 1, q, None), B.RD_EKITTI_ALIGN, "aligned")
    refused(f(p, 1, odd, None), B.RD_EKITTI_ALIGN, "aligned")

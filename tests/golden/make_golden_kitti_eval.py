"""Golden vectors for the KITTI devkit evaluation (csrc/kitti_eval.hip; radar_depth_amd.evaluation.kitti), produced by the
devkit's OWN functions from the reference checkout.

The devkit (misc/devkit/cpp: evaluate_depth.cpp, io_depth.h, log_colormap.h, utils.h) needs png++ (and its shipped binary
libpng12), and nothing here reads or writes a PNG.  So this script writes two files of its own into a temporary directory and compiles them with the
host g++ against the devkit's headers IN THE REFERENCE TREE (nothing of the reference's text is copied):
  * png++/png.hpp, a stand-in with a pixel container (get_pixel / set_pixel), a zero default rgb_pixel and zero-initialised images.
    That an image and a default rgb_pixel start at zero is png++'s documented behaviour and the ONE assumption made here: errorImage
    relies on it for its black background and for the colour of an n_err that no bin holds;
  * driver.cpp, which includes evaluate_depth.cpp with its main renamed and calls interpolateBackground, depthError, errorImage(.., true)
    and statMean / statMin / statMax on raw float32 files.  After the standard headers it pins fabs to the C double version: modern
    libstdc++ resolves fabs(float) to a float overload, and io_depth.h's std::min(fabs(float), 5.0) then does not compile.
Compiled with -O0 only (DepthImage::setInvalid lacks a return statement) and -fpermissive.

Inputs are seeded numpy arrays; outputs go to tests/golden/kitti_eval.npz: the planes after interpolateBackground, the nine errors,
the error images, and the three statistics over the error rows.  What the tests rely on is asserted here: the restatement
(tests/kitti_ref.py) reproduces every filled plane and error image bit for bit, every error case has n_valid <= 4000 and
k = (Sl2/n) / (Sl2/n - mean^2) <= 4, and the n_err ladder holds every bin bound with its float32 neighbours on both arms of the minimum.

    python tests/golden/make_golden_kitti_eval.py --reference PATH [--bench]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import kitti_ref as K  # noqa: E402

PNG_HPP = r"""
// stand-in for png++: a pixel container.  Images and a default rgb_pixel start at zero, as png++ documents.
#pragma once
#include <stddef.h>
#include <istream>
#include <string>
#include <vector>
namespace png {
typedef unsigned char byte;
struct rgb_pixel {
    byte red, green, blue;
    rgb_pixel(byte r = 0, byte g = 0, byte b = 0) : red(r), green(g), blue(b) {}
};
typedef unsigned short gray_pixel_16;
enum color_type { color_type_gray = 0, color_type_rgb = 2 };
template <class P> class image {
  public:
    image() : w_(0), h_(0) {}
    image(size_t w, size_t h) : w_(w), h_(h), d_(w * h, P()) {}
    explicit image(const std::string&) : w_(0), h_(0) { throw 1; }
    size_t get_width() const { return w_; }
    size_t get_height() const { return h_; }
    P get_pixel(size_t x, size_t y) const { return d_.at(y * w_ + x); }
    void set_pixel(size_t x, size_t y, P p) { d_.at(y * w_ + x) = p; }
    void write(const std::string&) {}
  private:
    size_t w_, h_;
    std::vector<P> d_;
};
template <class S> class reader {
  public:
    explicit reader(S&) {}
    void read_info() {}
    color_type get_color_type() const { return color_type_gray; }
    size_t get_bit_depth() const { return 16; }
    size_t get_width() const { return 0; }
    size_t get_height() const { return 0; }
};
}
"""

DRIVER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "dirent.h"
// fabs pinned to the C double version (see the generator's docstring)
static inline double fabs_c_double(double x) { return __builtin_fabs(x); }
#define fabs(x) fabs_c_double(x)
#define main devkit_main
#include "evaluate_depth.cpp"
#undef main

static std::vector<float> load(const char* path, size_t n) {
    std::vector<float> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(float), n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return v;
}
static void store(const char* path, const void* p, size_t bytes) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}
static double now() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }

int main(int argc, char** argv) {
    const std::string mode = argv[1];
    if (mode == "stats") {
        const int n = atoi(argv[2]);
        std::vector<float> flat = load(argv[3], (size_t)n * 9);
        std::vector<std::vector<float> > rows;
        for (int i = 0; i < n; ++i) rows.push_back(std::vector<float>(flat.begin() + 9 * i, flat.begin() + 9 * i + 9));
        for (int j = 0; j < 9; ++j) printf("%.9g %.9g %.9g\n", statMean(rows, j), statMin(rows, j), statMax(rows, j));
        return 0;
    }
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    const size_t n = (size_t)w * h;
    if (mode == "interp") {
        std::vector<float> in = load(argv[4], n);
        DepthImage D(in.data(), w, h);
        D.interpolateBackground();
        store(argv[5], D.data(), n * sizeof(float));
    } else if (mode == "errors") {
        std::vector<float> g = load(argv[4], n), p = load(argv[5], n);
        DepthImage G(g.data(), w, h), P(p.data(), w, h);
        std::vector<float> e = depthError(G, P);
        for (size_t j = 0; j < e.size(); ++j) printf("%.9g\n", e[j]);
    } else if (mode == "image") {
        std::vector<float> g = load(argv[4], n), p = load(argv[5], n);
        DepthImage G(g.data(), w, h), P(p.data(), w, h);
        png::image<png::rgb_pixel> I = P.errorImage(G, true);
        std::vector<unsigned char> rgb(3 * n);
        for (int v = 0; v < h; ++v)
            for (int u = 0; u < w; ++u) {
                const png::rgb_pixel q = I.get_pixel(u, v);
                rgb[3 * ((size_t)v * w + u)] = q.red, rgb[3 * ((size_t)v * w + u) + 1] = q.green, rgb[3 * ((size_t)v * w + u) + 2] = q.blue;
            }
        store(argv[6], rgb.data(), rgb.size());
    } else if (mode == "bench") {                    // one frame of eval(): fill, errors, error image, on one core
        std::vector<float> g = load(argv[4], n), p = load(argv[5], n);
        const int reps = atoi(argv[6]);
        DepthImage G(g.data(), w, h);
        double best = 1e30;
        for (int r = 0; r < reps; ++r) {
            DepthImage P(p.data(), w, h);
            const double t0 = now();
            P.interpolateBackground();
            std::vector<float> e = depthError(G, P);
            png::image<png::rgb_pixel> I = P.errorImage(G, true);
            const double t = now() - t0;
            if (t < best) best = t;
            if (e.size() != 9 || I.get_width() != (size_t)w) return 3;
        }
        printf("%.9g\n", best);
    } else {
        return 2;
    }
    return 0;
}
"""


def build_driver(reference, tmp):
    devkit = os.path.join(reference, "misc", "devkit", "cpp")
    assert os.path.exists(os.path.join(devkit, "evaluate_depth.cpp")), "no devkit under " + reference
    os.makedirs(os.path.join(tmp, "png++"))
    with open(os.path.join(tmp, "png++", "png.hpp"), "w") as fh:
        fh.write(PNG_HPP)
    with open(os.path.join(tmp, "driver.cpp"), "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "driver")
    subprocess.run(["g++", "-O0", "-fpermissive", "-w", "-I", tmp, "-I", devkit, os.path.join(tmp, "driver.cpp"), "-o", exe], check=True)
    return exe


class Devkit(object):
    def __init__(self, exe, tmp):
        self.exe, self.tmp = exe, tmp

    def _file(self, name, a):
        p = os.path.join(self.tmp, name)
        np.ascontiguousarray(a, dtype=np.float32).tofile(p)
        return p

    def _run(self, *args):
        return subprocess.run([self.exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout

    def interp(self, d):
        h, w = d.shape
        out = os.path.join(self.tmp, "out.f32")
        self._run("interp", w, h, self._file("in.f32", d), out)
        return np.fromfile(out, dtype=np.float32).reshape(h, w)

    def errors(self, gt, pred):
        h, w = gt.shape
        return np.array([float(x) for x in self._run("errors", w, h, self._file("gt.f32", gt), self._file("pred.f32", pred)).split()],
                        dtype=np.float32)

    def image(self, gt, pred):
        h, w = gt.shape
        out = os.path.join(self.tmp, "out.rgb")
        self._run("image", w, h, self._file("gt.f32", gt), self._file("pred.f32", pred), out)
        return np.fromfile(out, dtype=np.uint8).reshape(h, w, 3)

    def stats(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        t = np.array([[float(x) for x in ln.split()] for ln in self._run("stats", len(rows), self._file("rows.f32", rows)).splitlines()],
                     dtype=np.float32)
        return t[:, 0], t[:, 1], t[:, 2]

    def bench(self, gt, pred, reps):
        h, w = gt.shape
        return float(self._run("bench", w, h, self._file("gt.f32", gt), self._file("pred.f32", pred), reps))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- interpolation cases
def interp_cases(rng):
    cases = {}
    d = np.full((6, 130), -1, dtype=np.float32)
    d[0, 3:120] = rng.uniform(1, 80, 117)                    # a hole at the row start and one at the row end
    d[0, 40:50] = -1
    d[1, :] = rng.uniform(1, 80, 130)                        # a hole over lanes 64..127, valid at 63 and 128
    d[1, 64:128] = -1
    d[2, 10], d[2, 90] = 7.5, 7.5                            # equal neighbours
    d[3, 77] = 12.25                                         # a single valid pixel
    d[4, 0], d[4, 129] = 30.0, 2.0                           # valid only at both ends
    d[5, :] = rng.uniform(1, 80, 130)                        # a full row
    cases["holes"] = d
    d = np.full((9, 70), -1, dtype=np.float32)               # empty rows at the top, in the interior and at the bottom
    for y in (2, 3, 5, 6):
        keep = rng.uniform(size=70) < 0.3
        keep[rng.integers(0, 70)] = True
        d[y, keep] = rng.uniform(1, 80, int(keep.sum()))
    d[4, :] = np.linspace(-9, -2, 70)                        # (the interior row keeps its own invalid values)
    cases["rows"] = d
    cases["empty"] = np.full((4, 10), -1, dtype=np.float32)  # an all-invalid frame
    d = np.full((3, 12), -1, dtype=np.float32)               # 0.0 (and -0.0) as a valid depth
    d[0, [0, 4, 9]] = (5.0, 0.0, 3.0)
    d[1, [2, 6]] = (-0.0, 0.0)
    d[2, [1, 11]] = (0.0, 8.0)
    cases["zero"] = d
    d = rng.uniform(1, 80, (7, 66)).astype(np.float32)       # NaN is a hole
    d[rng.uniform(size=d.shape) < 0.4] = np.nan
    d[3, :] = np.nan
    d[0, :] = np.nan
    cases["nan"] = d
    d = np.full((48, 130), -1, dtype=np.float32)             # sparse: a few percent valid, some rows empty
    keep = rng.uniform(size=d.shape) < 0.04
    keep[:3] = False
    keep[20] = False
    keep[45:] = False
    d[keep] = rng.uniform(0.5, 90, int(keep.sum()))
    cases["sparse"] = d
    d = rng.uniform(0.5, 90, (17, 65)).astype(np.float32)    # dense with small holes
    d[rng.uniform(size=d.shape) < 0.2] = -1
    cases["dense"] = d
    cases["one"] = np.array([[-1, 4.0, -1]], dtype=np.float32).T.copy()      # W = 1: [3,1]
    return cases


# ---------------------------------------------------------------- error cases
def error_cases(rng):
    cases = {}

    def pair(h, w, frac, bias, sigma, lo=1.0, hi=80.0):
        gt = np.full((h, w), -1, dtype=np.float32)
        keep = rng.uniform(size=(h, w)) < frac
        gt[keep] = rng.uniform(lo, hi, int(keep.sum()))
        pred = (np.where(keep, gt, rng.uniform(lo, hi, (h, w))) * bias * np.exp(rng.normal(0, sigma, (h, w)))).astype(np.float32)
        return gt, pred
    cases["sparse"] = pair(48, 130, 0.2, 1.0, 0.15)
    cases["dense"] = pair(30, 130, 1.0, 1.1, 0.2)
    cases["biased"] = pair(40, 97, 0.5, 0.8, 0.3, 0.5, 20.0)
    cases["tiny"] = pair(3, 5, 1.0, 1.0, 0.05)
    gt, pred = pair(20, 33, 0.6, 1.05, 0.1)
    gt[rng.uniform(size=gt.shape) < 0.1] = np.nan            # NaN in the ground truth is invalid
    cases["nan"] = (gt, pred)
    return cases


# ---------------------------------------------------------------- error-image cases
def find_pair(t, arm):
    """(gt, pred) float32 whose n_err is exactly the float32 t, through arm "a" (d_err / 3) or "b" (20 d_err / d_mag) of the minimum;
    None if the search finds none."""
    t = np.float32(t)
    if arm == "a":
        # tiny ground truths: pred - gt is exact (the subnormal ones reach the float32 successor of 0)
        gts = np.concatenate([np.arange(1, 4097, dtype=np.float64) * 2.0 ** -20, np.arange(1, 65, dtype=np.float64) * 2.0 ** -149]).astype(np.float32)
        ideal = gts.astype(np.float64) + 3.0 * float(t)
    else:
        # the whole binade [64, 128): 20 d_err / d_mag reaches the predecessor of a power of two only in its upper part
        gts = (64.0 + np.arange(0, 1 << 23, 37, dtype=np.float64) * 2.0 ** -17).astype(np.float32)
        ideal = gts.astype(np.float64) * (1.0 + float(t) / 20.0)
    p0 = ideal.astype(np.float32)
    for step in (0, 1, -1, 2, -2, 3, -3):
        p = p0.copy()
        for _ in range(abs(step)):
            p = np.nextafter(p, np.float32(np.inf if step > 0 else -np.inf))
        with np.errstate(all="ignore"):
            d_err = np.abs(p - gts).astype(np.float64)
            a, b = d_err / 3.0, 20.0 * d_err / np.abs(gts).astype(np.float64)
            took_b = b < a
            ne = np.where(took_b, b, a).astype(np.float32)
        hit = np.nonzero((ne == t) & (took_b == (arm == "b")) & np.isfinite(p))[0]
        if hit.size:
            return float(gts[hit[0]]), float(p[hit[0]])
    return None


def image_cases(rng, table):
    cases, notes = {}, {}
    bounds = sorted(set([float(r[0]) for r in table] + [float(r[1]) for r in table]))
    ladder, missing = [], []
    for arm in "ab":
        for bnd in bounds:
            b32 = np.float32(bnd)
            for t in (np.nextafter(b32, np.float32(-np.inf)), b32, np.nextafter(b32, np.float32(np.inf))):
                if t < 0:
                    continue                                 # n_err is never negative
                if arm == "b" and t < 1e-30:
                    continue                                 # d_err = 0 gives a = b = 0 and std::min takes a; b needs d_mag > 60, and no
                                                             # float32 difference at that magnitude is small enough for 0's successor
                r = find_pair(t, arm)
                (ladder.append((arm, float(t)) + r) if r else missing.append((arm, float(t))))
    assert not missing, missing
    per_row = 43
    rows = (len(ladder) + per_row - 1) // per_row
    gt = np.full((3 * rows + 1, 130), -1, dtype=np.float32)
    pred = np.zeros_like(gt)
    for i, (_, _, g, p) in enumerate(ladder):
        v, u = 1 + 3 * (i // per_row), 1 + 3 * (i % per_row)
        gt[v, u], pred[v, u] = g, p
    cases["ladder"] = (gt, pred)
    notes["ladder"] = [[arm, t] for arm, t, _, _ in ladder]
    # d_mag = 0: 0/0 in arm b (n_err = a = 0) and x/0 = inf (n_err = a)
    gt = np.full((5, 11), -1, dtype=np.float32)
    pred = np.zeros_like(gt)
    gt[2, 2], pred[2, 2] = 0.0, 0.0
    gt[2, 5], pred[2, 5] = 0.0, 4.5
    gt[2, 8], pred[2, 8] = -0.0, 0.25
    cases["dmag0"] = (gt, pred)
    # every border pixel valid (never a centre), and centres next to each border
    gt = np.full((7, 9), -1, dtype=np.float32)
    gt[0, :] = gt[-1, :] = 10
    gt[:, 0] = gt[:, -1] = 10
    pred = gt * 1.5
    cases["border_only"] = (gt.copy(), pred.copy())
    gt[1, 1], gt[1, 7], gt[5, 1], gt[5, 7], gt[1, 4], gt[3, 1] = 10, 12, 14, 16, 18, 20
    pred = np.where(gt > 0, gt * np.float32(1.01), 0).astype(np.float32)
    pred[1, 7], pred[5, 1], pred[5, 7] = 12 * 1.2, 14 * 2, 16 * 30
    cases["border_next"] = (gt, pred)
    # two centres whose splats overlap, in each of the eight directions, at distance 1 and 2; the two have different colours
    dirs = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    gt = np.full((2 * 8, 8 * 8), -1, dtype=np.float32)
    pred = np.zeros_like(gt)
    for k, dist in enumerate((1, 2)):
        for j, (dv, du) in enumerate(dirs):
            v, u = 8 * k + 3, 8 * j + 3
            gt[v, u], pred[v, u] = 10, 10.05                          # first bin
            gt[v + dist * dv, u + dist * du], pred[v + dist * dv, u + dist * du] = 10, 16          # 2 <= n_err < 4 through arm a
    cases["overlap"] = (gt, pred)
    # NaN: an invalid ground truth, and a NaN prediction whose black splat covers a neighbour's colour
    gt = np.full((6, 12), -1, dtype=np.float32)
    pred = np.zeros_like(gt)
    gt[2, 2], pred[2, 2] = np.nan, 5
    gt[2, 6], pred[2, 6] = 10, 11
    gt[2, 7], pred[2, 7] = 10, np.nan
    gt[3, 9], pred[3, 9] = 10, np.inf
    cases["nan"] = (gt, pred)
    gt = rng.uniform(0.5, 90, (20, 37)).astype(np.float32)
    gt[rng.uniform(size=gt.shape) < 0.7] = -1
    pred = (np.abs(gt) * np.exp(rng.normal(0, 0.5, gt.shape))).astype(np.float32)
    cases["random"] = (gt, pred)
    gt = rng.uniform(0.5, 90, (9, 33)).astype(np.float32)
    cases["dense"] = (gt, (gt * np.exp(rng.normal(0, 0.05, gt.shape))).astype(np.float32))
    g = np.full((2, 5), 10, dtype=np.float32)
    cases["flat"] = (g, g * 2)                                       # H < 3: black
    g = np.full((3, 3), 10, dtype=np.float32)
    cases["three"] = (g, g * np.float32(1.3))                        # the one centre of a 3x3 frame
    return cases, notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--bench", action="store_true", help="time the devkit's per-frame work at 450x800 on one core and exit")
    args = ap.parse_args()
    with open(os.path.join(REPO, "radar_depth_amd", "kitti_log_colormap.json")) as fh:
        table = np.array(json.load(fh)["rows"], dtype=np.float32)
    rng = np.random.default_rng(20241)
    with tempfile.TemporaryDirectory() as tmp:
        dk = Devkit(build_driver(args.reference, tmp), tmp)
        if args.bench:
            for frac in (0.008, 1.0):
                gt = np.where(rng.uniform(size=(450, 800)) < frac, rng.uniform(1, 80, (450, 800)), -1).astype(np.float32)
                pred = rng.uniform(1, 80, (450, 800)).astype(np.float32)
                pred[rng.uniform(size=pred.shape) < 0.3] = -1
                print("devkit (-O0 build), one core, 450x800, %.1f %% valid ground truth: %.2f ms per frame"
                      % (100 * frac, 1e3 * dk.bench(gt, pred, 5)))
            return
        out = {"table": table}
        t0 = time.time()
        for name, d in interp_cases(rng).items():
            ref = dk.interp(d)
            assert np.array_equal(bits(K.interpolate(d)), bits(ref)), "restatement misses interpolateBackground on " + name
            out["interp_%s_in" % name], out["interp_%s_out" % name] = d, ref
        rows = []
        for name, (gt, pred) in error_cases(rng).items():
            ref = dk.errors(gt, pred)
            s = K.error_sums(gt, pred)
            n, k = s[9], (s[5] / s[9]) / (s[5] / s[9] - (s[6] / s[9]) ** 2)
            assert 0 < n <= 4000 and 0 < k <= 4, (name, n, k)
            assert np.all(np.isfinite(ref))
            out["err_%s_gt" % name], out["err_%s_pred" % name], out["err_%s_errors" % name] = gt, pred, ref
            rows.append(ref)
        cases, notes = image_cases(rng, table)
        for name, (gt, pred) in cases.items():
            ref = dk.image(gt, pred)
            assert np.array_equal(K.error_image(gt, pred, table), ref), "restatement misses errorImage on " + name
            out["img_%s_gt" % name], out["img_%s_pred" % name], out["img_%s_rgb" % name] = gt, pred, ref
        out["img_ladder_targets"] = np.array([t for _, t in notes["ladder"]], dtype=np.float32)
        out["img_ladder_arms"] = np.array([ord(a) for a, _ in notes["ladder"]], dtype=np.uint8)
        # statistics: the error rows above, then rows that show the quirks (every value above 1: the minimum stays 1)
        rows = np.array(rows, dtype=np.float32)
        for tag, r in (("stats", rows), ("statsbig", np.vstack([rows[:3] + 5, rows[:2] * 7 + 2]).astype(np.float32)),
                       ("statsnan", np.vstack([rows[:2], np.full((1, 9), np.nan), rows[2:4]]).astype(np.float32))):
            mean, mn, mx = dk.stats(r)
            out[tag + "_rows"], out[tag + "_mean"], out[tag + "_min"], out[tag + "_max"] = r, mean, mn, mx
        path = os.path.join(HERE, "kitti_eval.npz")
        np.savez_compressed(path, **out)
        print("%s: %d arrays, %d bytes, %.1f s" % (path, len(out), os.path.getsize(path), time.time() - t0))


if __name__ == "__main__":
    main()

"""numpy restatement of the reference's comparison rows (utils.py:114-153: colored_depthmap, merge_into_row, merge_into_row_with_gt) as
its save_image's ``astype('uint8')`` leaves them, with matplotlib's colormap call replaced by a 259 x 3 uint8 table.  What
csrc/visualize.hip computes, written so that every rounding is visible:

    d_min, d_max   float32 minimum / maximum over all depth planes of ONE frame
    rel            (d - d_min) / (d_max - d_min), float32 throughout, IEEE division
    xa             rel * 256 (float32, exact);  == 256 -> 255;  < 0 -> 256 (under);  >= 256 -> 257 (over);  NaN -> 258 (bad);  else trunc
    depth panel    table[index]
    rgb panel      trunc(float32(255) * x)

``mode`` selects the arithmetic of ``rel``: "exact" is the reference's; "reciprocal" (multiply by float32(1 / range)) and "float64"
(evaluate in float64) are the two shortcuts a port is tempted by -- the fixture's ladder frame tells all three apart.
tests/golden/make_golden_visualize.py asserts this file against the reference's own functions."""
import json
import os

import numpy as np

UNDER, OVER, BAD = 256, 257, 258
TABLE_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radar_depth_amd", "viridis_lut.json")


def package_table():
    """The table the package ships: uint8 [259,3]."""
    with open(TABLE_PATH) as fh:
        return np.array(json.load(fh)["rgb"], dtype=np.uint8)


def lut_index(depth, lo, denom, mode="exact"):
    """int64 table rows of a float32 array.  lo, denom: float32 scalars (d_min and the divisor d_max - d_min)."""
    depth, lo, denom = np.asarray(depth, np.float32), np.float32(lo), np.float32(denom)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if mode == "exact":
            xa = (depth - lo) / denom * np.float32(256)
        elif mode == "reciprocal":
            xa = (depth - lo) * (np.float32(1) / denom) * np.float32(256)
        elif mode == "float64":
            xa = ((depth.astype(np.float64) - np.float64(lo)) / np.float64(denom) * 256.0)
        else:
            raise ValueError(mode)
        bad, under, over, top = np.isnan(xa), xa < 0, xa >= 256, xa == 256
        idx = np.where(bad | under | over, 0, xa).astype(np.int64)
    idx[over] = OVER
    idx[top] = 255
    idx[under] = UNDER
    idx[bad] = BAD
    return idx


def frame_range(planes):
    """(d_min, d_max) of one frame as float32 scalars: over all of its planes together."""
    planes = [np.asarray(p, np.float32) for p in planes]
    return np.float32(min(p.min() for p in planes)), np.float32(max(p.max() for p in planes))


def given_range(d_min, d_max):
    """(lo, denom) as numpy forms them from Python floats: ``depth - d_min`` rounds d_min to float32, ``d_max - d_min`` is a float64
    difference that is rounded to float32 when the float32 array is divided by it."""
    return np.float32(float(d_min)), np.float32(float(d_max) - float(d_min))


def colored_depthmap(depth, table, d_min=None, d_max=None, mode="exact"):
    """uint8 [H,W,3] of a float32 [H,W] plane; the range is the plane's own unless both ends are given."""
    depth = np.asarray(depth, np.float32)
    if d_min is None and d_max is None:
        lo, hi = frame_range([depth])
        denom = np.float32(hi - lo)
    else:
        lo, denom = given_range(d_min, d_max)
    return table[lut_index(depth, lo, denom, mode)]


def merge_row(rgb, planes, table, mode="exact"):
    """One frame: rgb float32 [3,H,W] (or None), planes a list of float32 [H,W] -> uint8 [H, k*W, 3]."""
    lo, hi = frame_range(planes)
    denom = np.float32(hi - lo)
    panels = [] if rgb is None else [(np.float32(255) * np.transpose(np.asarray(rgb, np.float32), (1, 2, 0))).astype(np.uint8)]
    panels += [table[lut_index(p, lo, denom, mode)] for p in planes]
    return np.hstack(panels)


def merge_rows(rgb, planes, table, mode="exact"):
    """A batch: rgb [B,3,H,W], planes a list of [B,1,H,W] -> uint8 [B,H,k*W,3]; every frame with its own range."""
    B = planes[0].shape[0]
    return np.stack([merge_row(None if rgb is None else rgb[b], [p[b, 0] for p in planes], table, mode) for b in range(B)])

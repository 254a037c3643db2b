"""No-GPU checks of the distance-interval metrics (Result_multidist / AverageMeter_multidist, csrc/metrics_multidist.hip).

1. tests/multidist_ref.py -- the numpy restatement the GPU test holds the kernels to -- against the reference's own CPU results
   (tests/golden/multidist.npz, written by tests/golden/make_golden_multidist.py).  The project's bar for "against the reference's CPU
   results" is 1e-5 relative (tests/test_gpu_meter.py).  The reference sums in float32 and its lg10 term cancels, so the restatement
   (the same float32 terms, float64 sums) has to meet every value of the well-populated cases within 3e-6, a threefold headroom;
   measured worst: 1.3e-7 on `rand` (>= 962 pixels per interval), 1.4e-7 on the other cases with dozens of pixels per interval.  The
   boundary ladder, the tails and the frame with a handful of pixels per interval are held on counts, valid_label and NaN placement,
   which are exact (their few-pixel metrics sit at up to 3.4e-6, a 1-ulp logf over one pixel's lg10).
2. The ladder tells the reference's interval rule from half-open intervals and from 100 as the last upper bound.
3. The host classes: pickling under the reference's module path, the repaired update / AverageMeter_multidist against the values the
   fixture script formed from the reference's Result / AverageMeter.
4. Every RD_EMDIST_* code, through the library, with null or host pointers: each call returns in front of its launch."""
import ctypes as C
import os
import pickle
import sys
import types

import numpy as np
import pytest

import multidist_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
POPULATED = ("rand", "sparse", "single")
EXACT_ONLY = ("ladder", "empty", "tail5", "tail1")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "multidist.npz"))


def test_restatement_meets_the_reference_with_headroom(gold):
    worst = 0.0
    for name in POPULATED:
        m, valid = R.evaluate(gold[name + "_out"], gold[name + "_target"])
        assert np.array_equal(valid, gold[name + "_valid"]), name
        worst = max(worst, R.rel(m, gold[name + "_metrics"]))
    for k in (0, 1):
        m, valid = R.evaluate(gold["batch_out"][k], gold["batch_target"][k])
        assert np.array_equal(valid, gold["batch_valid"][k])
        worst = max(worst, R.rel(m, gold["batch_metrics"][k]))
    print("restatement vs the reference's CPU results: worst relative error %.3e" % worst)
    assert gold["rand_counts"].min() >= 500
    assert worst <= 3e-6


def test_counts_valid_labels_and_nan_placement_are_exact(gold):
    cases = [(n, gold[n + "_out"], gold[n + "_target"], gold[n + "_metrics"], gold[n + "_valid"], gold[n + "_counts"])
             for n in POPULATED + EXACT_ONLY]
    cases += [("batch%d" % k, gold["batch_out"][k], gold["batch_target"][k], gold["batch_metrics"][k], gold["batch_valid"][k],
               gold["batch_counts"][k]) for k in range(3)]
    for name, out, tgt, metrics, valid, counts in cases:
        s = R.sums(out, tgt)
        assert np.array_equal(s[:, 0], counts.astype(np.float64)), name
        m, v = R.metrics_from_sums(s)
        assert np.array_equal(v, valid), name
        assert np.array_equal(np.isnan(m), np.isnan(metrics)), name
        assert np.array_equal(np.isnan(m).all(axis=1), valid == 0), name
    assert gold["ladder_counts"].tolist() == [3, 4, 4, 4, 4, 4, 4, 4, 4, 7]       # every inner edge in two intervals, 100 in the last only
    assert (gold["sparse_valid"] == 0).sum() >= 4 and gold["single_valid"].sum() == 1 and gold["empty_valid"].sum() == 0
    assert len({tuple(v.tolist()) for v in gold["batch_valid"]}) == 3


def test_the_ladder_discriminates(gold):
    out, tgt, counts = gold["ladder_out"], gold["ladder_target"], gold["ladder_counts"]
    assert np.array_equal(R.sums(out, tgt)[:, 0], counts)
    half_open = R.sums(out, tgt, closed=False)[:, 0]
    bounded = R.sums(out, tgt, last_inf=False)[:, 0]
    assert not np.array_equal(half_open, counts) and half_open.sum() == counts.sum() - 9      # the nine inner edges counted once
    assert not np.array_equal(bounded, counts) and bounded[-1] == counts[-1] - 3             # succ(100), 105.25 and 1000 fall out
    # ... and on the metrics: the reference's own values reject both misreadings
    for rule in (dict(closed=False), dict(last_inf=False)):
        m, _ = R.evaluate(out, tgt, **rule)
        with pytest.raises(AssertionError):
            assert R.rel(m, gold["ladder_metrics"]) <= 1e-5


def _result_from(metrics, valid):
    from radar_depth_amd.evaluation.metrics import Result_multidist
    r = Result_multidist()
    for k, res in enumerate(r.result_lst):
        res.update(*[float(v) for v in metrics[k]], 0, 0)
        r.valid_label[k] = int(valid[k])
    return r


def _rows(r):
    return np.array([[getattr(res, n) for n in R.NAMES] for res in r.result_lst], dtype=np.float64)


def test_host_classes_against_the_fixture(gold):
    from radar_depth_amd.evaluation.metrics import AverageMeter_multidist, Result, Result_multidist
    r = Result_multidist()
    assert r.dist_interval == list(R.DIST_INTERVAL) and len(r.result_lst) == 10 and r.valid_label == [1] * 10
    assert all(isinstance(res, Result) for res in r.result_lst)
    r.set_to_worst()
    assert all(res.rmse == np.inf and res.delta1 == 0 for res in r.result_lst)
    # the sequence the fixture script drove through the reference's Result / AverageMeter
    per_case = {n: (gold[n + "_metrics"], gold[n + "_valid"]) for n in ("sparse", "single", "empty", "rand")}
    per_case.update({"batch%d" % k: (gold["batch_metrics"][k], gold["batch_valid"][k]) for k in range(3)})
    meter, restated = AverageMeter_multidist(), R.Meter()
    for name, n in zip(gold["seq_names"], gold["seq_weights"]):
        m, v = per_case[str(name)]
        meter.update(_result_from(m, v), n=float(n))
        restated.update(m, v, float(n))
    avg = meter.average()
    assert avg.valid_label == gold["seq_valid"].tolist()
    assert [a.count for a in meter.avg_lst] == gold["seq_counts"].tolist()
    assert R.rel(_rows(avg), gold["seq_averages"]) <= 1e-12
    ravg, rvalid = restated.average()
    assert np.array_equal(rvalid, gold["seq_valid"]) and R.rel(ravg, gold["seq_averages"]) <= 1e-12
    assert gold["seq_valid"].min() == 1
    # an interval that never received anything: the zero Result and valid_label 0, no division by zero
    lone = AverageMeter_multidist()
    lone.update(_result_from(*per_case["single"]), n=2)
    a = lone.average()
    assert a.valid_label == gold["single_valid"].tolist()
    assert R.rel(_rows(a)[4], gold["single_metrics"][4]) <= 1e-15 and not _rows(a)[[0, 9]].any()
    assert AverageMeter_multidist().average().valid_label == [0] * 10
    lone.reset()
    assert lone.average().valid_label == [0] * 10
    # the repaired Result_multidist.update: result_lst, lg10, each result's own times
    src = _result_from(*per_case["rand"])
    src.result_lst[3].gpu_time, src.result_lst[3].data_time = 0.5, 0.25
    dst = Result_multidist()
    dst.update(src)
    assert np.array_equal(_rows(dst), _rows(src)) and dst.result_lst[3].gpu_time == 0.5 and dst.result_lst[3].data_time == 0.25
    with pytest.raises(AssertionError):
        dst.update(Result())
    with pytest.raises(AssertionError):
        AverageMeter_multidist().update(Result_multidist([5., 50.]))


def test_pickles_under_the_reference_module_path(gold, tmp_path):
    """A Result_multidist written by the reference (class evaluation.metrics.Result_multidist holding evaluation.metrics.Result) loads
    as this package's classes once the reference's module path is aliased to ours (what utils' checkpoint loader does), and ours
    round-trips."""
    from radar_depth_amd.evaluation import metrics as ours
    src = _result_from(gold["sparse_metrics"], gold["sparse_valid"])
    back = pickle.loads(pickle.dumps(src))
    assert isinstance(back, ours.Result_multidist) and back.valid_label == src.valid_label and back.dist_interval == src.dist_interval
    assert R.rel(_rows(back), _rows(src)) == 0.0
    pkg, mod = types.ModuleType("evaluation"), types.ModuleType("evaluation.metrics")
    classes = {}
    for name in ("Result", "Result_multidist"):
        cls = type(name, (object,), {})
        cls.__module__, cls.__qualname__ = "evaluation.metrics", name
        setattr(mod, name, cls)
        classes[name] = cls
    pkg.metrics = mod
    ref = classes["Result_multidist"]()
    ref.dist_interval, ref.valid_label, ref.result_lst = list(src.dist_interval), list(src.valid_label), []
    for res in src.result_lst:
        one = classes["Result"]()
        one.__dict__.update(res.__dict__)
        ref.result_lst.append(one)
    sys.modules["evaluation"], sys.modules["evaluation.metrics"] = pkg, mod
    try:
        blob = pickle.dumps(ref)
    finally:
        del sys.modules["evaluation"], sys.modules["evaluation.metrics"]
    assert b"evaluation.metrics" in blob and b"Result_multidist" in blob
    sys.modules["evaluation"], sys.modules["evaluation.metrics"] = sys.modules["radar_depth_amd.evaluation"], ours
    try:
        got = pickle.loads(blob)
    finally:
        del sys.modules["evaluation"], sys.modules["evaluation.metrics"]
    assert isinstance(got, ours.Result_multidist) and isinstance(got.result_lst[0], ours.Result)
    assert got.valid_label == src.valid_label and R.rel(_rows(got), _rows(src)) == 0.0


# ------------------------------------------------------------------------------------------------ argument checks, no GPU
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
    return buf, (C.addressof(buf) + 15) // 16 * 16


def _edges(*v):
    return (C.c_float * len(v))(*v)


def test_every_emdist_code(L, host):
    from radar_depth_amd import _lib as B
    _, base = host
    vp = C.c_void_p
    o, t, ws, sums = vp(base), vp(base + 512), vp(base + 1024), vp(base + 2048)

    def binning(o=o, t=t, frames=1, hw=64, edges=None, n=10, ws=ws, sums=sums):
        return L.rd_depth_metrics_multidist(o, t, frames, hw, edges, n, ws, sums, None)

    def refused(rc, code, text):
        assert rc == code, (rc, code)
        assert text in L.rd_last_error(), L.rd_last_error()
    for kw in (dict(o=None), dict(t=None), dict(ws=None), dict(sums=None)):
        refused(binning(**kw), B.RD_EMDIST_NULL, b"null argument")
    for kw in (dict(frames=0), dict(frames=-1), dict(hw=0), dict(hw=-5)):
        refused(binning(**kw), B.RD_EMDIST_RANGE, b"at least one frame")
    for n in (0, -1, 17):
        refused(binning(n=n, edges=_edges(*range(1, 18))), B.RD_EMDIST_RANGE, b"n_intervals")
    refused(binning(n=4), B.RD_EMDIST_RANGE, b"default edges")                      # NULL edges are the reference's ten
    refused(binning(frames=65536), B.RD_EMDIST_FRAMES, b"65535")
    refused(binning(ws=vp(base + 1028)), B.RD_EMDIST_ALIGN, b"8-byte")
    refused(binning(sums=vp(base + 2052)), B.RD_EMDIST_ALIGN, b"8-byte")
    for bad in ((10., 10., 30.), (10., 5., 30.), (0., 5., 30.), (-1., 5., 30.), (1., float("nan"), 30.), (1., 2., float("inf"))):
        refused(binning(edges=_edges(*bad), n=3), B.RD_EMDIST_EDGES, b"strictly increasing")
    # the workspace query refuses what the call refuses, and sizes what it accepts
    q = L.rd_depth_metrics_multidist_workspace_floats
    assert q(0, 64, 10) == B.RD_EMDIST_RANGE and q(1, 0, 10) == B.RD_EMDIST_RANGE and q(1, 64, 17) == B.RD_EMDIST_RANGE
    assert q(65536, 64, 10) == B.RD_EMDIST_FRAMES
    assert q(1, 64, 10) == 2 * 100 and q(3, 4097, 16) == 2 * 3 * 3 * 160 and q(1, 1 << 40, 1) == 2 * 1024 * 10

    def update(sums=sums, rows=1, n=10, groups=1, meter=ws, last=o, valid=t):
        return L.rd_meter_update_multidist(sums, rows, n, None, None, groups, meter, last, valid, None)
    for kw in (dict(sums=None), dict(meter=None), dict(last=None), dict(valid=None)):
        refused(update(**kw), B.RD_EMDIST_NULL, b"null argument")
    refused(update(rows=0), B.RD_EMDIST_RANGE, b"rows")
    for n in (0, 17):
        refused(update(n=n), B.RD_EMDIST_RANGE, b"n_intervals")
    for groups in (0, 32):
        refused(update(groups=groups), B.RD_EMDIST_RANGE, b"n_groups")
    refused(update(meter=vp(base + 1028)), B.RD_EMDIST_ALIGN, b"aligned")
    refused(update(valid=vp(base + 514)), B.RD_EMDIST_ALIGN, b"aligned")


def test_device_meter_needs_no_gpu_to_construct():
    from radar_depth_amd.evaluation.metrics import DeviceAverageMeter_multidist
    m = DeviceAverageMeter_multidist(groups=3)
    assert m.dist_interval == list(R.DIST_INTERVAL) and m.groups == 3
    with pytest.raises(ValueError):
        DeviceAverageMeter_multidist(dist_interval=list(range(1, 18)))
    with pytest.raises(ValueError):
        DeviceAverageMeter_multidist(groups=32)

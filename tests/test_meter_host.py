"""No-GPU checks of the on-device metric meters: the fixture tests/golden/meter.npz (the real reference's Result / AverageMeter on the
CPU, tests/golden/make_golden_meter.py) against a float64 restatement of the definitions rd_meter_update implements, the opt-in
keyword of HipTrainStep, argument validation of the new entry points and the CPU-tensor error of DeviceAverageMeter."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10", "delta1", "delta2", "delta3")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "meter.npz"))


@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def ten_sums(out, target):
    """The ten sums of rd_depth_metrics: fp32 terms (as the reference forms them), summed in float64."""
    o, t = out.astype(np.float32).ravel(), target.astype(np.float32).ravel()
    v = t > 0
    o, t = o[v], t[v]
    ad = np.abs(o - t)
    ln10 = np.float32(np.log(10.0))
    lg = np.abs(np.log(o) / ln10 - np.log(t) / ln10)
    ratio = np.maximum(o / t, t / o)
    inv = np.abs(np.float32(1) / o - np.float32(1) / t)
    f64 = lambda x: float(np.sum(x.astype(np.float64)))
    return [float(v.sum()), f64(ad * ad), f64(ad), f64(lg), f64(ad / t), float((ratio < 1.25).sum()), float((ratio < 1.25 ** 2).sum()),
            float((ratio < 1.25 ** 3).sum()), f64(inv * inv), f64(inv)]


def finalise(s):
    """One row of ten sums -> the ten metrics in Result.update's order (the definitions of rd_meter_update)."""
    c = s[0]
    if c == 0:
        return np.full(10, np.nan)
    mse = s[1] / c
    return np.array([np.sqrt(s[8] / c), s[9] / c, mse, np.sqrt(mse), s[2] / c, s[4] / c, s[3] / c, s[5] / c, s[6] / c, s[7] / c])


def close(got, want, bar):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    assert (err <= bar).all(), (dict(zip(NAMES, err)), bar)
    return float(err.max()) if err.size else 0.0


def test_fixture_follows_the_definitions(gold):
    """1e-6 relative per metric: the reference's fp32 means sit within 1.4e-7 of a float64 mean of the same fp32 terms."""
    assert tuple(gold["names"]) == NAMES
    worst = 0.0
    cnt, acc = 0.0, np.zeros(10)
    for k in range(4):
        r = finalise(ten_sums(gold["step_out"][k], gold["step_target"][k]))
        w = gold["step_weights"][k]
        cnt, acc = cnt + w, acc + w * r
        worst = max(worst, close(r, gold["step_results"][k], 1e-6), close(acc / cnt, gold["step_averages"][k], 1e-6))
    cnt, acc = np.zeros(3), np.zeros((3, 10))
    for k in range(5):
        s = ten_sums(gold["frame_out"][k], gold["frame_target"][k])
        if k == 3:
            assert s[0] == 1.0
        for g in range(3):
            if gold["frame_groups"][k] >> g & 1:
                cnt[g], acc[g] = cnt[g] + 1, acc[g] + finalise(s)
    for g in range(3):
        worst = max(worst, close(acc[g] / cnt[g], gold["frame_averages"][g], 1e-6))
    empty = finalise(ten_sums(gold["empty_out"], gold["empty_target"]))
    assert np.isnan(empty).all() and np.isnan(gold["empty_result"]).all()
    print("fixture vs float64 definitions: worst relative error %.3e" % worst)


def test_train_step_keyword():
    from radar_depth_amd.main import HipTrainStep
    p = inspect.signature(HipTrainStep.__init__).parameters
    assert "metrics" in p and p["metrics"].default is False


def test_new_entry_points_validate_arguments(L):
    n = C.c_int64(16)
    for f in (L.rd_masked_l1_sums_metrics, L.rd_masked_l2_sums_metrics):
        assert f(None, None, n, None, None, None, None) == -1
    one = (C.c_double * 16)()
    # valid pointers, n <= 0: refused before any launch
    assert L.rd_masked_l1_sums_metrics(C.addressof(one), C.addressof(one), C.c_int64(0), C.addressof(one), C.addressof(one),
                                       C.addressof(one), None) == -1
    assert L.rd_depth_metrics_frames(None, None, 1, 16, None, None, None) == -1
    assert L.rd_depth_metrics_frames(C.addressof(one), C.addressof(one), 0, 16, C.addressof(one), C.addressof(one), None) == -1
    assert L.rd_depth_metrics_frames_workspace_floats(3, 1961) == 2 * 3 * 10 * L.rd_loss_tiles(C.c_int64(1961))
    assert L.rd_depth_metrics_frames_workspace_floats(0, 1961) == 0
    assert L.rd_meter_update(None, 1, None, None, 1, None, None, None) == -1
    assert L.rd_meter_update(C.addressof(one), 0, None, None, 1, C.addressof(one), C.addressof(one), None) == -1
    assert L.rd_meter_update(C.addressof(one), 1, None, None, 32, C.addressof(one), C.addressof(one), None) == -1
    assert b"n_groups" in L.rd_last_error()


def test_device_meter_rejects_cpu_tensors():
    from radar_depth_amd.evaluation.metrics import DeviceAverageMeter, daynight_mask, evaluate_batch
    m = DeviceAverageMeter(groups=3)
    x = torch.ones(2, 1, 5, 7)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.update(x, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        evaluate_batch(m, x, x)
    with pytest.raises(ValueError):
        DeviceAverageMeter(groups=0)
    # validate()'s branches (day / night x rain / sun), bit 0 = average_meter
    bits = lambda s: {k for k in range(9) if daynight_mask(s) >> k & 1}
    assert bits("day, rain") == {0, 1, 3, 5} and bits("day") == {0, 1, 4, 6}
    assert bits("night rain") == {0, 2, 3, 7} and bits("night") == {0, 2, 4, 8} and bits("dusk") == {0}

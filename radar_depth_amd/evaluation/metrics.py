"""MI355X-native counterpart of the reference's evaluation/metrics.py:
Result.evaluate (:34-58) as one fused masked reduction on the device + a single 80-byte readback (the reference issues
about a dozen blocking float() conversions per call), and the AverageMeter (:179-216).  Same attribute names."""
import ctypes as C
import math

import numpy as np
import torch

from .._lib import check, current_stream, lib, ptr


_ERRORS = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10")     # lower is better -> worst = +inf
_SCORES = ("delta1", "delta2", "delta3")                                # higher is better -> worst = 0
_TIMES = ("gpu_time", "data_time")
_METRICS = _ERRORS + _SCORES


class Result(object):
    """Record of one evaluation (same attribute names and `update` argument order as evaluation/metrics.py:10-31; picklable
    under the same module path so reference checkpoints' `best_result` round-trips)."""

    def __init__(self):
        self._assign(dict.fromkeys(_METRICS + _TIMES, 0))

    def _assign(self, values):
        for key, val in values.items():
            setattr(self, key, val)

    def set_to_worst(self):
        self._assign({**dict.fromkeys(_ERRORS, np.inf), **dict.fromkeys(_SCORES + _TIMES, 0)})

    def update(self, irmse, imae, mse, rmse, mae, absrel, lg10, delta1, delta2, delta3, gpu_time, data_time):
        self._assign(dict(zip(_METRICS + _TIMES, (irmse, imae, mse, rmse, mae, absrel, lg10, delta1, delta2, delta3,
                                                  gpu_time, data_time))))

    def evaluate(self, output, target):
        if not output.is_cuda:
            raise RuntimeError("radar_depth_amd metrics run on MI355X only (HIP kernels)")
        L = lib()
        output = output.contiguous().float()
        target = target.contiguous().float()
        n = output.numel()
        tiles = L.rd_loss_tiles(n)
        ws = torch.empty(10 * tiles, dtype=torch.float64, device=output.device)
        sums = torch.empty(10, dtype=torch.float64, device=output.device)
        check(L.rd_depth_metrics(ptr(output), ptr(target), n, ptr(ws), ptr(sums), current_stream()), "rd_depth_metrics")
        s = sums.cpu().numpy()          # the only host synchronisation
        cnt = s[0]
        mean = (lambda v: float(v / cnt)) if cnt > 0 else (lambda v: float("nan"))
        self.mse = mean(s[1])
        self.rmse = math.sqrt(self.mse) if cnt > 0 else float("nan")
        self.mae = mean(s[2])
        self.lg10 = mean(s[3])
        self.absrel = mean(s[4])
        self.delta1, self.delta2, self.delta3 = mean(s[5]), mean(s[6]), mean(s[7])
        self.data_time = 0
        self.gpu_time = 0
        self.irmse = math.sqrt(mean(s[8])) if cnt > 0 else float("nan")
        self.imae = mean(s[9])


class AverageMeter(object):
    _FIELDS = _METRICS

    def __init__(self):
        self.reset()

    def reset(self):
        self.count = 0.0
        for f in self._FIELDS:
            setattr(self, "sum_" + f, 0)
        self.sum_data_time, self.sum_gpu_time = 0, 0

    def update(self, result, gpu_time, data_time, n=1):
        self.count += n
        for f in self._FIELDS:
            setattr(self, "sum_" + f, getattr(self, "sum_" + f) + n * getattr(result, f))
        self.sum_data_time += n * data_time
        self.sum_gpu_time += n * gpu_time

    def average(self):
        avg = Result()
        c = self.count
        avg.update(self.sum_irmse / c, self.sum_imae / c, self.sum_mse / c, self.sum_rmse / c, self.sum_mae / c,
                   self.sum_absrel / c, self.sum_lg10 / c, self.sum_delta1 / c, self.sum_delta2 / c, self.sum_delta3 / c,
                   self.sum_gpu_time / c, self.sum_data_time / c)
        return avg


def _result_from_metrics(values, gpu_time=0, data_time=0):
    r = Result()
    r.update(*[float(v) for v in values], gpu_time, data_time)
    return r


class DeviceAverageMeter(object):
    """Result.evaluate + AverageMeter.update (evaluation/metrics.py:34-58, :192-206) without leaving the device: update() enqueues
    the metric sums and one rd_meter_update launch on the current stream and returns; average() / last() do the only readback.
    `groups` meters share one update (validate()'s day / night / rain meters, main.py:635-654): a frame goes to every meter whose
    bit is set in its mask.

    buf[groups][12] (float64): count, the ten weighted sums in Result.update's order, number of updates; last_buf[10]: the latest
    Result.  Both persist for the life of the object (HipTrainStep's captured step writes them on every replay)."""

    def __init__(self, groups=1, device=None):
        if not 1 <= int(groups) <= 31:
            raise ValueError("DeviceAverageMeter: groups must be 1..31 (one bit of an int32 mask each), got %r" % (groups,))
        self.groups = int(groups)
        self.device = None if device is None else torch.device(device)
        self._buf = self._last_buf = None
        self.sum_gpu_time, self.sum_data_time = 0, 0
        self._ws = {}               # (frames, hw) -> (workspace, sums): reused by every update of that geometry
        self._weights = {}          # weight -> one device double

    def _alloc(self):
        if self._buf is None:               # (on first use: constructing a meter needs no GPU)
            if not torch.cuda.is_available():
                raise RuntimeError("radar_depth_amd metrics run on MI355X only (HIP kernels)")
            if self.device is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            self._buf = torch.zeros(self.groups, 12, dtype=torch.float64, device=self.device)
            self._last_buf = torch.zeros(10, dtype=torch.float64, device=self.device)

    @property
    def buf(self):
        self._alloc()
        return self._buf

    @property
    def last_buf(self):
        self._alloc()
        return self._last_buf

    def reset(self):
        """Asynchronous: two fills on the current stream."""
        if self._buf is not None:
            self._buf.zero_()
            self._last_buf.zero_()
        self.sum_gpu_time, self.sum_data_time = 0, 0

    def add_times(self, gpu_time, data_time, n=1):
        """The host-side timings of AverageMeter.update (they never were device quantities)."""
        self.sum_gpu_time += n * gpu_time
        self.sum_data_time += n * data_time

    def _weight(self, n):
        w = self._weights.get(n)
        if w is None:
            w = self._weights[n] = torch.full((1,), float(n), dtype=torch.float64, device=self.device)
        return w

    def _group_masks(self, groups, frames):
        if groups is None:
            return None
        if torch.is_tensor(groups):
            if groups.dtype != torch.int32 or groups.numel() != frames:
                raise ValueError("DeviceAverageMeter: groups must be %d int32 bitmasks" % frames)
            return groups.to(self.device, non_blocking=True).contiguous()
        masks = [int(g) for g in groups]
        if len(masks) != frames or any(m < 0 or m >> self.groups for m in masks):
            raise ValueError("DeviceAverageMeter: groups must be %d bitmasks over %d meters, got %r" % (frames, self.groups, masks))
        return torch.tensor(masks, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)

    def update(self, pred, target, n=None, per_frame=False, groups=None):
        """per_frame=False: ONE Result over the whole tensor, weight n (default pred.size(0)) -- train()'s call (main.py:449-452).
        per_frame=True: every frame of [B,1,H,W] is its own Result with weight 1 -- validate() at batch 1 (main.py:625-654);
        groups: per-frame bitmasks (sequence, or int32 tensor: a device tensor costs no copy).  Never synchronises."""
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError("radar_depth_amd metrics run on MI355X only (HIP kernels)")
        if pred.shape != target.shape:
            raise ValueError("DeviceAverageMeter: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
        L = lib()
        self._alloc()
        pred = pred.detach().contiguous().float()
        target = target.detach().contiguous().float()
        frames = pred.size(0) if per_frame else 1
        hw = pred.numel() // frames
        masks = self._group_masks(groups, frames) if per_frame else (None if groups is None else self._group_masks([groups], 1))
        key = (frames, hw, per_frame)
        if key not in self._ws:
            nd = (int(L.rd_depth_metrics_frames_workspace_floats(frames, hw)) // 2 if per_frame else
                  10 * L.rd_loss_tiles(hw))
            self._ws[key] = (torch.empty(nd, dtype=torch.float64, device=self.device),
                             torch.empty(frames, 10, dtype=torch.float64, device=self.device))
        ws, sums = self._ws[key]
        s = current_stream()
        if per_frame:
            check(L.rd_depth_metrics_frames(ptr(pred), ptr(target), frames, hw, ptr(ws), ptr(sums), s), "rd_depth_metrics_frames")
            weights = None
        else:
            check(L.rd_depth_metrics(ptr(pred), ptr(target), hw, ptr(ws), ptr(sums), s), "rd_depth_metrics")
            weights = self._weight(pred.size(0) if n is None else n)
        check(L.rd_meter_update(ptr(sums), frames, ptr(weights), ptr(masks), self.groups, ptr(self.buf), ptr(self.last_buf), s),
              "rd_meter_update")

    def count(self, group=0):
        """Sum of the weights meter `group` has received (a readback)."""
        return float(self.buf[group, 0].item())

    def average(self, group=0):
        m = self.buf[group].cpu().numpy()           # the only host synchronisation
        c = float(m[0])
        if c == 0:
            raise ZeroDivisionError("float division by zero")       # AverageMeter.average() on an empty meter
        return _result_from_metrics(m[1:11] / c, self.sum_gpu_time / c, self.sum_data_time / c)

    def last(self):
        return _result_from_metrics(self.last_buf.cpu().numpy())


# ------------------------------------------------------------------------------------------------ distance intervals
# evaluation/metrics.py:61-176.  Interval k is [lo_k, hi_k], both ends closed: lo_0 = 0, lo_k = dist_interval[k-1],
# hi_k = dist_interval[k], and the LAST upper bound is +inf (the edge 100 is never a bound); a pixel is in it when
# target > 0 and lo_k <= target <= hi_k in float32, so a target exactly on an inner edge is counted in two intervals.
DIST_INTERVAL = (10., 20., 30., 40., 50., 60., 70., 80., 90., 100.)
_MAX_INTERVALS = 16


def _edges_arg(dist_interval):
    """The host array rd_depth_metrics_multidist takes (it is copied into the kernel arguments during the call)."""
    return (C.c_float * len(dist_interval))(*dist_interval)


def _multidist_from_rows(rows, valid, dist_interval, result=None):
    """rows[n][10] metrics (Result.update's order), valid[n] -> a Result_multidist."""
    out = Result_multidist(dist_interval) if result is None else result
    for k, res in enumerate(out.result_lst):
        res.update(*[float(v) for v in rows[k]], 0, 0)
        out.valid_label[k] = int(valid[k])
    return out


class Result_multidist(object):
    """One Result per distance interval (evaluation/metrics.py:62-138; same attributes, picklable under the same module path).
    evaluate() is ONE binning call and one readback where the reference makes a pass per interval; it sets every valid_label
    (the reference only ever clears them: there a Result_multidist is made fresh per evaluation).  update() is the reference's
    with its three slips repaired: it walks result.result_lst, reads lg10, and hands on each result's own gpu_time / data_time."""

    def __init__(self, dist_interval=None):
        self.dist_interval = [float(v) for v in (DIST_INTERVAL if dist_interval is None else dist_interval)]
        if not 1 <= len(self.dist_interval) <= _MAX_INTERVALS:
            raise ValueError("Result_multidist: 1..%d intervals, got %d" % (_MAX_INTERVALS, len(self.dist_interval)))
        self.result_lst = [Result() for _ in self.dist_interval]
        self.valid_label = [1 for _ in self.dist_interval]

    def set_to_worst(self):
        for res in self.result_lst:
            res.set_to_worst()

    def update(self, result):
        assert isinstance(result, Result_multidist)
        for idx, res in enumerate(result.result_lst):
            self.result_lst[idx].update(res.irmse, res.imae, res.mse, res.rmse, res.mae, res.absrel, res.lg10,
                                        res.delta1, res.delta2, res.delta3, res.gpu_time, res.data_time)

    def evaluate(self, output, target):
        if not output.is_cuda:
            raise RuntimeError("radar_depth_amd metrics run on MI355X only (HIP kernels)")
        L = lib()
        output = output.contiguous().float()
        target = target.contiguous().float()
        n, ni = output.numel(), len(self.dist_interval)
        nfl = int(L.rd_depth_metrics_multidist_workspace_floats(1, n, ni))
        check(min(nfl, 0), "rd_depth_metrics_multidist_workspace_floats")
        ws = torch.empty(nfl // 2, dtype=torch.float64, device=output.device)
        sums = torch.empty(ni, 10, dtype=torch.float64, device=output.device)
        check(L.rd_depth_metrics_multidist(ptr(output), ptr(target), 1, n, _edges_arg(self.dist_interval), ni, ptr(ws), ptr(sums),
                                           current_stream()), "rd_depth_metrics_multidist")
        s = sums.cpu().numpy()          # the only host synchronisation
        with np.errstate(invalid="ignore", divide="ignore"):
            c = s[:, 0]
            rows = np.stack([np.sqrt(s[:, 8] / c), s[:, 9] / c, s[:, 1] / c, np.sqrt(s[:, 1] / c), s[:, 2] / c, s[:, 4] / c, s[:, 3] / c,
                             s[:, 5] / c, s[:, 6] / c, s[:, 7] / c], axis=1)
        _multidist_from_rows(rows, c > 0, self.dist_interval, self)


class AverageMeter_multidist(object):
    """One AverageMeter per interval (evaluation/metrics.py:141-176), repaired where the reference's cannot run: update() hands
    AverageMeter.update its gpu_time / data_time (0, 0: they are quantities of the whole step), average() passes on the times and
    gives an interval that never received anything the zero Result with valid_label 0 instead of dividing by zero."""

    def __init__(self, dist_interval=None):
        self.dist_interval = [float(v) for v in (DIST_INTERVAL if dist_interval is None else dist_interval)]
        self.avg_lst = [AverageMeter() for _ in self.dist_interval]
        self.reset()

    def reset(self):
        for avg in self.avg_lst:
            avg.reset()

    def update(self, result, n=1):
        assert isinstance(result, Result_multidist)
        assert self.dist_interval == result.dist_interval
        for idx, res in enumerate(result.result_lst):
            if result.valid_label[idx] != 0:                # an interval without a pixel (NaN metrics) is passed over
                self.avg_lst[idx].update(res, 0, 0, n)

    def average(self):
        avg = Result_multidist(self.dist_interval)
        for idx, avg_obj in enumerate(self.avg_lst):
            if avg_obj.count == 0:
                avg.valid_label[idx] = 0
                continue
            res = avg_obj.average()
            avg.result_lst[idx].update(res.irmse, res.imae, res.mse, res.rmse, res.mae, res.absrel, res.lg10,
                                       res.delta1, res.delta2, res.delta3, res.gpu_time, res.data_time)
        return avg


class DeviceAverageMeter_multidist(DeviceAverageMeter):
    """Result_multidist.evaluate + AverageMeter_multidist.update without leaving the device, with DeviceAverageMeter's interface:
    update() enqueues one binning call (rd_depth_metrics_multidist: one read of pred and target for all intervals) and one
    rd_meter_update_multidist launch and returns; average() / last() / count() do the only readbacks.

    buf[groups][n][12] (float64): per interval the count, the ten weighted sums, the number of updates that reached it;
    last_buf[n][10] and valid_buf[n] (int32): the latest Result_multidist.  A frame leaves an interval it has no pixel in untouched."""

    def __init__(self, groups=1, dist_interval=None, device=None):
        DeviceAverageMeter.__init__(self, groups=groups, device=device)
        self.dist_interval = [float(v) for v in (DIST_INTERVAL if dist_interval is None else dist_interval)]
        if not 1 <= len(self.dist_interval) <= _MAX_INTERVALS:
            raise ValueError("DeviceAverageMeter_multidist: 1..%d intervals, got %d" % (_MAX_INTERVALS, len(self.dist_interval)))
        self._edges = _edges_arg(self.dist_interval)
        self._valid_buf = None

    def _alloc(self):
        if self._buf is None:
            if not torch.cuda.is_available():
                raise RuntimeError("radar_depth_amd metrics run on MI355X only (HIP kernels)")
            if self.device is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            ni = len(self.dist_interval)
            self._buf = torch.zeros(self.groups, ni, 12, dtype=torch.float64, device=self.device)
            self._last_buf = torch.zeros(ni, 10, dtype=torch.float64, device=self.device)
            self._valid_buf = torch.zeros(ni, dtype=torch.int32, device=self.device)

    @property
    def valid_buf(self):
        self._alloc()
        return self._valid_buf

    def reset(self):
        """Asynchronous: three fills on the current stream."""
        if self._buf is not None:
            self._valid_buf.zero_()
        DeviceAverageMeter.reset(self)

    def _buffers(self, frames, hw):
        """(workspace, sums[frames][n][10]) of one geometry: allocated on its first update, reused by every later one."""
        key = (frames, hw)
        if key not in self._ws:
            L, ni = lib(), len(self.dist_interval)
            nfl = int(L.rd_depth_metrics_multidist_workspace_floats(frames, hw, ni))
            check(min(nfl, 0), "rd_depth_metrics_multidist_workspace_floats")
            self._ws[key] = (torch.empty(nfl // 2, dtype=torch.float64, device=self.device),
                             torch.empty(frames, ni, 10, dtype=torch.float64, device=self.device))
        return self._ws[key]

    def update_ops(self, tag, pred, target, frames, hw, weights, masks, stream):
        """The two C-ABI calls of one update as (name, function, arguments): issued by update(), or kept in a step's op list."""
        self._alloc()
        L, ni = lib(), len(self.dist_interval)
        ws, sums = self._buffers(frames, hw)
        return [(tag + ".multidist", L.rd_depth_metrics_multidist, (ptr(pred), ptr(target), frames, hw, self._edges, ni, ptr(ws),
                                                                     ptr(sums), stream)),
                (tag + ".meter_multidist", L.rd_meter_update_multidist, (ptr(sums), frames, ni, ptr(weights), ptr(masks), self.groups,
                                                                         ptr(self._buf), ptr(self._last_buf), ptr(self._valid_buf), stream))]

    def update(self, pred, target, n=None, per_frame=False, groups=None):
        """DeviceAverageMeter.update's arguments and meaning, per interval.  Never synchronises; a second update of the same geometry
        allocates nothing."""
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError("radar_depth_amd metrics run on MI355X only (HIP kernels)")
        if pred.shape != target.shape:
            raise ValueError("DeviceAverageMeter_multidist: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
        self._alloc()
        pred = pred.detach().contiguous().float()
        target = target.detach().contiguous().float()
        frames = pred.size(0) if per_frame else 1
        hw = pred.numel() // frames
        masks = self._group_masks(groups, frames) if per_frame else (None if groups is None else self._group_masks([groups], 1))
        weights = None if per_frame else self._weight(pred.size(0) if n is None else n)
        for name, fn, args in self.update_ops("update", pred, target, frames, hw, weights, masks, current_stream()):
            check(fn(*args), name)

    def count(self, group=0):
        """Per interval, the sum of the weights meter `group` has received (a readback)."""
        return [float(v) for v in self.buf[group, :, 0].cpu().numpy()]

    def average(self, group=0):
        """A Result_multidist of the per-interval averages; valid_label[k] = 0 (and the zero Result) where interval k never received
        anything.  The times are add_times' sums over that interval's own count."""
        m = self.buf[group].cpu().numpy()           # the only host synchronisation
        out = Result_multidist(self.dist_interval)
        for k, res in enumerate(out.result_lst):
            c = float(m[k, 0])
            out.valid_label[k] = int(c > 0)
            if c > 0:
                res.update(*[float(v) for v in m[k, 1:11] / c], self.sum_gpu_time / c, self.sum_data_time / c)
        return out

    def last(self):
        self._alloc()
        return _multidist_from_rows(self._last_buf.cpu().numpy(), self._valid_buf.cpu().numpy(), self.dist_interval)


# validate()'s eight condition meters (main.py:546-562, :635-654) as bits of one DeviceAverageMeter(groups=9): bit 0 is
# average_meter itself
DAYNIGHT_GROUPS = ("all", "day", "night", "rain", "sun", "day_rain", "day_sun", "night_rain", "night_sun")


def daynight_mask(daynight_info):
    """Bitmask over DAYNIGHT_GROUPS of the meters that main.py:635-654 updates for one frame's `daynight_info` string."""
    bit = {name: 1 << k for k, name in enumerate(DAYNIGHT_GROUPS)}
    mask = bit["all"]
    rain = "rain" in daynight_info
    for time in ("day", "night"):
        if time in daynight_info:
            mask |= bit[time] | (bit["rain"] | bit[time + "_rain"] if rain else bit["sun"] | bit[time + "_sun"])
    return mask


def evaluate_batch(meter, preds, target, groups=None):
    """Batched validation: every frame of a HipInference output is evaluated on its own and enters the meter(s) with weight 1, so
    a batch of B frames leaves exactly what B passes of validate()'s batch-1 loop leave (main.py:625-654) -- one Result over the
    whole batch would pool the frames by valid-pixel count instead.  preds: the prediction [B,1,H,W], or the multistage dict;
    then `meter` may be a pair (average_meter, average_meter_stage1).  groups: per-frame bitmasks (see daynight_mask).
    The meters are DeviceAverageMeters or DeviceAverageMeter_multidists (the same update interface)."""
    stage1 = None
    if isinstance(meter, (tuple, list)):
        meter, stage1 = meter
    if isinstance(preds, dict):
        if stage1 is not None:
            stage1.update(preds["stage1"], target, per_frame=True, groups=groups)
        preds = preds["stage2"]
    elif stage1 is not None:
        raise ValueError("evaluate_batch: a stage-1 meter needs the multistage prediction dict")
    meter.update(preds, target, per_frame=True, groups=groups)

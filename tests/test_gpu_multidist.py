"""Distance-interval metrics on the device (csrc/metrics_multidist.hip: rd_depth_metrics_multidist, rd_meter_update_multidist;
evaluation.metrics.Result_multidist / DeviceAverageMeter_multidist / evaluate_batch; HipTrainStep(metrics="multidist")).

Bars.  The binning kernel forms the SAME fp32 terms as rd_depth_metrics (one metric_terms) and differs from it only in the order of
the float64 summation, so its expectation is formed the way tests/test_gpu_meter.py forms its own: rd_depth_metrics on the same
prediction with the target zeroed outside the interval (the interval rule itself comes from tests/multidist_ref.py), to that test's
1e-10 relative, counts exact.  Against the reference's own CPU results (tests/golden/multidist.npz) the well-populated cases are held
to the project's 1e-5 relative (the float64 restatement sits within 1.4e-7 of them on the host: tests/test_multidist_host.py).  The
ladder, the tails and the handful-of-pixels frame are held on counts, valid_label and NaN placement, which are exact, and their
metrics against the restatement only: 1e-5 relative, and for lg10 -- where a 1-ulp difference between two logf implementations does
not average out over two or three pixels -- 1e-5 relative plus 1e-6 absolute (logarithms of depths below 2^8 m are below 8, one ulp
there is 4.8e-7, two logarithms on either side and the factor 0.434: 8.3e-7).  The device meter against the host classes on the
same sequence of updates, float64 on both sides: 1e-10."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import multidist_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
LG10 = R.NAMES.index("lg10")
CASES = ("rand", "ladder", "sparse", "single", "empty", "tail5", "tail1")
POPULATED = ("rand", "sparse", "single")


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _ok(rc, what):
    from radar_depth_amd._lib import check
    check(rc, what)


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _f64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "multidist.npz"))


def _depth_metrics(o, t):
    L = _L()
    n = o.numel()
    ws, out = _f64(10 * L.rd_loss_tiles(C.c_int64(n))), _f64(10)
    _ok(L.rd_depth_metrics(_p(o), _p(t), C.c_int64(n), _p(ws), _p(out), _st()), "rd_depth_metrics")
    return out


def _binning(o, t, frames, hw, edges=None):
    """sums[frames][n][10] of one rd_depth_metrics_multidist call on device tensors (NaN-filled outputs: every word must be written)."""
    L = _L()
    n = 10 if edges is None else len(edges)
    arr = None if edges is None else (C.c_float * n)(*edges)
    nfl = int(L.rd_depth_metrics_multidist_workspace_floats(frames, hw, n))
    assert nfl > 0 and nfl % 2 == 0
    ws, out = _f64(nfl // 2), _f64(frames, n, 10)
    _ok(L.rd_depth_metrics_multidist(_p(o), _p(t), frames, hw, arr, n, _p(ws), _p(out), _st()), "rd_depth_metrics_multidist")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _expected(o, t, frames, hw, edges=R.DIST_INTERVAL):
    """The same sums from rd_depth_metrics, one call per frame and interval on the target zeroed outside the interval."""
    o, t = o.reshape(frames, hw), t.reshape(frames, hw)
    want = np.zeros((frames, len(edges), 10))
    for f in range(frames):
        mem = R.membership(t[f].cpu().numpy(), edges)
        for k in range(len(edges)):
            tk = torch.where(torch.from_numpy(mem[k]).to(DEV), t[f], torch.zeros_like(t[f])).contiguous()
            want[f, k] = _depth_metrics(o[f].contiguous(), tk).cpu().numpy()
            assert want[f, k, 0] == mem[k].sum()
    return want


def _sums_close(got, want, bar=1e-10):
    assert got.shape == want.shape
    for k in (0, 5, 6, 7):
        assert np.array_equal(got[..., k], want[..., k]), (k, got[..., k], want[..., k])
    assert np.array_equal(got[want[..., 0] == 0], np.zeros_like(got[want[..., 0] == 0]))          # an empty frame/interval: a row of zeros
    worst = R.rel(got, want)
    assert worst <= bar, (worst, bar)
    return worst


def _pair(n, share, seed, hi=110.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, generator=g) * (hi - 0.5) + 0.5
    o = t * (torch.rand(n, generator=g) * 1.7 + 0.5)
    t = torch.where(torch.rand(n, generator=g) < share, t, -torch.rand(n, generator=g))
    return o.to(DEV), t.to(DEV)


def _same_bits(a, b):
    """torch.equal on the words: a prediction below zero puts a NaN lg10 into the step's meters, in both steps alike."""
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _rows(r):
    return np.array([[getattr(res, n) for n in R.NAMES] for res in r.result_lst], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ binning
@pytest.mark.parametrize("case", CASES + ("batch",))
def test_binning_on_the_fixture(gold, case):
    o, t = _dev(gold[case + "_out"]), _dev(gold[case + "_target"])
    frames = 3 if case == "batch" else 1
    hw = o.numel() // frames
    got = _binning(o, t, frames, hw)
    counts = gold[case + "_counts"].reshape(frames, 10)
    assert np.array_equal(got[..., 0], counts.astype(np.float64)), (got[..., 0], counts)
    worst = _sums_close(got, _expected(o, t, frames, hw))
    metrics, valid = gold[case + "_metrics"].reshape(frames, 10, 10), gold[case + "_valid"].reshape(frames, 10)
    for f in range(frames):
        m, v = R.metrics_from_sums(got[f])
        assert np.array_equal(v, valid[f]) and np.array_equal(np.isnan(m), np.isnan(metrics[f]))
        rm = R.evaluate(o.reshape(frames, hw)[f].cpu().numpy(), t.reshape(frames, hw)[f].cpu().numpy())[0]
        others = [k for k in range(10) if k != LG10]
        e_other, e_lg = R.rel(m[:, others], rm[:, others]), np.nanmax(np.abs(m[:, LG10] - rm[:, LG10]) - 1e-5 * np.abs(rm[:, LG10]), initial=-1.0)
        print("%s frame %d: sums within %.2e of rd_depth_metrics; metrics within %.2e of the restatement, lg10 excess %.2e" %
              (case, f, worst, e_other, e_lg))
        assert e_other <= 1e-5 and e_lg <= 1e-6
        if case in POPULATED or (case == "batch" and f < 2):
            e_ref = R.rel(m, metrics[f])
            print("%s frame %d: within %.2e of the reference's CPU results" % (case, f, e_ref))
            assert e_ref <= 1e-5


@pytest.mark.parametrize("frames,hw,edges", [
    (3, 4097, None),                                                        # rows off the 16-byte grid, three blocks per frame, a tail
    (2, 4096, (35.5,)),                                                     # one interval: [0, inf]
    (2, 4100, tuple(2.0 ** (0.5 * k) for k in range(1, 17))),               # sixteen intervals, 1.41 .. 256 m
    (1, 2048 * 1024 + 4, None),                                             # past the 1024-block cap: a second trip, vector loads
    (1, 2048 * 1024 + 3, (5., 50., 60.)),                                   # ... and scalar loads
])
def test_binning_shapes(frames, hw, edges):
    o, t = _pair(frames * hw, 0.7, 40 + hw % 1000, hi=300.0 if edges and len(edges) == 16 else 110.0)
    if frames > 1:
        t.view(frames, hw)[1].fill_(0)                                      # a frame without a valid pixel
    got = _binning(o, t, frames, hw, edges)
    worst = _sums_close(got, _expected(o, t, frames, hw, R.DIST_INTERVAL if edges is None else edges))
    again = _binning(o, t, frames, hw, edges)
    assert np.array_equal(got, again)                                       # bit-reproducible
    if edges is not None and len(edges) == 1:                               # the single interval is everything rd_depth_metrics counts
        for f in range(frames):
            whole = _depth_metrics(o.view(frames, hw)[f].contiguous(), t.view(frames, hw)[f].contiguous()).cpu().numpy()
            assert got[f, 0, 0] == whole[0] and R.rel(got[f, 0], whole) <= 1e-10
    print("frames %d hw %d intervals %d: within %.2e of rd_depth_metrics" % (frames, hw, got.shape[1], worst))


def test_interval_counts_add_up_when_no_target_is_on_an_edge():
    n = 3 * 4097
    o, t = _pair(n, 0.6, 77)
    edges = torch.tensor(R.DIST_INTERVAL, device=DEV)
    on_edge = (t[:, None] == edges[None, :]).any(dim=1)
    t = torch.where(on_edge, t + 0.25, t).contiguous()
    assert not bool((t[:, None] == edges[None, :]).any())
    got = _binning(o, t, 1, n)
    whole = _depth_metrics(o, t).cpu().numpy()
    assert got[0, :, 0].sum() == whole[0] == float((t > 0).sum().item())
    for k in (5, 6, 7):
        assert got[0, :, k].sum() == whole[k]
    assert R.rel(got[0].sum(axis=0), whole) <= 1e-10


def test_one_interval_frame_equals_depth_metrics(gold):
    o, t = _dev(gold["single_out"]), _dev(gold["single_target"])
    got = _binning(o, t, 1, o.numel())
    whole = _depth_metrics(o, t).cpu().numpy()
    assert got[0, 4, 0] == whole[0] and R.rel(got[0, 4], whole) <= 1e-10
    assert not np.delete(got[0], 4, axis=0).any()
    assert np.array_equal(got, _binning(o, t, 1, o.numel()))


def test_result_multidist_evaluate(gold):
    from radar_depth_amd.evaluation.metrics import Result_multidist
    for case in POPULATED + ("empty",):
        r = Result_multidist()
        r.evaluate(_dev(gold[case + "_out"]), _dev(gold[case + "_target"]))
        assert r.valid_label == gold[case + "_valid"].tolist()
        assert R.rel(_rows(r), gold[case + "_metrics"]) <= 1e-5
        assert all(res.gpu_time == 0 and res.data_time == 0 for res in r.result_lst)
    r.evaluate(_dev(gold["rand_out"]), _dev(gold["rand_target"]))          # a reused object: every valid_label is set again
    assert r.valid_label == [1] * 10
    two = Result_multidist([35.5, 80.0])
    two.evaluate(_dev(gold["sparse_out"]), _dev(gold["sparse_target"]))
    want, valid = R.evaluate(gold["sparse_out"], gold["sparse_target"], (35.5, 80.0))
    assert two.valid_label == valid.tolist() and R.rel(_rows(two)[:, [k for k in range(10) if k != LG10]], want[:, [k for k in range(10) if k != LG10]]) <= 1e-5


# ------------------------------------------------------------------------------------------------ meters
def _seq(gold):
    """The fixture's sequence of whole-tensor updates: (prediction, target, weight)."""
    out = []
    for name, n in zip(gold["seq_names"], gold["seq_weights"]):
        name = str(name)
        if name.startswith("batch"):
            k = int(name[5:])
            out.append((_dev(gold["batch_out"][k:k + 1]), _dev(gold["batch_target"][k:k + 1]), float(n)))
        else:
            out.append((_dev(gold[name + "_out"]), _dev(gold[name + "_target"]), float(n)))
    return out


def test_meter_update_kernel(gold):
    """valid / last, empty rows, the update counter and the group routing, on rows of sums written by hand."""
    L = _L()
    rows, n, groups = 4, 3, 3
    g = torch.Generator().manual_seed(5)
    sums = torch.rand(rows, n, 10, generator=g, dtype=torch.float64) * 50 + 1
    sums[:, :, 0] = torch.tensor([[7., 0., 3.], [0., 0., 5.], [2., 0., 0.], [0., 0., 9.]], dtype=torch.float64)
    sums[sums[:, :, 0] == 0] = 0
    weights = torch.tensor([1., 2., 3., 4.], dtype=torch.float64)
    masks = torch.tensor([0b001, 0b011, 0b110, 0b111], dtype=torch.int32)
    start = torch.rand(groups, n, 12, generator=g, dtype=torch.float64)
    meter, last, valid = start.clone().to(DEV), _f64(n, 10), torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_sums, d_weights, d_masks = sums.to(DEV), weights.to(DEV), masks.to(DEV)
    _ok(L.rd_meter_update_multidist(_p(d_sums), rows, n, _p(d_weights), _p(d_masks), groups, _p(meter), _p(last), _p(valid), _st()),
        "rd_meter_update_multidist")
    torch.cuda.synchronize()
    want = start.clone().numpy()
    s = sums.numpy()
    for r in range(rows):
        m, v = R.metrics_from_sums(s[r])
        for gi in range(groups):
            if masks[r].item() >> gi & 1:
                for k in range(n):
                    if v[k]:
                        want[gi, k, 0] += weights[r].item()
                        want[gi, k, 1:11] += weights[r].item() * m[k]
                        want[gi, k, 11] += 1
    got = meter.cpu().numpy()
    assert np.array_equal(got[:, 1], start[:, 1].numpy())                  # interval 1 is empty in every row: untouched, counter included
    assert np.array_equal(got[..., 0], want[..., 0]) and np.array_equal(got[..., 11], want[..., 11])
    assert R.rel(got, want) <= 1e-12
    m, v = R.metrics_from_sums(s[rows - 1])
    assert valid.cpu().tolist() == v.tolist() == [0, 0, 1]
    assert R.rel(last.cpu().numpy(), m) <= 1e-12 and np.isnan(last.cpu().numpy()[:2]).all()
    # weights == NULL is 1, groups == NULL is bit 0
    meter2 = torch.zeros(groups, n, 12, dtype=torch.float64, device=DEV)
    _ok(L.rd_meter_update_multidist(_p(d_sums), rows, n, None, None, groups, _p(meter2), _p(last), _p(valid), _st()), "rd_meter_update_multidist")
    got2 = meter2.cpu().numpy()
    assert got2[0, :, 0].tolist() == [2., 0., 3.] and got2[0, :, 11].tolist() == [2., 0., 3.] and not got2[1:].any()


def test_device_meter_against_the_host_classes(gold):
    from radar_depth_amd.evaluation.metrics import AverageMeter_multidist, DeviceAverageMeter_multidist, Result_multidist
    masks = [0b001, 0b011, 0b101, 0b111, 0b010, 0b110, 0b001]
    dm = DeviceAverageMeter_multidist(groups=3)
    host = [AverageMeter_multidist() for _ in range(3)]
    with pytest.raises(RuntimeError):
        dm.update(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2))
    assert dm.average().valid_label == [0] * 10 and dm.count() == [0.0] * 10            # nothing received yet
    want_updates = np.zeros(10)                                                 # group 0: the updates that reached each interval
    for (o, t, n), mask in zip(_seq(gold), masks):
        dm.update(o, t, n=n, groups=mask)
        r = Result_multidist()
        r.evaluate(o, t)
        want_updates += np.array(r.valid_label) * (mask & 1)
        for gi in range(3):
            if mask >> gi & 1:
                host[gi].update(r, n=n)
        last = dm.last()
        assert last.valid_label == r.valid_label and R.rel(_rows(last)[np.array(r.valid_label) == 1], _rows(r)[np.array(r.valid_label) == 1]) <= 1e-10
        assert np.isnan(_rows(last)[np.array(r.valid_label) == 0]).all()
    worst = 0.0
    for gi in range(3):
        a, h = dm.average(gi), host[gi].average()
        assert a.valid_label == h.valid_label
        assert dm.count(gi) == [m.count for m in host[gi].avg_lst]
        worst = max(worst, R.rel(_rows(a), _rows(h)))
    print("device meter vs AverageMeter_multidist on the same updates: %.2e" % worst)
    assert worst <= 1e-10
    # group 0 received `sparse`, `single`, `empty`, batch0 ... : the update counters are per interval
    assert dm.buf[0, :, 11].cpu().numpy().tolist() == want_updates.tolist()
    assert want_updates.min() < want_updates.max()
    dm.add_times(0.5, 0.25, 2)
    c = dm.count(0)[4]
    assert dm.average(0).result_lst[4].gpu_time == 1.0 / c and dm.average(0).result_lst[4].data_time == 0.5 / c
    # the well-populated case against the reference's own CPU results, through the meter
    ref = DeviceAverageMeter_multidist()
    ref.update(_dev(gold["rand_out"]), _dev(gold["rand_target"]))
    assert ref.count() == [2.0] * 10
    e = max(R.rel(_rows(ref.last()), gold["rand_metrics"]), R.rel(_rows(ref.average()), gold["rand_metrics"]))
    print("device meter vs the reference's CPU results (rand): %.2e" % e)
    assert e <= 1e-5
    # a second update of the same geometry allocates nothing
    o, t = _dev(gold["rand_out"]), _dev(gold["rand_target"])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ref.update(o, t)
    assert torch.cuda.memory_allocated() == before
    dm.reset()
    assert dm.average().valid_label == [0] * 10 and dm.last().valid_label == [0] * 10


def test_evaluate_batch(gold):
    """A batch of three frames leaves what three batch-1 calls leave, in every group, the (meter, stage-1 meter) pair included."""
    from radar_depth_amd.evaluation.metrics import DeviceAverageMeter, DeviceAverageMeter_multidist, evaluate_batch
    o, t = _dev(gold["batch_out"]), _dev(gold["batch_target"])
    other = (o * 1.1 + 0.3).contiguous()
    masks = [0b01, 0b11, 0b10]
    b3, b3s, b1, b1s = [DeviceAverageMeter_multidist(groups=2) for _ in range(4)]
    plain3, plain1 = DeviceAverageMeter(groups=2), DeviceAverageMeter(groups=2)
    evaluate_batch((b3, b3s), {"stage1": other, "stage2": o}, t, groups=masks)
    evaluate_batch(plain3, o, t, groups=masks)
    for k in range(3):
        evaluate_batch((b1, b1s), {"stage1": other[k:k + 1], "stage2": o[k:k + 1]}, t[k:k + 1], groups=masks[k:k + 1])
        evaluate_batch(plain1, o[k:k + 1], t[k:k + 1], groups=masks[k:k + 1])
    for a, b in ((b3, b1), (b3s, b1s)):
        for gi in range(2):
            assert a.count(gi) == b.count(gi) and a.average(gi).valid_label == b.average(gi).valid_label
            assert R.rel(_rows(a.average(gi)), _rows(b.average(gi))) <= 1e-10
        assert torch.equal(a.buf, b.buf) and torch.equal(a.valid_buf, b.valid_buf)
    want = gold["batch_valid"]
    assert b3.count(0) == (want[0] + want[1]).astype(float).tolist() and b3.count(1) == (want[1] + want[2]).astype(float).tolist()
    assert b3.last().valid_label == want[2].tolist()
    assert torch.equal(plain3.buf, plain1.buf)                                  # the plain meters go on as before


# ------------------------------------------------------------------------------------------------ the training step
def _model(arch, h, w):
    from radar_depth_amd import main as hmain
    from radar_depth_amd.synthetic import procedural_fill_
    torch.manual_seed(0)
    made = hmain.create_model(types.SimpleNamespace(arch=arch, decoder="upproj", modality="rgbd", pretrained=False), [h, w])
    m, lw = made if isinstance(made, tuple) else (made, None)
    procedural_fill_(m)
    return m.cuda().train(), lw


def _batches(b, h, w, steps):
    from radar_depth_amd.synthetic import make_batch
    out = []
    for k in range(steps):
        x, t = make_batch(b, h, w, 300 + k, ref_pixels=h * w)
        out.append((x.contiguous().cuda(), t.cuda()))
    return out


def _step_check(arch, use_graph, steps=3):
    from radar_depth_amd.evaluation.metrics import DeviceAverageMeter_multidist
    from radar_depth_amd.main import HipTrainStep
    b, h, w = 2, 97, 161                                                        # tests/test_gpu_meter.py's step geometry
    data = _batches(b, h, w, steps)
    runs = {}
    for metrics in (True, "multidist"):
        m, lw = _model(arch, h, w)
        ts = HipTrainStep(m, b, h, w, lr=0.01, momentum=0.9, weight_decay=1e-4, loss_weights=lw, use_graph=use_graph, metrics=metrics)
        hand = [DeviceAverageMeter_multidist(), DeviceAverageMeter_multidist()]
        losses = []
        for x, t in data:
            loss, pred = ts.step(x, t)
            losses.append(loss.clone())
            if metrics == "multidist":
                for hm, pr in zip(hand, [pred] + ([ts.plans[0].pred] if ts.multistage else [])):
                    hm.update(pr, t, n=b)
        torch.cuda.synchronize()
        runs[metrics] = ([v.item() for v in losses], [p.detach().clone() for p in m.parameters()], ts, hand)
    l0, p0, ts0, _ = runs[True]
    l1, p1, ts, hand = runs["multidist"]
    assert ts0.meter_multidist is None and ts0.meter_multidist_stage1 is None
    assert not [name for name, _, _ in ts0._ops if "multidist" in name]
    names = [name for name, _, _ in ts._ops]
    assert [n for n in names if n not in ("loss.multidist", "loss.meter_multidist", "loss1.multidist", "loss1.meter_multidist", "loss2.multidist",
                                          "loss2.meter_multidist")] == [name for name, _, _ in ts0._ops]
    assert len([n for n in names if n.endswith(".multidist")]) == len([n for n in names if n.endswith(".meter_multidist")]) == len(ts.plans)
    assert l0 == l1, (l0, l1)                                                   # bit-equal losses
    assert all(torch.equal(a, c) for a, c in zip(p0, p1))
    assert _same_bits(ts.meter.buf, ts0.meter.buf) and _same_bits(ts.meter.last_buf, ts0.meter.last_buf)
    assert (ts.meter_multidist_stage1 is not None) == ts.multistage
    if ts.multistage:
        assert _same_bits(ts.meter_stage1.buf, ts0.meter_stage1.buf)
    worst = 0.0
    for dm, hm in zip([ts.meter_multidist] + ([ts.meter_multidist_stage1] if ts.multistage else []), hand):
        a, want = dm.average(), hm.average()
        assert sum(a.valid_label) >= 2 and a.valid_label == want.valid_label
        assert dm.count() == hm.count() and max(dm.count()) == float(b * steps)           # a captured step counts once
        assert torch.equal(dm.buf[0, :, 11], hm.buf[0, :, 11]) and float(dm.buf[0, :, 11].max().item()) == float(steps)
        worst = max(worst, R.rel(_rows(a), _rows(want)), R.rel(_rows(dm.last()), _rows(hm.last())))
    print("step %s graph=%s: step.meter_multidist within %.2e of a hand-fed DeviceAverageMeter_multidist" % (arch, use_graph, worst))
    assert worst <= 1e-10
    ts.close()
    ts0.close()


@pytest.mark.parametrize("use_graph", [False, True])
def test_step_latefusion(use_graph):
    _step_check("resnet18_latefusion", use_graph)


def test_step_multistage_uncertainty():
    _step_check("resnet18_multistage_uncertainty_fixs", False)


def test_step_rejects_an_unknown_metrics_value():
    from radar_depth_amd.main import HipTrainStep
    m, lw = _model("resnet18_latefusion", 97, 161)
    with pytest.raises(ValueError):
        HipTrainStep(m, 2, 97, 161, metrics="multi")

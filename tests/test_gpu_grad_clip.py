"""Gradient-norm clipping and the non-finite guard on the GPU: rd_grad_sumsq and rd_sgd_step_clip through the C ABI against float64
(tests/grad_clip_ref.py) and, bit for bit, against rd_sgd_step; then HipTrainStep(max_grad_norm=, skip_nonfinite=) against the CPU oracle
with torch.nn.utils.clip_grad_norm_, against a step without the options, under hipGraph replay and on the data-parallel path.

Bars: the sum of squares is a float64 sum of exact squares, only its order differs from the reference's (n * 2^-53 at worst): 1e-12
relative.  The coefficient is one float64 quotient rounded to fp32: one fp32 ulp.  The update: the 2^-22 bars of
tests/test_gpu_loss_opt.py::test_sgd_step, with its sign convention (every gradient has the sign of its parameter) for the reason its
docstring gives.  The step: the bars of tests/test_gpu_model.py::test_fused_step_matches_oracle (losses 2e-3, parameter norms 5e-3) and
the project's gradient-norm bar (1e-2, plus a floor of 1e-6 of the largest norm for tensors whose true gradient is zero)."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_clip_ref as R  # noqa: E402
from test_gpu_loss_opt import CANARY, SGD_HP  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
E22 = 2.0 ** -22
RED_BLOCKS = 1024
ARENA = 14710752            # floats of the late-fusion model's arenas
NS = [1, 2, 3, 4, 5, 1003, 4096, 2 * 256 * 8 * RED_BLOCKS + 5, ARENA]     # the eighth: a second grid-stride trip and a full set of partials
CAN = float(np.float32(CANARY))


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _ok(rc, what):
    from radar_depth_amd._lib import check
    check(rc, what)


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _p(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off)


def _arena(n, v=None):
    pad = ((n + 3) // 4) * 4 + 8 - n            # >= 4 floats of canary past n
    a = torch.full((n + pad,), CANARY, device=DEV)
    if v is not None:
        a[:n] = v.to(DEV)
    return a


@functools.lru_cache(maxsize=None)
def _case(n):
    """Shared and never modified: parameter, gradient and momentum arenas with canaries past n, the float64 sum of squares of the gradient
    (numpy on the host; torch on the device for the two largest sizes) and the device the float64 formulas run on."""
    dev = "cpu" if n <= (1 << 20) else DEV
    g = torch.Generator(device=dev).manual_seed(700 + n % 1000)
    sign = torch.where(torch.rand(n, generator=g, device=dev) < 0.5, -1.0, 1.0)
    p0 = sign * (torch.rand(n, generator=g, device=dev) * 1.75 + 0.25)
    gr = sign * (torch.rand(n, generator=g, device=dev) * 1.9 + 0.1)
    b0 = sign * (torch.rand(n, generator=g, device=dev) * 3.0 + 0.1)
    if dev == "cpu":
        S = R.sumsq(gr.numpy())
    else:
        S = float((gr.double() ** 2).sum().item())
    return dict(n=n, dev=dev, P=_arena(n, p0), G=_arena(n, gr), B=_arena(n, b0), S=S)


def _partials(n):
    k = _L().rd_grad_sumsq_partials(n)
    assert k == min(RED_BLOCKS, (n + 2047) // 2048)
    return torch.full((k + 2,), CANARY, dtype=torch.float64, device=DEV), k


def _sumsq(G, n):
    part, k = _partials(n)
    _ok(_L().rd_grad_sumsq(_p(G), n, _p(part), _st()), "rd_grad_sumsq")
    return part, k


def _clip(P, G, B, n, hp, max_norm, skip, part, k, stats):
    lr, mom, wd, gs = hp
    return _L().rd_sgd_step_clip(_p(P), _p(G), _p(B), n, lr, mom, wd, gs, max_norm, skip, _p(part), k, _p(stats), _st())


def _stats():
    return torch.zeros(4, dtype=torch.float64, device=DEV)


def _reference(c, P0, G, B0, hp, s):
    """float64 update of the first n elements with the fp32 gradient scale s (a Python float): p, buf, d on the case's device"""
    n, dev = c["n"], c["dev"]
    lrf, momf, wdf, _ = (float(np.float32(v)) for v in hp)
    p64, g64, b64 = (a[:n].to(dev).double() for a in (P0, G, B0))
    d64 = wdf * p64 + s * g64
    b64 = momf * b64 + d64
    return p64 - lrf * b64, b64, d64


def _same(a, b):
    return (a == b) | (a.isnan() & b.isnan())


def _assert_update(c, P0, G, B0, P, B, hp, s, what):
    """P, B against the float64 update of P0, B0: the 2^-22 bars where the reference is finite, the same inf / NaN where it is not"""
    n, dev = c["n"], c["dev"]
    lrf = float(np.float32(hp[0]))
    p64, b64, d64 = _reference(c, P0, G, B0, hp, s)
    gp, gb = P[:n].to(dev).double(), B[:n].to(dev).double()
    fin = torch.isfinite(p64) & torch.isfinite(b64)
    assert bool(_same(gp, p64)[~fin].all()) and bool(_same(gb, b64)[~fin].all()), (what, "non-finite elements differ")
    eb = ((gb - b64).abs() / (b64.abs() + d64.abs()))[fin]
    ep = ((gp - p64).abs() / (p64.abs() + lrf * b64.abs()))[fin]
    if eb.numel():
        print("%s n=%d: buf %.3e  p %.3e  (bar 2^-22 = %.3e)" % (what, n, eb.max().item(), ep.max().item(), E22))
        assert eb.max().item() <= E22 and ep.max().item() <= E22, (what, eb.max().item(), ep.max().item())
    for a in (P, B, G):
        assert bool((a[n:] == CAN).all()), "wrote past n"


# ------------------------------------------------------------------------------------------------ rd_grad_sumsq
@pytest.mark.parametrize("n", NS)
def test_grad_sumsq_accuracy_and_reproducibility(n):
    c = _case(n)
    G = c["G"].clone()
    part, k = _sumsq(G, n)
    part2, _ = _sumsq(G, n)
    torch.cuda.synchronize()
    got = float(part[:k].sum().item())
    print("rd_grad_sumsq n=%d: %d partials, sum %.17g, float64 %.17g, relative %.3e" % (n, k, got, c["S"], abs(got - c["S"]) / c["S"]))
    assert abs(got - c["S"]) <= 1e-12 * c["S"]
    assert torch.equal(part, part2), "two calls must give the same partials bit for bit"
    assert bool((part[k:] == CANARY).all()), "wrote past the partials"
    assert torch.equal(G, c["G"]), "the gradient arena is read-only"


# ------------------------------------------------------------------------------------------------ rd_sgd_step_clip
@pytest.mark.parametrize("hp", SGD_HP)
@pytest.mark.parametrize("n", NS)
def test_sgd_step_clip_with_coef_one_is_sgd_step(n, hp):
    c = _case(n)
    L = _L()
    lr, mom, wd, gs = hp
    P1, B1 = c["P"].clone(), c["B"].clone()
    _ok(L.rd_sgd_step(_p(P1), _p(c["G"]), _p(B1), n, lr, mom, wd, gs, 0, _st()), "rd_sgd_step")
    part, k = _sumsq(c["G"], n)
    norm = float(np.float32(gs)) * math.sqrt(c["S"])
    for max_norm in (4.0 * norm + 1.0, float("inf"), 0.0, -1.0):
        P, B, stats = c["P"].clone(), c["B"].clone(), _stats()
        _ok(_clip(P, c["G"], B, n, hp, max_norm, 0, part, k, stats), "rd_sgd_step_clip")
        torch.cuda.synchronize()
        assert torch.equal(P, P1) and torch.equal(B, B1), ("coef == 1 must give rd_sgd_step's bits", max_norm)
        assert stats.tolist()[1:] == [1.0, 0.0, 0.0] and abs(stats[0].item() - norm) <= 1e-12 * norm


@pytest.mark.parametrize("hp", SGD_HP)
@pytest.mark.parametrize("n", NS)
def test_sgd_step_clip_active(n, hp):
    c = _case(n)
    gs = hp[3]
    norm = R._f32(gs) * math.sqrt(c["S"])
    max_norm = 0.3 * norm
    want = R.clip_coef(norm, max_norm)
    assert 0.29 < want < 0.31
    part, k = _sumsq(c["G"], n)
    P, B, G, stats = c["P"].clone(), c["B"].clone(), c["G"].clone(), _stats()
    _ok(_clip(P, G, B, n, hp, max_norm, 0, part, k, stats), "rd_sgd_step_clip")
    torch.cuda.synchronize()
    st = stats.tolist()
    assert abs(st[0] - norm) <= 1e-12 * norm, (st[0], norm)
    assert abs(st[1] - want) <= float(np.spacing(np.float32(want))) and st[1] == float(np.float32(st[1])), (st[1], want)
    assert st[2:] == [0.0, 0.0]
    _assert_update(c, c["P"], G, c["B"], P, B, hp, R.scale(gs, st[1]), "active clip")
    assert torch.equal(G, c["G"]), "the gradient arena keeps the unclipped gradients"


@pytest.mark.parametrize("n", NS)
def test_nonfinite_elements(n):
    c = _case(n)
    hp = SGD_HP[0]
    norm = math.sqrt(c["S"])
    max_norm = 0.3 * norm
    part_ok, k = _sumsq(c["G"], n)
    stats = _stats()            # one statistics block through the whole test: the skip count only grows
    skipped = 0
    for bad in (float("inf"), float("nan")):
        for pos in sorted({0, n // 2, n - 1}):          # the last element is in the n & 3 tail for n = 1003 and n = 5
            G = c["G"].clone()
            G[pos] = bad
            part, _ = _sumsq(G, n)
            # skip_nonfinite = 1: nothing of p or buf is touched
            P, B = c["P"].clone(), c["B"].clone()
            _ok(_clip(P, G, B, n, hp, max_norm, 1, part, k, stats), "rd_sgd_step_clip, skip")
            torch.cuda.synchronize()
            skipped += 1
            st = stats.tolist()
            assert torch.equal(P, c["P"]) and torch.equal(B, c["B"]), (bad, pos)
            assert st[2] == float(skipped) and st[3] == 1.0 and not math.isfinite(st[0]), (bad, pos, st)
            # a following finite call: counted no further, updates normally
            _ok(_clip(P, c["G"], B, n, hp, max_norm, 1, part_ok, k, stats), "rd_sgd_step_clip, finite")
            torch.cuda.synchronize()
            st = stats.tolist()
            assert st[2] == float(skipped) and st[3] == 0.0 and abs(st[0] - norm) <= 1e-12 * norm, (bad, pos, st)
            _assert_update(c, c["P"], c["G"], c["B"], P, B, hp, R.scale(1.0, st[1]), "finite call after a skip")
            # skip_nonfinite = 0: torch's arithmetic as written -- coef = c / inf = 0 or NaN with the clip, the one element without
            for mn in (max_norm, 0.0):
                P, B, st0 = c["P"].clone(), c["B"].clone(), _stats()
                _ok(_clip(P, G, B, n, hp, mn, 0, part, k, st0), "rd_sgd_step_clip, no skip")
                torch.cuda.synchronize()
                tn = float("nan") if math.isnan(bad) else float("inf")
                want = R.clip_coef(tn, mn)
                got = st0.tolist()
                assert (got[1] == want or (math.isnan(got[1]) and math.isnan(want))) and got[2:] == [0.0, 0.0], (bad, pos, mn, got)
                assert math.isnan(got[0]) if math.isnan(bad) else got[0] == float("inf")
                _assert_update(c, c["P"], G, c["B"], P, B, hp, R.scale(1.0, want), "non-finite, no skip, max_norm %g" % mn)
                assert bool(P[:n].isnan().any()) or bool(P[:n].isinf().any())


def test_clip_rejects_bad_arguments():
    L = _L()
    n = 64
    t = [torch.zeros(n + 8, device=DEV) for _ in range(3)]
    part, k = _partials(n)
    part0 = part.clone()
    stats = torch.zeros(8, dtype=torch.float64, device=DEV)

    def call(offs=(0, 0, 0, 0, 0), n_part=k):
        return L.rd_sgd_step_clip(_p(t[0], offs[0]), _p(t[1], offs[1]), _p(t[2], offs[2]), n, 0.01, 0.9, 0.0, 1.0, 1.0, 1,
                                  _p(part, offs[3]), n_part, _p(stats, offs[4]), _st())

    for i in range(5):
        offs = [0] * 5
        offs[i] = 4 if i < 3 else 8
        assert call(offs) == EINVAL, "pointer %d misaligned must be rejected" % i
    assert call(n_part=k + 1) == EINVAL and call(n_part=0) == EINVAL
    assert L.rd_grad_sumsq(_p(t[1], 4), n, _p(part), _st()) == EINVAL and L.rd_grad_sumsq(_p(t[1]), n, _p(part, 8), _st()) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((x == 0).all()) for x in t) and torch.equal(part, part0) and bool((stats == 0).all()), "a refused call writes nothing"
    _ok(L.rd_grad_sumsq(_p(t[1]), n, _p(part), _st()), "rd_grad_sumsq")
    assert call() == 0 and call((16, 16, 16, 16, 16)) == 0
    torch.cuda.synchronize()
    assert all(bool((x == 0).all()) for x in t)            # (zero gradients: coef 1, nothing moves)


# ------------------------------------------------------------------------------------------------ the step
B_, H_, W_ = 2, 97, 161


def _build():
    from radar_depth_amd.model.models import ResNet_latefusion
    from radar_depth_amd.synthetic import procedural_fill_
    torch.manual_seed(0)
    m = ResNet_latefusion(18, "upproj", [H_, W_], 4, False)
    procedural_fill_(m)
    return m.cuda()


def _batch(seed):
    from radar_depth_amd.synthetic import make_batch
    x, t = make_batch(B_, H_, W_, seed, ref_pixels=H_ * W_)
    return x, t


@functools.lru_cache(maxsize=None)
def _oracle_run():
    """Three steps of the reference's loop with clip_grad_norm_ at half of its own unclipped first-step norm, on the CPU (shared by the
    two operand modes): the losses, the norm torch returns and the momentum-buffer norms after step 1 (clipped, and what they would be
    unclipped: d = g + wd p on a first step), the parameter norms after step 3."""
    from oracle.criteria import MaskedL1Loss as OL1
    from oracle.models import ResNet_latefusion as ORef
    from radar_depth_amd.synthetic import procedural_fill_
    torch.manual_seed(0)
    o = ORef(18, "upproj", [H_, W_], 4, False)
    procedural_fill_(o)
    o.train()
    opt = torch.optim.SGD(o.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    crit = OL1()
    out = dict(loss=[])
    params = list(o.parameters())
    for it in range(3):
        x, t = _batch(99 + it)
        lo = crit(o(x), t)
        opt.zero_grad()
        lo.backward()
        if it == 0:
            unclipped = float(torch.nn.utils.clip_grad_norm_(params, float("inf")))
            out["c"] = 0.5 * unclipped
            out["buf_unclipped"] = np.array([(p.grad.double() + 1e-4 * p.detach().double()).norm().item() for p in params])
            # tensors whose first momentum buffer is their gradient to 1 %: the weight-decay term does not blur the factor
            out["grad_dominates"] = np.array([p.grad.double().norm().item() > 100 * 1e-4 * p.detach().double().norm().item() for p in params])
        norm = float(torch.nn.utils.clip_grad_norm_(params, out["c"]))
        opt.step()
        out["loss"].append(lo.item())
        if it == 0:
            assert norm == unclipped
            out["norm"] = norm
            out["buf"] = np.array([opt.state[p]["momentum_buffer"].double().norm().item() for p in params])
    out["param_norms"] = np.array([p.double().norm().item() for p in params])
    out["conv3"] = o.conv3.weight.detach().double().clone()
    return out


def _misses(a, b):
    """tensors whose norm a is not within the gradient-norm bar of b"""
    floor = 1e-6 * b.max()
    return np.abs(a - b) > 1e-2 * b + floor


@pytest.mark.parametrize("operands", ["split", "fp32"])
def test_clipped_step_matches_oracle(operands):
    from radar_depth_amd.main import HipTrainStep
    want = _oracle_run()
    m = _build()
    ts = HipTrainStep(m, B_, H_, W_, lr=0.01, momentum=0.9, weight_decay=1e-4, operands=operands, max_grad_norm=want["c"])
    assert [name for name, _, _ in ts._sgd_ops()] == ["grad_sumsq", "sgd_step_clip"]
    for it in range(3):
        x, t = _batch(99 + it)
        lg, _ = ts.step(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        print("step %d: loss %.6f oracle %.6f; grad_norm %.6g clip_coef %.6g" % (it, lg.item(), want["loss"][it], ts.grad_norm, ts.clip_coef))
        assert abs(lg.item() - want["loss"][it]) / want["loss"][it] < 2e-3, (it, lg.item(), want["loss"][it])
        if it == 0:
            assert abs(ts.grad_norm - want["norm"]) <= 1e-2 * want["norm"], (ts.grad_norm, want["norm"])
            assert abs(ts.clip_coef - 0.5) < 1e-2 and ts.skipped == 0
            sd = ts.state_dict()["state"]
            buf = np.array([sd[i]["momentum_buffer"].double().norm().item() for i in range(len(sd))])
            assert len(buf) == len(want["buf"])
            bad = _misses(buf, want["buf"])
            assert not bad.any(), [(i, buf[i], want["buf"][i]) for i in np.nonzero(bad)[0][:8]]
            # a clip that is never applied cannot pass: against the unclipped oracle the same comparison fails by a factor of about 2
            big = want["grad_dominates"]
            ratio = want["buf_unclipped"][big] / buf[big]
            print("unclipped oracle / clipped step, momentum norms: %.3f .. %.3f over %d of %d tensors"
                  % (ratio.min(), ratio.max(), int(big.sum()), len(big)))
            assert int(big.sum()) >= len(big) // 2
            assert _misses(buf, want["buf_unclipped"])[big].all() and ratio.min() > 1.8 and ratio.max() < 2.2
    pg = np.array([p.double().norm().item() for p in m.parameters()])
    assert np.abs(want["param_norms"] - pg).max() / want["param_norms"].max() < 5e-3
    a_, c_ = m.conv3.weight.detach().cpu().double(), want["conv3"]
    assert ((a_ - c_).norm() / c_.norm()).item() < 5e-3
    ts.close()


def _arenas_equal(a, b):
    return torch.equal(a.st["arena"], b.st["arena"]) and torch.equal(a.st["mom"], b.st["mom"])


def test_inert_clip_is_the_plain_step():
    from radar_depth_amd.main import HipTrainStep
    m, twin = _build(), _build()
    ts = HipTrainStep(m, B_, H_, W_, max_grad_norm=float("inf"), skip_nonfinite=False)
    plain = HipTrainStep(twin, B_, H_, W_)
    assert plain.grad_stats is None and plain.grad_norm is None and plain.clip_coef is None and plain.skipped is None
    assert [(name, fn.__name__) for name, fn, _ in plain._sgd_ops()] == [("sgd_step", "rd_sgd_step")]
    assert not hasattr(plain, "_sumsq_partials")
    assert ts.grad_stats.dtype == torch.float64 and tuple(ts.grad_stats.shape) == (4,)
    for it in range(2):
        x, t = _batch(300 + it)
        l1, _ = ts.step(x.cuda(), t.cuda())
        l2, _ = plain.step(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        assert l1.item() == l2.item() and _arenas_equal(ts, plain), it
        assert ts.clip_coef == 1.0 and ts.grad_norm > 0 and ts.skipped == 0
    assert torch.equal(ts.st["grads"], plain.st["grads"])
    ts.close()
    plain.close()


def test_graph_replay_and_set_max_grad_norm():
    from radar_depth_amd.main import HipTrainStep
    m1, m2 = _build(), _build()
    g = HipTrainStep(m1, B_, H_, W_, use_graph=True, max_grad_norm=float("inf"), skip_nonfinite=True)
    p = HipTrainStep(m2, B_, H_, W_, use_graph=False, max_grad_norm=float("inf"), skip_nonfinite=True)
    coefs = []
    for it in range(5):
        x, t = _batch(400 + it)
        l1, _ = g.step(x.cuda(), t.cuda())
        l2, _ = p.step(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        assert l1.item() == l2.item() and _arenas_equal(g, p), it
        assert torch.equal(g.grad_stats, p.grad_stats), it
        coefs.append(g.clip_coef)
        if it == 0:                                     # takes effect on the next step, on the graph route too
            c = 0.1 * g.grad_norm                       # (well below the norms of the next steps, whatever the first update does to them)
            g.set_max_grad_norm(c)
            p.set_max_grad_norm(c)
            assert g.graphs is None and g._table is None
        if it in (1, 2, 3):
            assert g.graphs is not None, "steps 2.. replay hipGraphs"
        if it == 3:
            g.set_max_grad_norm(None)                   # skip_nonfinite stays: the norm is still measured, nothing is clipped
            p.set_max_grad_norm(float("inf"))
    print("clip coefficients over the five steps:", coefs)
    assert coefs[0] == 1.0 and all(c < 1.0 for c in coefs[1:4]) and coefs[4] == 1.0 and g.skipped == 0
    with pytest.raises(ValueError):
        g.set_max_grad_norm(0.0)
    g.close()
    p.close()


@pytest.mark.parametrize("comm", ["torch", "rccl"])
def test_data_parallel_path_single_rank_with_clip(comm, tmp_path, monkeypatch):
    """tests/test_gpu_model.py::test_data_parallel_path_single_rank (torch.distributed's communicator) and the native communicator of
    tests/test_gpu_configs.py::test_native_rccl_comm_single_rank with the options on: the norm pass and the clipped SGD run behind the
    exchange, as segment graphs and as plain launches, and reproduce the single-GPU step bit for bit."""
    import torch.distributed as dist
    from radar_depth_amd import comm as rd_comm
    from radar_depth_amd.main import HipTrainStep
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29617")
    kw = dict(max_grad_norm=float("inf"), skip_nonfinite=True)
    ref = _build()
    ts_ref = HipTrainStep(ref, B_, H_, W_, use_graph=True, **kw)
    if comm == "torch":
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    else:
        rd_comm.init_from_file(str(tmp_path / "rccl_token"), 0, 1)
    try:
        monkeypatch.setenv("RD_FORCE_DP", "1")
        m, m2 = _build(), _build()
        ts = HipTrainStep(m, B_, H_, W_, use_graph=comm == "torch", **kw)       # (segment graphs: the route the torch test takes)
        ts2 = HipTrainStep(m2, B_, H_, W_, **kw)
        assert ts.dp and ts2.dp and not ts_ref.dp and ts.comm == ts2.comm == comm
        steps = (ts_ref, ts, ts2)
        for it in range(3):
            x, t = _batch(300 + it)
            losses = [s.step(x.cuda(), t.cuda())[0] for s in steps]
            torch.cuda.synchronize()
            assert losses[0].item() == losses[1].item() == losses[2].item()
            assert torch.equal(ts_ref.grad_stats, ts.grad_stats) and torch.equal(ts_ref.grad_stats, ts2.grad_stats), it
            if it == 0:
                c = 0.1 * ts_ref.grad_norm              # (well below the norms of the next steps, whatever the first update does to them)
                for s in steps:
                    s.set_max_grad_norm(c)
            else:
                assert ts.clip_coef < 1.0
        assert _arenas_equal(ts_ref, ts) and _arenas_equal(ts_ref, ts2)
        for s in steps:
            s.close()
    finally:
        if comm == "torch":
            dist.destroy_process_group()
        else:
            rd_comm.destroy()


def test_uncertainty_arch_norm_covers_every_parameter():
    import types

    from radar_depth_amd import main as hmain
    from radar_depth_amd.synthetic import procedural_fill_
    args = types.SimpleNamespace(arch="resnet18_multistage_uncertainty_fixs", decoder="upproj", modality="rgbd", pretrained=False)
    torch.manual_seed(0)
    hm, lw = hmain.create_model(args, [H_, W_])
    procedural_fill_(hm)
    hm = hm.cuda()
    ts = hmain.HipTrainStep(hm, B_, H_, W_, loss_weights=lw, max_grad_norm=float("inf"))
    x, t = _batch(500)
    ts.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    st = ts.st
    grads = st["grads"]
    whole = float(grads.double().norm().item())
    names = [n for n, _ in hm.named_parameters()]
    assert "w_stage1" in names and "w_stage2" in names
    views = [st["gviews"][id(p)] for p in hm.parameters()]
    per_param = math.sqrt(sum(float((v.double() ** 2).sum().item()) for v in views))
    covered = torch.zeros(st["total"], dtype=torch.bool, device=DEV)
    for v in views:
        off = (v.data_ptr() - grads.data_ptr()) // 4
        covered[off:off + v.numel()] = True
    n_pad = int((~covered).sum().item())
    print("grad_norm %.12g, arena %.12g, per parameter %.12g; %d padding words; w grads %g %g"
          % (ts.grad_norm, whole, per_param, n_pad, hm._grad_view(hm.w_stage1).item(), hm._grad_view(hm.w_stage2).item()))
    assert n_pad >= 6 and bool((grads[~covered] == 0).all()), "the arena's padding words must be zero: the norm runs over all of it"
    assert hm._grad_view(hm.w_stage1).item() != 0.0 and hm._grad_view(hm.w_stage2).item() != 0.0
    assert abs(ts.grad_norm - whole) <= 1e-6 * whole and abs(ts.grad_norm - per_param) <= 1e-6 * per_param
    ts.close()


def test_skip_nonfinite_step():
    """A finite step, a batch whose image has one inf pixel, a finite step.  BatchNorm running statistics (and meters) have been
    updated by the middle step's forward; parameters and momentum have not."""
    from radar_depth_amd.main import HipTrainStep
    m = _build()
    ts = HipTrainStep(m, B_, H_, W_, skip_nonfinite=True)
    assert ts.max_grad_norm is None and ts.grad_stats is not None
    x, t = _batch(600)
    ts.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert ts.skipped == 0 and ts.clip_coef == 1.0 and math.isfinite(ts.grad_norm)
    arena, mom = ts.st["arena"].clone(), ts.st["mom"].clone()
    assert bool(mom.any())
    xb, tb = _batch(601)
    xb[0, 1, 40, 60] = float("inf")
    ts.step(xb.cuda(), tb.cuda())
    torch.cuda.synchronize()
    assert torch.equal(ts.st["arena"], arena) and torch.equal(ts.st["mom"], mom)
    assert ts.skipped == 1 and not math.isfinite(ts.grad_norm) and ts.grad_stats[3].item() == 1.0 and ts.steps == 2
    x, t = _batch(602)
    loss, _ = ts.step(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert ts.skipped == 1 and ts.grad_stats[3].item() == 0.0 and math.isfinite(ts.grad_norm) and math.isfinite(loss.item())
    assert not torch.equal(ts.st["arena"], arena) and not torch.equal(ts.st["mom"], mom)
    assert bool(torch.isfinite(ts.st["arena"]).all()) and bool(torch.isfinite(ts.st["mom"]).all())
    ts.close()

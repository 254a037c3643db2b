"""Gradient-norm clipping and the non-finite guard of the fused step, without a GPU: the numpy restatement (tests/grad_clip_ref.py)
against torch.nn.utils.clip_grad_norm_ + torch.optim.SGD on the CPU, the validation of HipTrainStep's max_grad_norm, and the three
entry points in the compiled prototype table, the header and the op table (nothing is launched)."""
import ctypes as C
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_clip_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E22 = 2.0 ** -22
SHAPES = [(1,), (3,), (16, 3, 7, 7), (64,), (5, 13), (1003,), (129, 31)]
LR, MOM, WD = 0.01, 0.9, 1e-4


def _tensors(seed, grad_gain):
    """Parameters of either sign and gradients of their parameter's sign (tests/test_gpu_loss_opt.py::test_sgd_step: a count of
    roundings bounds the error relative to the result only while the sums of the update do not cancel)."""
    g = torch.Generator().manual_seed(seed)
    ps, signs = [], []
    for sh in SHAPES:
        sign = torch.where(torch.rand(sh, generator=g) < 0.5, -1.0, 1.0)
        ps.append(sign * (torch.rand(sh, generator=g) * 1.75 + 0.25))
        signs.append(sign)
    grads = lambda: [s * (torch.rand(s.shape, generator=g) * 1.9 + 0.1) * grad_gain for s in signs]      # noqa: E731
    return ps, grads


def _two_steps_against_torch(max_norm, grad_gain, seed):
    ps, grads = _tensors(seed, grad_gain)
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.SGD(params, LR, momentum=MOM, weight_decay=WD)
    coefs = []
    for it in range(2):
        gs = grads()
        # the float64 state is reloaded from torch's fp32 state before each step, so errors do not compound
        p0 = [p.detach().numpy().copy() for p in params]
        b0 = [opt.state[p]["momentum_buffer"].numpy().copy() if it else np.zeros(p.shape, np.float32) for p in params]      # (a missing buffer starts as d = 0.9 * 0 + d)
        for p, g_ in zip(params, gs):
            p.grad = g_.clone()
        norm_t = float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0, error_if_nonfinite=False))
        coef_t = [float((p.grad.double() / g_.double()).mean()) for p, g_ in zip(params, gs)]       # what torch multiplied by
        opt.step()
        p64, b64, d64, st = R.step(p0, [g_.numpy() for g_ in gs], b0, LR, MOM, WD, 1.0, max_norm)
        print("step %d: total_norm torch %.9g restatement %.9g; clip_coef torch %.9g restatement %.9g"
              % (it, norm_t, st["total_norm"], coef_t[-1], st["clip_coef"]))
        assert abs(norm_t - st["total_norm"]) <= 1e-6 * st["total_norm"]
        assert all(abs(c - st["clip_coef"]) <= 1e-6 * st["clip_coef"] for c in coef_t)
        lrf = float(np.float32(LR))
        for p, pw, bw, dw in zip(params, p64, b64, d64):
            gp, gb = p.detach().double().numpy(), opt.state[p]["momentum_buffer"].double().numpy()
            assert (np.abs(gb - bw) <= E22 * (np.abs(bw) + np.abs(dw))).all(), ("buf", it, (np.abs(gb - bw) / (np.abs(bw) + np.abs(dw))).max())
            assert (np.abs(gp - pw) <= E22 * (np.abs(pw) + lrf * np.abs(bw))).all(), ("p", it, (np.abs(gp - pw) / (np.abs(pw) + lrf * np.abs(bw))).max())
        coefs.append(st["clip_coef"])
    return coefs


def test_restatement_matches_torch():
    """Two steps of clip_grad_norm_ + SGD(0.01, 0.9, 1e-4) on mixed sizes: total_norm and clip_coef within 1e-6 relative (torch forms
    them in fp32), parameters and momentum within the 2^-22 bars of test_sgd_step."""
    n_all = math.sqrt(sum(int(np.prod(s)) for s in SHAPES))
    coefs = _two_steps_against_torch(0.7 * n_all, 1.0, 11)           # gradients of rms ~1.2: the clip is active
    assert all(0.5 < c < 1.0 for c in coefs), coefs


def test_restatement_inert_and_strong_clip():
    n_all = math.sqrt(sum(int(np.prod(s)) for s in SHAPES))
    assert _two_steps_against_torch(10.0 * n_all, 1.0, 12) == [1.0, 1.0]
    assert all(c < 0.5 for c in _two_steps_against_torch(0.25 * n_all, 1.0, 13))
    assert _two_steps_against_torch(float("inf"), 1.0, 14) == [1.0, 1.0]


def test_restatement_grad_scale_and_nonfinite():
    ps, grads = _tensors(15, 1.0)
    gs = [g.numpy() for g in grads()]
    g8 = [g * np.float32(8.0) for g in gs]                           # (exact: a power of two)
    assert R.total_norm(g8, 1.0 / 8) == R.total_norm(gs, 1.0)
    # the averaged gradients are what is clipped: the same step from eightfold gradients at scale 1/8
    p0, b0 = [p.numpy() for p in ps], [np.zeros(p.shape, np.float32) for p in ps]
    c = 0.5 * R.total_norm(gs)
    a, b = R.step(p0, gs, b0, LR, MOM, WD, 1.0, c), R.step(p0, g8, b0, LR, MOM, WD, 1.0 / 8, c)
    assert a[3] == b[3] and 0.49 < a[3]["clip_coef"] < 0.51
    assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    # no clip: max_norm None, 0 and negative
    assert [R.clip_coef(3.0, v) for v in (None, 0.0, -1.0)] == [1.0, 1.0, 1.0] and R.clip_coef(3.0, float("inf")) == 1.0
    # a non-finite element: torch's arithmetic as written (coef = c / inf = 0, or NaN), or the step skipped
    for bad in (float("inf"), float("nan")):
        gb = [g.copy() for g in gs]
        gb[3][5] = bad
        norm = R.total_norm(gb)
        assert not np.isfinite(norm)
        coef = R.clip_coef(norm, c)
        assert (coef == 0.0) if bad == float("inf") else math.isnan(coef)
        p1, b1, _, st = R.step(p0, gb, b0, LR, MOM, WD, 1.0, c)
        assert not st["skipped"] and np.isnan(p1[3][5]) and np.isnan(b1[3][5])
        assert np.isnan(p1[0]).all() == math.isnan(coef)
        p2, b2, d2, st = R.step(p0, gb, b0, LR, MOM, WD, 1.0, c, skip_nonfinite=True)
        assert st["skipped"] and d2 is None and all(np.array_equal(x, y) for x, y in zip(p2 + b2, p0 + b0))
        params = [torch.nn.Parameter(p.clone()) for p in ps]
        for p, g_ in zip(params, gb):
            p.grad = torch.from_numpy(g_.copy())
        nt = float(torch.nn.utils.clip_grad_norm_(params, c))
        assert (nt == norm) or (math.isnan(nt) and math.isnan(norm))
        assert np.array_equal(np.isnan(params[0].grad.numpy()), np.isnan(coef * gb[0]))


# ------------------------------------------------------------------------------------------------ Python surface
def test_train_step_validates_max_grad_norm():
    from radar_depth_amd.main import HipTrainStep
    par = inspect.signature(HipTrainStep.__init__).parameters
    names = list(par)
    assert names[names.index("berhu_thresh") + 1:] == ["max_grad_norm", "skip_nonfinite"]
    assert par["max_grad_norm"].default is None and par["skip_nonfinite"].default is False
    for v in (0, -1, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):         # before the model or the GPU is touched
            HipTrainStep(None, 1, 8, 8, max_grad_norm=v)
    for v in (float("inf"), None, 2.5):                                # pass validation: the None model is what stops them
        with pytest.raises(AttributeError):
            HipTrainStep(None, 1, 8, 8, max_grad_norm=v)
    assert HipTrainStep._checked_max_grad_norm(float("inf")) == float("inf") and HipTrainStep._checked_max_grad_norm(None) is None
    assert HipTrainStep._checked_max_grad_norm(3) == 3.0


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def _header_signature(hdr, name):
    """'<ret>:<args>' of a declaration in the header, in the type characters of the prototype table (csrc/abi.cpp)"""
    m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, hdr, re.M)
    assert m, name

    def code(t):
        t = t.strip()
        if "*" in t:
            return "p"
        return {"int64_t": "l", "int32_t": "i", "int": "i", "float": "f", "double": "d"}[t.split()[0]]
    return code(m.group(1)) + ":" + "".join(code(a) for a in m.group(2).split(","))


def test_abi_lists_the_three_entries(L):
    table = dict(L.rd_abi_entry(i).decode().split(" ") for i in range(L.rd_abi_entries()))
    hdr = open(os.path.join(ROOT, "include", "radar_depth_hip.h")).read()
    want = {"rd_grad_sumsq_partials": "i:l", "rd_grad_sumsq": "i:plpp", "rd_sgd_step_clip": "i:ppplffffdipipp"}
    for name, sig in want.items():
        assert table[name] == sig == _header_signature(hdr, name), name
        assert len(getattr(L, name).argtypes) == len(sig.split(":")[1])
    assert _header_signature(hdr, "rd_sgd_step") == table["rd_sgd_step"] == "i:ppplffffip"          # the parser reads an old one right
    # the two launchable ones are replayable by the op table (and so capturable)
    assert L.rd_optable_entry_args(b"rd_grad_sumsq") == 4 and L.rd_optable_entry_args(b"rd_sgd_step_clip") == 14
    # one partial per workgroup: the reductions' grid of n alone (256 threads x 8 elements, at most 1024 workgroups)
    got = [L.rd_grad_sumsq_partials(n) for n in (1, 2048, 2049, 2 * 256 * 8 * 1024 + 5, 14710752, 1 << 33, 0, -4)]
    assert got == [1, 1, 2, 1024, 1024, 1024, 0, 0] and L.rd_grad_sumsq_partials(14710752) == L.rd_loss_tiles(14710752)


def test_abi_rejects_bad_arguments_without_gpu(L):
    """Null pointers, a misaligned pointer and a wrong n_partials are refused before anything reaches the GPU (host dummies: never followed)."""
    big = C.create_string_buffer(1 << 12)
    base = (C.addressof(big) + 15) & ~15
    opt = lambda v: None if v is None else C.c_void_p(base + v)        # noqa: E731
    n = 64

    def sumsq(g=0, part=1024, n=n):
        return L.rd_grad_sumsq(opt(g), n, opt(part), None)

    def clip(p=0, g=256, buf=512, part=1024, stats=1280, n=n, n_part=1):
        return L.rd_sgd_step_clip(opt(p), opt(g), opt(buf), n, 0.01, 0.9, 1e-4, 1.0, 1.0, 0, opt(part), n_part, opt(stats), None)

    assert [sumsq(g=None), sumsq(part=None), sumsq(n=0), sumsq(g=4), sumsq(part=1032)] == [-1] * 5
    assert b"grad_sumsq" in L.rd_last_error()
    assert [clip(p=None), clip(g=None), clip(buf=None), clip(part=None), clip(stats=None), clip(n=0)] == [-1] * 6
    assert [clip(p=4), clip(g=260), clip(buf=520), clip(part=1032), clip(stats=1288)] == [-1] * 5 and b"16-byte" in L.rd_last_error()
    assert [clip(n_part=0), clip(n_part=2), clip(n_part=1024)] == [-1] * 3 and b"n_partials" in L.rd_last_error()

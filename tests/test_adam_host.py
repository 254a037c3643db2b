"""Adam / AdamW kernels, without a GPU: the measurement of the bars (torch.optim.Adam / AdamW on the CPU in fp32 against the float64
evaluation, tests/adam_ref.py), the numpy restatement against torch over a trajectory and at the edges, and the two entry points in the
compiled prototype table, the header and the op table (nothing is launched).

Bars: measure_bars() gives the reference's own fp32 error per output, normalised by the magnitudes entering the output's last operation;
everything of this project (the restatement here, the kernels in tests/test_gpu_adam.py) is held to twice that, the factor covering an
equally valid order of operations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (3,), (16, 3, 7, 7), (64,), (5, 13), (1003,), (129, 31)]          # the clip host test's seven tensors: 1 .. 3999 elements
U = 2.0 ** -24


def test_bars_are_the_references_own_error():
    rows, worst = A.measure_bars()
    for case, e_torch, e_rest in rows:
        print("%-5s t=%-4d wd=%-5g  torch p %.3e m %.3e v %.3e   restatement p %.3e m %.3e v %.3e" % (case + e_torch + e_rest))
    print("worst of torch (p, m, v): %.3e %.3e %.3e = %.2f %.2f %.2f x 2^-24; the bars are twice those"
          % (worst + tuple(w / U for w in worst)))
    # each output's last operation alone rounds once (2^-24 of a result no larger than its normaliser): a measurement far outside
    # [2^-26, 8 x 2^-24] would mean the normalisation or the float64 evaluation is wrong, not that torch is
    assert all(U / 4 < w < 8 * U for w in worst), worst
    bars = A.bars()
    for case, _, e_rest in rows:
        assert all(e <= b for e, b in zip(e_rest, bars)), (case, e_rest, bars)


def _torch_optimizer(mode, params, wd, **hp):
    cls = torch.optim.Adam if mode == "adam" else torch.optim.AdamW
    return cls(params, weight_decay=wd, foreach=False, fused=False, **hp)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("mode", ["adam", "adamw"])
def test_restatement_follows_torch_over_five_steps(mode, wd):
    """Both run in fp32 from the same start and keep their own state, so the bars accumulate: per step each of the two is entitled to one
    bar against the float64 evaluation of its own state (torch's fused multiply-adds are "an equally valid order"), so two bars of the
    step's normalisers are added per step to an absolute allowance per element, which the update itself carries on to first order:
        am = beta1 am + omb1 dg + 2 bar_m (|m0| + |g|)
        av = beta2 av + 2 omb2 |g| dg + 2 bar_v (|v0| + g^2)
        ap = ap + 2 bar_p (|p0| + step |m| / d) + step (am / d + |m| / d^2 * av / (2 sqrt(v) bc2s))
    dg, coupled weight decay only (g = s grad + wd p depends on p and is itself rounded): wd ap + 2^-24 (|s grad| + |wd p|) -- the
    product and the sum round once each here, the sum once in torch's fused form, half an ulp each; where the two terms cancel, or on
    the empty state of a first step, nothing of |m0| + |g| covers that.  An allowance relative to the step's own normalisers alone
    would be wrong too: after a large gradient m0 is a tenth of what entered it."""
    r = np.random.RandomState(5)
    ps = [(np.where(r.rand(*s) < 0.5, -1.0, 1.0) * r.uniform(0.25, 2.0, s)).astype(np.float32) for s in SHAPES]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = _torch_optimizer(mode, params, wd, **A.HP)
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    allow = [[np.zeros(s), np.zeros(s), np.zeros(s)] for s in SHAPES]            # ap, am, av
    blk = A.new_block(weight_decay=wd, **A.HP)
    bp, bm, bv = (2.0 * b for b in A.bars())
    worst = [0.0, 0.0, 0.0]
    for k in range(1, 6):
        gs = [(np.where(r.rand(*s) < 0.5, -1.0, 1.0) * 10.0 ** r.uniform(-6.0, 2.0, s)).astype(np.float32) for s in SHAPES]
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g.copy())
        before = [(p.detach().double().numpy().copy(),) for p in params]
        opt.step()
        A.prepare(blk)
        assert blk[A.W_T] == k
        omb1, beta2, omb2, bc2s, step = (blk[i] for i in (A.W_OMB1, A.W_BETA2F, A.W_OMB2, A.W_BC2S, A.W_STEP))
        for i, (p, g) in enumerate(zip(params, gs)):
            ref = A.step_f64(ps[i], g, ms[i], vs[i], blk, mode)
            ps[i], ms[i], vs[i] = A.step_f32(ps[i], g, ms[i], vs[i], blk, mode)
            ap, am, av = allow[i]
            dg = wd * ap + U * (np.abs(blk[A.W_S] * g.astype(np.float64)) + np.abs(wd * before[i][0])) if mode == "adam" and wd else 0.0
            am = (1.0 - omb1) * am + omb1 * dg + bm * ref["nm"]
            av = beta2 * av + 2.0 * omb2 * np.abs(ref["g"]) * dg + bv * ref["nv"]
            root = np.maximum(np.sqrt(ref["v"]), 1e-300)
            ap = ap + bp * ref["np_"] + step * (am / ref["d"] + np.abs(ref["m"]) / ref["d"] ** 2 * av / (2.0 * root * bc2s))
            allow[i] = [ap, am, av]
            st = opt.state[p]
            assert float(st["step"]) == blk[A.W_T]
            got = (ps[i], ms[i], vs[i])
            tor = (p.detach().double().numpy(), st["exp_avg"].double().numpy(), st["exp_avg_sq"].double().numpy())
            for j, (a, b, tol) in enumerate(zip(got, tor, allow[i])):
                ratio = float((np.abs(a.astype(np.float64) - b) / tol).max())
                worst[j] = max(worst[j], ratio)
                assert ratio <= 1.0, (mode, wd, k, SHAPES[i], "pmv"[j], ratio)
    print("%s wd=%g: worst distance to torch over five steps, in accumulated allowances (p, m, v): %.3f %.3f %.3f" % ((mode, wd) + tuple(worst)))


def test_large_t_corrections_underflow_to_one():
    """t = 8000 multiplications with betas (0.9, 0.9): both running products underflow (they come to rest at a few units of the smallest
    denormal, where x * 0.9 rounds back to x; torch's beta ** step gives 0), both corrections are exactly 1, step_size is lr and bc2s 1."""
    hp = dict(lr=1e-3, betas=(0.9, 0.9), eps=1e-8)
    blk = A.new_block(t=8000, **hp)
    assert blk[A.W_T] == 8000 and 0.0 <= blk[A.W_B1T] == blk[A.W_B2T] < 1e-320
    mid = A.new_block(t=400, **hp)                       # 0.9^400 = 5e-19 < 2^-53: not zero, but 1 - it is 1
    assert 0.0 < mid[A.W_B1T] < 2.0 ** -53 and 1.0 - mid[A.W_B1T] == 1.0
    A.prepare(mid)
    A.prepare(blk)
    for b in (mid, blk):
        assert b[A.W_STEP] == float(np.float32(1e-3)) and b[A.W_BC2S] == 1.0
    assert blk[A.W_T] == 8001 and 0.0 <= blk[A.W_B1T] < 1e-320
    p, g, m, v = A.random_state(4001, 9, 8000)
    ref = A.step_f64(p, g, m, v, blk, "adam")
    got = A.step_f32(p, g, m, v, blk, "adam")
    tor = A.torch_one_step(p, g, m, v, "adam", 8000, 0.0, **hp)
    assert all(np.isfinite(a).all() for a in got)
    e_got, e_tor = A.errors(*got, ref), A.errors(*tor, ref)
    print("t = 8000: restatement %s torch %s" % (e_got, e_tor))
    assert all(e <= b for e, b in zip(e_got, A.bars())) and all(e <= b for e, b in zip(e_tor, A.bars()))


@pytest.mark.parametrize("mode", ["adam", "adamw"])
def test_eps_zero_and_v_zero_is_nan_as_in_torch(mode):
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=0.0)
    p, g, m, v = A.random_state(9, 11, 0)
    for i in (0, 4, 8):
        g[i] = m[i] = v[i] = 0.0                         # d = sqrt(0) / bc2s + 0 = 0 and m / d = 0 / 0
    blk = A.prepare(A.new_block(**hp))
    got = A.step_f32(p, g, m, v, blk, mode)
    tor = A.torch_one_step(p, g, m, v, mode, 0, 0.0, **hp)
    want = np.zeros(9, bool)
    want[[0, 4, 8]] = True
    assert np.array_equal(np.isnan(got[0]), want) and np.array_equal(np.isnan(tor[0]), want)
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all() and (got[2][want] == 0).all()
    ref = A.step_f64(p, g, m, v, blk, mode)
    assert all(e <= b for e, b in zip(A.errors(*got, ref), A.bars()))


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_abi_lists_the_two_entries(L):
    from test_grad_clip_host import _header_signature
    table = dict(L.rd_abi_entry(i).decode().split(" ") for i in range(L.rd_abi_entries()))
    hdr = open(os.path.join(ROOT, "include", "radar_depth_hip.h")).read()
    want = {"rd_adam_prepare": "i:plfdipipp", "rd_adam_step": "i:pppplipp"}
    for name, sig in want.items():
        assert table[name] == sig == _header_signature(hdr, name), name
        assert len(getattr(L, name).argtypes) == len(sig.split(":")[1])
        assert L.rd_optable_entry_args(name.encode()) == len(sig.split(":")[1])          # replayable by the op table, and so capturable
    assert "#define RD_ADAM_BLOCK_WORDS %d\n" % A.BLOCK_WORDS in hdr
    assert "#define RD_ADAM 0\n" in hdr and "#define RD_ADAMW 1\n" in hdr and A.MODES == {"adam": 0, "adamw": 1}


def test_abi_rejects_bad_arguments_without_gpu(L):
    """Null pointers, misaligned pointers, n < 1, an unknown mode and a wrong n_partials are refused before anything reaches the GPU
    (host dummies: never followed)."""
    big = C.create_string_buffer(1 << 12)
    base = (C.addressof(big) + 15) & ~15
    opt = lambda v: None if v is None else C.c_void_p(base + v)        # noqa: E731
    n = 64

    def prep(blk=0, part=1024, stats=1280, n=n, n_part=1):
        return L.rd_adam_prepare(opt(blk), n, 1.0, 1.0, 0, opt(part), n_part, opt(stats), None)

    def step(p=0, g=256, m=512, v=768, blk=1024, n=n, mode=0):
        return L.rd_adam_step(opt(p), opt(g), opt(m), opt(v), n, mode, opt(blk), None)

    assert [prep(blk=None), prep(part=None), prep(stats=None), prep(n=0), prep(n=-3), prep(part=None, stats=None, n_part=0, n=0)] == [-1] * 6
    assert b"rd_adam_prepare" in L.rd_last_error()
    assert [prep(blk=8), prep(part=1032), prep(stats=1288)] == [-1] * 3 and b"16-byte" in L.rd_last_error()
    assert [prep(n_part=0), prep(n_part=2), prep(n_part=1024), prep(part=None, stats=None, n_part=1)] == [-1] * 4
    assert b"rd_adam_prepare" in L.rd_last_error()
    assert prep(n_part=2, n=2049 - 1) == -1 and b"n_partials" in L.rd_last_error()
    assert [step(p=None), step(g=None), step(m=None), step(v=None), step(blk=None), step(n=0)] == [-1] * 6 and b"rd_adam_step" in L.rd_last_error()
    assert [step(p=4), step(g=260), step(m=520), step(v=772), step(blk=1032)] == [-1] * 5 and b"16-byte" in L.rd_last_error()
    assert [step(mode=2), step(mode=-1)] == [-1] * 2 and b"mode" in L.rd_last_error() and b"rd_adam_step" in L.rd_last_error()

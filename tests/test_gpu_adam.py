"""Adam / AdamW on the GPU at kernel level: rd_adam_prepare and rd_adam_step through the C ABI, bit for bit against the numpy restatement
and within the measured bars of float64 (tests/adam_ref.py), with and without the norm pass, over skipped steps, and the refusals.

Bars: twice the error of torch's own fp32 step against float64 (adam_ref.measure_bars: about 4.0, 1.9 and 3.9 x 2^-24 for p, m, v
relative to the magnitudes entering each output's last operation)."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as A  # noqa: E402
import grad_clip_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
CANARY = -777.25
NS = [1, 2, 3, 4, 5, 1003, 4096, A.BAR_SAMPLES]      # the last: 1048577 16-byte words on 256 x 4096 lanes, a second grid-stride trip, and a tail
MODES = ["adam", "adamw"]


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
    return None if t is None else C.c_void_p(t.data_ptr() + byte_off)


def _arena(x):
    n = x.size
    a = torch.full((((n + 3) // 4) * 4 + 8,), CANARY, device=DEV)         # >= 4 floats of canary past n
    a[:n] = torch.from_numpy(x).to(DEV)
    return a


@functools.lru_cache(maxsize=None)
def _case(n):
    """Shared and never modified: fp32 p, grad, m, v on the host and as arenas with canaries past n, the gradients' float64 sum of squares"""
    p, g, m, v = A.random_state(n, 700 + n % 1000, 0)
    return dict(n=n, p=p, g=g, m=m, v=v, P=_arena(p), G=_arena(g), M=_arena(m), V=_arena(v), S=R.sumsq(g))


def _block(words):
    b = torch.full((A.BLOCK_WORDS + 2,), CANARY, dtype=torch.float64, device=DEV)
    b[:A.BLOCK_WORDS] = torch.from_numpy(words).to(DEV)
    return b


def _prepare(blk, n, gs=1.0, max_norm=0.0, skip=0, part=None, k=0, stats=None):
    _ok(_L().rd_adam_prepare(_p(blk), n, gs, max_norm, skip, _p(part), k, _p(stats), _st()), "rd_adam_prepare")


def _step(P, G, M, V, n, mode, blk):
    _ok(_L().rd_adam_step(_p(P), _p(G), _p(M), _p(V), n, A.MODES[mode], _p(blk), _st()), "rd_adam_step")


def _sumsq(G, n):
    k = _L().rd_grad_sumsq_partials(n)
    part = torch.full((k + 2,), CANARY, dtype=torch.float64, device=DEV)
    _ok(_L().rd_grad_sumsq(_p(G), n, _p(part), _st()), "rd_grad_sumsq")
    return part, k


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _assert_bits(c, P, M, V, blk, p, m, v, words, what):
    """the three arenas and the block against the restatement, bit for bit; canaries intact"""
    n = c["n"]
    torch.cuda.synchronize()
    for name, dev, host in (("p", P, p), ("m", M, m), ("v", V, v)):
        got = dev[:n].cpu().numpy()
        diff = _bits(got) != _bits(host)
        assert not diff.any(), (what, name, int(diff.sum()), "first at", int(np.argmax(diff)), got[np.argmax(diff)], host[np.argmax(diff)])
        assert bool((dev[n:] == CANARY).all()), (what, name, "wrote past n")
    got = blk.cpu().numpy()
    assert (_bits(got[:A.BLOCK_WORDS]) == _bits(words)).all(), (what, "block", got[:A.BLOCK_WORDS], words)
    assert (got[A.BLOCK_WORDS:] == CANARY).all(), (what, "wrote past the block")


def _assert_bars(P, M, V, n, ref, what):
    e = A.errors(P[:n].cpu().numpy(), M[:n].cpu().numpy(), V[:n].cpu().numpy(), ref)
    bars = A.bars()
    print("%s n=%d: p %.3e m %.3e v %.3e  (bars %.3e %.3e %.3e)" % ((what, n) + e + bars))
    assert all(x <= b for x, b in zip(e, bars)), (what, e, bars)


# ------------------------------------------------------------------------------------------------ rd_adam_prepare + rd_adam_step
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", NS)
def test_adam_bit_for_bit_and_within_the_bars(n, mode, wd):
    c = _case(n)
    P, M, V, G = c["P"].clone(), c["M"].clone(), c["V"].clone(), c["G"].clone()
    words = A.new_block(weight_decay=wd, **A.HP)
    blk = _block(words)
    p, m, v = c["p"], c["m"], c["v"]
    first = None
    for call in (1, 2, 3):
        _prepare(blk, n)
        _step(P, G, M, V, n, mode, blk)
        A.prepare(words)
        ref = A.step_f64(p, c["g"], m, v, words, mode)
        p, m, v = A.step_f32(p, c["g"], m, v, words, mode)
        if call in (1, 3):
            what = "%s wd=%g call %d" % (mode, wd, call)
            _assert_bits(c, P, M, V, blk, p, m, v, words, what)
            _assert_bars(P, M, V, n, ref, what)
            assert words[A.W_T] == call
        if call == 1:
            first = (P.clone(), M.clone(), V.clone(), blk.clone())
    assert torch.equal(G, c["G"]), "the gradient arena is read-only"
    # a second run of the first call: the same bits
    P, M, V, blk = c["P"].clone(), c["M"].clone(), c["V"].clone(), _block(A.new_block(weight_decay=wd, **A.HP))
    _prepare(blk, n)
    _step(P, G, M, V, n, mode, blk)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((P, M, V, blk), first)), "two runs must give the same bits"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", NS)
def test_clip_coefficient(n, mode):
    c = _case(n)
    wd, gs = 1e-2, 0.5
    norm = R._f32(gs) * math.sqrt(c["S"])
    part, k = _sumsq(c["G"], n)

    def run(**kw):
        P, M, V, blk = c["P"].clone(), c["M"].clone(), c["V"].clone(), _block(A.new_block(weight_decay=wd, **A.HP))
        _prepare(blk, n, gs, **kw)
        _step(P, c["G"], M, V, n, mode, blk)
        torch.cuda.synchronize()
        return P, M, V, blk

    base = run()                                                      # no norm pass at all
    for max_norm in (4.0 * norm + 1.0, float("inf"), 0.0):            # a coefficient of 1: the unclipped call's bits
        stats = torch.zeros(4, dtype=torch.float64, device=DEV)
        got = run(max_norm=max_norm, part=part, k=k, stats=stats)
        assert all(torch.equal(a, b) for a, b in zip(got, base)), max_norm
        st = stats.tolist()
        assert st[1:] == [1.0, 0.0, 0.0] and abs(st[0] - norm) <= 1e-12 * norm, st
    max_norm = 0.3 * norm
    want = R.clip_coef(norm, max_norm)
    assert 0.0 < want < 0.31 and (want > 0.29 or norm < 1e-3)          # (the 1e-6 in the quotient: a single tiny gradient at n = 1 gives less)
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    P, M, V, blk = run(max_norm=max_norm, part=part, k=k, stats=stats)
    st = stats.tolist()
    assert abs(st[0] - norm) <= 1e-12 * norm and st[2:] == [0.0, 0.0], st
    assert abs(st[1] - want) <= float(np.spacing(np.float32(want))) and st[1] == float(np.float32(st[1])), (st[1], want)      # the clip test's
    words = A.prepare(A.new_block(weight_decay=wd, **A.HP), gs, st[1])
    assert words[A.W_S] == R.scale(gs, st[1])
    ref = A.step_f64(c["p"], c["g"], c["m"], c["v"], words, mode)
    p, m, v = A.step_f32(c["p"], c["g"], c["m"], c["v"], words, mode)
    _assert_bits(c, P, M, V, blk, p, m, v, words, "active clip")
    _assert_bars(P, M, V, n, ref, "%s active clip, s = %.9g" % (mode, words[A.W_S]))
    assert blk[A.W_S].item() < base[3][A.W_S].item() == 0.5 and not torch.equal(V, base[2])          # the clipped gradient entered the update
    assert torch.equal(part[k:], torch.full((2,), CANARY, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("n", NS)
def test_nonfinite_step_is_skipped_whole(n):
    c = _case(n)
    mode, wd = "adamw", 1e-2
    norm = math.sqrt(c["S"])
    max_norm = 0.3 * norm
    part_ok, k = _sumsq(c["G"], n)
    start = A.new_block(weight_decay=wd, t=2, **A.HP)
    # a run that never sees a bad step
    P0, M0, V0, blk0, st0 = c["P"].clone(), c["M"].clone(), c["V"].clone(), _block(start), torch.zeros(4, dtype=torch.float64, device=DEV)
    _prepare(blk0, n, 1.0, max_norm, 1, part_ok, k, st0)
    _step(P0, c["G"], M0, V0, n, mode, blk0)
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)         # one statistics block through the whole test: the skip count only grows
    skipped = 0
    for bad in (float("inf"), float("nan")):
        for pos in sorted({0, n // 2, n - 1}):                      # the last element is in the n & 3 tail for n = 1003, 5 and 4194309
            G = c["G"].clone()
            G[pos] = bad
            part, _ = _sumsq(G, n)
            P, M, V, blk = c["P"].clone(), c["M"].clone(), c["V"].clone(), _block(start)
            _prepare(blk, n, 1.0, max_norm, 1, part, k, stats)
            _step(P, G, M, V, n, mode, blk)
            torch.cuda.synchronize()
            skipped += 1
            st = stats.tolist()
            assert torch.equal(P, c["P"]) and torch.equal(M, c["M"]) and torch.equal(V, c["V"]), (bad, pos)
            want = start.copy()
            want[A.W_SKIP] = 1.0                                     # the one word a skipped step writes
            assert (_bits(blk[:A.BLOCK_WORDS].cpu().numpy()) == _bits(want)).all(), (bad, pos, blk)
            assert st[2] == float(skipped) and st[3] == 1.0 and not math.isfinite(st[0]), (bad, pos, st)
            # the next, finite call equals the run that never saw the bad step
            _prepare(blk, n, 1.0, max_norm, 1, part_ok, k, stats)
            _step(P, c["G"], M, V, n, mode, blk)
            torch.cuda.synchronize()
            st = stats.tolist()
            assert st[2] == float(skipped) and st[3] == 0.0 and st[:2] == st0.tolist()[:2], (bad, pos, st)
            assert torch.equal(P, P0) and torch.equal(M, M0) and torch.equal(V, V0) and torch.equal(blk, blk0), (bad, pos)
    assert blk0[A.W_T].item() == 3.0 and not torch.equal(P0, c["P"])


def test_adam_rejects_bad_arguments():
    L = _L()
    n = 64
    t = [torch.full((n + 8,), CANARY, device=DEV) for _ in range(4)]
    blk = _block(A.new_block(**A.HP))
    blk0 = blk.clone()
    k = L.rd_grad_sumsq_partials(n)
    part = torch.full((k + 2,), CANARY, dtype=torch.float64, device=DEV)
    stats = torch.full((6,), CANARY, dtype=torch.float64, device=DEV)

    def step(offs=(0, 0, 0, 0, 0), n=n, mode=0):
        return L.rd_adam_step(_p(t[0], offs[0]), _p(t[1], offs[1]), _p(t[2], offs[2]), _p(t[3], offs[3]), n, mode, _p(blk, offs[4]), _st())

    def prep(offs=(0, 0, 0), n=n, n_part=k, with_part=True):
        return L.rd_adam_prepare(_p(blk, offs[0]), n, 1.0, 1.0, 1, _p(part, offs[1]) if with_part else None, n_part,
                                 _p(stats, offs[2]) if with_part else None, _st())

    for i in range(5):
        offs = [0] * 5
        offs[i] = 4 if i < 4 else 8
        assert step(offs) == EINVAL, "pointer %d misaligned must be rejected" % i
    assert [step(n=0), step(n=-1), step(mode=2), step(mode=-1)] == [EINVAL] * 4 and b"rd_adam_step" in L.rd_last_error()
    for i in range(3):
        offs = [0] * 3
        offs[i] = 8
        assert prep(offs) == EINVAL, "pointer %d misaligned must be rejected" % i
    assert [prep(n=0), prep(n_part=k + 1), prep(n_part=0), prep(with_part=False)] == [EINVAL] * 4 and b"rd_adam_prepare" in L.rd_last_error()
    torch.cuda.synchronize()
    assert all(bool((x == CANARY).all()) for x in t + [part, stats]) and torch.equal(blk, blk0), "a refused call writes nothing"
    assert prep(n_part=0, with_part=False) == 0
    torch.cuda.synchronize()
    assert blk[A.W_T].item() == 1.0 and bool((stats == CANARY).all())

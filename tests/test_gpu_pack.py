"""Bit-for-bit GPU tests of the kernels that produce what the matrix kernels consume -- rd_pack_weights, rd_pack_weights_bf16,
rd_pack_weights_batched (csrc/layout.hip), rd_wino_pack[_batched] (csrc/wino_split.hip) -- and of rd_bn_eval_coeffs[_batched]
(csrc/norm_act.hip), rd_nchw_to_nhwc / rd_nhwc_to_nchw and rd_fill, against tests/pack_ref.py, the numpy restatement of the header.

Every pack is a permutation, a correctly rounded conversion or a short chain of fp64 / fp32 steps numpy repeats exactly: the comparisons
are array_equal on the bits, over the WHOLE destination -- filled with a sentinel first, guards on either side -- so an element the job
does not own (columns beyond its range, the rows of other jobs, the other planes, the guards) must still hold the sentinel.  The eval
coefficients are held to two derived bars (pack_ref.coeff_bars); single and batched must agree in every bit.

The operands are those of tests/pack_cases.py; tests/test_pack_host.py shows that each shortcut of pack_ref.MODES changes one of them."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_cases as PC
import pack_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
G = PC.GUARD


def _L():
    from radar_depth_amd._lib import lib
    return lib()


def _st():
    from radar_depth_amd._lib import current_stream
    return current_stream()


def _dev(a):
    """numpy array -> device tensor with the same bits (uint32 / uint16 travel as int32 / int16)."""
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def _bits(t):
    a = t.detach().cpu().contiguous()
    if a.dtype == torch.bfloat16:
        a = a.view(torch.int16)
    if a.dtype == torch.float32:
        a = a.view(torch.int32)
    n = a.numpy()
    return n.view({2: np.uint16, 4: np.uint32}[n.dtype.itemsize]).reshape(-1)


def _p(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _sentinel(j):
    wide = j["quad"] in (0, 1)
    return np.full(PC.buffer_elems(j) + 2 * G, PC.SENT32 if wide else PC.SENT16, dtype=np.uint32 if wide else np.uint16)


def _single(j, w_dev, dst, plane=0):
    """One single-tensor launch for job j (quad 1: rd_pack_weights, quad 2: rd_pack_weights_bf16) into dst behind its guard."""
    fn = _L().rd_pack_weights if j["quad"] == 1 else _L().rd_pack_weights_bf16
    return fn(_p(w_dev), _p(dst, G + plane), j["O"], j["I"], j["k"], j["k"], j["ldc"], j["off"], j["rows_total"], j["transpose"], _st())


# ------------------------------------------------------------------------------------------------ single-tensor kernels
@pytest.mark.parametrize("shape", PC.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("transpose", [0, 1], ids=["forward", "transposed"])
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_single_tensor_pack(kind, transpose, shape):
    """Tight and padded geometry of every shape.  (8, 4, 1) forward with rd_pack_weights_bf16 is a refusal, not a pack: I = 4 reduction
    rows are no multiple of the bf16 layout's eight, so the call must return RD_EINVAL and leave the sentinel-filled buffer alone."""
    for j in PC.single_case(kind, transpose, shape):
        want = _sentinel(j) if j["refused"] else PC.expected([j])[j["buf"]]          # (the restatement also asserts that the job stays inside)
        dst = _dev(_sentinel(j))
        rc = _single(j, _dev(j["w"]), dst)
        torch.cuda.synchronize()
        if j["refused"]:          # the reduction rows are no multiple of the interleave: refused, nothing written
            assert rc == -1 and b"multiple of" in _L().rd_last_error()
        else:
            assert rc == 0, _L().rd_last_error()
        assert np.array_equal(_bits(dst), want), (j["buf"], int((_bits(dst) != want).sum()))


@pytest.mark.parametrize("transpose", [0, 1], ids=["forward", "transposed"])
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_single_tensor_pack_concatenation(kind, transpose):
    jobs = PC.concat_case(kind, transpose)
    want = PC.expected(jobs)["cat"]
    dst = _dev(_sentinel(jobs[0]))
    for j in jobs:
        assert _single(j, _dev(j["w"]), dst) == 0, _L().rd_last_error()
    torch.cuda.synchronize()
    assert (want[G:-G] == want[0]).any()                       # columns 24 .. 39 / nothing here: somebody's absence is part of the check
    assert np.array_equal(_bits(dst), want)


# ------------------------------------------------------------------------------------------------ the batched kernel
def test_batched_pack_one_launch_every_layout_path_and_fold():
    L = _L()
    jobs = PC.batched_jobs()
    want = PC.expected(jobs)
    chunk = L.rd_pack_chunk()
    first, table = R.block_table([R.pack_blocks(j["O"], j["I"], j["T"], chunk) for j in jobs])
    dst = {}
    for j in jobs:
        if j["buf"] not in dst:
            dst[j["buf"]] = _dev(_sentinel(j))
    keep, recs = [], []
    for j, fb in zip(jobs, first):
        w, s = _dev(j["w"]), (_dev(j["scale"]) if j["scale"] is not None else None)
        keep += [w, s]
        recs.append(R.PackJob(w.data_ptr(), _p(dst[j["buf"]], G).value, s.data_ptr() if s is not None else None, j["O"], j["I"], j["T"], j["ldc"],
                              j["off"], j["rows_total"], j["transpose"], fb, j["quad"], j["scale_col"]))
    assert all(fb != 0 for fb in first[1:]) and len(table) > len(jobs)
    # (a unit-path job whose block count, sized for the element-wise form, exceeds the blocks its units fill: the surplus must do nothing)
    assert any(PC.takes_unit_path(j) and R.pack_blocks(j["O"], j["I"], j["T"], chunk) > -(-(PC.rows(j) // 8 * j["ldc"]) // 256) for j in jobs)
    recs_dev, table_dev = _dev(R.records(recs)), _dev(table)          # (named: both stay allocated until the launch has run)
    rc = L.rd_pack_weights_batched(_p(recs_dev), _p(table_dev), len(table), _st())
    assert rc == 0, L.rd_last_error()
    torch.cuda.synchronize()
    got = {k: _bits(t) for k, t in dst.items()}
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    # jobs with no fold: the single-tensor kernels write the same bits (quad 3: the pieces, each bf16-representable, packed plane by plane)
    seen = set()
    for j in jobs:
        if j["fold"] != "none" or j["quad"] == 0:
            continue
        one = _dev(_sentinel(j))
        if j["quad"] == 3:
            plane = R.plane_elems(j["T"], PC.rows(j), j["ldc"])
            for p, piece in enumerate(R.split3(j["w"])):
                assert _single(dict(j, quad=2), _dev(R.bf16_to_f32(piece)), one, p * plane) == 0, L.rd_last_error()
        else:
            assert _single(j, _dev(j["w"]), one) == 0, L.rd_last_error()
        torch.cuda.synchronize()
        idx = PC.owned(j)
        assert np.array_equal(_bits(one)[idx], got[j["buf"]][idx]), j["buf"]
        seen.add((j["quad"], PC.takes_unit_path(j)))
    assert seen >= {(1, False), (2, True), (2, False), (3, True), (3, False)}


# ------------------------------------------------------------------------------------------------ Winograd operands
def test_wino_pack_single_and_batched_are_the_restatement():
    L = _L()
    want = [PC.wino_expected(n) for n in range(len(PC.WINO))]
    ws = [_dev(PC.wino_weights(n)) for n in range(len(PC.WINO))]
    single = [_dev(np.full_like(e, PC.SENT16)) for e in want]
    batched = [_dev(np.full_like(e, PC.SENT16)) for e in want]
    counts = []
    for n, (O, I, flip) in enumerate(PC.WINO):
        assert L.rd_wino_packed_bytes(O, I, flip) == 2 * (want[n].size - 2 * G) == 2 * R.wino_packed_elems(O, I, flip)
        assert L.rd_wino_pack(_p(ws[n]), O, I, flip, _p(single[n], G), _st()) == 0, L.rd_last_error()
        counts.append(L.rd_wino_pack_blocks(O, I, flip))
    assert counts[-1] == 5                                       # (80, 128, flip): two output tiles, five chunks, five blocks
    first, table = R.block_table(counts)
    recs = [R.WinoJob(ws[n].data_ptr(), _p(batched[n], G).value, O, I, flip, first[n]) for n, (O, I, flip) in enumerate(PC.WINO)]
    recs_dev, table_dev = _dev(R.records(recs)), _dev(table)
    assert L.rd_wino_pack_batched(_p(recs_dev), _p(table_dev), len(table), _st()) == 0, L.rd_last_error()
    torch.cuda.synchronize()
    for n in range(len(PC.WINO)):
        s, b = _bits(single[n]), _bits(batched[n])
        assert np.array_equal(s, b), PC.WINO[n]
        assert np.array_equal(s, want[n]), (PC.WINO[n], int((s != want[n]).sum()))


# ------------------------------------------------------------------------------------------------ eval coefficients
def _coeff_check(scale, shift, gamma, beta, rm, rv, eps):
    """-> (largest scale error, largest shift error) in units of their bars; asserts both <= 1."""
    s64, h64 = R.eval_coeffs(gamma, beta, rm, rv, eps)
    bs, bh = R.coeff_bars(s64, h64, rm)
    es = np.abs(scale.astype(np.float64) - s64) / np.maximum(bs, 1e-300)
    eh = np.abs(shift.astype(np.float64) - h64) / np.maximum(bh, 1e-300)
    assert np.isfinite(scale).all() and np.isfinite(shift).all()
    assert es.max() <= 1.0 and eh.max() <= 1.0, (es.max(), eh.max())
    return float(es.max()), float(eh.max())


def test_eval_coeffs_single_equals_batched_and_float64():
    L = _L()
    ins = [PC.eval_inputs(n) for n in range(len(PC.EVAL_C))]
    dev = [[_dev(a) for a in t] for t in ins]
    nan = lambda c: torch.full((c + 2 * G,), float("nan"), device="cuda")
    out1 = [(nan(c), nan(c)) for c in PC.EVAL_C]
    outb = [(nan(c), nan(c)) for c in PC.EVAL_C]
    for c, d, (sc, sh) in zip(PC.EVAL_C, dev, out1):
        assert L.rd_bn_eval_coeffs(c, *[_p(t) for t in d], C.c_float(PC.EPS), _p(sc, G), _p(sh, G), _st()) == 0, L.rd_last_error()
    recs = [R.EvalCoefJob(*[t.data_ptr() for t in d], _p(sc, G).value, _p(sh, G).value, c, 0) for c, d, (sc, sh) in zip(PC.EVAL_C, dev, outb)]
    recs_dev = _dev(R.records(recs))
    assert L.rd_bn_eval_coeffs_batched(_p(recs_dev), len(recs), C.c_float(PC.EPS), _st()) == 0, L.rd_last_error()
    torch.cuda.synchronize()
    worst = [0.0, 0.0]
    for c, t, o1, ob in zip(PC.EVAL_C, ins, out1, outb):
        for a, b in zip(o1, ob):
            assert np.array_equal(_bits(a), _bits(b)), "single and batched coefficients differ in a bit (C = %d)" % c
            assert torch.isnan(a[:G]).all() and torch.isnan(a[G + c:]).all()
        e = _coeff_check(o1[0][G:G + c].cpu().numpy(), o1[1][G:G + c].cpu().numpy(), *t, PC.EPS)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print("eval coefficients: largest scale error %.3f of its bar, largest shift error %.3f of its bar" % tuple(worst))


# ------------------------------------------------------------------------------------------------ transposes and fill
@pytest.mark.parametrize("n,c,h,w", [(2, 3, 5, 7), (1, 33, 31, 33), (3, 64, 1, 1), (1, 1, 9, 40)])
def test_layout_transposes(n, c, h, w):
    L = _L()
    x = np.random.default_rng(n * 1000 + c).standard_normal((n, c, h, w)).astype(F)
    x.reshape(-1)[:4] = np.array([0x80000000, 0x7fc12345, 0x00000001, 0xff800000], dtype=np.uint32).view(F)      # -0, a NaN payload, a denormal, -inf
    size = x.size

    def guarded():
        return torch.full((size + 2 * G,), -7.5, device="cuda")

    def run(fn, src):
        dst = guarded()
        assert fn(_p(src, G), _p(dst, G), n, c, h, w, _st()) == 0, L.rd_last_error()
        torch.cuda.synchronize()
        assert bool((dst[:G] == -7.5).all()) and bool((dst[G + size:] == -7.5).all())
        return dst
    src = guarded()
    src[G:G + size] = _dev(x).reshape(-1)
    nhwc = run(L.rd_nchw_to_nhwc, src)
    assert np.array_equal(_bits(nhwc[G:G + size]), np.ascontiguousarray(x.transpose(0, 2, 3, 1)).view(np.uint32).reshape(-1))
    back = run(L.rd_nhwc_to_nchw, nhwc)
    assert np.array_equal(_bits(back[G:G + size]), x.view(np.uint32).reshape(-1))
    assert np.array_equal(_bits(src), np.concatenate([np.full(G, -7.5, F), x.reshape(-1), np.full(G, -7.5, F)]).view(np.uint32))


@pytest.mark.parametrize("n", [0, 1, 1000003])
def test_fill(n):
    """n = 0 with a NULL pointer returns RD_OK without a launch; n = 1000003 starts one float past a 16-byte boundary and is more than
    one sweep of the capped grid (8 workgroups of 256 threads per CU).  -0.0 and a NaN with a payload arrive as bits."""
    L = _L()
    if n == 0:
        assert L.rd_fill(None, C.c_int64(0), C.c_float(1.0), _st()) == 0
        assert L.rd_fill(None, C.c_int64(-3), C.c_float(1.0), _st()) == 0
        return
    for bits in (0x80000000, 0x7fc12345):
        buf = _dev(np.full(n + 2 * G + 1, PC.SENT32, dtype=np.uint32))
        assert (buf.data_ptr() + 4 * (G + 1)) % 16 == 4
        v = C.c_float.from_buffer_copy(np.uint32(bits).tobytes())
        assert L.rd_fill(_p(buf, G + 1), C.c_int64(n), v, _st()) == 0, L.rd_last_error()
        torch.cuda.synchronize()
        want = np.full(n + 2 * G + 1, PC.SENT32, dtype=np.uint32)
        want[G + 1:G + 1 + n] = bits
        assert np.array_equal(_bits(buf), want)


# ------------------------------------------------------------------------------------------------ the plans' own jobs
# plan -> what its job lists must contain (so that the cases cannot silently vanish): "colscale" a _ColScale job, "tr_scale" a transposed
# job with a scale ("tr_rowscale": indexed by row), "fwd_colscale" a forward job with a column scale, "qN" a job of layout N, "winoF" a
# Winograd job of that flip (at 97 x 161 the planner's rule H W <= 1536 and Cin <= 128 selects layer 1 and layer 2)
PLANS = {
    "inf_lf_upproj": ("ResNet_latefusion", "upproj", (0, 4), "inference", {"q0", "q1"}),
    "inf_lf_deconv2": ("ResNet_latefusion", "deconv2", (0, 4), "inference", {"q0", "q1", "colscale", "tr_scale"}),
    "inf_lf_deconv3": ("ResNet_latefusion", "deconv3", (0, 4), "inference", {"q0", "q1", "colscale", "tr_scale"}),
    "inf_lf_upconv": ("ResNet_latefusion", "upconv", (0, 4), "inference", {"q0", "q1"}),
    "inf_rn_rgb_deconv2": ("ResNet", "deconv2", (0, 3), "inference", {"q0", "q1", "colscale", "tr_scale"}),
    "pnp_lf_upproj": ("ResNet_latefusion", "upproj", (0, 4), "pnp", {"q0", "q1", "tr_scale", "tr_rowscale"}),
    "pnp_lf_deconv2": ("ResNet_latefusion", "deconv2", (0, 4), "pnp", {"q0", "q1", "colscale", "fwd_colscale", "tr_scale"}),
    "inf_lf_upproj_bf16_storage": ("ResNet_latefusion", "upproj", (0, 4), "inference_bf16", {"q0", "q2"}),
    "train_lf_upproj_split": ("ResNet_latefusion", "upproj", (0, 4), "train", {"q0", "q1", "q3", "wino0", "wino1"}),
}


def _run_plan(case):
    """Build the plan, run it once -> (plan, the object that holds it)."""
    from radar_depth_amd import main
    from radar_depth_amd.model import models
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    cls, dec, ch, kind, _ = PLANS[case]
    h, w = 97, 161
    b = 2 if kind == "train" else 1
    torch.manual_seed(0)
    m = getattr(models, cls)(18, dec, [h, w], ch[1] - ch[0], False)
    procedural_fill_(m)
    m = m.cuda()
    x, t = make_batch(b, h, w, 900, ref_pixels=h * w)
    x, t = x[:, ch[0]:ch[1]].contiguous().cuda(), t.cuda()
    if kind == "train":
        obj = main.HipTrainStep(m, b, h, w, lr=0.0, momentum=0.0, weight_decay=0.0)      # (lr = 0: the weights the pack read are still there)
        obj.step(x, t)
    elif kind == "pnp":
        obj = main.HipPnPInference(m, b, h, w, iters=2)
        obj(x)
    else:
        obj = main.HipInference(m, b, h, w, storage="bf16" if kind == "inference_bf16" else "fp32")
        obj(x)
    torch.cuda.synchronize()
    return (obj.plans[0] if hasattr(obj, "plans") else obj.plan), obj


def _reader(plan):
    """-> read(address, n floats) from whichever tensor of the plan holds that address."""
    tensors = [t for t in plan.keep if isinstance(t, torch.Tensor) and t.dtype == torch.float32]

    def read(addr, n):
        for t in tensors:
            off = addr - t.data_ptr()
            if 0 <= off and off + 4 * n <= t.numel() * 4:
                return t.reshape(-1)[off // 4:off // 4 + n].cpu().numpy()
        raise AssertionError("no plan tensor holds %x" % addr)
    return read


@pytest.mark.parametrize("case", sorted(PLANS))
def test_plan_pack_jobs_are_the_restatement(case):
    from radar_depth_amd.engine import BN_EPS, _ColScale
    plan, obj = _run_plan(case)
    need = PLANS[case][4]
    # the folded coefficients against float64, at the derived bars
    read = _reader(plan)
    worst = [0.0, 0.0]
    for c, bn, sc, sh in plan.evalcoef_jobs:
        e = _coeff_check(read(sc.value, c), read(sh.value, c), *[a.detach().cpu().numpy() for a in (bn.weight, bn.bias, bn.running_mean, bn.running_var)],
                         BN_EPS)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    assert bool(plan.evalcoef_jobs) == PLANS[case][3].startswith(("inference", "pnp"))
    print("%s: %d folds, largest scale error %.3f of its bar, largest shift error %.3f of its bar" % ((case, len(plan.evalcoef_jobs)) + tuple(worst)))
    # every pack job, none skipped: the destination rebuilt by the restatement from the device's own scale slice
    tags, by_dst = set(), {}
    for (src, dst, o, i, tt, ldc, off, rows, tr, scale, quad) in plan.pack_jobs:
        tags.add("q%d" % quad)
        col = isinstance(scale, _ColScale)
        if scale is not None:
            tags |= ({"colscale"} if col else set()) | ({"tr_scale"} if tr else set()) | ({"tr_rowscale"} if tr and not col else set()) | (
                {"fwd_colscale"} if col and not tr else set())
        wide = quad in (0, 1)
        assert dst.dtype == (torch.float32 if wide else torch.bfloat16)
        if dst.data_ptr() not in by_dst:
            by_dst[dst.data_ptr()] = (dst, np.zeros(dst.numel(), dtype=np.uint32 if wide else np.uint16), np.zeros(dst.numel(), dtype=np.uint8))
        _, exp, count = by_dst[dst.data_ptr()]
        s = None if scale is None else (scale.t if col else scale).detach().cpu().numpy()
        idx = R.pack_into(exp, src.detach().cpu().numpy(), o, i, tt, ldc, off, rows, tr, quad, s, int(col))
        count[idx] += 1
    for dst, exp, count in by_dst.values():
        assert (count == 1).all(), "the jobs of one buffer own every element once"
        got = _bits(dst)
        assert np.array_equal(got, exp), (case, tuple(dst.shape), int((got != exp).sum()))
    for (w, u, o, i, flip) in plan.wino_jobs:
        tags.add("wino%d" % flip)
        want = R.wino_u(w.detach().cpu().numpy(), flip)
        got = _bits(u)
        assert got.size == want.size and np.array_equal(got, want), (case, o, i, flip, int((got != want).sum()))
    assert tags >= need, (case, sorted(need - tags))
    del obj

"""The operands tests/test_gpu_pack.py packs on the device and tests/test_pack_host.py shows to be sensitive to every shortcut of
pack_ref.MODES: weights (random normals with pack_ref.rounding_ladder() written into the first elements), the geometry of every job,
and the expected destination -- guards and sentinel included -- from the restatement.  numpy only.

A destination is GUARD sentinel elements, the operand, GUARD sentinel elements; the operand itself starts out as sentinels too, so that
"every element the job does not own is untouched" is one array_equal over the whole buffer."""
import numpy as np

import pack_ref as R

F = np.float32
GUARD = 16
SENT32 = 0x7fc5a5a5          # a NaN with a payload: no pack writes it
SENT16 = 0x7fd5              # a bf16 NaN
SHAPES = [(8, 4, 1), (16, 8, 3), (24, 16, 5), (32, 16, 3)]          # (32, 16, 3): 4608 elements, more than one 2048-element chunk
WINO = [(64, 16, 0), (64, 64, 0), (64, 64, 1), (128, 80, 0), (80, 128, 1)]
EVAL_C = [1, 64, 257, 1000]
EPS = 1e-5


def weights(O, I, k, seed):
    w = (np.random.default_rng(seed).standard_normal(O * I * k * k) * 0.1).astype(F)
    lad = R.rounding_ladder()[:w.size]
    w[:lad.size] = lad
    return w.reshape(O, I, k, k)


def scales(n, seed):
    return (0.25 + 3.75 * np.random.default_rng(seed).random(n)).astype(F)


def job(buf, O, I, k, ldc, off, rows_total, transpose, quad, fold="none", seed=0):
    """One pack job; fold: "none", "row" (scale[o]) or "col" (scale[i], scale_col = 1)."""
    j = dict(buf=buf, O=O, I=I, T=k * k, k=k, ldc=ldc, off=off, rows_total=rows_total if transpose else I, transpose=transpose, quad=quad, fold=fold,
             w=weights(O, I, k, 1000 + seed), scale=None, scale_col=int(fold == "col"))
    if fold != "none":
        j["scale"] = scales(I if fold == "col" else O, 2000 + seed)
    return j


def rows(j):
    return j["rows_total"] if j["transpose"] else j["I"]


def buffer_elems(j):
    return (3 if j["quad"] == 3 else 1) * R.plane_elems(j["T"], rows(j), j["ldc"])


def expected(jobs, mode="exact"):
    """-> {buffer name: expected destination with guards} for jobs that share buffers by name (uint32 / uint16 bit patterns)."""
    out = {}
    for j in jobs:
        wide = j["quad"] in (0, 1)
        if j["buf"] not in out:
            out[j["buf"]] = np.full(buffer_elems(j) + 2 * GUARD, SENT32 if wide else SENT16, dtype=np.uint32 if wide else np.uint16)
        assert out[j["buf"]].size == buffer_elems(j) + 2 * GUARD, "jobs of one buffer agree on its geometry"
        R.pack_into(out[j["buf"]], j["w"], j["O"], j["I"], j["T"], j["ldc"], j["off"], j["rows_total"], j["transpose"], j["quad"],
                    j["scale"], j["scale_col"], base=GUARD, mode=mode)
    return out


def owned(j):
    """Indices (guards included in the offset) one job writes."""
    scratch = np.zeros(buffer_elems(j) + 2 * GUARD, dtype=np.uint32 if j["quad"] in (0, 1) else np.uint16)
    return R.pack_into(scratch, j["w"], j["O"], j["I"], j["T"], j["ldc"], j["off"], j["rows_total"], j["transpose"], j["quad"], j["scale"],
                       j["scale_col"], base=GUARD)


# ------------------------------------------------------------------------------------------------ single-tensor kernels
def single_case(kind, transpose, shape):
    """rd_pack_weights (kind "fp32", quad 1) / rd_pack_weights_bf16 ("bf16", quad 2) on one tensor -> two jobs, each with a buffer of its
    own: the tight geometry (ldc = the columns, offset 0) and a padded one (columns / rows of nobody on either side of the job's).
    ["refused"]: the reduction rows are no multiple of the interleave -- the entry point must refuse and leave the buffer alone."""
    O, I, k = shape
    quad = 1 if kind == "fp32" else 2
    seed = 17 * O + I + k
    if not transpose:
        js = [job("tight", O, I, k, O, 0, I, 0, quad, seed=seed), job("padded", O, I, k, O + 3, 1, I, 0, quad, seed=seed)]
    else:
        js = [job("tight", O, I, k, I, 0, O, 1, quad, seed=seed), job("padded", O, I, k, I + 3, 3, O + 8, 1, quad, seed=seed)]
    for j in js:
        j["refused"] = rows(j) % (4 if quad == 1 else 8) != 0
    return js


def concat_case(kind, transpose):
    """Two tensors, O = 16 and O = 8, into ldc = 40 at offsets 0 and 16 (forward) / as rows of rows_total = 24 (transposed)."""
    quad = 1 if kind == "fp32" else 2
    if not transpose:
        return [job("cat", 16, 8, 3, 40, 0, 8, 0, quad, seed=1), job("cat", 8, 8, 3, 40, 16, 8, 0, quad, seed=2)]
    return [job("cat", 16, 8, 3, 11, 0, 24, 1, quad, seed=3), job("cat", 8, 8, 3, 11, 16, 24, 1, quad, seed=4)]


def all_single_jobs():
    for kind in ("fp32", "bf16"):
        for tr in (0, 1):
            for shape in SHAPES:
                yield [j for j in single_case(kind, tr, shape) if not j["refused"]]
            yield concat_case(kind, tr)


# ------------------------------------------------------------------------------------------------ the batched kernel: ONE launch
def batched_jobs():
    """Every layout (quad 0..3), forward and transposed, fold none / by row / by column, the unit-per-thread and the element-wise path of
    the bf16 layouts side by side, jobs that share a buffer, columns and rows nobody owns."""
    J = job
    return [
        J("stem", 64, 4, 7, 64, 0, 4, 0, 0, seed=10),                               # the plain 7x7 stem operand
        J("stem_fold", 16, 2, 7, 19, 2, 2, 0, 0, "row", seed=11),                   # plain, folded, columns of nobody on either side
        J("q1_cat", 16, 8, 3, 40, 0, 8, 0, 1, "row", seed=12),                      # fp32 by four: two tensors side by side, 24 .. 39 nobody's
        J("q1_cat", 8, 8, 3, 40, 16, 8, 0, 1, seed=13),
        J("q1_rows", 16, 8, 3, 12, 0, 24, 1, 1, seed=14),                           # ... as rows of 24, transposed
        J("q1_rows", 8, 8, 3, 12, 16, 24, 1, 1, "row", seed=15),
        J("q1_deconv", 12, 20, 2, 20, 0, 12, 1, 1, "col", seed=16),                 # a transposed convolution's forward operand: fold by column
        J("q1_deconv_d", 12, 20, 2, 14, 1, 20, 0, 1, "col", seed=17),               # ... and its input-gradient operand (forward form, fold by i = row)
        J("q2_idle", 32, 16, 3, 32, 0, 16, 0, 2, "row", seed=18),                   # 4608 elements = 3 blocks, 64 units: two blocks find nothing to do
        J("q2_unit", 16, 12, 3, 14, 0, 24, 1, 2, seed=19),                          # bf16, transposed, O and off multiples of 8: unit path
        J("q2_unit", 8, 12, 3, 14, 16, 24, 1, 2, seed=20),
        J("q2_elem", 12, 12, 3, 14, 0, 24, 1, 2, "col", seed=21),                   # O = off = 12: element path
        J("q2_elem", 12, 12, 3, 14, 12, 24, 1, 2, seed=22),
        J("q3_fwd", 16, 24, 2, 20, 2, 24, 0, 3, "col", seed=23),                    # three planes, forward, fold by column, unit path
        J("q3_fwd_plain", 32, 16, 3, 32, 0, 16, 0, 3, seed=24),
        J("q3_unit", 16, 12, 3, 14, 0, 24, 1, 3, seed=25),                          # three planes, transposed: unit path ...
        J("q3_unit", 8, 12, 3, 14, 16, 24, 1, 3, "row", seed=26),
        J("q3_elem", 12, 12, 3, 14, 0, 24, 1, 3, seed=27),                          # ... and element path in the same 24 rows
        J("q3_elem", 12, 12, 3, 14, 12, 24, 1, 3, "row", seed=28),
    ]


def takes_unit_path(j):
    """The kernel's documented choice (csrc/layout.hip): a bf16 layout whose job starts and ends on whole 8-row units."""
    if j["quad"] < 2:
        return False
    return (j["O"] | j["off"] | j["rows_total"]) % 8 == 0 if j["transpose"] else j["I"] % 8 == 0


# ------------------------------------------------------------------------------------------------ Winograd operands
def wino_weights(n):
    """... with one planted filter (the last): U[1][1] = (g00 + g11) / 4 = 1 + 3 * 2^-8 - 2^-30 in float64, which rounds to the float32
    1 + 3 * 2^-8 -- exactly between two bf16 values, the kept mantissa odd: the operand's p0, the double rounded once to bf16, goes down; bf16
    of the float32 would go up to the even neighbour (pack_ref's "wino_p0_from_float")."""
    O, I, _ = WINO[n]
    w = weights(O, I, 3, 3000 + n)
    w[-1, -1] = 0
    w[-1, -1, 0, 0], w[-1, -1, 1, 1] = F(4 * (1 + 3 * 2.0 ** -8)), F(-2.0 ** -28)
    return w


def wino_expected(n, mode="exact"):
    O, I, flip = WINO[n]
    u = R.wino_u(wino_weights(n), flip, mode)
    assert u.size == R.wino_packed_elems(O, I, flip)
    out = np.full(u.size + 2 * GUARD, SENT16, dtype=np.uint16)
    out[GUARD:GUARD + u.size] = u
    return out


# ------------------------------------------------------------------------------------------------ eval coefficients
def eval_inputs(n):
    C = EVAL_C[n]
    rng = np.random.default_rng(4000 + n)
    gamma, beta, rm = (rng.standard_normal(C).astype(F), rng.standard_normal(C).astype(F), (2 * rng.standard_normal(C)).astype(F))
    rv = (10.0 ** (-3 + 4 * rng.random(C))).astype(F)          # [1e-3, 10]
    rv[0] = 0.0                                                  # plus one exact 0
    return gamma, beta, rm, rv

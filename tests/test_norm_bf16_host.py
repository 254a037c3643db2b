"""CPU-only checks of what tests/test_gpu_norm_bf16.py stands on (tests/norm_bf16_cases.py):

  - the reference, rounded to bf16 where a kernel stores, passes its own intervals and fp32 bars on every case;
  - the cap: on every case with at least 15 rows at most 5 % of the elements of a stored output have an interval that holds more than
    one bf16 value (the shares are printed: run with -s);
  - the criterion has teeth: every shortcut of norm_bf16_cases.MODES, applied to the reference, leaves its intervals or bars -- WHERE
    says in which family and on which outputs, and the test asserts exactly that;
  - the planted zeros, signed shifts and the constant channel survive the rounding of the data to bf16 (asserted where the data is
    made), and the constructed tie case holds ties on which ties-to-even and ties-away differ."""
import functools

import numpy as np
import pytest

import norm_bf16_cases as B
import norm_cases as NC

F, D = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _chain():
    """[(case, data, coefficients, exact reference)] of every chain case, the planted shifts included."""
    out = []
    for c in NC.CHAIN:
        d = B.chain_data(*c)
        co = NC.plant_shift(d, NC.ref_coefs(d))
        out.append((c, d, co, B.chain_want(d, co)))
    return out


@functools.lru_cache(maxsize=None)
def _pool():
    out = []
    for c in NC.POOL:
        p = B.pool_data(*c[:5])
        out.append((c, p, B.pool_want(p)))
    return out


@functools.lru_cache(maxsize=None)
def _ties():
    out = []
    for act in (0, 1):
        d, co = B.tie_data(act)
        out.append((("tie", act), d, co, B.chain_want(d, co)))
    return out


def test_the_rounded_reference_passes_and_the_cap_holds(capsys):
    lines = []
    for c, d, co, w in _chain() + _ties():
        h, fr = B.chain_held(B.stored(w, B.CHAIN_STORED), w, d)
        lines.append(B.line(NC.case_id(c), h, fr))
        assert not B.outside(h) and NC.worst(fr) <= 1.0, (c, B.outside(h), fr)
        assert not B.capped(h, d["M"]), (c, B.capped(h, d["M"]))
        assert set(h) >= ({"y"} if d["dy"] is None else {"y", "g", "g_x", "dx1", "dx1_x"})
    for c, p, w in _pool():
        h, fr = B.pool_held(B.stored(w, B.POOL_STORED), w, p)
        lines.append(B.line("pool " + NC.case_id(c), h, fr))
        assert not B.outside(h) and NC.worst(fr) <= 1.0, (c, B.outside(h), fr)
        assert not B.capped(h, p["N"] * p["H"] * p["W"]), (c, B.capped(h, p["N"] * p["H"] * p["W"]))
        assert set(h) == {"y", "g", "dx"}
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_tie_case_holds_ties():
    """About a quarter of the exact products are bf16 ties (235 of 1024); on 118 of them ties-to-even and ties-away differ."""
    for c, d, co, w in _ties():
        n, differ = B.n_ties(d, co)
        assert (n, differ) == (235, 118)
        assert (w["y_bar"] == 0).all()


def test_directed_rounding_and_intervals():
    a = np.array([1.0 + 2.0 ** -30, -1.0 - 2.0 ** -30, 0.1, 3.0, -0.0])
    lo, hi = B.f32_directed(a, False).astype(D), B.f32_directed(a, True).astype(D)
    assert (lo <= a).all() and (hi >= a).all() and np.array_equal(lo[3:], a[3:]) and np.array_equal(hi[3:], a[3:])
    assert hi[0] == 1 + 2.0 ** -23 and lo[0] == 1 and lo[1] == -1 - 2.0 ** -23 and hi[1] == -1
    # a value just below / above a bf16 tie: one-valued intervals on either side, a two-valued one across it
    tie = 1.0 + 2.0 ** -8
    assert B.interval(tie - 5e-7, tie - 3e-7) == (1.0, 1.0) and B.interval(tie + 3e-7, tie + 5e-7) == (1 + 2.0 ** -7, 1 + 2.0 ** -7)
    assert B.interval(tie - 3e-7, tie + 3e-7) == (1.0, 1 + 2.0 ** -7)
    h = B.held(np.array([-0.0, np.nan, 1.0]), np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 1.0]), np.array([0.0, 0.5, 1.0]))
    assert h["out"] == 1 and h["n"] == 3, "-0.0 == +0.0; NaN is outside every interval"


# mode -> {family: outputs that must leave their interval / bar}, and on which cases
LEAKY = lambda c: c[2] == 2
WHERE = dict(
    truncate=dict(chain=("y", lambda c: c[0] >= 15), pool=("y", lambda c: c[1] * c[2] >= 15)),
    half_up=dict(tie=("y", lambda c: True)),
    halves_swapped=dict(chain=("y", lambda c: True), pool=("y", lambda c: True)),
    ld_as_C=dict(chain=("y", lambda c: c[0] > 1)),
    c0_ignored=dict(chain=("y", lambda c: True)),
    sums_of_rounded_g=dict(chain=("sums", lambda c: LEAKY(c) and c[0] >= 15), pool=("sums", lambda c: c[1] * c[2] >= 15)),
    dx_from_unrounded_g=dict(chain=("dx1", lambda c: LEAKY(c) and c[0] >= 15)),
    dx_x_from_rounded_g=dict(chain=("dx1_x", lambda c: LEAKY(c) and c[0] >= 15)),
    pool_dx_from_unrounded_g=dict(pool=("dx", lambda c: c[1] * c[2] >= 15)),
    y_rounded_twice=dict(chain=("y", lambda c: LEAKY(c) and c[0] >= 15)),
)


def _missed(h, fr):
    return sorted(list(B.outside(h)) + [k for k, v in fr.items() if v > 1.0])


@pytest.mark.parametrize("mode", B.MODES)
def test_every_shortcut_leaves_its_interval(mode, capsys):
    """On EVERY case WHERE names, the output it names must miss; the misses are printed."""
    seen, lines = 0, []
    for family, (key, on) in WHERE[mode].items():
        if family in ("chain", "tie"):
            for c, d, co, w in (_chain() if family == "chain" else _ties()):
                src = w if mode in ("truncate", "half_up") else B.chain_want(d, co, mode=mode)
                h, fr = B.chain_held(B.stored(src, B.CHAIN_STORED, mode), w, d)
                lines.append("%s %s %s: %s" % (mode, family, NC.case_id(c), _missed(h, fr)))
                if on(c):
                    assert key in _missed(h, fr), (mode, c, key, h.get(key), fr.get(key))
                    seen += 1
        else:
            for c, p, w in _pool():
                if c[1] * c[2] >= 10000:          # (the 224 x 224 pool: the cap and the reference above; the 49 x 81 one has every path)
                    continue
                src = w if mode in ("truncate", "half_up") else B.pool_want(p, mode=mode)
                h, fr = B.pool_held(B.stored(src, B.POOL_STORED, mode), w, p)
                lines.append("%s pool %s: %s" % (mode, NC.case_id(c), _missed(h, fr)))
                if on(c):
                    assert key in _missed(h, fr), (mode, c, key, h.get(key), fr.get(key))
                    seen += 1
    assert seen >= 2, mode
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_truncation_leaves_the_interval_on_a_large_share_of_y():
    """Storing by truncation is wrong on roughly half of all values: at least 15 % of the y elements of every chain case of 15 rows
    or more leave their interval."""
    for c, d, co, w in _chain():
        if d["M"] >= 15:
            h, _ = B.chain_held(B.stored(w, ("y",), "truncate"), w, d)
            assert h["y"]["out"] >= 0.15 * h["y"]["n"], (c, h["y"])


def test_rounded_and_unrounded_g_differ_only_where_the_table_says():
    """No activation / ReLU: g = dy * {0, 1} is exact in bf16 (the chain's rounded and unrounded g are the same numbers);
    LeakyReLU: they differ."""
    for c, d, co, w in _chain():
        same = np.array_equal(B.rb(w["g"].astype(F)).astype(D), w["g"])
        assert same == (d["act"] != 2 or d["M"] < 3), c

"""CPU-only checks of what tests/test_gpu_norm_fp64.py stands on:

  - tests/norm_ref.py, the float64 restatement of csrc/norm_act.hip's contract, against torch float64 autograd (F.batch_norm in
    training mode, ReLU / leaky_relu(0.2), the residual forms, the running statistics) and against ATen's max_pool2d with indices --
    planted exact zeros and planted ties included, which settles "gradient at 0" and "first maximum wins" against torch;
  - the case list of tests/norm_cases.py has teeth: the restatement evaluated with each named shortcut of norm_ref.MODES misses the
    bars on at least one case, while an fp32-rounded copy of the correct results passes every one of them;
  - the conditioning (1 + mean^2 / var) of the BatchNorm inputs of the oracle network, which README records, against the range the
    conditioning cases cover;
  - the launchers of csrc/norm_act.hip check their arguments before the first launch."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import norm_cases as NC
import norm_ref as R

D, F = np.float64, np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a, grad=False: torch.tensor(np.asarray(a, D), dtype=torch.float64, requires_grad=grad)


def _chan_rel(got, want):
    """Per channel (last axis): the worst error over the channel's largest magnitude."""
    got, want = np.asarray(got, D), np.asarray(want, D)
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    den = np.abs(want).max(0)
    return float((np.abs(got - want).max(0) / np.where(den == 0, 1.0, den)).max())


def _tact(z, act):
    return {0: z, 1: torch.relu(z), 2: TF.leaky_relu(z, 0.2)}[act]


# ------------------------------------------------------------------------------------------------ the restatement against torch
@pytest.mark.parametrize("case", [c for c in NC.CHAIN if 1 < c[0] <= 5000], ids=NC.case_id)
def test_ref_matches_torch_float64_autograd(case):
    M, C, act, res = case
    d = NC.chain_data(M, C, act, res, planted=False)
    x1, g1, b1 = T(d["x1"], True), T(d["gamma1"], True), T(d["beta1"], True)
    rm, rv = torch.randn(C, dtype=torch.float64), torch.rand(C, dtype=torch.float64) + 0.5
    rm0, rv0 = rm.numpy().copy(), rv.numpy().copy()
    z = TF.batch_norm(x1, rm, rv, g1, b1, True, 0.1, 1e-5)
    if res == "bn":
        x2, g2, b2 = T(d["x2"], True), T(d["gamma2"], True), T(d["beta2"], True)
        z = z + TF.batch_norm(x2, None, None, g2, b2, True, 0.1, 1e-5)
    elif res == "id":
        x2 = T(d["x2"], True)
        z = z + x2
    y = _tact(z, act)
    y.backward(T(d["dy"]))
    # the restatement, through the same entry-point shaped functions the GPU test uses, all in float64
    co = {}
    for k in ("1", "2") if res == "bn" else ("1",):
        w = R.finalize(R.stats_sums(d["x" + k])[0][None], 1, C, 0, C, M, d["gamma" + k], d["beta" + k], 1e-5, 0.1, rm0 if k == "1" else None,
                       rv0 if k == "1" else None, 0 if k == "1" else None)
        co.update({n + k: w[n] for n in ("mean", "invstd", "scale", "shift")})
        if k == "1":
            assert _chan_rel(w["rm"][None], rm.numpy()[None]) < 1e-12 and _chan_rel(w["rv"][None], rv.numpy()[None]) < 1e-12 and w["nbt"] == 1
    want_y, _ = R.bn_act(d["x1"], co["scale1"], co["shift1"], d["x2"], co.get("scale2"), co.get("shift2"), act)
    assert _chan_rel(want_y, y.detach().numpy()) < 1e-12
    g = R.bwd_g(d["dy"], want_y, act)
    sums, _ = R.bwd_sums(g, d["x1"], co["mean1"], d["x2"] if res == "bn" else None, co.get("mean2"))
    for w, (x, gm, bt) in ((1, (x1, g1, b1)), (2, (x2, g2, b2))) if res == "bn" else ((1, (x1, g1, b1)),):
        k = str(w)
        cw = R.bwd_coeffs(sums[None], 1, C, w, M, d["gamma" + k], co["invstd" + k])
        dx, _ = R.bwd_dx(g, d["x" + k], co["mean" + k], cw["A"], cw["B"], cw["K"])
        assert _chan_rel(dx, x.grad.numpy()) < 1e-12, "dx" + k
        # (dgamma / dbeta are one number per channel: relative to the sum of the absolute terms they are sums of)
        assert np.all(np.abs(cw["dgamma"] - gm.grad.numpy()) <= 1e-12 * np.abs(np.asarray(co["invstd" + k]) * np.abs(g * (np.asarray(d["x" + k], D) - co["mean" + k])).sum(0)))
        assert np.all(np.abs(cw["dbeta"] - bt.grad.numpy()) <= 1e-12 * np.abs(g).sum(0))
    if res == "id":
        assert _chan_rel(g, x2.grad.numpy()) < 1e-12


@pytest.mark.parametrize("act", [1, 2])
def test_activation_gradient_at_exact_zero_matches_torch(act):
    """scale*x + shift = +0.0 and -0.0 exactly (x = 0, shift = +-0, the -0.0 through a negative scale), next to ordinary values:
    torch's ReLU gradient there is 0, its leaky_relu gradient the slope -- the header's convention."""
    s, t = np.array([1.5, -2.0, 3.0, -0.5]), np.array([0.0, -0.0, 0.25, 0.0])
    x = np.array([[0.0, 0.0, 1.0, 2.0], [0.0, 0.0, -1.0, -3.0], [1.0, 1.0, 0.0, 0.0]])
    z32 = (s.astype(F) * x.astype(F) + t.astype(F))
    assert z32[0, 0] == 0 and not np.signbit(z32[0, 0]) and z32[0, 1] == 0 and np.signbit(z32[0, 1]), "the planted signs survive fp32"
    xt = T(x, True)
    z = xt * T(s) + T(t)
    assert torch.equal(torch.signbit(z.detach()), torch.tensor(np.signbit(z32)))
    y = _tact(z, act)
    dy = np.arange(1.0, 13.0).reshape(3, 4)
    y.backward(T(dy))
    zr, _ = R.pre_act(x, s, t)
    assert np.array_equal(np.signbit(zr), np.signbit(z32))
    want = R.bwd_g(dy, zr, act) * s
    assert np.array_equal(want, xt.grad.numpy())
    assert np.array_equal(R.bwd_g(dy, R.act_fwd(zr, act), act), R.bwd_g(dy, zr, act)), "the sign read from y and from z agree"
    assert np.array_equal(R.act_fwd(zr, act), y.detach().numpy())
    zero = zr == 0
    assert np.array_equal(R.act_grad(zr, act)[zero], np.full(int(zero.sum()), 0.0 if act == 1 else 0.2))


@pytest.mark.parametrize("case", [c for c in NC.POOL if c[1] * c[2] < 10000], ids=NC.case_id)
def test_pool_restatement_matches_aten(case):
    """max_pool2d(3, 2, 1) with indices in float64 on the planted data: nine equal values, two equal maxima, border windows full of
    equal maxima, windows that are all zero after ReLU -- ATen's CPU kernel keeps the first maximum, and so does the restatement."""
    N, H, W, C, act, _ = case
    p = NC.pool_data(N, H, W, C, act)
    xt = T(p["x"], True)
    z = _tact(xt * T(p["scale"]) + T(p["shift"]), act)
    y, ind = TF.max_pool2d(z.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    y.backward(T(p["dy"]).permute(0, 3, 1, 2))
    zr, _ = R.pre_act(p["x"], np.asarray(p["scale"], D), np.asarray(p["shift"], D))
    ar = R.act_fwd(zr, act)
    want_y, idx = R.pool_fwd(ar)
    assert np.array_equal(want_y, y.detach().permute(0, 2, 3, 1).numpy())
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    ind = ind.permute(0, 2, 3, 1).numpy()
    oh, ow = np.arange(Ho)[None, :, None, None], np.arange(Wo)[None, None, :, None]
    code = (ind // W - (2 * oh - 1)) * 3 + (ind % W - (2 * ow - 1))
    assert np.array_equal(code, idx), "first maximum wins, position code kh*3+kw"
    assert np.array_equal(R.pool_pick(ar, idx), want_y)
    if act == 1 and H >= 4 and W >= 4:
        assert want_y[0, 1, 1, 0] == 0 and idx[0, 1, 1, 0] == 0          # nine zeros after ReLU: position 0
    assert (idx[:, 0, 0, 1] == 4).all()                                    # the corner window: its first valid position holds the 7
    g, _ = R.pool_bwd(p["dy"], idx, zr, act)
    got = g * np.asarray(p["scale"], D)
    want = xt.grad.numpy()
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), "gather and activation factor"


def test_chain_lengths_and_tile_counts():
    assert [R.row_lanes(c) for c in (4, 64, 80, 1024)] == [256, 16, 12, 1]
    assert R.stats_tiles(70000) == 1094 and R.bwd_tiles(70000, 4) == 1094 and R.bwd_tiles(700, 512) == 88
    assert R.chain(70000, 4, True) == 1 + 256 + 1 and R.chain(48, 1024, False) == 48 + 1 + 1 and R.chain(700, 512, True) == 4 + 2 + 1
    assert R.chain(5000, 16, False) == 1 + 64 + 1
    assert R.pool_chain(1, 224, 224, 64, 784) == 4 + 16 + 1


# ------------------------------------------------------------------------------------------------ the case list has teeth
@functools.lru_cache(maxsize=None)
def _families():
    """(name, cases, want(case, mode), fracs(got, want, case), keys) of every family of cases; exact results computed once."""
    fin = NC.fin_cases()
    red = [dict(part=NC.synth_red(n, 16, i), n_tiles=n, C=16, which=1 + i % 2, count=7 * n + 1, gamma=NC.fin_case(n, (None, 0, 16))["gamma"],
                invstd=np.linspace(0.5, 40, 16).astype(F)) for i, n in enumerate(NC.N_TILES)]
    chain = [NC.chain_data(*c) for c in NC.CHAIN]
    pool = [NC.pool_data(*c[:5]) for c in NC.POOL if c[1] * c[2] < 10000]
    return [
        ("finalize", fin, NC.fin_want, lambda g, w, c: NC.fin_fracs(g, w), ("mean", "invstd", "scale", "shift", "rm", "rv", "nbt", "shift_terms")),
        ("coeffs", red, lambda c, mode="exact": R.bwd_coeffs(c["part"], c["n_tiles"], c["C"], c["which"], c["count"], c["gamma"], c["invstd"], mode),
         lambda g, w, c: NC.coef_fracs(g, w), ("dgamma", "dbeta", "A", "B", "K")),
        ("chain", chain, lambda c, mode="exact": NC.chain_want(c, NC.plant_shift(c, NC.ref_coefs(c)), mode), lambda g, w, c: _chain_fracs(g, w, c),
         NC.CHAIN_KEYS + ("g_x",)),
        ("pool", pool, NC.pool_want, lambda g, w, c: NC.pool_fracs(g, w, c), NC.POOL_KEYS),
    ]


def _chain_fracs(got, want, d):
    fr = NC.chain_fracs(got, want, d)
    fr["g_x"] = NC.frac(got["g_x"], want["g_x"], NC.U * np.abs(want["g_x"]))
    return fr


@functools.lru_cache(maxsize=None)
def _exact(family):
    name, cases, want, fracs, keys = _families()[family]
    return [want(c) for c in cases]


def test_fp32_rounded_correct_results_pass_every_bar():
    for i, (name, cases, want, fracs, keys) in enumerate(_families()):
        for c, w in zip(cases, _exact(i)):
            fr = fracs(NC.rounded(w, keys), w, c)
            assert NC.worst(fr) <= 1.0, (name, {k: v for k, v in fr.items() if v > 1.0})


def test_planted_zeros_reach_the_outputs():
    """The planted rows give y = +-0 exactly, and the chain's gradient there is 0 (ReLU) or slope * dy (LeakyReLU) in both forms."""
    seen = 0
    for d, w in zip(_families()[2][1], _exact(2)):
        if d["plant"] and d["act"]:
            rows, cols = d["plant"]["rows"], [d["plant"]["pos"], d["plant"]["neg"]]
            assert (w["y"][np.ix_(rows, cols)] == 0).all()
            k = 0.0 if d["act"] == 1 else R.SLOPE
            assert np.array_equal(w["g_x"][np.ix_(rows, cols)], np.asarray(d["dy"], D)[np.ix_(rows, cols)] * k)
            assert np.array_equal(w["g"], w["g_x"])
            seen += 1
    assert seen >= 6


WHERE = dict(c0_ignored="finalize", ld_as_C="finalize", last_tile_dropped="finalize coeffs", tiles_from_768_dropped="finalize coeffs",
             biased_running_var="finalize", momentum_term_dropped="finalize", count_minus_1_at_1="finalize", nbt_not_incremented="finalize",
             var_not_clamped="finalize", mean_not_subtracted="chain pool", which_swapped="coeffs chain", relu_grad_1_at_0="chain pool",
             leaky_grad_1_at_0="chain pool", last_max_wins="pool", window_clipped="pool", K_dropped="chain pool")


@pytest.mark.parametrize("mode", [m for m in R.MODES if m != "neighbour_column"])
def test_every_named_shortcut_misses_a_bar(mode):
    """In EVERY family the shortcut can occur in, at least one case must miss."""
    for i, (name, cases, want, fracs, keys) in enumerate(_families()):
        if name not in WHERE[mode].split():
            continue
        missed = []
        for c, w in zip(cases, _exact(i)):
            fr = fracs(NC.rounded(want(c, mode), keys), w, c)
            if NC.worst(fr) > 1.0:
                missed.append(sorted(k for k, v in fr.items() if v > 1.0))
        assert missed, (mode, name)
        if mode in ("relu_grad_1_at_0", "leaky_grad_1_at_0") and name == "chain":
            assert any("g_x" in m for m in missed), "the planted zeros show it in the forms that recompute the sign from x"
        if mode == "tiles_from_768_dropped":
            assert len(missed) == sum(1 for c in cases if c["n_tiles"] > 768)


def test_a_neighbour_column_written_is_noticed():
    a = np.ones((5, 8), F)
    for ld, c0 in ((24, 8), (12, 4), (8 + 16, 0)):
        assert NC.writes_ok(NC.wide(a, ld, c0), ld, c0, 8)
        assert not NC.writes_ok(NC.wide(a, ld, c0, "neighbour_column"), ld, c0, 8)
    bad = NC.wide(a, 24, 8)
    bad[3, 9] = np.inf
    assert not NC.writes_ok(bad, 24, 8, 8)
    for C in (4, 48, 1024):
        for name, (ld, c0) in NC.layout(C).items():
            assert ld % 4 == 0 and c0 % 4 == 0 and c0 + C <= ld and ld > C, name


def test_end_to_end_cases_are_well_conditioned():
    """The end-to-end figures are asked of well-conditioned cases only: 1 + mean^2/var below 2 and backward sums whose absolute terms
    are at most 16 times the sum, in every channel."""
    for c in NC.E2E:
        cond = NC.e2e_want(NC.chain_data(*c, e2e=True))["cond"]
        assert all(v < 2.0 for k, v in cond.items() if k.startswith("stats")) and all(v < 16.0 for k, v in cond.items() if k.startswith("sum")), (c, cond)


# ------------------------------------------------------------------------------------------------ conditioning of the real network
def test_network_conditioning_is_inside_the_tested_range(capsys):
    """Largest 1 + mean^2 / var over the inputs of every BatchNorm2d of the oracle's ResNet_latefusion(18, "upproj"), float64, a
    procedural_fill_ed model on a make_batch batch (synthetic data on the CPU, not a training run).  README records the value; the
    conditioning cases of the GPU test reach at least ten times as far."""
    from oracle.models import ResNet_latefusion
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    b, h, w = 2, 97, 161
    torch.manual_seed(0)
    net = ResNet_latefusion(18, "upproj", [h, w], 4, False)
    procedural_fill_(net)
    net = net.double().train()
    seen = {}

    def hook(name):
        def f(mod, inp):
            x = inp[0].detach()
            m, v = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
            seen[name] = float((1 + m * m / v).max())
        return f
    for name, mod in net.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.register_forward_pre_hook(hook(name))
    x, _ = make_batch(b, h, w, 99, ref_pixels=h * w)
    with torch.no_grad():
        net(x.double())
    assert len(seen) >= 40
    worst_name = max(seen, key=seen.get)
    worst = seen[worst_name]
    with capsys.disabled():
        print("\nlargest 1 + mean^2/var over %d BatchNorm inputs: %.4g (%s)" % (len(seen), worst, worst_name))
    reach = max(float(np.nanmin(NC.cond_want(NC.cond_data(M, C, NC.COND_RATIOS[-1]))[2])) for M, C in NC.COND)
    assert reach >= 10 * worst, (reach, worst)
    readme = open(os.path.join(REPO, "README.md")).read()
    assert ("1 + mean²/var` of %.1f" % worst) in readme, "README records %.1f" % worst


# ------------------------------------------------------------------------------------------------ the launchers' checks
def test_launchers_check_before_they_launch():
    src = open(os.path.join(REPO, "radar_depth_amd", "csrc", "norm_act.hip")).read()
    for fn in NC.LAUNCHERS:
        assert NC.checks_precede_launches(src, fn), fn

"""Short last tap groups of the direct split kernels (csrc/gconv_split.hip: gconv_split_kernel and gconv_sp2_kernel walk a phase's taps
in groups of three; a last group of one or two taps runs only those steps).  Cases and checks: tests/tap_group_cases.py.

  (a) every output and every statistics row within 2e-5 of the tensor's largest magnitude of a float64 evaluation of the descriptor
      (the kernel bar of tests/test_gpu_gconv_split.py), with and without the residual addend, with BatchNorm statistics, and through
      the _bnbwd entries; NaN-poisoned LDS and NaN-filled outputs: nothing unwritten may be consumed or left behind;
  (b) bit for bit the result of the same convolution with explicit zero-weight taps in place of the skipped steps (same plan);
  (c) run-to-run bitwise reproducibility with two launches in flight on two streams.

The tile-forcing knobs are read once per process, so every forced (MT, NT) runs in a process of its own; all of them are started
together when the first test of this file needs one."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SPLIT_TILES = [(3, 2), (2, 2), (1, 2), (2, 1), (1, 1)]      # plan_gconv_split's forms, indexed by RD_GCONV_SPLIT_FORCE
SP2_TILES = [(2, 2), (1, 2), (2, 1), (1, 1), (3, 1)]        # plan_sp2's, indexed by RD_GCONV_SP2_FORCE
# two-workgroups-per-CU kernel for pre-split input + double-buffered 8-wave kernel / 8-wave kernel for both, single patch buffer when staging
FORCED = {"sp2-%d" % i: {"RD_GCONV_SPLIT_FORCE": str(i), "RD_GCONV_SP2_FORCE": str(i)} for i in range(5)}
FORCED.update({"8wave-%d" % i: {"RD_GCONV_SPLIT_FORCE": str(i), "RD_GCONV_SP2": "0", "RD_GCONV_SPLIT_NOPDB": "1"} for i in range(5)})
BAR = 2e-5


@pytest.fixture(scope="module")
def workers(tmp_path_factory):
    out = tmp_path_factory.mktemp("tap_groups")
    procs = {}
    for name, knobs in FORCED.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("RD_")}
        env.update(knobs, OMP_NUM_THREADS="1")
        log = open(out / (name + ".log"), "w")
        procs[name] = (subprocess.Popen([sys.executable, os.path.join(HERE, "tap_group_cases.py"), str(out / (name + ".json"))], env=env, stdout=log,
                                        stderr=subprocess.STDOUT), log, out / (name + ".json"), out / (name + ".log"))
    yield procs
    for p, log, _, _ in procs.values():
        if p.poll() is None:
            p.kill()
            p.wait()
        log.close()


def _check(records, want_staged=None, want_pre=None, pdb=None):
    ran = [r for r in records if r["supported"]]
    assert ran, "no case was planned"
    for r in ran:
        print("%-44s %-6s tile %dx%d  out %.2e  stat %.2e %.2e  zero-tap run: %s%s" % (
            r["case"], r["epi"], r["tile"][0], r["tile"][1], r["err_out"], r["err_stat"][0], r["err_stat"][1], r["padded"],
            "" if "bitwise" not in r else (" equal" if r["bitwise"] else " DIFFERENT")))
    for r in ran:
        assert not r["nan"], r
        assert r["err_out"] < BAR and max(r["err_stat"]) < BAR, r
        want = want_pre if r["pre"] else want_staged
        assert want is None or tuple(r["tile"]) == want, r
        assert pdb is None or r["pre"] or r["pdb"] == pdb, r
        if r["case"].startswith("conv3x3"):
            assert r["padded"] == "no short group", r
        elif r["case"].startswith("upproj_dgrad"):
            assert r["padded"] == "inexpressible", r              # 25 taps: filling up to 27 exceeds RD_MAX_TAPS -- (a) only
        else:
            assert r["padded"] == "same plan" and r["bitwise"], r
    return ran


def test_short_tap_groups_default_plan():
    """The tiles the planners pick by themselves, every descriptor x map x channel count x epilogue."""
    import tap_group_cases
    ran = _check(tap_group_cases.run_all())
    names = {r["case"].split()[0] for r in ran}
    assert names == {"dgrad_s2_k3", "upproj_fwd", "upproj_dgrad", "deconv_dgrad_k2", "conv3x3"}
    assert {r["epi"] for r in ran} == {"plain", "addend", "bnb"} and {r["pre"] for r in ran} == {True, False}


@pytest.mark.parametrize("name", sorted(FORCED))
def test_short_tap_groups_forced_tile(name, workers):
    """One (MT, NT) of each kernel forced wherever the planner accepts the shape under it (a 64-wide tile needs more than 32 output channels)."""
    p, _, res, log = workers[name]
    rc = p.wait(timeout=300)
    assert rc == 0, open(log).read()[-4000:]
    i = int(name.split("-")[1])
    sp2 = name.startswith("sp2")
    ran = _check(json.load(open(res)), want_staged=SPLIT_TILES[i], want_pre=SP2_TILES[i] if sp2 else SPLIT_TILES[i], pdb=None if sp2 else 0)
    assert {r["pre"] for r in ran} == {True, False}, "both entry points must have accepted the forced tile somewhere"


def test_short_group_launches_in_flight_are_bitwise_reproducible():
    """A stride-2 3x3 input gradient (phases of 1 / 2 / 2 / 4 taps: one-step, two-step and full + one-step groups) on both entry points,
    eight rounds of two launches in flight on two streams: every output and statistics tile bit-identical to the first."""
    import torch
    from radar_depth_amd import convdesc as cd, ops
    from radar_depth_amd._lib import lib
    prev = lib().rd_gconv_split_plan_all(1)
    try:
        n, h, w, c = 2, 57, 100, 64
        d, _ = cd.conv_dgrad(n, h, w, c, c, 3, 2, 1)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(n, d.Hi, d.Wi, c, generator=g).cuda()
        wp = ops.pack_weights_split((torch.randn(c, c, 3, 3, generator=g) * 0.06).cuda(), transpose=True)
        xp = ops.split_pieces(x)
        tiles = {False: ops.gconv_split_stat_tiles(d), True: ops.gconv_split_pre_stat_tiles(d)}
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        got = {False: [], True: []}
        for _ in range(8):
            for pre in (False, True):
                for s in streams:
                    with torch.cuda.stream(s):
                        out = torch.zeros(n, h, w, c, device="cuda")
                        stat = torch.zeros(tiles[pre], 2, c, device="cuda")
                        (ops.gconv_split_pre if pre else ops.gconv_split)(d, xp if pre else x, wp, out, stat=stat)
                        got[pre].append((out, stat))
        torch.cuda.synchronize()
        for pre in (False, True):
            for out, stat in got[pre][1:]:
                assert torch.equal(out, got[pre][0][0]) and torch.equal(stat, got[pre][0][1])
    finally:
        lib().rd_gconv_split_plan_all(1 if prev == 1 else 0)

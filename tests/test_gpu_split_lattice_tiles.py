"""The six-term product of rd_gconv_split and rd_gconv_split_pre bit for bit under EVERY tile form of csrc/gconv_split.hip: the
integer-lattice classes of tests/wino_cases.py (A: the activation's three pieces, B: the weight's, C: the cross term; the dropped
products exactly zero, every partial sum below 2^24 quanta, so the stored output IS the float64 result -- no tolerance) on the 3x3 map
of test_gpu_split_lattice.py, on multi-phase descriptors (UpProj forward 9 / 6 / 6 / 4 taps, stride-2 input gradient 1 / 2 / 2 / 4, UpProj
input gradient 25) and on a 3x3 with partial 64-channel blocks, once under the plan the library picks and once under each of the ten
forced configurations of test_gpu_tap_groups.py (one table: FORCED, SPLIT_TILES, SP2_TILES are imported from there).

The library's own plan runs the 2x7x10 map on the 1x1 tile, so the 3x2 rotating-fragment form, the 2x2 / 1x2 / 2x1 forms, the
two-workgroups-per-CU kernel with its own tile list and the single-patch-buffer 8-wave form are reached only here.  The tile-forcing
knobs are read once per process: one worker per configuration (tests/split_lattice_tile_cases.py run as a script), ten at once, all
waited on with a time limit; a worker that ended on a signal fails every configuration after it without anything further being run.
`pytest -s` prints one line per launch (profiles/r19_split_lattice_forms.txt)."""
import json
import os
import subprocess
import sys
import time

import pytest

import split_lattice_tile_cases as TC
from test_gpu_tap_groups import FORCED, SP2_TILES, SPLIT_TILES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# Observed on an MI355X: the ten workers, started together, had all ended 5.5 s later (the slowest spent 4.4 s of that in its 30
# launches, data and references included; the same 30 launches on the default plan, in the parent, take 0.13 s once the library is
# loaded).  The wait is 20 times the slowest worker.
WAIT = 110
ORDER = sorted(FORCED)


@pytest.fixture(scope="module")
def workers(tmp_path_factory):
    """name -> (return code or None when it ran out of time, records file, log file); every worker has ended when this returns."""
    out = tmp_path_factory.mktemp("split_lattice_tiles")
    procs = {}
    t0 = time.monotonic()
    for name in ORDER:
        env = {k: v for k, v in os.environ.items() if not k.startswith("RD_")}
        env.update(FORCED[name], OMP_NUM_THREADS="1")
        log = open(out / (name + ".log"), "w")
        procs[name] = (subprocess.Popen([sys.executable, os.path.join(HERE, "split_lattice_tile_cases.py"), str(out / (name + ".json"))], env=env,
                                        stdout=log, stderr=subprocess.STDOUT), log)
    assert len(procs) == 10
    done = {}
    try:
        for name in ORDER:
            p = procs[name][0]
            try:
                rc = p.wait(timeout=max(1.0, t0 + WAIT - time.monotonic()))
            except subprocess.TimeoutExpired:
                rc = None
            done[name] = (rc, out / (name + ".json"), out / (name + ".log"), time.monotonic() - t0)
    finally:
        for p, log in procs.values():          # leftovers: out of time, or the wait itself was interrupted
            if p.poll() is None:
                p.kill()
                p.wait()
            log.close()
    yield done


def _show(label, records):
    for r in records:
        if "seconds" in r:
            print("LATTICE-TILES %-8s all launches of the process: %.1f s" % (label, r["seconds"]))
        else:
            print("LATTICE-TILES %-8s %-32s class %s tile %dx%d plan[7] %4d differing elements: %d %s" % (
                label, r["kernel"], r["cls"], r["tile"][0], r["tile"][1], r["marker"], r["n_bad"], r["first"]))


def _check(label, records, want_staged=None, want_pre=None):
    _show(label, records)
    ran = [r for r in records if "seconds" not in r]
    assert {(r["kernel"], r["cls"]) for r in ran} == {(k, c) for k in TC.KERNELS for c in "ABC"} and len(ran) == 3 * len(TC.KERNELS)
    for r in ran:
        want = want_pre if r["pre"] else want_staged
        assert want is None or tuple(r["tile"]) == want, r
        assert r["marker"] != 1000, r                 # (1000: a one-tap descriptor on gemm1_split)
        assert r["n_bad"] == 0, r
    return ran


def _records(name, workers):
    """The records of a forced configuration, after asserting that it and every configuration before it ended well."""
    for prev in ORDER[:ORDER.index(name)]:
        rc = workers[prev][0]
        assert rc is None or rc >= 0, "worker %s ended on signal %d: nothing after it counts" % (prev, -rc)
    rc, res, log, secs = workers[name]
    assert rc is not None, "worker %s did not finish within %d s" % (name, WAIT)
    assert rc == 0, open(log).read()[-4000:]
    print("LATTICE-TILES %-8s worker had ended %.1f s after the ten were started (wait: %d s)" % (name, secs, WAIT))
    return json.load(open(res))


def _want(name):
    i = int(name.split("-")[1])
    return SPLIT_TILES[i], SP2_TILES[i] if name.startswith("sp2") else SPLIT_TILES[i]


def test_lattice_default_plan():
    """Every kind and class on both entry points under the tiles the planners pick by themselves."""
    ran = _check("default", TC.run_all())
    assert {r["pre"] for r in ran} == {True, False}


@pytest.mark.parametrize("name", ORDER)
def test_lattice_forced_tile(name, workers):
    """One (MT, NT) of each kernel forced: every record runs on the table's tile and differs from float64 in no element."""
    staged, pre = _want(name)
    ran = _check(name, _records(name, workers), want_staged=staged, want_pre=pre)
    if name.startswith("8wave"):          # plan_info[7] // 100: the staging kernel's patch is double-buffered
        assert all(r["marker"] // 100 == 0 for r in ran if not r["pre"]), "RD_GCONV_SPLIT_NOPDB: the single patch buffer"
    else:                                 # (where two patches fit the LDS: not the 25-tap patch under the larger tiles)
        assert any(r["marker"] // 100 == 1 for r in ran if not r["pre"])


def test_every_entry_point_and_tile_was_run(workers):
    """Across the forced configurations: rd_gconv_split on its five tiles; rd_gconv_split_pre on the five of the two-workgroups-per-CU
    kernel and the five of the 8-wave kernel; every descriptor kind and class on each of them."""
    seen = {}
    for name in ORDER:
        for r in _records(name, workers):
            if "seconds" not in r and r["n_bad"] == 0:
                seen.setdefault((name.split("-")[0], r["pre"], tuple(r["tile"])), set()).add((r["kernel"], r["cls"]))
    want = {(f, False, t) for f in ("sp2", "8wave") for t in SPLIT_TILES} | {("sp2", True, t) for t in SP2_TILES} | {("8wave", True, t) for t in SPLIT_TILES}
    assert set(seen) == want and len(want) == 20, (sorted(seen), sorted(want))
    assert {t for (_, pre, t) in want if not pre} == set(SPLIT_TILES) and {t for (_, pre, t) in want if pre} == set(SP2_TILES) | set(SPLIT_TILES)
    for (fam, pre, tile), ran in seen.items():
        assert ran == {(k, c) for k in TC.KERNELS if ("_pre_" in k) == pre for c in "ABC"}, (fam, pre, tile)

"""Cases of tests/test_gpu_split_lattice_tiles.py: the integer-lattice classes of tests/wino_cases.py (flat_data / run_flat_plan) on
rd_gconv_split and rd_gconv_split_pre, for the 3x3 map of test_gpu_split_lattice.py and the descriptor kinds of WC.FLAT_TILE_KINDS.
run_all() runs every (kernel, class) under the tile choice of THIS process and returns one record per launch; the tile-forcing knobs are
read once per process, so the test starts this file as a script once per forced configuration:
    python tests/split_lattice_tile_cases.py OUT.json"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import wino_cases as WC  # noqa: E402

KERNELS = ("gconv_split_3x3", "gconv_split_pre_3x3") + WC.FLAT_TILE_KERNELS


def run_all():
    """-> one record per (kernel, class): entry point, plan_info[:2] (the tile), plan_info[7], the elements that differ from the float64
    result and the first few of them; the last record carries the seconds the whole run took."""
    t0 = time.perf_counter()
    records = []
    for kernel in KERNELS:
        for cls in sorted(WC.LATTICE):
            plan, n_bad, first = WC.run_flat_plan(kernel, cls)
            records.append({"kernel": kernel, "cls": cls, "pre": "_pre_" in kernel, "tile": plan[:2], "marker": plan[7], "n_bad": n_bad,
                            "first": first})
    records.append({"seconds": time.perf_counter() - t0})
    return records


if __name__ == "__main__":
    with open(sys.argv[1], "w") as fh:
        json.dump(run_all(), fh)

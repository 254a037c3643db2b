"""GPU section of the op-list pin (tests/test_plan_oplists_host.py): real, not dry-run, plans at the tuned table's shape.  A dry-run
plan skips _tune (the table pin plus rd_gconv_tune_commit), which has to run before a descriptor's statistics tiles and workspace are
sized -- the ordering a reshuffle of the convolution builders can break.  The plans are built only, never run.

The library keeps the committed plan of every descriptor for the life of the process, and a descriptor an earlier plan committed is
not pinned again (autotune.pin_from_table), so table_pins depends on what the process built before: every plan is built in a fresh
process of its own, exactly as the fixture was recorded."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_fingerprint as F  # noqa: E402
from test_plan_oplists_host import compare  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(F.GPU_CONFIGS))
def test_gpu_plan_oplists(name, tmp_path):
    gen = os.path.join(os.path.dirname(F.FIXTURE), "make_golden_plan_oplists.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RD_")}      # (the build-time knobs at their defaults)
    r = subprocess.run([sys.executable, gen, "--gpu", "--only", name, "--out", str(tmp_path / "got.json"), "--dump", str(tmp_path)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    compare("gpu", name, open(tmp_path / (name + ".txt")).read(), json.load(open(tmp_path / "got.json"))["gpu"][name])

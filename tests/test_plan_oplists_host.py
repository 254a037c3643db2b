"""The op lists of the execution plans, pinned: every configuration of tests/plan_fingerprint.py is rebuilt as a dry-run plan and its
canonical text (op names, C functions, meta families, every argument) compared with tests/golden/plan_oplists.json -- so a change of
engine.py that alters a launch says exactly which one.  Regenerate the fixture only in a change that means to alter the op lists
(tests/golden/make_golden_plan_oplists.py)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_fingerprint as F  # noqa: E402


def first_difference(name, text):
    """The first canonical line that differs from the dump of the fixture's commit (RD_OPLISTS_DUMP=DIR), else how to produce that dump."""
    dump = os.environ.get("RD_OPLISTS_DUMP")
    path = os.path.join(dump, name + ".txt") if dump else None
    if not path or not os.path.exists(path):
        return "to see the first differing line: %s, and run this test with RD_OPLISTS_DUMP=DIR of the fixture's commit" % F.REGENERATE
    want, got = open(path).read().split("\n"), text.split("\n")
    for k, (a, b) in enumerate(zip(want, got)):
        if a != b:
            return "first difference at line %d:\n  fixture: %s\n  now:     %s" % (k + 1, a, b)
    return "the first %d lines agree; fixture has %d lines, now %d" % (min(len(want), len(got)), len(want), len(got))


def compare(section, name, text, got):
    want = json.load(open(F.FIXTURE))[section][name]
    assert got["ops"] == want["ops"], "%s: op counts %s, fixture %s\n%s" % (name, got["ops"], want["ops"], first_difference(name, text))
    assert got["table_pins"] == want["table_pins"], "%s: table pins %s, fixture %s" % (name, got["table_pins"], want["table_pins"])
    assert got["sha256"] == want["sha256"], "%s: the op lists differ from the fixture\n%s" % (name, first_difference(name, text))


def test_fixture_covers_the_matrix():
    fx = json.load(open(F.FIXTURE))
    assert sorted(fx["host"]) == sorted(F.CONFIGS) and sorted(fx["gpu"]) == sorted(F.GPU_CONFIGS)


@pytest.mark.parametrize("name", sorted(F.CONFIGS))
def test_plan_oplists(name, monkeypatch):
    build, env = F.CONFIGS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    compare("host", name, *F.record(build()))

"""Writes tests/golden/plan_oplists.json: per configuration of tests/plan_fingerprint.py the op count of each list and a SHA-256 of
the plan's canonical text -- recorded results of this project's own engine, with the library built.

    python tests/golden/make_golden_plan_oplists.py [--out FILE] [--dump DIR] [--gpu] [--only SUBSTRING]

--dump DIR   also write the full canonical text per configuration (DIR/<configuration>.txt), so that two trees can be diffed
--gpu        (on the MI355X) record the real, tuned plans of the fixture's GPU section as well
--only S     rebuild only the configurations whose name contains S; every other entry of an existing FILE is carried over

Regenerate only in a change that means to alter the op lists, from the commit in front of it, and say so there.  Two runs in two fresh
processes give identical files."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import plan_fingerprint as F  # noqa: E402


def build_record(name, build, env, dev="cpu"):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return F.record(build(dev))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=F.FIXTURE)
    ap.add_argument("--dump")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out = {"host": old.get("host", {}), "gpu": old.get("gpu", {})}      # (configurations not rebuilt in this run are carried over)
    todo = [("host", n, b, e, "cpu") for n, (b, e) in F.CONFIGS.items()]
    if a.gpu:
        todo += [("gpu", n, b, e, "cuda:0") for n, (b, e) in F.GPU_CONFIGS.items()]
    for section, name, build, env, dev in todo:
        if a.only not in name:
            continue
        text, rec = build_record(name, build, env, dev)
        out[section][name] = rec
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            with open(os.path.join(a.dump, name + ".txt"), "w") as f:
                f.write(text)
        print(name, rec["ops"], rec["sha256"][:12], flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

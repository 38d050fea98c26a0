#!/usr/bin/env python3
"""Writes tests/golden/trainer_surface.json from the trainers as they stand (needs the MI355X):
    python tools/gen_golden_trainers.py
For every case of tests/test_trainer_surface.py it runs that module's record() -- the public surface after construction, then
three steps and one evaluate() on fixed data -- twice, and refuses to write where the two runs differ: the kernels are
deterministic on one architecture, so a difference is a finding.  The file holds data only: attribute names, types, dtypes and
shapes, method names and SHA-256 digests.  Run it on the commit BEFORE a change of the trainers' host code; the test then holds
the change to that commit's surface and bits."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import test_trainer_surface as T
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    args = ap.parse_args()
    out = {}
    for kind, with_eval in T.CASES:
        name = T.case_id(kind, with_eval)
        first, second = (json.loads(json.dumps(T.record(kind, with_eval))) for _ in range(2))
        if first != second:
            differ = sorted(k for k in first["bits"] if first["bits"][k] != second["bits"].get(k))
            raise SystemExit("%s: two runs differ in %s" % (name, differ or "the surface"))
        out[name] = first
        print("%s: %d attributes, %d digests" % (name, len(first["surface"]["attributes"]), len(first["bits"])), file=sys.stderr)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)), file=sys.stderr)


if __name__ == "__main__":
    main()

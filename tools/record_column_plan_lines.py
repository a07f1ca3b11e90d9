#!/usr/bin/env python3
"""Record one backend's section of tests/golden/column_plan_lines.json: the FV3_DEBUG_FD lines of the column height chain for the cases of
tests/test_column_plan_lines.py (its collect()).  Not part of the suite.

The file pins what the operators reported BEFORE a change, so it is recorded from a checkout of that commit: build its libraries, copy
tests/test_column_plan_lines.py into its tests/ (the module only uses case builders that commit already has), and from its root run

    python <this script> --backend hostemu|hip:gfx950 --out column_plan_lines.json

once per backend; the section of the backend is added to (or replaced in) the file."""
import argparse
import json
import os
import sys
import tempfile


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--backend", required=True, choices=["hostemu", "hip:gfx950"])
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    root = os.getcwd()
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    from pace_amd import build, lib

    if a.backend == "hostemu":
        build.build(64, hostemu=True, verbose=False)
    else:
        lib.load(64)  # fails loudly if the HIP library is missing
    import test_column_plan_lines as t

    assert os.path.dirname(os.path.abspath(t.__file__)) == os.path.join(root, "tests"), "run from the root of the checkout to record, with the test module in its tests/"
    with tempfile.TemporaryDirectory() as tmp:
        section = t.collect(a.backend, tmp)
    golden = json.load(open(a.out)) if os.path.exists(a.out) else {}
    golden[a.backend] = section
    with open(a.out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(section)} cases, {sum(len(v) for v in section.values())} lines on {a.backend} from {build.src_hash()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

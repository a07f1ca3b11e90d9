#!/usr/bin/env python3
"""One or more named cases of tests/test_column_solver_edges.py on one backend, in a process of their own: the library's outputs go to
an .npz that the parent test compares with the oracle.

    [FV3_RIEM_MODE=columns|wave] [FV3_RIEM_REGS=0] python tests/column_case.py --cases riem:floor:79,riem:floor:80 --backend hip:gfx950|hostemu --out out.npz

The kernel forms of the Riemann solvers (FV3_RIEM_MODE, FV3_RIEM_REGS) are chosen once per process, so a test that wants another form
than the default starts this script with the setting in the environment.  Lives under tests/ because it imports the test module's case
builders."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", required=True, help="comma-separated case names: riem:<smooth|floor>:<levels>")
    ap.add_argument("--backend", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    from pace_amd import build, lib

    if a.backend == "hostemu":
        build.build(64, hostemu=True, verbose=False)
    else:
        lib.load(64)  # fails loudly if the HIP library is missing
    from test_column_solver_edges import library_outputs

    out = {}
    for case in a.cases.split(","):
        out.update(library_outputs(case, a.backend))
    np.savez(a.out, **out)
    print(f"column_case: {len(out)} arrays of {a.cases} on {a.backend} ({', '.join(f'{k}={v}' for k, v in os.environ.items() if k.startswith('FV3_RIEM_')) or 'default forms'})")
    return 0


if __name__ == "__main__":
    sys.exit(main())

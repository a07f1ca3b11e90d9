#!/usr/bin/env python3
"""One or more named cases of tests/test_height_pgf_operator_edges.py on one backend, in a process of their own: the library's update_dz_d outputs go to an .npz
that the parent test compares with the oracle and with the default form's.

    [FV3_EDGE_PROFILE_GENERIC=1] [FV3_TP2D_MODE=staged] ... python tests/height_pgf_forms_case.py --cases c24_2x2:8,c12:79 --backend hip:gfx950|hostemu --out out.npz

The forms of edge_profile, of fv_tp_2d and of the del-n fluxes behind FV3_EDGE_PROFILE_GENERIC / _REG / _LDS, FV3_EP_ONE_LAUNCH, FV3_TP2D_MODE, FV3_DEL6_MODE and
FV3_TP2D_FA are chosen once per process, so a test that wants another form than the default starts this script with the setting in the environment.  Lives under
tests/ because it imports the test module's case builders."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

SWITCHES = ("FV3_EDGE_PROFILE_", "FV3_EP_ONE_LAUNCH", "FV3_TP2D_", "FV3_DEL6_MODE")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", required=True, help="comma-separated case names: <shape of SHAPES>:<levels>")
    ap.add_argument("--backend", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    from pace_amd import build, lib

    if a.backend == "hostemu":
        build.build(64, hostemu=True, verbose=False)
    else:
        lib.load(64)  # fails loudly if the HIP library is missing
    from test_height_pgf_operator_edges import library_outputs

    out = {}
    for case in a.cases.split(","):
        out.update(library_outputs(case, a.backend))
    np.savez(a.out, **out)
    print(f"height_pgf_forms_case: {len(out)} arrays of {a.cases} on {a.backend} ({', '.join(f'{k}={v}' for k, v in os.environ.items() if k.startswith(SWITCHES)) or 'default forms'})")
    return 0


if __name__ == "__main__":
    sys.exit(main())

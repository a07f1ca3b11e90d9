"""c_sw's window geometry (pace_amd/csrc/fv3_csw_plan.h): every point of a stage's domain box has exactly one owner.

CPU only, no library build.  A stand-alone program includes nothing but the header and walks, for the forms fused / abc / two_row, every stage A - E,
nx and ny in {16, 17, 21, 24} independently and all 16 combinations of the tile-edge flags, every point of the stage's domain box: the point is owned by the
interior kernel of the form (csw_interior_owns: the predicate the stage kernels return on), or lies in exactly one of the four window boxes (csw_frame: what
the stage launches), or both -- a window thread that returns.  Never neither (a cell nobody writes), never two windows (a cell written twice), and every
window lies inside the domain box.  Where a form has no interior kernel for a stage the launch is the domain box itself and the interior owns nothing.

The boxes at nx = ny = 24 are compared with literals copied by hand from the launch sites as they stood before the table existed (fv3_c_sw's five
launch_frame calls and their launch3 fall-backs), so the table says what the operator launched, not what this code prints."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pace_amd", "csrc")

PROGRAM = r"""
#include "fv3_csw_plan.h"
#include <cstdio>
static bool in(const Box &b, int i, int j) { return i >= b.i0 && i <= b.i1 && j >= b.j0 && j <= b.j1; }
int main() {
  const int sizes[4] = {16, 17, 21, 24}, forms[3] = {CSW_FUSED, CSW_ABC, CSW_TWO_ROW};
  const char *fname[4] = {"generic", "two_row", "abc", "fused"};
  long points = 0, both = 0, framed_cases = 0, bad = 0;
  for (int form : forms)
    for (int nx : sizes)
      for (int ny : sizes)
        for (int fl = 0; fl < 16; ++fl)
          for (int st = CSW_ST_A; st <= CSW_ST_E; ++st) {
            const int npx = nx + 1, npy = ny + 1;  // (a sub-domain's own extents: what it has with a tile edge on that side)
            const CswGeom q = csw_geom(nx, ny, npx, npy, form, st);
            const Box dom = csw_domain(st, nx, ny, 3);
            Box win[4];
            int nwin = 1;
            win[0] = dom;  // (no interior kernel for the stage: one launch over the domain box)
            if (csw_framed(form, st)) {
              const Frame fr = csw_frame(st, nx, ny, 3);
              nwin = 4;
              ++framed_cases;
              for (int w = 0; w < 4; ++w) {
                win[w] = fr.w[w];
                if (!(win[w].i0 >= dom.i0 && win[w].i1 <= dom.i1 && win[w].j0 >= dom.j0 && win[w].j1 <= dom.j1 && win[w].i0 <= win[w].i1 && win[w].j0 <= win[w].j1)) {
                  ++bad;
                  printf("BAD window %d outside the domain or empty: %s nx %d ny %d fl %d stage %c\n", w, fname[form], nx, ny, fl, 'A' + st);
                }
              }
              if (fr.w[0].k0 != 0 || fr.w[0].k1 != 2 || dom.k0 != 0 || dom.k1 != 2) ++bad, printf("BAD level chunks\n");
            }
            for (int j = dom.j0; j <= dom.j1; ++j)
              for (int i = dom.i0; i <= dom.i1; ++i) {
                int n = 0;
                for (int w = 0; w < nwin; ++w) n += in(win[w], i, j);
                const bool own = csw_interior_owns(q, st, fl, i, j);
                ++points;
                both += own && n == 1;
                if (n > 1 || (n == 0 && !own) || (nwin == 1 && own)) {
                  ++bad;
                  if (bad < 40) printf("BAD %s nx %d ny %d fl %d stage %c (%d, %d): interior %d, windows %d\n", fname[form], nx, ny, fl, 'A' + st, i, j, (int)own, n);
                }
              }
          }
  printf("points %ld both %ld framed %ld bad %ld\n", points, both, framed_cases, bad);
  for (int st = CSW_ST_A; st <= CSW_ST_E; ++st) {
    const Box d = csw_domain(st, 24, 24, 3);
    const Frame fr = csw_frame(st, 24, 24, 3);
    printf("DOM %c %d %d %d %d %d %d\n", 'A' + st, d.i0, d.i1, d.j0, d.j1, d.k0, d.k1);
    for (int w = 0; w < 4; ++w) printf("WIN %c %c %d %d %d %d %d %d\n", 'A' + st, "WESN"[w], fr.w[w].i0, fr.w[w].i1, fr.w[w].j0, fr.w[w].j1, fr.w[w].k0, fr.w[w].k1);
  }
  return bad != 0;
}
"""

# nx = ny = 24, three level chunks (nkc - 1 = 2); by hand from the launch sites before the table:
#   A  Box{-1, 5, -1, ny + 2, 0, nkc - 1}, Box{e0, e0 + 5, -1, ny + 2, 0, 0}, Box{6, nx - 4, -1, 5, 0, 0}, Box{6, nx - 4, ny - 4, ny + 2, 0, 0}    e0 = nx - 3
#   B  Box{0, 5, 0, ny + 2, 0, nkc - 1},   Box{e0, e0 + 5, 0, ny + 2, 0, 0},  Box{6, nx - 4, 0, 5, 0, 0},  Box{6, nx - 4, ny - 4, ny + 2, 0, 0}    e0 = nx - 3
#   C  Box{1, 5, 1, ny + 1, 0, npair - 1}, Box{e0, e0 + 4, 1, ny + 1, 0, 0},  Box{6, nx - 4, 1, 5, 0, 0},  Box{6, nx - 4, ny - 3, ny + 1, 0, 0}    e0 = nx - 3
#   D  Box{0, 6, 0, ny + 1, 0, nkc - 1},   Box{e0, e0 + 5, 0, ny + 1, 0, 0},  Box{7, nx - 5, 0, 6, 0, 0},  Box{7, nx - 5, ny - 4, ny + 1, 0, 0}    e0 = nx - 4
#   E  Box{1, 6, 1, ny + 1, 0, nke},       Box{e0, e0 + 5, 1, ny + 1, 0, 0},  Box{7, nx - 5, 1, 6, 0, 0},  Box{7, nx - 5, ny - 4, ny + 1, 0, 0}    e0 = nx - 4
# and the launch3 boxes {-1, nx + 2, -1, ny + 2}, {0, nx + 2, 0, ny + 2}, {1, nx + 1, 1, ny + 1}, {0, nx + 1, 0, ny + 1}, {1, nx + 1, 1, ny + 1}
WINDOWS_AT_24 = {
    "A": {"W": (-1, 5, -1, 26, 0, 2), "E": (21, 26, -1, 26, 0, 0), "S": (6, 20, -1, 5, 0, 0), "N": (6, 20, 20, 26, 0, 0)},
    "B": {"W": (0, 5, 0, 26, 0, 2), "E": (21, 26, 0, 26, 0, 0), "S": (6, 20, 0, 5, 0, 0), "N": (6, 20, 20, 26, 0, 0)},
    "C": {"W": (1, 5, 1, 25, 0, 2), "E": (21, 25, 1, 25, 0, 0), "S": (6, 20, 1, 5, 0, 0), "N": (6, 20, 21, 25, 0, 0)},
    "D": {"W": (0, 6, 0, 25, 0, 2), "E": (20, 25, 0, 25, 0, 0), "S": (7, 19, 0, 6, 0, 0), "N": (7, 19, 20, 25, 0, 0)},
    "E": {"W": (1, 6, 1, 25, 0, 2), "E": (20, 25, 1, 25, 0, 0), "S": (7, 19, 1, 6, 0, 0), "N": (7, 19, 20, 25, 0, 0)},
}
DOMAINS_AT_24 = {"A": (-1, 26, -1, 26, 0, 2), "B": (0, 26, 0, 26, 0, 2), "C": (1, 25, 1, 25, 0, 2), "D": (0, 25, 0, 25, 0, 2), "E": (1, 25, 1, 25, 0, 2)}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """The program's output (it is compiled as plain C++: no HIP, no FV3_HD) and its exit status."""
    tmp = tmp_path_factory.mktemp("csw_plan")
    src, exe = tmp / "walk.cpp", tmp / "walk"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout


def test_every_point_of_every_stage_has_one_owner(walk):
    code, out = walk
    bad = [ln for ln in out.splitlines() if ln.startswith("BAD")]
    assert not bad and code == 0, "\n".join(bad[:40])
    m = re.search(r"^points (\d+) both (\d+) framed (\d+) bad (\d+)$", out, re.M)
    points, both, framed, nbad = map(int, m.groups())
    # 3 forms x 16 size pairs x 16 flag sets x 5 stages; framed: fused 5 stages, abc 3, two_row 2
    assert nbad == 0 and framed == 16 * 16 * (5 + 3 + 2) and points > 3 * 16 * 16 * 5 * 16 * 16 and both > 0


def test_boxes_at_24_are_the_literals_of_the_old_launch_sites(walk):
    _, out = walk
    wins = {(m[1], m[2]): tuple(map(int, m[3].split())) for m in re.finditer(r"^WIN (\w) (\w) ([-\d ]+)$", out, re.M)}
    doms = {m[1]: tuple(map(int, m[2].split())) for m in re.finditer(r"^DOM (\w) ([-\d ]+)$", out, re.M)}
    assert wins == {(st, w): box for st, ws in WINDOWS_AT_24.items() for w, box in ws.items()}
    assert doms == DOMAINS_AT_24


def test_c_sw_asks_the_switch_table_only_in_its_plan():
    """every fv3_sw / fv3_sw_is query of fv3_csw.hip sits inside csw_plan(): no decision is taken between launches"""
    lines = open(os.path.join(CSRC, "fv3_csw.hip")).read().splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith("static CswPlan csw_plan("))
    end = next(i for i in range(start, len(lines)) if lines[i] == "}")
    asks = [i for i, ln in enumerate(lines) if re.search(r"\bfv3_sw(_is)?\(", ln)]
    assert asks and all(start < i < end for i in asks), [lines[i] for i in asks if not start < i < end]
    assert not any(re.search(r"\bstatic const (int|bool)\b.*fv3_sw", ln) for ln in lines)

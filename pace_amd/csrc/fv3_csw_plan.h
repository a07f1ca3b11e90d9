// fv3_csw_plan.h -- c_sw's geometry in one place: the interior rectangle of a sub-domain, the regions of it that the interior kernels own stage by
// stage, and the table of the four boundary windows the generic stage kernels run on.  Plain C++ (no HIP): fv3_csw.hip includes it, and so does the
// stand-alone program of tests/test_c_sw_plan.py, which checks for every stage, form and tile-edge combination that each point of a stage's domain has
// exactly one owner -- the interior kernel, or one window.
#pragma once
#include "fv3_box.h"
#ifndef FV3_HD
#define FV3_HD
#endif

// generic: per-point stage kernels everywhere | two_row: two-row stage-B kernel on the interior (with ua / va), A and B on windows, C - E everywhere |
// abc: stages A - C of the interior as a march, D and E everywhere | fused: the whole interior as one march, every stage on windows
enum CswForm { CSW_GENERIC = 0, CSW_TWO_ROW, CSW_ABC, CSW_FUSED };
enum CswStage { CSW_ST_A = 0, CSW_ST_B, CSW_ST_C, CSW_ST_D, CSW_ST_E };

// interior rectangle R0 of a sub-domain: columns [i_lo, i_hi], rows [j_lo, j_hi] -- the points whose whole stencil uses the interior formulas
struct CswRect {
  int i_lo, i_hi, j_lo, j_hi;
};
FV3_HD inline CswRect csw_rect(int fl, int nx, int ny, int npx, int npy) {
  CswRect r;
  r.i_lo = (fl & FV3_W) ? 6 : 0;
  r.i_hi = (fl & FV3_E) ? npx - 5 : nx + 1;
  r.j_lo = (fl & FV3_S) ? 6 : 0;
  r.j_hi = (fl & FV3_N) ? npy - 5 : ny + 1;
  return r;
}
// the two-row kernel needs an even row count: an odd rectangle hands its last row to the N window
FV3_HD inline CswRect csw_even_rows(CswRect r) {
  r.j_hi = r.j_lo + 2 * ((r.j_hi - r.j_lo + 1) / 2) - 1;
  return r;
}

// Regions of the rectangle, as the comment above csw_fused_stream names them:
//   R0  ua va uc0 vc0 ut vt: the rectangle                     RC  divgd: the corners of R0 from (1, 1)
//   RD  delpc ptc omga ke: R0 minus its last column / row       VR  vorticity: the corners of R0 from (i_lo + 1, j_lo + 1)
//   RE  final uc / vc: R0 minus a one-cell rim
FV3_HD inline bool csw_R0(const CswRect &r, int i, int j) { return i >= r.i_lo && i <= r.i_hi && j >= r.j_lo && j <= r.j_hi; }
FV3_HD inline bool csw_RC(const CswRect &r, int i, int j) { return i >= r.i_lo && i >= 1 && i <= r.i_hi && j >= r.j_lo && j >= 1 && j <= r.j_hi; }
FV3_HD inline bool csw_RD(const CswRect &r, int i, int j) { return i >= r.i_lo && i <= r.i_hi - 1 && j >= r.j_lo && j <= r.j_hi - 1; }
FV3_HD inline bool csw_VR(const CswRect &r, int i, int j) { return i >= r.i_lo + 1 && i <= r.i_hi && j >= r.j_lo + 1 && j <= r.j_hi; }
FV3_HD inline bool csw_RE(const CswRect &r, int i, int j) { return i >= r.i_lo + 1 && i <= r.i_hi - 1 && j >= r.j_lo + 1 && j <= r.j_hi - 1; }

// does the stage run on the four windows (its kernel then leaves the interior kernel's points alone) or on its whole domain box?
FV3_HD inline bool csw_framed(int form, int stage) { return form >= (stage <= CSW_ST_B ? CSW_TWO_ROW : stage == CSW_ST_C ? CSW_ABC : CSW_FUSED); }
// what a stage kernel captures of the call: the sub-domain's sizes, whether an interior kernel shares the stage with it (framed), and the two-row rule.
// (Member order: the stage B kernel sits at its scalar-register limit, and with the four sizes adjacent its fp32 build takes one vector register more.)
struct CswGeom {
  int nx, ny;
  bool framed, two_row;
  int npx, npy;
  FV3_HD CswRect rect(int fl) const {
    const CswRect r = csw_rect(fl, nx, ny, npx, npy);
    return two_row ? csw_even_rows(r) : r;
  }
};
inline CswGeom csw_geom(int nx, int ny, int npx, int npy, int form, int stage) { return CswGeom{nx, ny, csw_framed(form, stage), form == CSW_TWO_ROW, npx, npy}; }
// "this point belongs to the interior kernel": the stage kernel has nothing to do there (stage D: neither the cell, RD, nor its corner, VR)
FV3_HD inline bool csw_interior_owns(const CswGeom &q, int stage, int fl, int i, int j) {
  if (!q.framed) return false;
  const CswRect r = q.rect(fl);
  return stage <= CSW_ST_B ? csw_R0(r, i, j) : stage == CSW_ST_C ? csw_RC(r, i, j) : stage == CSW_ST_D ? csw_RD(r, i, j) && csw_VR(r, i, j) : csw_RE(r, i, j);
}

// One row per stage: the domain box [i0, nx + i1] x [j0, ny + j1] and its four windows -- W: columns i0 .. w1, E: columns nx + e0 .. nx + i1 (both over every
// row of the domain), S: rows j0 .. s1, N: rows ny + n0 .. ny + j1 (both over the columns between W and E).  The windows are the same for every sub-domain: on
// a side without a tile edge the rectangle reaches under them and their threads return there.
struct CswWinRow {
  int i0, i1, j0, j1, w1, e0, s1, n0;
};
inline CswWinRow csw_win_row(int stage) {
  static const CswWinRow rows[5] = {
      // A, B: N starts ON the rectangle's last row j_hi = ny - 4 where E starts one column past i_hi = nx - 4.  The two-row form needs it (csw_even_rows can
      // hand that row to the window); in the march forms the row is launched and every thread of it returns.  Kept as it is.
      {-1, 2, -1, 2, 5, -3, 5, -4},
      {0, 2, 0, 2, 5, -3, 5, -4},
      {1, 1, 1, 1, 5, -3, 5, -3},  // C: corners
      {0, 1, 0, 1, 6, -4, 6, -4},  // D, E: one cell deeper (the rim R0 \ RE and the last column / row of R0 are theirs)
      {1, 1, 1, 1, 6, -4, 6, -4}};
  return rows[stage];
}
// the stage's domain box and its frame of windows, nkc level chunks deep (launch_frame takes the level range of w[0])
inline Box csw_domain(int stage, int nx, int ny, int nkc) {
  const CswWinRow r = csw_win_row(stage);
  return Box{r.i0, nx + r.i1, r.j0, ny + r.j1, 0, nkc - 1};
}
inline Frame csw_frame(int stage, int nx, int ny, int nkc) {
  const CswWinRow r = csw_win_row(stage);
  return Frame{{Box{r.i0, r.w1, r.j0, ny + r.j1, 0, nkc - 1}, Box{nx + r.e0, nx + r.i1, r.j0, ny + r.j1, 0, 0}, Box{r.w1 + 1, nx + r.e0 - 1, r.j0, r.s1, 0, 0},
                Box{r.w1 + 1, nx + r.e0 - 1, ny + r.n0, ny + r.j1, 0, 0}}};
}

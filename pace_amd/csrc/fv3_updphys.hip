// fv3_updphys.hip -- ApplyPhysicsToDycore: cell-centre tendencies (u_dt eastward, v_dt northward, t_dt) applied to the D-grid winds
// and the temperature (FV3 fv_update_phys.F90: the temperature update and update_dwinds_phys; pyFV3's ApplyPhysicsToDycore).
//
//   pt(i,j) += dt t_dt(i,j)                                                     compute cells
//   V(i,j)   = u_dt vlon + v_dt vlat                                            Cartesian tendency at the cell centre
//   u(i,j)  += dt 1/2 (V(i,j-1) + V(i,j)) . es(i,j)                             i = 1..nx, j = 1..ny+1
//   v(i,j)  += dt 1/2 (V(i-1,j) + V(i,j)) . ew(i,j)                             i = 1..nx+1, j = 1..ny
// vlon / vlat: the centre's east / north unit vectors (halo cells at their true positions; vlon has no z component), es / ew: the
// unit tangents of the x-face / y-face at their mid-points.  On a face of a tile edge the two centres straddle the kink of the grid
// lines and their mean is accurate where their great circle crosses the edge, not at the face mid-point: the averaged vector is
// interpolated along the edge, (1 - w) Vbar_f + w Vbar_f', with the neighbouring face f' on the side of the edge's middle
// (ev_um / ev_up hold w where f' is face i-1 / i+1 of the south / north edge, ev_vm / ev_vp for j-1 / j+1 of the west / east edge;
// zero on every other face).  The caller updates one halo cell of u_dt, v_dt first; cube-corner halo blocks are never read.
//
// One thread per column of the (nx+1) x (ny+1) box: the metric terms of the thread's two faces are contracted once into the
// coefficients of the tendencies they multiply, the level loop then reads u_dt, v_dt at three cells (five on a tile edge) and
// updates u, v, pt in place.  Memory-bound: per cell 3 reads of tendencies, 3 reads and 3 writes of state; the neighbours' tendencies
// are the adjacent lanes' / rows' cache lines.
#include <cmath>

#include "fv3_common.h"

namespace {
struct FaceCoef {
  // coefficients of u_dt (a) / v_dt (b) at the face's two cells (0, 1) and at the two cells of the neighbouring face f' (2, 3)
  Real a0, b0, a1, b1, a2, b2, a3, b3;
  int off;  // storage offset of f' relative to the face (0: no tile-edge interpolation)
};
}  // namespace

extern "C" int fv3_apply_tendencies(fv3_ctx *c, const fv3_field *u_, const fv3_field *v_, const fv3_field *pt_, const fv3_field *u_dt_,
                                    const fv3_field *v_dt_, const fv3_field *t_dt_, const fv3_field *vlon_x_, const fv3_field *vlon_y_,
                                    const fv3_field *vlat_x_, const fv3_field *vlat_y_, const fv3_field *vlat_z_, const fv3_field *es_x_,
                                    const fv3_field *es_y_, const fv3_field *es_z_, const fv3_field *ew_x_, const fv3_field *ew_y_,
                                    const fv3_field *ew_z_, const fv3_field *ev_um_, const fv3_field *ev_up_, const fv3_field *ev_vm_,
                                    const fv3_field *ev_vp_, double dt, void *stream) {
  if (!(dt > -HUGE_VAL && dt < HUGE_VAL)) return fv3_fail(c, FV3_ERR_ARG, "apply_tendencies: dt must be finite");
  FV3_FIELD(u, u_) FV3_FIELD(v, v_) FV3_FIELD(pt, pt_) FV3_FIELD(u_dt, u_dt_) FV3_FIELD(v_dt, v_dt_) FV3_FIELD(t_dt, t_dt_)
  FV3_FIELD2D(vlon_x, vlon_x_) FV3_FIELD2D(vlon_y, vlon_y_) FV3_FIELD2D(vlat_x, vlat_x_) FV3_FIELD2D(vlat_y, vlat_y_) FV3_FIELD2D(vlat_z, vlat_z_)
  FV3_FIELD2D(es_x, es_x_) FV3_FIELD2D(es_y, es_y_) FV3_FIELD2D(es_z, es_z_) FV3_FIELD2D(ew_x, ew_x_) FV3_FIELD2D(ew_y, ew_y_) FV3_FIELD2D(ew_z, ew_z_)
  FV3_FIELD2D(ev_um, ev_um_) FV3_FIELD2D(ev_up, ev_up_) FV3_FIELD2D(ev_vm, ev_vm_) FV3_FIELD2D(ev_vp, ev_vp_)
  const Real *st3[3] = {u, v, pt}, *td3[3] = {u_dt, v_dt, t_dt};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b)
      if (st3[a] == td3[b]) return fv3_fail(c, FV3_ERR_ARG, "apply_tendencies: a tendency must not alias u / v / pt");
    for (int b = a + 1; b < 3; ++b)
      if (st3[a] == st3[b]) return fv3_fail(c, FV3_ERR_ARG, "apply_tendencies: u, v and pt must be three fields");
  }
  const Geo g = c->g;
  if (g.nh < 1) return fv3_fail(c, FV3_ERR_ARG, "apply_tendencies: needs one halo cell");
  const Real rdt = (Real)dt;
  launch2(c, (fv3_stream_t)stream, Box{1, g.nx + 1, 1, g.ny + 1, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const bool has_u = i <= g.nx, has_v = j <= g.ny;
    if (!has_u && !has_v) return;
    const int p = (int)IX(i, j);
    const int sj = g.sj32;
    const long m0 = t * g.st2;
    // the face's tangent e and the interpolation weights -> coefficients of the tendencies at cells p0, p1 (and p0 + off, p1 + off)
    auto coef = [&](int p0, int p1, Real e0, Real e1, Real e2, Real wm, Real wp, int step, FaceCoef &f) {
      const Real w = wm != (Real)0 ? wm : wp;
      f.off = wm != (Real)0 ? -step : (wp != (Real)0 ? step : 0);
      const Real h0 = (Real)0.5 * ((Real)1 - w), h1 = (Real)0.5 * w;
      auto one = [&](int cell, Real h, Real &a, Real &b) {
        const long q = m0 + cell;
        a = h * (vlon_x[q] * e0 + vlon_y[q] * e1);
        b = h * (vlat_x[q] * e0 + vlat_y[q] * e1 + vlat_z[q] * e2);
      };
      one(p0, h0, f.a0, f.b0);
      one(p1, h0, f.a1, f.b1);
      f.a2 = f.b2 = f.a3 = f.b3 = (Real)0;
      if (f.off != 0) {
        one(p0 + f.off, h1, f.a2, f.b2);
        one(p1 + f.off, h1, f.a3, f.b3);
      }
    };
    FaceCoef fu = {}, fv = {};
    if (has_u) coef(p - sj, p, es_x[m0 + p], es_y[m0 + p], es_z[m0 + p], ev_um[m0 + p], ev_up[m0 + p], 1, fu);
    if (has_v) coef(p - 1, p, ew_x[m0 + p], ew_y[m0 + p], ew_z[m0 + p], ev_vm[m0 + p], ev_vp[m0 + p], sj, fv);
    const long q = t * g.st + p;
    const Real *ud = u_dt + q, *vd = v_dt + q, *td = t_dt + q;
    Real *uk = u + q, *vk = v + q, *tk = pt + q;
    for (int k = 0; k < g.nz; ++k, ud += g.sk, vd += g.sk, td += g.sk, uk += g.sk, vk += g.sk, tk += g.sk) {
      const Real u1 = ud[0], v1 = vd[0];
      if (has_u) {
        Real d = fu.a0 * ud[-sj] + fu.b0 * vd[-sj] + fu.a1 * u1 + fu.b1 * v1;
        if (fu.off != 0) d += (fu.a2 * ud[fu.off - sj] + fu.b2 * vd[fu.off - sj]) + (fu.a3 * ud[fu.off] + fu.b3 * vd[fu.off]);
        *uk += rdt * d;
      }
      if (has_v) {
        Real d = fv.a0 * ud[-1] + fv.b0 * vd[-1] + fv.a1 * u1 + fv.b1 * v1;
        if (fv.off != 0) d += (fv.a2 * ud[fv.off - 1] + fv.b2 * vd[fv.off - 1]) + (fv.a3 * ud[fv.off] + fv.b3 * vd[fv.off]);
        *vk += rdt * d;
      }
      if (has_u && has_v) *tk += rdt * *td;
    }
  });
  return fv3_post(c, (fv3_stream_t)stream, "apply_tendencies");
}

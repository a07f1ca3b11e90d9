// fv3_moist.h -- moist_cv of FV3 (fv_mapz.F90) for six water species, per cell: the condensate mixing ratio q_con, the moist heat
// capacity at constant volume cvm and the moist R / c_p (cappa).  Shared by the cell kernels of fv3_moist.hip and the closing column
// kernel of fv3_remap.hip, so that every place forms the three values with the same expressions:
//   qv = qvapor;  ql = qliquid + qrain;  qs = (qice + qsnow) + qgraupel
//   q_con = ql + qs
//   cvm   = (((1 - (qv + q_con)) * cv_air + qv * cv_vap) + ql * c_liq) + qs * c_ice
//   cappa = rdgas / (rdgas + cvm / (1 + zvir * qv))
// in the build's Real, every sum, product and quotient rounded on its own in the order written (the build has no contraction).
// A species that is absent is read as 0: every sum is still formed, so the result is bitwise what a field of zeros gives.
#pragma once
#include "fv3_common.h"

struct MoistIn {
  const Real *qv, *ql, *qr, *qi, *qs, *qg;  // qv is never null; the others may be
  Real rdgas, zvir, cv_air, cv_vap, c_liq, c_ice;
};

struct MoistCell {
  Real qv, q_con, cvm, cappa;
};

// an optional species at element p of its field (the test is uniform over the launch)
FV3_HD inline Real moist_opt(const Real *f, long p) { return f ? f[p] : (Real)0; }

// the three values from the six species of a cell held in registers (the one place the formulas stand)
FV3_HD inline MoistCell moist_values(const MoistIn &m, Real qv, Real qliquid, Real qrain, Real qice, Real qsnow, Real qgraupel) {
  MoistCell o;
  o.qv = qv;
  const Real ql = qliquid + qrain;
  const Real qs = (qice + qsnow) + qgraupel;
  o.q_con = ql + qs;
  o.cvm = ((((Real)1.0 - (o.qv + o.q_con)) * m.cv_air + o.qv * m.cv_vap) + ql * m.c_liq) + qs * m.c_ice;
  o.cappa = m.rdgas / (m.rdgas + o.cvm / ((Real)1.0 + m.zvir * o.qv));
  return o;
}

FV3_HD inline MoistCell moist_cell(const MoistIn &m, long p) {
  return moist_values(m, m.qv[p], moist_opt(m.ql, p), moist_opt(m.qr, p), moist_opt(m.qi, p), moist_opt(m.qs, p), moist_opt(m.qg, p));
}

struct MoistNamed {
  const char *name;
  const void *ptr;
};

// The fv3_water of an entry, checked against the context layout: the species pointers and the constants in the build's Real.
// FV3_ERR_ARG with a message that names the species (a null struct, a null qvapor, a species of another shape); `op` starts the message.
int fv3_moist_in(fv3_ctx *c, const char *op, const fv3_water *w, MoistIn *out);
// the species of `m` as (name, pointer) pairs for the alias checks; returns how many are present
int fv3_moist_named(const MoistIn &m, MoistNamed out[6]);

// fv3_moist.hip -- moist thermodynamics of DynamicalCore.step_dynamics: q_con and cappa from the six water species (FV3 moist_cv,
// fv_mapz.F90, the nwat = 6 formula; fv3_moist.h holds the arithmetic).
//
//   fv3_moist_cv                    q_con, cappa (and cvm where asked) from the species
//   fv3_pt_from_temperature_moist   the preamble of fv_dynamics with moist_cv inside the cell: q_con, cappa and
//       fac = (1 + zvir * qv) * (1 - q_con) are formed from the species, then the formulas of fv3_pt_from_temperature (fv3_thermo.hip):
//       tv = pt * fac;  pz = exp(cappa * log(rrg * delp / delz * tv));  pkz = pz;  pt = tv / pz
//     -- bit for bit fv3_moist_cv followed by fv3_pt_from_temperature with qvapor, in 13 field passes (6 species + pt, delp, delz read;
//     pt, pkz, q_con, cappa written) instead of 16.
// The third moist entry, fv3_remap_moist, is in fv3_remap.hip.
//
// Compute cells and levels 0 .. nz-1 of every sub-domain; no halo cell, no pad level and no input field is written.
//
// Streaming cell kernels of the fv3_thermo.hip family: lanes run along i, every access of a wave is one coalesced row, a thread walks
// four levels (launch3<4>), the outputs are written once with streaming stores.  No LDS, no scratch.  Which of the five optional
// species are present is a run-time test that is uniform over the launch; cvm present / absent is a template parameter.
#include "fv3_moist.h"

int fv3_moist_in(fv3_ctx *c, const char *op, const fv3_water *w, MoistIn *out) {
  if (!w) return fv3_fail(c, FV3_ERR_ARG, std::string(op) + ": the fv3_water is null");
  const fv3_field *f[6] = {w->qvapor, w->qliquid, w->qrain, w->qice, w->qsnow, w->qgraupel};
  static const char *const names[6] = {"qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel"};
  const Real *p[6];
  for (int n = 0; n < 6; ++n) {
    p[n] = nullptr;
    if (n > 0 && !f[n]) continue;  // (qvapor must be there: fv3_chk reports it as null)
    p[n] = fv3_chk(c, f[n], names[n]);
    if (!p[n]) return FV3_ERR_ARG;
  }
  const fv3_constants &k = c->cst;
  *out = MoistIn{p[0], p[1], p[2], p[3], p[4], p[5], (Real)k.rdgas, (Real)(k.rvgas / k.rdgas - 1.0), (Real)(k.cp_air - k.rdgas), (Real)w->cv_vap, (Real)w->c_liq, (Real)w->c_ice};
  return FV3_OK;
}

int fv3_moist_named(const MoistIn &m, MoistNamed out[6]) {
  const MoistNamed all[6] = {{"qvapor", m.qv}, {"qliquid", m.ql}, {"qrain", m.qr}, {"qice", m.qi}, {"qsnow", m.qs}, {"qgraupel", m.qg}};
  int n = 0;
  for (const MoistNamed &a : all)
    if (a.ptr) out[n++] = a;
  return n;
}

namespace {

template <bool CVM>
void moist_cv_cells(fv3_ctx *c, fv3_stream_t s, const MoistIn m, Real *q_con, Real *cappa, Real *cvm) {
  const Geo g = c->g;
  launch3<4>(c, s, Box{1, g.nx, 1, g.ny, 0, g.nz - 1}, [=] FV3_HD(int t, int k, int i, int j) {
    const long p = t * g.st + k * g.sk + IX(i, j);
    const MoistCell o = moist_cell(m, p);
    FV3_ST_NT(q_con[p], o.q_con);
    FV3_ST_NT(cappa[p], o.cappa);
    if constexpr (CVM) FV3_ST_NT(cvm[p], o.cvm);
  });
}

void moist_preamble_cells(fv3_ctx *c, fv3_stream_t s, const MoistIn m, Real *pt, Real *pkz, const Real *delp, const Real *delz, Real *q_con, Real *cappa) {
  const Geo g = c->g;
  const Real rrg = (Real)(-c->cst.rdgas / c->cst.grav);
  launch3<4>(c, s, Box{1, g.nx, 1, g.ny, 0, g.nz - 1}, [=] FV3_HD(int t, int k, int i, int j) {
    const long p = t * g.st + k * g.sk + IX(i, j);
    const MoistCell o = moist_cell(m, p);
    // fv3_thermo.hip's fac with qvapor, from the values of this cell
    const Real dry = (Real)1.0 - o.q_con;
    const Real zq = m.zvir * o.qv;
    const Real fac = ((Real)1.0 + zq) * dry;
    const Real tv = pt[p] * fac;
    const Real pz = exp(o.cappa * log(rrg * delp[p] / delz[p] * tv));
    FV3_ST_NT(q_con[p], o.q_con);
    FV3_ST_NT(cappa[p], o.cappa);
    FV3_ST_NT(pkz[p], pz);
    FV3_ST_NT(pt[p], tv / pz);
  });
}

// the written fields may alias neither each other nor a field that is read: the result would depend on the order of the cells
int moist_alias(fv3_ctx *c, const char *op, const MoistNamed *out, int n_out, const MoistNamed *in, int n_in) {
  for (int a = 0; a < n_out; ++a) {
    if (!out[a].ptr) continue;
    for (int b = a + 1; b < n_out; ++b)
      if (out[b].ptr == out[a].ptr) return fv3_fail(c, FV3_ERR_ARG, std::string(op) + ": " + out[a].name + " and " + out[b].name + " are the same field");
    for (int b = 0; b < n_in; ++b)
      if (in[b].ptr == out[a].ptr) return fv3_fail(c, FV3_ERR_ARG, std::string(op) + ": " + out[a].name + " is the " + in[b].name + " field (" + in[b].name + " is only read)");
  }
  return FV3_OK;
}

}  // namespace

extern "C" int fv3_moist_cv(fv3_ctx *c, const fv3_water *water, const fv3_field *q_con_, const fv3_field *cappa_, const fv3_field *cvm_, void *stream) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "moist_cv: the context is null");
  MoistIn m;
  if (int st = fv3_moist_in(c, "moist_cv", water, &m)) return st;
  FV3_FIELD(q_con, q_con_) FV3_FIELD(cappa, cappa_)
  Real *cvm = nullptr;
  if (cvm_) {
    cvm = fv3_chk(c, cvm_, "cvm_");
    if (!cvm) return FV3_ERR_ARG;
  }
  const MoistNamed out[] = {{"q_con", q_con}, {"cappa", cappa}, {"cvm", cvm}};
  MoistNamed in[6];
  const int n_in = fv3_moist_named(m, in);
  if (int st = moist_alias(c, "moist_cv", out, 3, in, n_in)) return st;
  fv3_stream_t s = (fv3_stream_t)stream;
  if (cvm)
    moist_cv_cells<true>(c, s, m, q_con, cappa, cvm);
  else
    moist_cv_cells<false>(c, s, m, q_con, cappa, cvm);
  return fv3_post(c, s, "moist_cv");
}

extern "C" int fv3_pt_from_temperature_moist(fv3_ctx *c, const fv3_field *pt_, const fv3_field *pkz_, const fv3_field *delp_, const fv3_field *delz_, const fv3_field *q_con_,
                                             const fv3_field *cappa_, const fv3_water *water, void *stream) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "pt_from_temperature_moist: the context is null");
  MoistIn m;
  if (int st = fv3_moist_in(c, "pt_from_temperature_moist", water, &m)) return st;
  FV3_FIELD(pt, pt_) FV3_FIELD(pkz, pkz_) FV3_FIELD(delp, delp_) FV3_FIELD(delz, delz_) FV3_FIELD(q_con, q_con_) FV3_FIELD(cappa, cappa_)
  const MoistNamed out[] = {{"pt", pt}, {"pkz", pkz}, {"q_con", q_con}, {"cappa", cappa}};
  MoistNamed in[8] = {{"delp", delp}, {"delz", delz}};
  const int n_in = 2 + fv3_moist_named(m, in + 2);
  if (int st = moist_alias(c, "pt_from_temperature_moist", out, 4, in, n_in)) return st;
  fv3_stream_t s = (fv3_stream_t)stream;
  moist_preamble_cells(c, s, m, pt, pkz, delp, delz, q_con, cappa);
  return fv3_post(c, s, "pt_from_temperature_moist");
}

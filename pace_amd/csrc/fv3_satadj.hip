// fv3_satadj.hip -- the saturation adjustment (FV3 fv_cmp.F90, subroutine fv_sat_adj with its table set-up qs_init; the non-hydrostatic
// form).  fv3_satadj.h holds the cell; this file holds the saturation tables, the argument checks shared with fv3_remap_moist_sat
// (fv3_remap.hip) and the stand-alone entry.
//
//   fv3_sat_adj         the adjustment in place on the compute cells of levels kmp .. nz-1: the six species, tv, then q_con and cappa
//                       (moist_cv of the adjusted species, fv3_moist.h) and pkz = exp(cappa * log(rrg * delp / delz * tv))
//   fv3_sat_adj_level0  kmp, the first level whose reference mid-pressure exceeds 10 hPa
//   fv3_sat_adj_tables  the four tables as the kernels hold them
//
// Tables: tablew, table2 (ice below t_ice, two entries smoothed across the join), and their differences desw, des2; FV3_SAT_NTAB entries
// each, formed on the host in double with libm and cast to the build's Real, in one device array the context owns.  The kernels read
// them from global memory: the lanes of a wave hold neighbouring columns of one level, whose temperatures fall on a few neighbouring
// entries, and the whole set (84 KB in fp64) stays in L2.
//
// Streaming cell kernel of the fv3_moist.hip family: lanes run along i, every access of a wave is one coalesced row, a thread walks four
// levels (launch3<4>): nine fields read, ten written.  No LDS.
#include <cmath>

#include "fv3_moist.h"
#include "fv3_satadj.h"

namespace {

// qs_init of FV3: entry n (0-based here) is at T = (t_ice - 160) + 0.1 n
void build_tables(double rvgas, double cv_vap, double c_liq, double c_ice, double hlv, double hlf, double t_ice, std::vector<Real> &out) {
  const int n = FV3_SAT_NTAB;
  const double e00 = 611.21;
  const double dc_vap = (cv_vap + rvgas) - c_liq, lv0 = hlv - dc_vap * t_ice;
  const double dc_ice = c_liq - c_ice, li00 = hlf - dc_ice * t_ice;
  const double d2ice = dc_vap + dc_ice, li2 = lv0 + li00;
  const double tmin = t_ice - 160.0;
  std::vector<double> tw(n), t2(n), dw(n), d2(n);
  for (int i = 0; i < n; ++i) {
    const double t = tmin + 0.1 * i;
    tw[i] = e00 * std::exp((dc_vap * std::log(t / t_ice) + lv0 * (t - t_ice) / (t * t_ice)) / rvgas);
    t2[i] = i < 1600 ? e00 * std::exp((d2ice * std::log(t / t_ice) + li2 * (t - t_ice) / (t * t_ice)) / rvgas) : tw[i];
  }
  // entries 1600 and 1601 (1-based) of table2, smoothed from the unsmoothed values
  const double s0 = 0.25 * (t2[1598] + 2.0 * t2[1599] + t2[1600]), s1 = 0.25 * (t2[1599] + 2.0 * t2[1600] + t2[1601]);
  t2[1599] = s0;
  t2[1600] = s1;
  out.resize(4 * (size_t)n);
  // the differences are those of the entries the kernel holds (formed in Real from the cast tables)
  for (int i = 0; i < n; ++i) {
    out[i] = (Real)tw[i];
    out[n + i] = (Real)t2[i];
  }
  for (int which = 0; which < 2; ++which) {
    const Real *tab = out.data() + which * n;
    Real *des = out.data() + (2 + which) * n;
    for (int i = 0; i < n - 1; ++i) des[i] = fv3_max((Real)0, tab[i + 1] - tab[i]);
    des[n - 1] = des[n - 2];
  }
}

int sat_level0(const fv3_ctx *c) {
  const int nz = c->g.nz;
  for (int k = 0; k < nz; ++k) {
    const double p0 = c->ak[k] + c->bk[k] * 1.0e5, p1 = c->ak[k + 1] + c->bk[k + 1] * 1.0e5;
    const double pfull = (p1 - p0) / std::log(p1 / p0);
    if (pfull > 1.0e3) return k;
  }
  return nz;
}

struct SatCellArgs {
  Real *tv, *q_con, *cappa, *pkz;
  const Real *delp, *delz;
  Real rrg;
};

void sat_adj_cells(fv3_ctx *c, fv3_stream_t s, const SatK k, const SatFields f, const MoistIn m, const SatCellArgs a) {
  const Geo g = c->g;
  launch3<4>(c, s, Box{1, g.nx, 1, g.ny, k.kmp, g.nz - 1}, [=] FV3_HD(int t, int kl, int i, int j) {
    const long p = t * g.st + kl * g.sk + IX(i, j);
    Real tv = a.tv[p], qv = f.qv[p], ql = f.ql[p], qr = f.qr[p], qi = f.qi[p], qs = f.qs[p], qg = f.qg[p];
    const Real dp = a.delp[p], dz = a.delz[p];
    sat_adj_cell(k, tv, qv, ql, qr, qi, qs, qg, dp, dz);
    const MoistCell o = moist_values(m, qv, ql, qr, qi, qs, qg);
    const Real pz = exp(o.cappa * log(a.rrg * dp / dz * tv));
    f.qv[p] = qv;
    f.ql[p] = ql;
    f.qr[p] = qr;
    f.qi[p] = qi;
    f.qs[p] = qs;
    f.qg[p] = qg;
    a.tv[p] = tv;
    FV3_ST_NT(a.q_con[p], o.q_con);
    FV3_ST_NT(a.cappa[p], o.cappa);
    FV3_ST_NT(a.pkz[p], pz);
  });
}

}  // namespace

int fv3_sat_setup(fv3_ctx *c, const char *op_, const fv3_water *water, const fv3_latent *latent, const fv3_sat_params *pr, double mdt, int last_step, SatK *k, SatFields *f) {
  const std::string op = std::string(op_) + ": ";
  if (!water) return fv3_fail(c, FV3_ERR_ARG, op + "the fv3_water is null");
  if (!latent) return fv3_fail(c, FV3_ERR_ARG, op + "the fv3_latent is null");
  if (!pr) return fv3_fail(c, FV3_ERR_ARG, op + "the fv3_sat_params is null");
  const fv3_field *fl[6] = {water->qvapor, water->qliquid, water->qrain, water->qice, water->qsnow, water->qgraupel};
  static const char *const names[6] = {"qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel"};
  Real *q[6];
  for (int n = 0; n < 6; ++n) {  // (all six: a phase that is absent cannot be paid into)
    q[n] = fv3_chk(c, fl[n], names[n]);
    if (!q[n]) return FV3_ERR_ARG;
  }
  for (int n = 0; n < 6; ++n)
    for (int l = 0; l < n; ++l)
      if (q[l] == q[n]) return fv3_fail(c, FV3_ERR_ARG, op + names[l] + " and " + names[n] + " are the same field");
  if (!(mdt > 0.0)) return fv3_fail(c, FV3_ERR_ARG, op + "mdt = " + std::to_string(mdt) + " is not positive");
  if (last_step != 0 && last_step != 1) return fv3_fail(c, FV3_ERR_ARG, op + "last_step = " + std::to_string(last_step) + " (0 or 1)");
  const double taus[7] = {pr->tau_i2s, pr->tau_v2l, pr->tau_l2v, pr->tau_imlt, pr->tau_r2g, pr->tau_smlt, pr->tau_l2r};
  static const char *const tau_names[7] = {"tau_i2s", "tau_v2l", "tau_l2v", "tau_imlt", "tau_r2g", "tau_smlt", "tau_l2r"};
  for (int n = 0; n < 7; ++n)
    if (!(taus[n] > 0.0)) return fv3_fail(c, FV3_ERR_ARG, op + tau_names[n] + " = " + std::to_string(taus[n]) + " is not positive");
  const fv3_constants &cs = c->cst;
  // ---- the tables: built by the context's first adjusting call; a call with other constants rebuilds them in place
  const double key[7] = {cs.rvgas, water->cv_vap, water->c_liq, water->c_ice, latent->hlv, latent->hlf, latent->t_ice};
  bool same = c->sat_tab != nullptr;
  for (int n = 0; n < 7; ++n) same = same && key[n] == c->sat_key[n];
  if (!same) {
    if (!c->sat_tab) {
      c->sat_tab = (Real *)fv3_dev_alloc(c, sizeof(Real) * 4 * FV3_SAT_NTAB);
      if (!c->sat_tab) return fv3_fail(c, FV3_ERR_NOMEM, op + "table allocation failed");
    } else {
#ifndef FV3_HOST_EMU
      (void)hipDeviceSynchronize();  // (kernels in flight may still read the tables that are about to change)
#endif
    }
    build_tables(key[0], key[1], key[2], key[3], key[4], key[5], key[6], c->sat_tab_h);
    fv3_h2d(c->sat_tab, c->sat_tab_h.data(), sizeof(Real) * 4 * FV3_SAT_NTAB);
    for (int n = 0; n < 7; ++n) c->sat_key[n] = key[n];
  }
  // ---- the constants, formed in double and cast once
  const double sdt = 0.5 * mdt;
  const double d0_vap = water->cv_vap - water->c_liq, dc_ice = water->c_liq - water->c_ice;
  k->cv_air = (Real)(cs.cp_air - cs.rdgas);
  k->cv_vap = (Real)water->cv_vap;
  k->c_liq = (Real)water->c_liq;
  k->c_ice = (Real)water->c_ice;
  k->d0_vap = (Real)d0_vap;
  k->lv00 = (Real)(latent->hlv - d0_vap * latent->t_ice);
  k->dc_ice = (Real)dc_ice;
  k->li00 = (Real)(latent->hlf - dc_ice * latent->t_ice);
  k->zvir = (Real)(cs.rvgas / cs.rdgas - 1.0);
  k->rvgas = (Real)cs.rvgas;
  k->grav = (Real)cs.grav;
  k->tice = (Real)latent->t_ice;
  k->tice0 = (Real)(latent->t_ice - 0.01);
  k->t_wfr = (Real)(latent->t_ice - 40.0);
  k->lat2 = (Real)((latent->hlv + latent->hlf) * (latent->hlv + latent->hlf));
  k->sdt = (Real)sdt;
  k->dt_bigg = (Real)mdt;
  k->fac_i2s = (Real)(1.0 - std::exp(-mdt / pr->tau_i2s));
  k->fac_r2g = (Real)(1.0 - std::exp(-mdt / pr->tau_r2g));
  k->fac_l2r = (Real)(1.0 - std::exp(-mdt / pr->tau_l2r));
  k->fac_smlt = (Real)(1.0 - std::exp(-mdt / pr->tau_smlt));
  k->fac_v2l = (Real)(1.0 - std::exp(-sdt / pr->tau_v2l));
  k->fac_imlt = (Real)(1.0 - std::exp(-sdt / pr->tau_imlt));
  const double l2v = 1.0 - std::exp(-sdt / pr->tau_l2v);
  k->fac_l2v = (Real)(pr->sat_adj0 < l2v ? pr->sat_adj0 : l2v);
  k->ql_gen = (Real)pr->ql_gen;
  k->qi_gen = (Real)pr->qi_gen;
  k->qi_lim = (Real)pr->qi_lim;
  k->ql_mlt = (Real)pr->ql_mlt;
  k->qs_mlt = (Real)pr->qs_mlt;
  k->ql0_max = (Real)pr->ql0_max;
  k->qi0_max = (Real)pr->qi0_max;
  k->sat_adj0 = (Real)pr->sat_adj0;
  k->t_sub = (Real)pr->t_sub;
  k->tab = c->sat_tab;
  k->kmp = sat_level0(c);
  k->last_step = last_step;
  *f = SatFields{q[0], q[1], q[2], q[3], q[4], q[5]};
  return FV3_OK;
}

extern "C" int fv3_sat_adj(fv3_ctx *c, const fv3_water *water, const fv3_latent *latent, const fv3_sat_params *params, const fv3_field *tv_, const fv3_field *delp_,
                           const fv3_field *delz_, const fv3_field *q_con_, const fv3_field *cappa_, const fv3_field *pkz_, double mdt, int last_step, void *stream) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "sat_adj: the context is null");
  Real *tv = fv3_chk(c, tv_, "tv");
  if (!tv) return FV3_ERR_ARG;
  Real *delp = fv3_chk(c, delp_, "delp");
  if (!delp) return FV3_ERR_ARG;
  Real *delz = fv3_chk(c, delz_, "delz");
  if (!delz) return FV3_ERR_ARG;
  Real *q_con = fv3_chk(c, q_con_, "q_con");
  if (!q_con) return FV3_ERR_ARG;
  Real *cappa = fv3_chk(c, cappa_, "cappa");
  if (!cappa) return FV3_ERR_ARG;
  Real *pkz = fv3_chk(c, pkz_, "pkz");
  if (!pkz) return FV3_ERR_ARG;
  // a cell reads its nine inputs before it writes its ten outputs, cells are independent: what must not happen is a field given twice
  const MoistNamed own[6] = {{"tv", tv}, {"delp", delp}, {"delz", delz}, {"q_con", q_con}, {"cappa", cappa}, {"pkz", pkz}};
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < a; ++b)
      if (own[a].ptr == own[b].ptr)
        return fv3_fail(c, FV3_ERR_ARG, std::string("sat_adj: ") + own[b].name + " and " + own[a].name + " are the same field" + (b == 1 || b == 2 ? std::string(" (") + own[b].name + " is only read)" : ""));
  if (water) {
    const fv3_field *fl[6] = {water->qvapor, water->qliquid, water->qrain, water->qice, water->qsnow, water->qgraupel};
    static const char *const names[6] = {"qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel"};
    for (int n = 0; n < 6; ++n)
      for (const MoistNamed &o : own)
        if (fl[n] && fl[n]->ptr == o.ptr) return fv3_fail(c, FV3_ERR_ARG, std::string("sat_adj: ") + o.name + " is the " + names[n] + " field");
  }
  SatK k;
  SatFields f;
  if (int st = fv3_sat_setup(c, "sat_adj", water, latent, params, mdt, last_step, &k, &f)) return st;
  MoistIn m;
  if (int st = fv3_moist_in(c, "sat_adj", water, &m)) return st;
  fv3_stream_t s = (fv3_stream_t)stream;
  sat_adj_cells(c, s, k, f, m, SatCellArgs{tv, q_con, cappa, pkz, delp, delz, (Real)(-c->cst.rdgas / c->cst.grav)});
  return fv3_post(c, s, "sat_adj");
}

extern "C" int fv3_sat_adj_level0(fv3_ctx *c, int *kmp) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "sat_adj_level0: the context is null");
  if (!kmp) return fv3_fail(c, FV3_ERR_ARG, "sat_adj_level0: kmp is null");
  *kmp = sat_level0(c);
  return FV3_OK;
}

extern "C" int fv3_sat_adj_tables(fv3_ctx *c, double *out, long n) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "sat_adj_tables: the context is null");
  if (!out) return fv3_fail(c, FV3_ERR_ARG, "sat_adj_tables: out is null");
  if (n != 4L * FV3_SAT_NTAB) return fv3_fail(c, FV3_ERR_ARG, "sat_adj_tables: n = " + std::to_string(n) + " (four tables of " + std::to_string(FV3_SAT_NTAB) + " entries)");
  if (c->sat_tab_h.empty()) return fv3_fail(c, FV3_ERR_ARG, "sat_adj_tables: the tables are built by the context's first fv3_sat_adj or fv3_remap_moist_sat call");
  for (long i = 0; i < n; ++i) out[i] = (double)c->sat_tab_h[i];
  return FV3_OK;
}

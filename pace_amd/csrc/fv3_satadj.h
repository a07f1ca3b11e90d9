// fv3_satadj.h -- the saturation adjustment of FV3 (fv_cmp.F90, subroutine fv_sat_adj in its non-hydrostatic form) for one cell:
// phase changes between the six water species with the latent heat booked on the temperature.  Shared by the cell kernel of
// fv3_satadj.hip (fv3_sat_adj) and the closing column kernel of fv3_remap.hip (fv3_remap_moist_sat), so that both run the same
// expressions.  include/fv3_mi355x.h holds the algorithm step by step; the numbers in the comments below are its step numbers.
// In the build's Real, every sum, product and quotient rounded on its own in the order written (the build has no contraction);
// min / max are fv3_min / fv3_max (plain IEEE selects), min of three is min(min(a, b), c), max of three max(max(a, b), c).
// Not built: the energy-fixer branch (consv_te is 0 in every configuration), the out_dt tendency, the cloud fraction (do_qa / qa).
#pragma once
#include "fv3_common.h"

#define FV3_SAT_NTAB 2621  // entries of a saturation table: 0.1 K steps from t_ice - 160 K

// What a launch carries: the constants, formed in double and cast once, and the four tables on the device (each FV3_SAT_NTAB long,
// one after the other: tablew, table2, desw, des2)
struct SatK {
  Real cv_air, cv_vap, c_liq, c_ice, d0_vap, lv00, dc_ice, li00;
  Real zvir, rvgas, grav;
  Real tice, tice0, t_wfr, lat2, sdt, dt_bigg;
  Real fac_i2s, fac_r2g, fac_l2r, fac_smlt, fac_v2l, fac_imlt, fac_l2v;
  Real ql_gen, qi_gen, qi_lim, ql_mlt, qs_mlt, ql0_max, qi0_max, sat_adj0, t_sub;
  const Real *tab;
  int kmp;        // first level the adjustment covers
  int last_step;  // the second pass to full saturation (step 8)
};

// the six species of the entry as writable fields (all six are needed: a phase that is absent cannot be paid into)
struct SatFields {
  Real *qv, *ql, *qr, *qi, *qs, *qg;
};

FV3_HD inline Real sat_min3(Real a, Real b, Real c) { return fv3_min(fv3_min(a, b), c); }
FV3_HD inline Real sat_max3(Real a, Real b, Real c) { return fv3_max(fv3_max(a, b), c); }
FV3_HD inline Real sat_dim(Real a, Real b) { return fv3_max(a - b, (Real)0); }

// wqs2 (which = 0: tablew / desw) and iqs2 (which = 1: table2 / des2): saturation mixing ratio at temperature t and density den and
// its derivative in t, interpolated in the table.  The 1-based entries of the specification are tab[it - 1] here.  `it` of the
// derivative is kept at 1 or above: FV3 reads entry 0 of its table for t < t_ice - 159.95 K.
FV3_HD inline void sat_qs2(const SatK &k, int which, Real t, Real den, Real &qs, Real &dqdt) {
  const Real *const tab = k.tab + which * FV3_SAT_NTAB, *const des = k.tab + (2 + which) * FV3_SAT_NTAB;
  const Real ap1 = fv3_min((Real)FV3_SAT_NTAB, (Real)10 * sat_dim(t, k.tice - (Real)160) + (Real)1);
  int it = (int)ap1;
  it = it < 1 ? 1 : it;
  const Real es = tab[it - 1] + (ap1 - (Real)it) * des[it - 1];
  const Real rtd = k.rvgas * t * den;
  qs = es / rtd;
  int id = (int)(ap1 - (Real)0.5);
  id = id < 1 ? 1 : (id > FV3_SAT_NTAB - 1 ? FV3_SAT_NTAB - 1 : id);
  const Real d0 = des[id - 1], d1 = des[id];
  dqdt = (Real)10 * (d0 + (ap1 - (Real)id) * (d1 - d0)) / rtd;
}

// One cell.  tv: T * (1 + zvir * qv) * (1 - q_con), in and out; dp, delz: the layer's pressure thickness (Pa) and height (m, negative).
FV3_HD inline void sat_adj_cell(const SatK &k, Real &tv, Real &qv, Real &ql, Real &qr, Real &qi, Real &qs, Real &qg, Real dp, Real delz) {
  const Real zero = (Real)0, one = (Real)1;
  // ---- 1
  Real q_liq = ql + qr, q_sol = (qi + qs) + qg;
  Real qpz = q_liq + q_sol;
  Real pt1 = tv / ((one + k.zvir * qv) * (one - qpz));
  qpz = qpz + qv;
  const Real den = dp / (-k.grav * delz);
  const Real mc_air = (one - qpz) * k.cv_air;
  Real cvm, lhl, lhi, lcp2, icp2;
#define SAT_CVM() cvm = ((mc_air + qv * k.cv_vap) + q_liq * k.c_liq) + q_sol * k.c_ice
#define SAT_LAT()                    \
  lhl = k.lv00 + k.d0_vap * pt1;     \
  lhi = k.li00 + k.dc_ice * pt1;     \
  lcp2 = lhl / cvm;                  \
  icp2 = lhi / cvm
#define SAT_HEAT(s, L) \
  SAT_CVM();           \
  pt1 = pt1 + (s) * (L) / cvm
  SAT_CVM();
  SAT_LAT();
  // ---- 2
  if (qi < zero) {
    qs = qs + qi;
    qi = zero;
  }
  // ---- 3: melting of cloud ice
  if (qi > (Real)1.0e-8 && pt1 > k.tice) {
    const Real sink = fv3_min(qi, k.fac_imlt * (pt1 - k.tice) / icp2);
    qi = qi - sink;
    const Real tmp = fv3_min(sink, sat_dim(k.ql_mlt, ql));
    ql = ql + tmp;
    qr = qr + (sink - tmp);
    q_liq = q_liq + sink;
    q_sol = q_sol - sink;
    SAT_HEAT(-sink, lhi);
    SAT_LAT();
  }
  // ---- 4
  if (qs < zero) {
    qg = qg + qs;
    qs = zero;
  } else if (qg < zero) {
    const Real tmp = fv3_min(-qg, fv3_max(zero, qs));
    qg = qg + tmp;
    qs = qs - tmp;
  }
  // ---- 5
  if (ql < zero) {
    const Real tmp = fv3_min(-ql, fv3_max(zero, qr));
    ql = ql + tmp;
    qr = qr - tmp;
  } else if (qr < zero) {
    const Real tmp = fv3_min(-qr, fv3_max(zero, ql));
    ql = ql - tmp;
    qr = qr + tmp;
  }
  // ---- 6 / 9: freezing of cloud water below a threshold temperature
#define SAT_FREEZE(dtmp_expr)                                                      \
  {                                                                                \
    const Real dtmp = (dtmp_expr);                                                 \
    if (ql > zero && dtmp > zero) {                                                \
      const Real sink = sat_min3(ql, ql * dtmp * (Real)0.125, dtmp / icp2);        \
      ql = ql - sink;                                                              \
      qi = qi + sink;                                                              \
      q_liq = q_liq - sink;                                                        \
      q_sol = q_sol + sink;                                                        \
      SAT_HEAT(sink, lhi);                                                         \
      SAT_LAT();                                                                   \
    }                                                                              \
  }
  SAT_FREEZE((k.tice - (Real)48) - pt1)
  // ---- 7 / 8: condensation and evaporation; the second pass goes to full saturation
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1 && !k.last_step) break;
    Real wqsat, dq2dt;
    sat_qs2(k, 0, pt1, den, wqsat, dq2dt);
    const Real dq0 = (qv - wqsat) / (one + lcp2 * dq2dt);
    Real src;
    if (dq0 > zero) {
      src = pass == 1 ? dq0 : fv3_min(k.sat_adj0 * dq0, fv3_max(k.ql_gen - ql, k.fac_v2l * dq0));
    } else {
      const Real factor = -fv3_min(one, k.fac_l2v * (Real)10 * (one - qv / wqsat));
      src = -fv3_min(ql, factor * dq0);
    }
    qv = qv - src;
    ql = ql + src;
    q_liq = q_liq + src;
    SAT_HEAT(src, lhl);
    SAT_LAT();
  }
  // ---- 9: homogeneous freezing
  SAT_FREEZE(k.t_wfr - pt1)
  // ---- 10: Bigg freezing
  {
    const Real tc = k.tice0 - pt1;
    if (ql > zero && tc > zero) {
      Real sink = (Real)3.3333e-10 * k.dt_bigg * (exp((Real)0.66 * tc) - one) * den * ql * ql;
      sink = sat_min3(ql, tc / icp2, sink);
      ql = ql - sink;
      qi = qi + sink;
      q_liq = q_liq - sink;
      q_sol = q_sol + sink;
      SAT_HEAT(sink, lhi);
      SAT_LAT();
    }
  }
  // ---- 11: rain to graupel
  {
    const Real dtmp = (k.tice - (Real)0.1) - pt1;
    if (qr > (Real)1.0e-7 && dtmp > zero) {
      const Real x = dtmp * (Real)0.025;
      const Real tmp = fv3_min(one, x * x) * qr;
      const Real sink = fv3_min(tmp, k.fac_r2g * dtmp / icp2);
      qr = qr - sink;
      qg = qg + sink;
      q_liq = q_liq - sink;
      q_sol = q_sol + sink;
      SAT_HEAT(sink, lhi);
      SAT_LAT();
    }
  }
  // ---- 12: snow melt
  {
    const Real dtmp = pt1 - (k.tice + (Real)0.1);
    if (qs > (Real)1.0e-7 && dtmp > zero) {
      const Real x = dtmp * (Real)0.1;
      Real tmp = fv3_min(one, x * x) * qs;
      const Real sink = fv3_min(tmp, k.fac_smlt * dtmp / icp2);
      tmp = fv3_min(sink, sat_dim(k.qs_mlt, ql));
      qs = qs - sink;
      ql = ql + tmp;
      qr = qr + (sink - tmp);
      q_liq = q_liq + sink;
      q_sol = q_sol - sink;
      SAT_HEAT(-sink, lhi);
    }
  }
  // ---- 13: autoconversion of cloud water
  if (ql > k.ql0_max) {
    const Real sink = k.fac_l2r * (ql - k.ql0_max);
    qr = qr + sink;
    ql = ql - sink;
  }
  SAT_LAT();
  const Real tcp2 = lcp2 + icp2;
  // ---- 14: deposition and sublimation
  {
    Real src = zero;
    if (pt1 < k.t_sub) {
      src = sat_dim(qv, (Real)1.0e-6);
    } else if (pt1 < k.tice0) {
      Real qsi, dqsdt;
      sat_qs2(k, 1, pt1, den, qsi, dqsdt);
      const Real dq = qv - qsi;
      const Real sink = k.sat_adj0 * dq / (one + tcp2 * dqsdt);
      Real pidep = zero;
      if (qi > (Real)1.0e-8)
        pidep = k.sdt * dq * (Real)349138.78 * exp((Real)0.875 * log(qi * den)) / (qsi * den * k.lat2 / ((Real)0.0243 * k.rvgas * pt1 * pt1) + (Real)4.42478e4);
      if (dq > zero) {
        const Real tmp = k.tice - pt1;
        const Real qi_crt = k.qi_gen * fv3_min(k.qi_lim, (Real)0.1 * tmp) / den;
        src = sat_min3(sink, fv3_max(qi_crt - qi, pidep), tmp / tcp2);
      } else {
        pidep = pidep * fv3_min(one, sat_dim(pt1, k.t_sub) * (Real)0.2);
        src = sat_max3(pidep, sink, -qi);
      }
    }
    qv = qv - src;
    qi = qi + src;
    q_sol = q_sol + src;
    SAT_HEAT(src, (lhl + lhi));
  }
  // ---- 15: the new virtual temperature
  {
    const Real q_con = q_liq + q_sol;
    tv = pt1 * (one + k.zvir * qv) * (one - q_con);
  }
  // ---- 16
  if (qg < zero) {
    const Real tmp = fv3_min(-qg, fv3_max(zero, qi));
    qg = qg + tmp;
    qi = qi - tmp;
  }
  // ---- 17: autoconversion of cloud ice
  {
    const Real qim = k.qi0_max / den;
    if (qi > qim) {
      const Real sink = k.fac_i2s * (qi - qim);
      qi = qi - sink;
      qs = qs + sink;
    }
  }
#undef SAT_FREEZE
#undef SAT_HEAT
#undef SAT_LAT
#undef SAT_CVM
}

// The arguments of an adjusting entry, checked (FV3_ERR_ARG with a message that starts with `op`: a null struct, a species that is null
// or of another shape, mdt <= 0, last_step other than 0 / 1, a tau_* that is not positive), the constants formed, the tables built and
// uploaded on the context's first use (rebuilt in place when the constants they are made of change).  fv3_satadj.hip.
int fv3_sat_setup(fv3_ctx *c, const char *op, const fv3_water *water, const fv3_latent *latent, const fv3_sat_params *params, double mdt, int last_step, SatK *k,
                  SatFields *f);

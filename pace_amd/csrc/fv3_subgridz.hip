// fv3_subgridz.hip -- dry convective adjustment of the sponge layers (FV3 fv_sg.F90, subroutine fv_subgrid_z in its non-hydrostatic
// form; pyFV3 DryConvectiveAdjustment, which the reference driver runs after every step_dynamics when fv_sg_adj > 0).  On the top
// kbot levels of a column a pair of neighbouring levels whose Richardson number is below a reference value exchanges mass: momentum,
// total energy, w and every tracer are mixed, the temperature follows from the mixed energy.  Three passes of growing strength, then a
// relaxation with dt / tau; the wind change leaves as tendencies u_dt, v_dt, the temperature, w and the tracers change in place.
// include/fv3_mi355x.h (fv3_subgrid_z) holds the formulas; every sum, product and quotient is rounded on its own in the order written.
//
// A thread owns a column (i fastest: every level access of a wave is one coalesced row).  A pass is one walk UP from level kbot-1: the
// lower level of the current pair stays in registers (u0, v0, w0, t0, te, gz, delp, pkz, qcon, cvm, the six species), gz and te of a
// level are formed as it enters the walk (gz is a running sum over delz from kbot-1 up, te needs only the level's own values before
// the pass mixed them), the record of level k-2 is requested before the arithmetic of pair (k-1, k), level k is stored once that pair
// is done and level k-1 is carried up.  The three passes and the closing walk run one after the other in one launch: a column is
// private to its thread, so nothing has to be ordered between threads.
//
// The incoming pt, w and tracers must survive until the relaxation, so the working copy lives in the caller's work fields (t0, w0 and
// one per tracer; u0, v0 live in u_dt, v_dt): pass 1 reads the inputs and writes the copy, passes 2 and 3 read the copy and rewrite the
// levels they changed, the closing walk relaxes, writes the outputs and the tendencies.  A column in which no pair mixed is not
// stored at all (its tendencies are written as zeros): `a + (a - a) * fra` is never formed for it.
//
// Tracers that are not water species see only the exchanged mass mc of every pair.  When there are any, the main walk stores mc of
// each pass into three more work fields and a second, light kernel (subgridz_passive) mixes them, up to four per launch sharing the
// reads of mc and delp; a tracer's bits do not depend on which launch carries it.  No LDS, no scratch.
#include <cmath>
#include <vector>

#include "fv3_moist.h"

namespace {

struct SgIn {
  const Real *ua, *va, *w, *pt, *delp, *delz, *peln, *pkz;  // (w, pt: read here, written by the closing walk through w_out, pt_out)
  Real *w_out, *pt_out, *u_dt, *v_dt;
  Real *w0, *t0;        // working copies (u0, v0 are u_dt, v_dt)
  Real *q[6], *q0[6];   // the species qv, ql, qr, qi, qs, qg and their working copies (null: absent, read as 0)
  Real *mc[3];          // the exchanged mass of every pair per pass, at the pair's lower level (null: no passive tracers)
  Real grav, g2, cv_air, cv_vap, c_liq, c_ice, xvir, t_min, t_max, fra, rdt;
  int kbot, blend;
};

// level k of a field at the thread's column: wave-uniform plane base + 32-bit in-plane offset
#define SG(ptr, k) FV3_EL((ptr) + tb + (long)(k)*sk, pix)

// what is loaded of a level, and the level as the walk holds it
struct SgRaw {
  Real u, v, w, t, dp, dz, pkz, pe, q[6];
};
struct SgLev {
  Real u, v, w, t, te, gz, dp, pkz, qcon, cvm, q[6];
};

template <bool MOIST>
FV3_HD inline void sg_cvm(const SgIn &m, SgLev &l) {
  if constexpr (MOIST) {
    const Real q_liq = l.q[1] + l.q[2];
    const Real q_sol = (l.q[3] + l.q[4]) + l.q[5];
    l.cvm = ((((Real)1 - ((l.q[0] + q_liq) + q_sol)) * m.cv_air + l.q[0] * m.cv_vap) + q_liq * m.c_liq) + q_sol * m.c_ice;
    l.qcon = (((l.q[1] + l.q[3]) + l.q[4]) + l.q[2]) + l.q[5];
  } else {
    l.cvm = m.cv_air;
    l.qcon = (Real)0;
  }
}

FV3_HD inline Real sg_tvol(const SgLev &l) { return l.gz + (Real)0.5 * ((l.u * l.u + l.v * l.v) + l.w * l.w); }

// h0 = mc (X[k] - X[m]);  X[m] += h0 / delp[m];  X[k] -= h0 / delp[k]
FV3_HD inline void sg_mix(Real mc, Real dpm, Real dpk, Real &xm, Real &xk) {
  const Real h0 = mc * (xk - xm);
  xm = xm + h0 / dpm;
  xk = xk - h0 / dpk;
}

template <bool MOIST>
void subgridz_columns(fv3_ctx *c, fv3_stream_t s, const SgIn m) {
  const Geo g = c->g;
  launch2(c, s, Box{1, g.nx, 1, g.ny, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const int nz = g.nz, kb = m.kbot;
    const long tb = t * g.st, sk = g.sk;
    const unsigned pix = IX(i, j);
    const Real zero = (Real)0, one = (Real)1;
    bool any = false;
    if (kb >= 3) {
      for (int pass = 0; pass < 3; ++pass) {
        const Real ratio = (Real)(pass + 1) / (Real)3;
        const bool first = pass == 0;
        Real *const mcp = pass == 0 ? m.mc[0] : (pass == 1 ? m.mc[1] : m.mc[2]);  // (no run-time index into the kernel's arguments)
        const Real *su = first ? m.ua : m.u_dt, *sv = first ? m.va : m.v_dt, *sw = first ? m.w : m.w0, *st = first ? m.pt : m.t0;
        auto load = [&](int k) {
          SgRaw r;
          r.u = SG(su, k), r.v = SG(sv, k), r.w = SG(sw, k), r.t = SG(st, k);
          r.dp = SG(m.delp, k), r.dz = SG(m.delz, k), r.pkz = SG(m.pkz, k), r.pe = SG(m.peln, k);
#pragma unroll
          for (int n = 0; n < 6; ++n) r.q[n] = zero;
          if constexpr (MOIST) {
#pragma unroll
            for (int n = 0; n < 6; ++n)
              if (m.q[n]) r.q[n] = SG(first ? m.q[n] : m.q0[n], k);
          }
          return r;
        };
        Real gzh = zero;
        // a level enters the walk: gz from the running sum, cvm and qcon from its species, te from its values before this pass's mixing
        auto enter = [&](const SgRaw &r) {
          SgLev l;
          l.u = r.u, l.v = r.v, l.w = r.w, l.t = r.t, l.dp = r.dp, l.pkz = r.pkz;
#pragma unroll
          for (int n = 0; n < 6; ++n) l.q[n] = r.q[n];
          l.gz = gzh - m.g2 * r.dz;
          gzh = gzh - m.grav * r.dz;
          sg_cvm<MOIST>(m, l);
          l.te = l.cvm * l.t + sg_tvol(l);
          return l;
        };
        auto store = [&](const SgLev &l, int k) {
          SG(m.u_dt, k) = l.u;
          SG(m.v_dt, k) = l.v;
          SG(m.w0, k) = l.w;
          SG(m.t0, k) = l.t;
          if constexpr (MOIST) {
#pragma unroll
            for (int n = 0; n < 6; ++n)
              if (m.q0[n]) SG(m.q0[n], k) = l.q[n];
          }
        };
        SgRaw nx = load(kb - 1);
        Real pe_below = SG(m.peln, kb), pe_lo = nx.pe;
        SgLev lo = enter(nx);
        bool lo_dirty = false;
        nx = load(kb - 2);
        for (int k = kb - 1; k >= 1; --k) {
          const SgRaw cur = nx;  // level k-1
          nx = load(k >= 2 ? k - 2 : 0);  // (requested before the arithmetic of this pair; on the last pair level 0 again, not used)
          SgLev up = enter(cur);
          // ---- the pair: upper level m = k-1 (up), lower level k (lo)
          const Real tv1 = up.t * ((one + m.xvir * up.q[0]) - up.qcon), tv2 = lo.t * ((one + m.xvir * lo.q[0]) - lo.qcon);
          const Real pt1 = tv1 / up.pkz, pt2 = tv2 / lo.pkz;
          const Real du = up.u - lo.u, dv = up.v - lo.v;
          Real ri = ((up.gz - lo.gz) * (pt1 - pt2)) / (((Real)0.5 * (pt1 + pt2)) * ((du * du + dv * dv) + (Real)1.0e-4));
          if (tv1 > m.t_max && tv1 > tv2)
            ri = zero;
          else if (tv2 < m.t_min)
            ri = fv3_min(ri, (Real)0.1);
          const Real pm = lo.dp / (pe_below - pe_lo);
          const Real dimp = fv3_max((Real)400.0e2 - pm, zero);
          Real ri_ref = fv3_min(one, (Real)0.25 + (((one - (Real)0.25)) * dimp) / (Real)200.0e2);
          if (k == 1) ri_ref = (Real)4 * ri_ref;
          if (k == 2) ri_ref = (Real)2 * ri_ref;
          if (k == 3) ri_ref = (Real)1.5 * ri_ref;
          const Real r = one - fv3_max(zero, ri / ri_ref);
          const Real mc = ri < ri_ref ? (((ratio * up.dp) * lo.dp) / (up.dp + lo.dp)) * (r * r) : zero;
          bool up_dirty = false;
          if (mc > zero) {
            any = true;
            lo_dirty = up_dirty = true;
            if constexpr (MOIST) {
#pragma unroll
              for (int n = 0; n < 6; ++n)
                if (m.q[n]) sg_mix(mc, up.dp, lo.dp, up.q[n], lo.q[n]);
            }
            sg_mix(mc, up.dp, lo.dp, up.u, lo.u);
            sg_mix(mc, up.dp, lo.dp, up.v, lo.v);
            sg_mix(mc, up.dp, lo.dp, up.te, lo.te);
            sg_mix(mc, up.dp, lo.dp, up.w, lo.w);
            sg_cvm<MOIST>(m, up);
            up.t = (up.te - sg_tvol(up)) / up.cvm;
            sg_cvm<MOIST>(m, lo);
            lo.t = (lo.te - sg_tvol(lo)) / lo.cvm;
          }
          if (mcp) SG(mcp, k) = mc;
          if (first || lo_dirty) store(lo, k);  // level k is final for this pass
          lo = up;
          lo_dirty = up_dirty;
          pe_below = pe_lo;
          pe_lo = cur.pe;
        }
        if (first || lo_dirty) store(lo, 0);
      }
    }
    // ---- the closing walk: relaxation, outputs, tendencies; a column without a mixed pair keeps its pt, w and species untouched
    for (int k = 0; k < nz; ++k) {
      Real ud = zero, vd = zero;
      if (k < kb && any) {
        auto relax = [&](Real x, Real x_in) { return m.blend ? x_in + (x - x_in) * m.fra : x; };
        const Real u_in = SG(m.ua, k), v_in = SG(m.va, k);
        ud = m.rdt * (relax(SG(m.u_dt, k), u_in) - u_in);
        vd = m.rdt * (relax(SG(m.v_dt, k), v_in) - v_in);
        SG(m.pt_out, k) = relax(SG(m.t0, k), SG(m.pt, k));
        SG(m.w_out, k) = relax(SG(m.w0, k), SG(m.w, k));
        if constexpr (MOIST) {
#pragma unroll
          for (int n = 0; n < 6; ++n)
            if (m.q[n]) SG(m.q[n], k) = relax(SG(m.q0[n], k), SG(m.q[n], k));
        }
      }
      SG(m.u_dt, k) = ud;
      SG(m.v_dt, k) = vd;
    }
  });
}

template <int NG>
struct SgPassive {
  Real *q[NG], *q0[NG];
  const Real *mc[3], *delp;
  Real fra;
  int kbot, blend;
};

// tracers that only see mc: the same three walks and the closing walk, the pair's mc read instead of formed
template <int NG>
void subgridz_passive(fv3_ctx *c, fv3_stream_t s, const SgPassive<NG> m) {
  const Geo g = c->g;
  launch2(c, s, Box{1, g.nx, 1, g.ny, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const int kb = m.kbot;
    const long tb = t * g.st, sk = g.sk;
    const unsigned pix = IX(i, j);
    const Real zero = (Real)0;
    bool any = false;
    for (int pass = 0; pass < 3; ++pass) {
      const bool first = pass == 0;
      const Real *const mcp = pass == 0 ? m.mc[0] : (pass == 1 ? m.mc[1] : m.mc[2]);
      Real lo[NG], up[NG];
#pragma unroll
      for (int n = 0; n < NG; ++n) lo[n] = SG(first ? m.q[n] : m.q0[n], kb - 1);
      Real dpk = SG(m.delp, kb - 1);
      bool lo_dirty = false;
      for (int k = kb - 1; k >= 1; --k) {
        const Real mc = SG(mcp, k), dpm = SG(m.delp, k - 1);
#pragma unroll
        for (int n = 0; n < NG; ++n) up[n] = SG(first ? m.q[n] : m.q0[n], k - 1);
        bool up_dirty = false;
        if (mc > zero) {
          any = true;
          lo_dirty = up_dirty = true;
#pragma unroll
          for (int n = 0; n < NG; ++n) sg_mix(mc, dpm, dpk, up[n], lo[n]);
        }
        if (first || lo_dirty) {
#pragma unroll
          for (int n = 0; n < NG; ++n) SG(m.q0[n], k) = lo[n];
        }
#pragma unroll
        for (int n = 0; n < NG; ++n) lo[n] = up[n];
        lo_dirty = up_dirty;
        dpk = dpm;
      }
      if (first || lo_dirty) {
#pragma unroll
        for (int n = 0; n < NG; ++n) SG(m.q0[n], 0) = lo[n];
      }
    }
    if (!any) return;
    for (int k = 0; k < kb; ++k) {
#pragma unroll
      for (int n = 0; n < NG; ++n) {
        const Real x = SG(m.q0[n], k), x_in = SG(m.q[n], k);
        SG(m.q[n], k) = m.blend ? x_in + (x - x_in) * m.fra : x;
      }
    }
  });
}

template <int NG>
void passive_launch(fv3_ctx *c, fv3_stream_t s, Real *const *q, Real *const *q0, const SgIn &in) {
  SgPassive<NG> p;
  for (int n = 0; n < NG; ++n) p.q[n] = q[n], p.q0[n] = q0[n];
  for (int n = 0; n < 3; ++n) p.mc[n] = in.mc[n];
  p.delp = in.delp, p.fra = in.fra, p.kbot = in.kbot, p.blend = in.blend;
  subgridz_passive<NG>(c, s, p);
}

struct SgNamed {
  std::string name;
  const void *ptr;
  bool written;
};

}  // namespace

extern "C" int fv3_subgrid_z(fv3_ctx *c, const fv3_subgridz_params *p, const fv3_water *water, int n_tracers, const fv3_field *const *tracers,
                             const fv3_field *ua, const fv3_field *va, const fv3_field *w, const fv3_field *pt, const fv3_field *delp,
                             const fv3_field *delz, const fv3_field *peln, const fv3_field *pkz, const fv3_field *u_dt, const fv3_field *v_dt,
                             int n_work, const fv3_field *const *work, void *stream) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: the context is null");
  if (!p) return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: the fv3_subgridz_params is null");
  if (!(p->dt > 0.0) || !(p->dt < HUGE_VAL)) return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: dt must be finite and > 0");
  if (!(p->tau > 0.0)) return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: tau must be > 0");
  if (p->kbot < 0) return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: kbot = " + std::to_string(p->kbot) + " is negative");
  if (n_tracers < 0) return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: n_tracers = " + std::to_string(n_tracers) + " is negative");
  if (n_tracers > 0 && !tracers) return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: the tracer list is null with n_tracers = " + std::to_string(n_tracers));
  SgIn m{};
  std::vector<SgNamed> all;
  auto field = [&](const fv3_field *f, const char *name, bool written) -> Real * {
    Real *q = fv3_chk(c, f, name);  // (every 3-D field of the context's layout has nz + 1 levels: peln's interfaces fit)
    if (q) all.push_back(SgNamed{name, q, written});
    return q;
  };
  if (!(m.ua = field(ua, "ua", false)) || !(m.va = field(va, "va", false)) || !(m.w_out = field(w, "w", true)) || !(m.pt_out = field(pt, "pt", true)) ||
      !(m.delp = field(delp, "delp", false)) || !(m.delz = field(delz, "delz", false)) || !(m.peln = field(peln, "peln", false)) ||
      !(m.pkz = field(pkz, "pkz", false)) || !(m.u_dt = field(u_dt, "u_dt", true)) || !(m.v_dt = field(v_dt, "v_dt", true)))
    return FV3_ERR_ARG;
  m.w = m.w_out, m.pt = m.pt_out;
  std::vector<Real *> q(n_tracers);
  for (int n = 0; n < n_tracers; ++n) {
    const std::string name = "tracer " + std::to_string(n);
    if (!(q[n] = field(tracers[n], name.c_str(), true))) return FV3_ERR_ARG;
  }
  // the species are tracers of the list: they are mixed by the main walk, the others by the passive kernel
  std::vector<int> role(n_tracers, -1);
  MoistIn mi{};
  if (water) {
    if (int st = fv3_moist_in(c, "subgrid_z", water, &mi)) return st;
    const Real *sp[6] = {mi.qv, mi.ql, mi.qr, mi.qi, mi.qs, mi.qg};
    static const char *const names[6] = {"qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel"};
    for (int a = 0; a < 6; ++a) {
      if (!sp[a]) continue;
      int at = -1;
      for (int n = 0; n < n_tracers; ++n)
        if (q[n] == sp[a] && at < 0) at = n;
      if (at < 0) return fv3_fail(c, FV3_ERR_ARG, std::string("subgrid_z: ") + names[a] + " is not among the tracers (the species are mixed like every tracer)");
      if (role[at] >= 0) return fv3_fail(c, FV3_ERR_ARG, std::string("subgrid_z: ") + names[role[at]] + " and " + names[a] + " are the same field");
      role[at] = a;
    }
  }
  int n_passive = 0;
  for (int n = 0; n < n_tracers; ++n) n_passive += role[n] < 0;
  const int need = 2 + n_tracers + (n_passive ? 3 : 0);
  if (n_work < need || (need > 0 && !work))
    return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: " + std::to_string(n_work < 0 ? 0 : n_work) + " work fields given, " + std::to_string(need) +
                                        " needed (t0, w0, one per tracer, and three for the exchanged mass when a tracer is not a water species)");
  std::vector<Real *> wk(need);
  for (int n = 0; n < need; ++n) {
    const std::string name = "work " + std::to_string(n);
    if (!(wk[n] = field(work[n], name.c_str(), true))) return FV3_ERR_ARG;
  }
  // a thread reads a level of every field before it writes any of them: a written field given twice would make the result depend on the order
  for (size_t a = 0; a < all.size(); ++a)
    for (size_t b = 0; b < a; ++b)
      if (all[a].ptr == all[b].ptr && (all[a].written || all[b].written))
        return fv3_fail(c, FV3_ERR_ARG, "subgrid_z: " + all[b].name + " and " + all[a].name + " are the same field");
  const Geo &g = c->g;
  const fv3_constants &k = c->cst;
  m.w0 = wk[1], m.t0 = wk[0];
  std::vector<Real *> pq, pq0;
  for (int n = 0; n < n_tracers; ++n) {
    if (role[n] >= 0)
      m.q[role[n]] = q[n], m.q0[role[n]] = wk[2 + n];
    else
      pq.push_back(q[n]), pq0.push_back(wk[2 + n]);
  }
  if (n_passive)
    for (int n = 0; n < 3; ++n) m.mc[n] = wk[2 + n_tracers + n];
  m.grav = (Real)k.grav, m.g2 = (Real)(0.5 * k.grav), m.cv_air = (Real)(k.cp_air - k.rdgas);
  m.xvir = water ? (Real)(k.rvgas / k.rdgas - 1.0) : (Real)0;
  m.cv_vap = water ? (Real)water->cv_vap : (Real)0, m.c_liq = water ? (Real)water->c_liq : (Real)0, m.c_ice = water ? (Real)water->c_ice : (Real)0;
  m.t_min = (Real)p->t_min, m.t_max = (Real)p->t_max;
  m.fra = (Real)(p->dt / p->tau), m.rdt = (Real)(1.0 / p->dt);
  m.blend = m.fra < (Real)1;
  m.kbot = p->kbot < g.nz ? p->kbot : g.nz;
  fv3_stream_t s = (fv3_stream_t)stream;
  if (water)
    subgridz_columns<true>(c, s, m);
  else
    subgridz_columns<false>(c, s, m);
  if (m.kbot >= 3) {
    for (int n0 = 0; n0 < n_passive; n0 += 4) {
      const int ng = n_passive - n0 < 4 ? n_passive - n0 : 4;
      if (ng == 4)
        passive_launch<4>(c, s, pq.data() + n0, pq0.data() + n0, m);
      else if (ng == 3)
        passive_launch<3>(c, s, pq.data() + n0, pq0.data() + n0, m);
      else if (ng == 2)
        passive_launch<2>(c, s, pq.data() + n0, pq0.data() + n0, m);
      else
        passive_launch<1>(c, s, pq.data() + n0, pq0.data() + n0, m);
    }
  }
  return fv3_post(c, s, "subgrid_z");
}

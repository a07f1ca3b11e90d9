// fv3_hs.hip -- Held-Suarez (1994) forcing as cell-centre tendencies: Newtonian relaxation of the temperature to an analytic
// equilibrium and Rayleigh friction on the low-level winds (Held & Suarez, Bull. Amer. Meteor. Soc. 75 (1994) 1825-1830; FV3 carries
// the same forcing in fv_phys.F90).  Restated from the paper:
//   sigma = p / ps,  s = max(0, (sigma - sigma_b) / (1 - sigma_b))
//   k_v = k_f s,     k_T = k_a + (k_s - k_a) s cos^4(lat)
//   T_eq = max(T_min, [315 - dT_y sin^2(lat) - dth_z ln(p / p0) cos^2(lat)] (p / p0)^kappa)
// and the tendencies in the implicit form (stable for any dt; dt -> 0 is the paper's explicit form):
//   u_dt = -k_v / (1 + dt k_v) ua,  v_dt likewise from va,  t_dt = -k_T / (1 + dt k_T) (T - T_eq).
// The kernel is stateless and forms the pressure itself: the interface pressures are a downward scan pe(k+1) = pe(k) + delp(k) from
// pe(0) = ptop, ps = pe(nz), p = 0.5 (pe(k) + pe(k+1)).
//
// One thread per column, lanes along i (every level access is one coalesced row); the latitude terms are formed once per column.
// The first sweep over delp only forms ps, the second one reads it again with ua, va, pt: 5 reads + 3 writes per cell, memory-bound.
#include "fv3_common.h"
#include "fv3_math.h"

extern "C" int fv3_held_suarez_tend(fv3_ctx *c, const fv3_held_suarez *hs, const fv3_field *ua_, const fv3_field *va_, const fv3_field *pt_,
                                    const fv3_field *delp_, const fv3_field *lat_, const fv3_field *u_dt_, const fv3_field *v_dt_,
                                    const fv3_field *t_dt_, double ptop, double dt, void *stream) {
  if (!hs) return fv3_fail(c, FV3_ERR_ARG, "held_suarez_tend: null parameters");
  if (!(dt >= 0.0) || !(dt < HUGE_VAL)) return fv3_fail(c, FV3_ERR_ARG, "held_suarez_tend: dt must be finite and >= 0");
  if (!(ptop >= 0.0)) return fv3_fail(c, FV3_ERR_ARG, "held_suarez_tend: ptop must be >= 0");
  if (!(hs->sigma_b >= 0.0 && hs->sigma_b < 1.0) || !(hs->p0 > 0.0) || !(hs->k_f >= 0.0) || !(hs->k_a >= 0.0) || !(hs->k_s >= 0.0))
    return fv3_fail(c, FV3_ERR_ARG, "held_suarez_tend: parameters (0 <= sigma_b < 1, p0 > 0, k_f, k_a, k_s >= 0)");
  FV3_FIELD(ua, ua_) FV3_FIELD(va, va_) FV3_FIELD(pt, pt_) FV3_FIELD(delp, delp_)
  FV3_FIELD(u_dt, u_dt_) FV3_FIELD(v_dt, v_dt_) FV3_FIELD(t_dt, t_dt_)
  FV3_FIELD2D(lat, lat_)
  const Real *in[4] = {ua, va, pt, delp};
  Real *out[3] = {u_dt, v_dt, t_dt};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 4; ++b)
      if (out[a] == in[b]) return fv3_fail(c, FV3_ERR_ARG, "held_suarez_tend: u_dt / v_dt / t_dt must not alias ua / va / pt / delp");
    for (int b = a + 1; b < 3; ++b)
      if (out[a] == out[b]) return fv3_fail(c, FV3_ERR_ARG, "held_suarez_tend: u_dt, v_dt and t_dt must be three fields");
  }
  const Geo g = c->g;
  const Real sigma_b = (Real)hs->sigma_b, k_f = (Real)hs->k_f, k_a = (Real)hs->k_a, k_s = (Real)hs->k_s, dty = (Real)hs->delta_t_y,
             dthz = (Real)hs->delta_theta_z, rp0 = (Real)hs->p0, kappa = (Real)hs->kappa, t_min = (Real)hs->t_min;
  const Real top = (Real)ptop, rdt = (Real)dt;
  launch2(c, (fv3_stream_t)stream, Box{1, g.nx, 1, g.ny, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const unsigned p = IX(i, j);
    const Real phi = lat[t * g.st2 + p];
    const Real sl = sin(phi), cl = cos(phi);
    const Real s2 = sl * sl, c2 = cl * cl;
    const Real c4 = c2 * c2;
    const long q = t * g.st + p;
    Real ps = top;
    {
      const Real *dk = delp + q;
      for (int k = 0; k < g.nz; ++k, dk += g.sk) ps += *dk;
    }
    const Real one_sb = (Real)1 - sigma_b, dks = k_s - k_a;
    Real pe = top;
    const Real *dk = delp + q, *uk = ua + q, *vk = va + q, *tk = pt + q;
    Real *udk = u_dt + q, *vdk = v_dt + q, *tdk = t_dt + q;
    for (int k = 0; k < g.nz; ++k, dk += g.sk, uk += g.sk, vk += g.sk, tk += g.sk, udk += g.sk, vdk += g.sk, tdk += g.sk) {
      const Real pe1 = pe + *dk;
      const Real pm = (Real)0.5 * (pe + pe1);
      pe = pe1;
      const Real s = fv3_max((Real)0, (pm / ps - sigma_b) / one_sb);
      const Real kv = k_f * s;
      const Real kt = k_a + (dks * s) * c4;
      const Real lr = fv3_log(pm / rp0);
      const Real teq = fv3_max(t_min, (((Real)315 - dty * s2) - (dthz * lr) * c2) * fv3_exp(kappa * lr));
      const Real fv = kv / ((Real)1 + rdt * kv);
      FV3_ST_NT(*udk, -fv * *uk);
      FV3_ST_NT(*vdk, -fv * *vk);
      FV3_ST_NT(*tdk, -(kt / ((Real)1 + rdt * kt)) * (*tk - teq));
    }
  });
  return fv3_post(c, (fv3_stream_t)stream, "held_suarez_tend");
}

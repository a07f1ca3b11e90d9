// fv3_negadj.hip -- negative water species at the end of DynamicalCore.step_dynamics (FV3 fv_sg.F90, subroutine neg_adj3 in its
// non-hydrostatic form; pyFV3 AdjustNegativeTracerMixingRatio, run between the last remap and CubedToLatLon when nwat = 6).  A negative
// condensate is paid for out of another phase, the latent heat booked on the temperature; negative vapour is repaid from the layer
// below.  Column-local, in place, on the compute cells and levels 0 .. nz-1; dp (delp) is only read.
//
// Per cell, from the cell's incoming values (every sum, product and quotient rounded on its own in the order written):
//   q_liq = max(0, ql + qr);  q_sol = max(0, qi + qs)                                                      (graupel is not in q_sol)
//   cpm   = (((1 - ((qv + q_liq) + q_sol)) * cv_air + qv * cv_vap) + q_liq * c_liq) + q_sol * c_ice
//   lcpk  = (lv00 + d0_vap * pt) / cpm;  icpk = (li00 + dc_ice * pt) / cpm
// then, each test seeing the results of the ones before it:
//   qi < 0: qs += qi, qi = 0;   qs < 0: qg += qs, qs = 0;   qg < 0: qr += qg, pt -= qg * icpk, qg = 0;
//   qr < 0: ql += qr, qr = 0;   ql < 0: qv += ql, pt -= ql * lcpk, ql = 0
// Per column, after the cell step of all its levels (vapour only):
//   k = 0 .. km-2 in increasing order, qv[k] < 0: qv[k+1] += (qv[k] * dp[k]) / dp[k+1], qv[k] = 0
//   bottom: qv[km-1] < 0 and qv[km-2] > 0: dq = min(-qv[km-1] * dp[km-1], qv[km-2] * dp[km-2]);
//           qv[km-2] -= dq / dp[km-2], qv[km-1] += dq / dp[km-1]
// Comparisons are plain IEEE (-0.0 and NaN take no branch); max(0, x) is `x > 0 ? x : 0`, min(a, b) is `a < b ? a : b`.
//
// A thread owns a column (i fastest: every level access of a wave is one coalesced row) and walks down it ONCE: the cell step of level
// k reads qv[k] before anything is added to it, so "cell step of k, add the carry from k-1, test and pass the carry on" gives the
// two-loop result bit for bit.  The eight loads of level k+1 are issued before the arithmetic of level k.  qv and dp of the previous
// level stay in registers until the next level has been handled, so the bottom step can still change level km-2.  cpm, lcpk and icpk
// (the quotients of a cell) are formed only in the cells that take a heating branch.  A value is stored only where a branch changed
// it (one dirty bit per value): on data without negatives the kernel reads 8 fields and writes nothing.  No LDS, no scratch.
#include "fv3_common.h"

namespace {

struct NegAdjIn {
  Real *qv, *ql, *qr, *qi, *qs, *qg, *pt;
  const Real *dp;
  Real cv_air, cv_vap, c_liq, c_ice, d0_vap, lv00, dc_ice, li00;
};

// level k of a field at the thread's column: wave-uniform plane base + 32-bit in-plane offset
#define NA(ptr, k) FV3_EL((ptr) + tb + (long)(k)*sk, pix)

void neg_adj_columns(fv3_ctx *c, fv3_stream_t s, const NegAdjIn m) {
  const Geo g = c->g;
  launch2(c, s, Box{1, g.nx, 1, g.ny, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const int km = g.nz;
    const long tb = t * g.st, sk = g.sk;
    const unsigned pix = IX(i, j);
    const Real zero = (Real)0;
    // the level in flight (n*: the prefetched next one) and what is held back of the previous one: its vapour, its dp, its dirty bit
    Real qv = NA(m.qv, 0), ql = NA(m.ql, 0), qr = NA(m.qr, 0), qi = NA(m.qi, 0), qs = NA(m.qs, 0), qg = NA(m.qg, 0), pt = NA(m.pt, 0), dp = NA(m.dp, 0);
    Real qv_p = zero, dp_p = (Real)1;
    bool dirty_p = false;
    for (int k = 0; k < km; ++k) {
      const int kn = k + 1 < km ? k + 1 : km - 1;  // (the pad level is never read: the last level again)
      const Real nqv = NA(m.qv, kn), nql = NA(m.ql, kn), nqr = NA(m.qr, kn), nqi = NA(m.qi, kn), nqs = NA(m.qs, kn), nqg = NA(m.qg, kn), npt = NA(m.pt, kn), ndp = NA(m.dp, kn);
      // ---- the cell step of level k; bits of `hit`: 1 qi, 2 qs, 4 qg, 8 qr, 16 ql took its branch
      const Real qv0 = qv, pt0 = pt, sl = ql + qr, ss = qi + qs;
      unsigned hit = 0u;
      if (qi < zero) {
        qs = qs + qi;
        qi = zero;
        hit |= 1u;
      }
      if (qs < zero) {
        qg = qg + qs;
        qs = zero;
        hit |= 2u;
      }
      const Real qg_neg = qg;
      if (qg < zero) {
        qr = qr + qg;
        qg = zero;
        hit |= 4u;
      }
      if (qr < zero) {
        ql = ql + qr;
        qr = zero;
        hit |= 8u;
      }
      const Real ql_neg = ql;
      if (ql < zero) {
        qv = qv + ql;
        ql = zero;
        hit |= 16u;
      }
      if (hit & 20u) {  // a heating branch: the moist heat capacity and the latent heats over it, from the incoming values
        const Real q_liq = sl > zero ? sl : zero, q_sol = ss > zero ? ss : zero;
        const Real cpm = ((((Real)1 - ((qv0 + q_liq) + q_sol)) * m.cv_air + qv0 * m.cv_vap) + q_liq * m.c_liq) + q_sol * m.c_ice;
        if (hit & 4u) {
          const Real icpk = (m.li00 + m.dc_ice * pt0) / cpm;
          pt = pt - qg_neg * icpk;
        }
        if (hit & 16u) {
          const Real lcpk = (m.lv00 + m.d0_vap * pt0) / cpm;
          pt = pt - ql_neg * lcpk;
        }
        NA(m.pt, k) = pt;
      }
      if (hit) {  // (rare: a value is stored where its own branch or the one that feeds it was taken)
        if (hit & 1u) NA(m.qi, k) = qi;
        if (hit & 3u) NA(m.qs, k) = qs;
        if (hit & 6u) NA(m.qg, k) = qg;
        if (hit & 12u) NA(m.qr, k) = qr;
        if (hit & 24u) NA(m.ql, k) = ql;
      }
      bool dirty = (hit & 16u) != 0u;
      // ---- the carry from level k-1 arrives; on the last level the bottom step follows; level k-1 is then final
      if (k >= 1) {
        if (qv_p < zero) {
          qv = qv + (qv_p * dp_p) / dp;
          qv_p = zero;
          dirty_p = dirty = true;
        }
        if (k == km - 1 && qv < zero && qv_p > zero) {
          const Real up = -qv * dp, av = qv_p * dp_p;
          const Real dq = up < av ? up : av;
          qv_p = qv_p - dq / dp_p;
          qv = qv + dq / dp;
          dirty_p = dirty = true;
        }
        if (dirty_p) NA(m.qv, k - 1) = qv_p;
      }
      qv_p = qv;
      dp_p = dp;
      dirty_p = dirty;
      qv = nqv, ql = nql, qr = nqr, qi = nqi, qs = nqs, qg = nqg, pt = npt, dp = ndp;
    }
    if (dirty_p) NA(m.qv, km - 1) = qv_p;
  });
}

}  // namespace

extern "C" int fv3_neg_adj3(fv3_ctx *c, const fv3_water *water, const fv3_latent *latent, const fv3_field *pt_, const fv3_field *delp_, void *stream) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "neg_adj3: the context is null");
  if (!water) return fv3_fail(c, FV3_ERR_ARG, "neg_adj3: the fv3_water is null");
  if (!latent) return fv3_fail(c, FV3_ERR_ARG, "neg_adj3: the fv3_latent is null");
  const fv3_field *f[6] = {water->qvapor, water->qliquid, water->qrain, water->qice, water->qsnow, water->qgraupel};
  static const char *const names[6] = {"qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel"};
  Real *q[6];
  for (int n = 0; n < 6; ++n) {  // (all six: a species that is absent cannot be paid from, or into)
    q[n] = fv3_chk(c, f[n], names[n]);
    if (!q[n]) return FV3_ERR_ARG;
  }
  Real *pt = fv3_chk(c, pt_, "pt");
  if (!pt) return FV3_ERR_ARG;
  Real *delp = fv3_chk(c, delp_, "delp");
  if (!delp) return FV3_ERR_ARG;
  // a thread reads a level of all eight fields before it writes any: a field given twice would make the result depend on the order
  for (int n = 0; n < 6; ++n) {
    for (int k = 0; k < n; ++k)
      if (q[k] == q[n]) return fv3_fail(c, FV3_ERR_ARG, std::string("neg_adj3: ") + names[k] + " and " + names[n] + " are the same field");
    if (q[n] == pt) return fv3_fail(c, FV3_ERR_ARG, std::string("neg_adj3: pt is the ") + names[n] + " field");
    if (q[n] == delp) return fv3_fail(c, FV3_ERR_ARG, std::string("neg_adj3: delp is the ") + names[n] + " field (delp is only read)");
  }
  if (pt == delp) return fv3_fail(c, FV3_ERR_ARG, "neg_adj3: pt and delp are the same field (delp is only read)");
  if (c->g.nz < 2) return fv3_fail(c, FV3_ERR_UNSUPPORTED, "neg_adj3: needs at least 2 levels (nz = " + std::to_string(c->g.nz) + ")");
  const fv3_constants &k = c->cst;
  NegAdjIn m;
  m.qv = q[0], m.ql = q[1], m.qr = q[2], m.qi = q[3], m.qs = q[4], m.qg = q[5], m.pt = pt, m.dp = delp;
  m.cv_air = (Real)(k.cp_air - k.rdgas);
  m.cv_vap = (Real)water->cv_vap;
  m.c_liq = (Real)water->c_liq;
  m.c_ice = (Real)water->c_ice;
  m.d0_vap = (Real)(water->cv_vap - water->c_liq);
  m.lv00 = (Real)(latent->hlv - (water->cv_vap - water->c_liq) * latent->t_ice);
  m.dc_ice = (Real)(water->c_liq - water->c_ice);
  m.li00 = (Real)(latent->hlf - (water->c_liq - water->c_ice) * latent->t_ice);
  fv3_stream_t s = (fv3_stream_t)stream;
  neg_adj_columns(c, s, m);
  return fv3_post(c, s, "neg_adj3");
}

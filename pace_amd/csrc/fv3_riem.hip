// fv3_riem.hip -- the SIM1 Riemann solvers of the non-hydrostatic height chain: Riem_Solver_c, Riem_Solver3.  CPU twin: oracle/fv3_oracle/nh.py.
// [SURVEY A.5-A.12]
//
// Each operator is: field checks, riem_plan() -- the form, the gam storage, the hand-off of update_dz_d's scan and the waves of the pass, decided by the
// pure functions of fv3_col_plan.h -- then the wave stage or the column stage.
//
// Column kernels: one thread per (i, j) column walks k; because i is the fastest index every
// per-level access of a wavefront is one coalesced row.  Per-level temporaries that do not fit
// registers (tridiagonal gam / pp / w) live in context scratch fields with the same layout.
#include "fv3_ops.h"
#include "fv3_kwalk.h"
#include "fv3_col_plan.h"
#include "fv3_math.h"
#include "fv3_agpr.h"

namespace {

// SIM1_solver (MOIST_CAPPA form).  On entry: DZ = layer thickness (negative), W2 = w, PM = layer
// mean pressure; delp / cappa / pt are the column inputs.  PP (nz+1), GAM, W2 are scratch.
// On exit: W2 = new w, DZ = new dz, PE (nz+1) = non-hydrostatic pressure perturbation.
struct Sim1 {
  Geo g;
  Real rgas, rgrav, p_fac, ptop;
  // setup(k, pm, dz): produces (and stores) the layer-mean pressure and thickness of level k; called once per
  //   level, in increasing k, from inside the first sweep (the caller's own prefix sums live in the functor);
  // finish(k, dz): consumes the new thickness of level k; called once per level, in decreasing k, from inside
  //   the last sweep;
  // wout (optional): receives the new w (written in the pressure-perturbation sweep, after the old w is read).
  // The sweeps are fused where their directions agree: 6 column walks instead of 8, no read-back of PM / DZ
  // in the first one and of DZ / W2 in the last one.
  template <class Setup, class Finish>
  FV3_HD void run(long tb, unsigned pix, Real dt, const Real *delp, const Real *cappa, const Real *pt, const Real *w1, Real ws, Real *PM, Real *DZ, Real *W2, Real *PP,
                  Real *GAM, Real *PE, Real *wout, Setup setup, Finish finish) const {
    const int nz = g.nz;
    const Real t1g = (Real)2.0 * dt * dt, rdt = (Real)1.0 / dt, r3 = (Real)(1.0 / 3.0);
    auto DM = [&](int k) { return K_(delp, k) * rgrav; };
    auto GM = [&](int k) { return (Real)1.0 / ((Real)1.0 - K_(cappa, k)); };
    // ---- sweep 1 (up): caller's setup + forward elimination for pp
    {
      Real pm_k, dz_k;
      setup(0, pm_k, dz_k);
      Real dm_m = (Real)0, dm_k = DM(0);
      Real pe_k = fv3_exp(GM(0) * fv3_log(-dm_k / dz_k * rgas * K_(pt, 0))) - pm_k;
      Real bet = (Real)0;
      K_(PP, 0) = (Real)0;
      for (int k = 0; k < nz; ++k) {
        Real bb, dd;
        Real pe_n = (Real)0, dm_n = (Real)0;
        if (k < nz - 1) {
          Real pm_n, dz_n;
          setup(k + 1, pm_n, dz_n);
          dm_n = DM(k + 1);
          const Real g_rat = dm_k / dm_n;
          pe_n = fv3_exp(GM(k + 1) * fv3_log(-dm_n / dz_n * rgas * K_(pt, k + 1))) - pm_n;
          bb = (Real)2.0 * ((Real)1.0 + g_rat);
          dd = (Real)3.0 * (pe_k + g_rat * pe_n);
        } else {
          bb = (Real)2.0;
          dd = (Real)3.0 * pe_k;
        }
        if (k == 0) {
          bet = bb;
          K_(PP, 1) = dd / bet;
        } else {
          const Real g_prev = dm_m / dm_k;
          const Real gam = g_prev / bet;
          K_(GAM, k) = gam;
          bet = bb - gam;
          K_(PP, k + 1) = (dd - K_(PP, k)) / bet;
        }
        pe_k = pe_n;
        dm_m = dm_k;
        dm_k = dm_n;
      }
      // ---- sweep 2 (down): back substitution
      for (int k = nz - 1; k >= 1; --k) K_(PP, k) = K_(PP, k) - K_(GAM, k) * K_(PP, k + 1);
    }
    // ---- sweep 3 (up): forward elimination for w
    {
      // pem[k] rolling prefix sum (same operation order as the setup pass)
      Real pem_k = ptop;  // pem[0]
      auto AA = [&](int k, Real pem_at_k) {
        return t1g * (Real)0.5 * (GM(k - 1) + GM(k)) / (K_(DZ, k - 1) + K_(DZ, k)) * (pem_at_k + K_(PP, k));
      };
      Real pem1 = pem_k + K_(delp, 0);  // pem[1]
      Real aa_k1 = AA(1, pem1);         // aa[1]
      Real bet = DM(0) - aa_k1;
      K_(W2, 0) = (DM(0) * K_(w1, 0) + dt * K_(PP, 1)) / bet;
      Real pem_cur = pem1;  // pem[k] for k = 1
      Real aa_k = aa_k1;
      for (int k = 1; k < nz - 1; ++k) {
        const Real pem_next = pem_cur + K_(delp, k);  // pem[k+1]
        const Real aa_n = AA(k + 1, pem_next);
        const Real gam = aa_k / bet;
        K_(GAM, k) = gam;
        bet = DM(k) - (aa_k + aa_n + aa_k * gam);
        K_(W2, k) = (DM(k) * K_(w1, k) + dt * (K_(PP, k + 1) - K_(PP, k)) - aa_k * K_(W2, k - 1)) / bet;
        aa_k = aa_n;
        pem_cur = pem_next;
      }
      // pem_cur = pem[nz-1]; bottom
      const Real pem_nz = pem_cur + K_(delp, nz - 1);
      const Real p1 = t1g * GM(nz - 1) / K_(DZ, nz - 1) * (pem_nz + K_(PP, nz));
      const Real gam = aa_k / bet;
      K_(GAM, nz - 1) = gam;
      bet = DM(nz - 1) - (aa_k + p1 + aa_k * gam);
      K_(W2, nz - 1) = (DM(nz - 1) * K_(w1, nz - 1) + dt * (K_(PP, nz) - K_(PP, nz - 1)) - p1 * ws - aa_k * K_(W2, nz - 2)) / bet;
      // ---- sweep 4 (down): back substitution
      for (int k = nz - 2; k >= 0; --k) K_(W2, k) = K_(W2, k) - K_(GAM, k + 1) * K_(W2, k + 1);
    }
    // ---- sweep 5 (up): new pressure perturbation (+ the new w leaves through wout)
    K_(PE, 0) = (Real)0;
    for (int k = 0; k < nz; ++k) {
      const Real w2k = K_(W2, k);
      K_(PE, k + 1) = K_(PE, k) + DM(k) * (w2k - K_(w1, k)) * rdt;
      if (wout) K_(wout, k) = w2k;
    }
    // ---- sweep 6 (down): new layer thickness, handed to the caller's finish
    Real p1 = (K_(PE, nz - 1) + (Real)2.0 * K_(PE, nz)) * r3;
    {
      const Real dzn = -DM(nz - 1) * rgas * K_(pt, nz - 1) * fv3_exp((K_(cappa, nz - 1) - (Real)1.0) * fv3_log(fv3_max(p_fac * K_(PM, nz - 1), p1 + K_(PM, nz - 1))));
      K_(DZ, nz - 1) = dzn;
      finish(nz - 1, dzn);
    }
    for (int k = nz - 2; k >= 0; --k) {
      const Real g_rat = DM(k) / DM(k + 1);
      const Real bb = (Real)2.0 * ((Real)1.0 + g_rat);
      p1 = (K_(PE, k) + bb * K_(PE, k + 1) + g_rat * K_(PE, k + 2)) * r3 - g_rat * p1;
      const Real dzn = -DM(k) * rgas * K_(pt, k) * fv3_exp((K_(cappa, k) - (Real)1.0) * fv3_log(fv3_max(p_fac * K_(PM, k), p1 + K_(PM, k))));
      K_(DZ, k) = dzn;
      finish(k, dzn);
    }
  }
};

// ---------------------------------------------------------------------------------------------
// SIM1 as a wave kernel.  The column solver above moves ~45 full-field passes through HBM per call
// (every tridiagonal temporary is a context scratch field); here a lane owns one column, the
// PP -> W2 -> PE chain of temporaries lives in ONE LDS line per lane (slot k of a column's line
// holds PP(k+1), then W2(k), then PE(k+1): each value dies exactly where its successor is born),
// the two gam arrays live in the lane's ACCUMULATION registers (RA form, fv3_agpr.h: a wave at one wave per SIMD owns 512
// registers per lane and the solver uses a third of them), only PM still goes through memory, and the old thickness is
// recomputed from the interface heights instead of being stored.  nz * 512 B of LDS per wave = 4 waves / CU at L79, so
// memory-level parallelism comes from explicit register prefetch: KWALK keeps U levels of every input in flight while the U
// levels loaded before are being computed.  At one wave per SIMD nothing hides a wave's own VALU time: fields are addressed as
// scalar base + 32-bit byte offset (KW_), divisions use the unscaled sequence (fv3_div), log / exp are range-specific (fv3_math.h).
// Operation order per value is the one of Sim1::run (bitwise the same results).
// ---------------------------------------------------------------------------------------------
// RA form of Sim1W::run: the tridiagonal `gam` of a column lives in the lane's accumulation registers (fv3_agpr.h) instead of going
// through the scratch field GAM -- four field passes less per call.  80 levels at most, fp64 build; deeper columns keep the scratch field.
#define FV3_KREG_LEVELS (sizeof(Real) == 8 ? FV3_AGPR_LEVELS : FV3_AGPR_LEVELS_F32)
#if defined(__HIP_DEVICE_COMPILE__)
// (level k of the column sits in slot k + 1: the forward sweeps produce gam(m - 1) while they walk level m, so the four values of a
//  U = 4 loop iteration are the slots c_ .. c_ + 3 = ONE aligned group, stored by one access site per sweep: KREG_SET4)
#define KREG_DECL(n)
#define KREG_SET(n, k, v) fv3_agpr_set((k) + 1, (Real)(v))
#define KREG_GET(n, k) fv3_kreg_get((Real)0, (k) + 1)
#define KREG_SET4(n, c, q) fv3_agpr_set4((c) >> 2, (q)[0], (q)[1], (q)[2], (q)[3])
__device__ __attribute__((always_inline)) inline double fv3_kreg_get(double, int k) { return fv3_agpr_get(k); }
__device__ __attribute__((always_inline)) inline float fv3_kreg_get(float, int k) { return fv3_agpr_get_f32(k); }
#else
#define KREG_DECL(n) Real n[FV3_AGPR_LEVELS_F32 + 4]
#define KREG_SET(n, k, v) n[(k) + 1] = (v)
#define KREG_GET(n, k) n[(k) + 1]
#define KREG_SET4(n, c, q) n[c] = (q)[0], n[(c) + 1] = (q)[1], n[(c) + 2] = (q)[2], n[(c) + 3] = (q)[3]
#endif

struct Sim1W {
  long sk;
  int nz;
  Real rgas, rgrav, p_fac, ptop;
  // cl.pm(k, delp_k, qcon_k): layer-mean pressure of level k (called once per level, increasing k);
  // cl.out_pe(k1, pe, delp_k): new pressure perturbation at interface k1 = k + 1 (increasing k);
  // cl.finish(k, dz): new thickness of level k (decreasing k).
  // A = this lane's LDS line (stride FV3_WAVE); zint = interface heights (nz + 1 levels) the old
  // thickness comes from; wout (optional, may alias w1) receives the new w.
  // GL: the gam arrays live in a second LDS line B (2 waves / CU at L79) instead of the scratch field GAM.
  // RA: gam lives in the lane's accumulation registers (KREG_*; nz <= FV3_KREG_LEVELS): four field passes less per call.
  // ZL: sweep 1 takes the interface heights from the LDS line A instead of zint -- z(k + 1) in slot k, z(0) = z0 (riem_solver3's pre-sweep put them
  //     there; slot m is read at step m and overwritten with PP at step m + 1); sweep 3 reads zint as always.
  template <bool GL, bool RA, bool ZL = false, class C>
  FV3_HD void run(Real *A, Real *B, long tb, unsigned pix, Real dt, const Real *delp, const Real *cappa, const Real *pt, const Real *qcon, const Real *zint, const Real *w1,
                  Real ws, Real *PM, Real *GAM, Real *wout, C &cl, Real z0 = (Real)0) const {
    const Real t1g = (Real)2.0 * dt * dt, rdt = (Real)1.0 / dt, r3 = (Real)(1.0 / 3.0);
    constexpr int U = FV3_RIEM_U, U1 = FV3_RIEM_U1;
    constexpr int UB = RA ? 1 : U1;  // the back substitutions: nothing to prefetch when gam is in registers (one access site)
    Real pp_nz;
    KREG_DECL(rg);  // gam
#ifdef FV3_RIEM_NO_G4  // (A/B: one access site per level of the unrolled body)
    constexpr bool G4 = false;
#else
    constexpr bool G4 = RA && U == 4;  // the forward sweeps store the four gam of a loop iteration through one access site
#endif
    Real gq[4] = {(Real)0, (Real)0, (Real)0, (Real)0};
    (void)gq;
#define GAM_PUT(k, v)                       \
  do {                                      \
    if constexpr (RA) KREG_SET(rg, k, v);   \
    else if (GL) B[(k)*FV3_WAVE] = (v);     \
    else KW_(GAM, k) = (v);                 \
  } while (0)
// (inside a KWALK body: u_ is the body's static position in its group)
#define GAM_PUT_U(k, v)                     \
  do {                                      \
    if constexpr (G4) gq[u_ & 3] = (v);     \
    else GAM_PUT(k, v);                     \
  } while (0)
#define GAM_FLUSH4()                        \
  do {                                      \
    if constexpr (G4) {                     \
      KREG_SET4(rg, c_, gq);                \
      gq[0] = gq[1] = gq[2] = gq[3] = (Real)0; \
    }                                       \
  } while (0)
    // ---- sweep 1 (up): layer pressures, forward elimination for pp.  PP(k+1) -> slot k
    {
      Real g_prev = (Real)0, dm_k = (Real)0, pe_k = (Real)0, bet = (Real)0, pp_k = (Real)0;  // g_prev = dm(k-1) / dm(k) = the previous step's g_rat
      Real z_top = ZL ? z0 : KW_(zint, 0);
      auto ld = [&](int k) {
        KRec<5> q;
        q.v[0] = KW_(delp, k);
        q.v[1] = KW_(cappa, k);
        q.v[2] = KW_(pt, k);
        q.v[3] = KW_(qcon, k);
        q.v[4] = ZL ? (Real)0 : KW_(zint, k + 1);
        return q;
      };
      KWALK_E(5, U, true, ld, GAM_FLUSH4(), {
        const int m = K;
        const Real pm_n = cl.pm(m, r.v[0], r.v[3]);
        KW_(PM, m) = pm_n;
        const Real z_lo = ZL ? A[m * FV3_WAVE] : r.v[4];  // (ZL: before this step's PP goes to slot m - 1)
        const Real dz_n = z_lo - z_top;
        z_top = z_lo;
        const Real dm_n = r.v[0] * rgrav;
        const Real pe_n = fv3_exp(fv3_div((Real)1.0, (Real)1.0 - r.v[1]) * fv3_log(fv3_div(-dm_n, dz_n) * rgas * r.v[2])) - pm_n;
        if (m >= 1) {
          const int k = m - 1;
          const Real g_rat = fv3_div(dm_k, dm_n);
          const Real bb = (Real)2.0 * ((Real)1.0 + g_rat);
          const Real dd = (Real)3.0 * (pe_k + g_rat * pe_n);
          if (k == 0) {
            bet = bb;
            pp_k = fv3_div(dd, bet);
          } else {
            const Real gam = fv3_div(g_prev, bet);
            GAM_PUT_U(k, gam);
            bet = bb - gam;
            pp_k = fv3_div(dd - pp_k, bet);
          }
          A[k * FV3_WAVE] = pp_k;
          g_prev = g_rat;
        }
        dm_k = dm_n;
        pe_k = pe_n;
      })
      {
        const int k = nz - 1;
        const Real bb = (Real)2.0, dd = (Real)3.0 * pe_k;
        const Real gam = fv3_div(g_prev, bet);
        GAM_PUT(k, gam);
        bet = bb - gam;
        pp_k = fv3_div(dd - pp_k, bet);
        A[k * FV3_WAVE] = pp_k;
      }
      pp_nz = pp_k;
    }
    auto ld_gam = [&](int k) {
      KRec<1> q;
      q.v[0] = GL || RA ? (Real)0 : KW_(GAM, k > 0 ? k : 1);
      return q;
    };
    // ---- sweep 2 (down): back substitution, PP(k) = PP(k) - gam(k) PP(k+1), k = nz-1 .. 1
    {
      Real pp_next = pp_nz;
      KWALK(1, UB, false, ld_gam, {
        if (K >= 1) {
          Real gk;
          if constexpr (RA) gk = KREG_GET(rg, K); else gk = GL ? B[K * FV3_WAVE] : r.v[0];
          const Real ppv = A[(K - 1) * FV3_WAVE] - gk * pp_next;
          A[(K - 1) * FV3_WAVE] = ppv;
          pp_next = ppv;
        }
      })
    }
    // ---- sweep 3 (up): forward elimination for w.  W2(k) -> slot k (PP(k+1) has been taken out one level earlier)
    {
      Real pem = ptop, gm_p = (Real)0, dz_p = (Real)0, aa_k = (Real)0, dmp = (Real)0, w1p = (Real)0, pp_lo = (Real)0, pp_lo2 = (Real)0, bet = (Real)0,
           w2_prev = (Real)0;
      Real z_top = KW_(zint, 0);
      auto ld = [&](int k) {
        KRec<4> q;
        q.v[0] = KW_(delp, k);
        q.v[1] = KW_(cappa, k);
        q.v[2] = KW_(zint, k + 1);
        q.v[3] = KW_(w1, k);
        return q;
      };
      KWALK_E(4, U, true, ld, GAM_FLUSH4(), {
        const int m = K;
        const Real gm_n = fv3_div((Real)1.0, (Real)1.0 - r.v[1]);
        const Real dz_n = r.v[2] - z_top;
        z_top = r.v[2];
        const Real pp_hi = A[m * FV3_WAVE];  // PP(m+1)
        if (m >= 1) {
          const Real aa_n = fv3_div(t1g * (Real)0.5 * (gm_p + gm_n), dz_p + dz_n) * (pem + pp_lo);
          const int k = m - 1;
          if (k == 0) {
            bet = dmp - aa_n;
            w2_prev = fv3_div(dmp * w1p + dt * pp_lo, bet);
          } else {
            const Real gam = fv3_div(aa_k, bet);
            GAM_PUT_U(k, gam);
            bet = dmp - (aa_k + aa_n + aa_k * gam);
            w2_prev = fv3_div(dmp * w1p + dt * (pp_lo - pp_lo2) - aa_k * w2_prev, bet);
          }
          A[k * FV3_WAVE] = w2_prev;
          aa_k = aa_n;
        }
        pem = pem + r.v[0];
        gm_p = gm_n;
        dz_p = dz_n;
        dmp = r.v[0] * rgrav;
        w1p = r.v[3];
        pp_lo2 = pp_lo;
        pp_lo = pp_hi;
      })
      {
        const Real p1 = fv3_div(t1g * gm_p, dz_p) * (pem + pp_lo);
        const Real gam = fv3_div(aa_k, bet);
        GAM_PUT(nz - 1, gam);
        bet = dmp - (aa_k + p1 + aa_k * gam);
        w2_prev = fv3_div(dmp * w1p + dt * (pp_lo - pp_lo2) - p1 * ws - aa_k * w2_prev, bet);
        A[(nz - 1) * FV3_WAVE] = w2_prev;
      }
      // ---- sweep 4 (down): back substitution, W2(k) = W2(k) - gam(k+1) W2(k+1), k = nz-2 .. 0
      Real w2_next = w2_prev;
      KWALK(1, UB, false, ld_gam, {
        if (K >= 1) {
          Real gk;
          if constexpr (RA) gk = KREG_GET(rg, K); else gk = GL ? B[K * FV3_WAVE] : r.v[0];
          const Real wv = A[(K - 1) * FV3_WAVE] - gk * w2_next;
          A[(K - 1) * FV3_WAVE] = wv;
          w2_next = wv;
        }
      })
    }
    // ---- sweep 5 (up): new pressure perturbation.  PE(k+1) -> slot k; the new w leaves through wout
    {
      Real pe_run = (Real)0;
      auto ld = [&](int k) {
        KRec<2> q;
        q.v[0] = KW_(delp, k);
        q.v[1] = KW_(w1, k);
        return q;
      };
      KWALK(2, U1, true, ld, {
        const Real w2k = A[K * FV3_WAVE];
        pe_run = pe_run + r.v[0] * rgrav * (w2k - r.v[1]) * rdt;
        A[K * FV3_WAVE] = pe_run;
        if (wout) FV3_ST_NT(KW_(wout, K), w2k);
        cl.out_pe(K + 1, pe_run, r.v[0]);
      })
    }
    // ---- sweep 6 (down): new layer thickness, handed to the caller's finish
    {
      Real p1 = (Real)0, dm_below = (Real)0, pe1 = A[(nz - 1) * FV3_WAVE], pe2 = (Real)0;
      auto ld = [&](int k) {
        KRec<4> q;
        q.v[0] = KW_(delp, k);
        q.v[1] = KW_(pt, k);
        q.v[2] = KW_(cappa, k);
        q.v[3] = KW_(PM, k);
        return q;
      };
      KWALK(4, U, false, ld, {
        const Real dm = r.v[0] * rgrav;
        const Real pe_k = K >= 1 ? A[(K - 1) * FV3_WAVE] : (Real)0;
        if (K == nz - 1) {
          p1 = (pe_k + (Real)2.0 * pe1) * r3;
        } else {
          const Real g_rat = fv3_div(dm, dm_below);
          const Real bb = (Real)2.0 * ((Real)1.0 + g_rat);
          p1 = (pe_k + bb * pe1 + g_rat * pe2) * r3 - g_rat * p1;
        }
        const Real pmk = r.v[3];
        const Real dzn = -dm * rgas * r.v[1] * fv3_exp((r.v[2] - (Real)1.0) * fv3_log(fv3_max(p_fac * pmk, p1 + pmk)));
        cl.finish(K, dzn);
        pe2 = pe1;
        pe1 = pe_k;
        dm_below = dm;
      })
    }
#undef GAM_PUT
#undef GAM_PUT_U
#undef GAM_FLUSH4
  }
};

static_assert(FV3_COL_WAVE == FV3_WAVE, "fv3_col_plan.h sizes the LDS lines for this wave width");

// the arguments of one call after the field checks
struct RiemCArgs {
  Real *cappa, *phis, *ws, *ptc, *q_con, *delpc, *gz, *pef, *w3;
  Real dt2, ptop;
};
struct Riem3Args {
  Real *cappa, *zs, *wsd, *delz, *q_con, *delp, *pt, *zh, *pe, *ppe, *pk3, *pk, *peln, *w;
  Real dt, ptop;
  Real *zn;  // plan.pre: the marched heights update_dz_d left, and its dz_min
  Real dzm;
};

// f(std::true_type{}) or f(std::false_type{}): a flag of the plan as a template argument of the kernel
template <class F>
void with_tag(bool b, F &&f) {
  if (b)
    f(std::true_type{});
  else
    f(std::false_type{});
}
// riem_solver3's kernels exist for (LAST, RA, PRE) in {000, 100, 010, 110, 011, 111}: the pre-sweep in the register forms only (riem_plan checks it)
template <class F>
void riem3_tags(const RiemPlan &plan, F &&go) {
  with_tag(plan.last, [&](auto last) {
    if (plan.pre)
      go(last, std::true_type{}, std::true_type{});
    else
      with_tag(plan.form.gam == GAM_REGS, [&](auto ra) { go(last, ra, std::false_type{}); });
  });
}
}  // namespace

// What this call does: the ONLY function of this file that asks the switch table.  heavy: riem_solver3.  With the marched heights of update_dz_d waiting
// (src) the plan must be the one update_dz_d foresaw -- dz_scan_defers, the predicate it decided with: false otherwise (the caller fails; nothing is solved
// without the scan).
static bool riem_plan(const fv3_ctx *c, bool heavy, bool last_call, const Real *src, RiemPlan &plan) {
  const Geo &g = c->g;
  static_assert(FV3_AGPR_LEVELS == 80 && FV3_AGPR_LEVELS_F32 == 128, "riem_kreg_levels (fv3_col_plan.h) states the levels of fv3_agpr.h");
  plan.form = riem_form(g.nz, sizeof(Real), g.sk, heavy, fv3_sw(FV3SW_RIEM_MODE), fv3_sw(FV3SW_RIEM_REGS));
  if (fv3_sw(FV3SW_DEBUG_FD)) fprintf(stderr, "[%s] %s form\n", heavy ? "riem_solver3" : "riem_solver_c", plan.form.wave ? "wave" : "column");
  plan.last = last_call;
  plan.pre = src != nullptr;
  // Round 6: inside the sequencer only the LAST sub-step of an acoustic call stores the layer thickness -- the sub-steps between work from zh, and what reads delz
  // (the heights of the next call, the diffusive heating, the remap) comes after the last one: one field write less in five of six sub-steps.  FV3_SEQ_DELZ=every: A/B.
  plan.store_delz = !(c->seq.delz_dead && !fv3_sw_is(FV3SW_SEQ_DELZ, "every"));
  // Frame-first passes of the sequencer (a transport is present): the columns are numbered frame first (ColumnOrder), pass 1 solves
  // the waves that hold frame columns, the halo updates of zh / pkc start, pass 2 solves the rest beside them.  Columns are
  // independent: the same values in any order.
  const int pass = heavy ? c->seq.frame_pass : 0;
  const int ncol = heavy ? g.nx * g.ny : (g.nx + 2) * (g.ny + 2);
  const ColumnOrder ord{g.nx, g.ny, pass != 0 ? FV3_FRAME_W : 0};
  riem_wave_range((ncol + FV3_WAVE - 1) / FV3_WAVE, pass != 0 ? (ord.n_frame() + FV3_WAVE - 1) / FV3_WAVE : 0, pass, plan.w_lo, plan.w_hi);
  return !plan.pre || dz_scan_defers(true, plan.form, fv3_sw_is(FV3SW_DZ_SCAN, "separate"));
}

// ---------------------------------------------------------------------------------------------
static void fv3_riem_solver_c_wave(fv3_ctx *c, fv3_stream_t s, const RiemPlan &plan, const RiemCArgs &a) {
  const Geo g = c->g;
  Real *cappa = a.cappa, *phis = a.phis, *ws = a.ws, *ptc = a.ptc, *q_con = a.q_con, *delpc = a.delpc, *gz = a.gz, *pef = a.pef, *w3 = a.w3;
  const Real dt2 = a.dt2, ptop = a.ptop, grav = (Real)c->cst.grav;
  Real *PM = c->scratch[SC_A], *GAM = c->scratch[SC_E];
  const int nz = g.nz;
  {
    const Sim1W sw{g.sk, nz, (Real)c->cst.rdgas, (Real)1.0 / (Real)c->cst.grav, (Real)c->cfg.p_fac, ptop};
    const int i0 = 0, j0 = 0, ni = g.nx + 2, ncol = ni * (g.ny + 2);
    const long st = g.st, st2 = g.st2, sk = g.sk;
    const int sj32 = g.sj32, go = g.o;
    const bool gl = plan.form.gam == GAM_LDS;
    auto go_ = [&](auto ra_tag) {
    constexpr bool RA = decltype(ra_tag)::value;
    launch_waves<1>(c, s, (ncol + FV3_WAVE - 1) / FV3_WAVE, 1, g.nsub, sizeof(Real) * nz * FV3_WAVE * (gl ? 2 : 1), [=] FV3_HD(const Blk &blk, char *smem_) {
      const int t = blk.bz;
      const long tb = t * st;
      FV3_LANES(blk, lane, l) {
        const int cidx = blk.bx * FV3_WAVE + lane;
        if (cidx >= ncol) continue;
        const int jr = cidx / ni;
        const unsigned pix = (unsigned)((j0 + jr + go) * sj32 + (i0 + cidx - jr * ni) + go);
        struct Cl {
          long tb, sk;
          unsigned pix;
          Real peg, pem, z, grav;
          Real *pef, *gz;
          FV3_HD Real pm(int, Real dm, Real qc) {
            const Real peg_n = peg + dm * ((Real)1.0 - qc);
            const Real v = fv3_div(peg_n - peg, fv3_log(fv3_div(peg_n, peg)));
            peg = peg_n;
            return v;
          }
          FV3_HD void out_pe(int k1, Real pe, Real dm) {
            pem = pem + dm;
            FV3_ST_NT(KW_(pef, k1), pe + pem);
          }
          FV3_HD void finish(int k, Real dz) {
            z = z - dz * grav;
            FV3_ST_NT(KW_(gz, k), z);
          }
        };
        const Real z_bot = phis[t * st2 + pix];
        Cl cl{tb, sk, pix, ptop, ptop, z_bot, grav, pef, gz};
        KW_(pef, 0) = ptop;
        sw.run<FV3_RIEM_GL != 0, RA>((Real *)smem_ + lane, (Real *)smem_ + nz * FV3_WAVE + lane, tb, pix, dt2, delpc, cappa, ptc, q_con, gz, w3, ws[t * st2 + pix], PM, GAM, (Real *)nullptr, cl);
        KW_(gz, nz) = z_bot;
      }
    });
    };
    with_tag(plan.form.gam == GAM_REGS, go_);
  }
}

static void fv3_riem_solver_c_columns(fv3_ctx *c, fv3_stream_t s, const RiemCArgs &a) {
  const Geo g = c->g;
  Real *cappa = a.cappa, *phis = a.phis, *ws = a.ws, *ptc = a.ptc, *q_con = a.q_con, *delpc = a.delpc, *gz = a.gz, *pef = a.pef, *w3 = a.w3;
  const Real dt2 = a.dt2, ptop = a.ptop, grav = (Real)c->cst.grav;
  Sim1 sim{g, (Real)c->cst.rdgas, (Real)1.0 / (Real)c->cst.grav, (Real)c->cfg.p_fac, ptop};
  Real *PM = c->scratch[SC_A], *DZ = c->scratch[SC_B], *W2 = c->scratch[SC_C], *PP = c->scratch[SC_D], *GAM = c->scratch[SC_E];
  const int nz = g.nz;
  launch2(c, s, Box{0, g.nx + 1, 0, g.ny + 1, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const long tb = t * g.st;
    const unsigned pix = IX(i, j);
    const long p = tb + pix;
    (void)p;
    // setup (inside the solver's first sweep): layer-mean pressure without condensate, thickness
    Real peg = ptop;
    auto setup = [&](int k, Real &pm, Real &dz) {
      const Real dm = K_(delpc, k);
      const Real peg_n = peg + dm * ((Real)1.0 - K_(q_con, k));
      pm = (peg_n - peg) / fv3_log(peg_n / peg);
      dz = K_(gz, k + 1) - K_(gz, k);
      K_(PM, k) = pm;
      K_(DZ, k) = dz;
      peg = peg_n;
    };
    // finish (inside the last sweep): geopotential from the new thickness
    Real z = phis[t * g.st2 + IX(i, j)];
    const Real z_bot = z;
    auto finish = [&](int k, Real dz) {
      z = z - dz * grav;
      K_(gz, k) = z;
    };
    sim.run(tb, pix, dt2, delpc, cappa, ptc, w3, ws[t * g.st2 + IX(i, j)], PM, DZ, W2, PP, GAM, pef, (Real *)nullptr, setup, finish);
    K_(gz, nz) = z_bot;  // (after the solve: setup reads the incoming gz[nz])
    // full interface pressure
    Real pem = ptop;
    K_(pef, 0) = ptop;
    for (int k = 0; k < nz; ++k) {
      pem = pem + K_(delpc, k);
      K_(pef, k + 1) = K_(pef, k + 1) + pem;
    }
  });
}

extern "C" int fv3_riem_solver_c(fv3_ctx *c, double dt2d, const fv3_field *cappa_, double ptopd, const fv3_field *phis_, const fv3_field *ws_,
                                 const fv3_field *ptc_, const fv3_field *q_con_, const fv3_field *delpc_, const fv3_field *gz_, const fv3_field *pef_,
                                 const fv3_field *w3_, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(cappa, cappa_) FV3_FIELD2D(phis, phis_) FV3_FIELD2D(ws, ws_) FV3_FIELD(ptc, ptc_) FV3_FIELD(q_con, q_con_) FV3_FIELD(delpc, delpc_)
  FV3_FIELD(gz, gz_) FV3_FIELD(pef, pef_) FV3_FIELD(w3, w3_)
  fv3_stream_t s = (fv3_stream_t)stream;
  const RiemCArgs a{cappa, phis, ws, ptc, q_con, delpc, gz, pef, w3, (Real)dt2d, (Real)ptopd};
  RiemPlan plan;
  riem_plan(c, false, false, nullptr, plan);
  if (plan.form.wave)
    fv3_riem_solver_c_wave(c, s, plan, a);
  else
    fv3_riem_solver_c_columns(c, s, a);
  return fv3_post(c, s, "riem_solver_c");
}

// ---------------------------------------------------------------------------------------------
static void fv3_riem_solver3_wave(fv3_ctx *c, fv3_stream_t s, const RiemPlan &plan, const Riem3Args &a) {
  const Geo g = c->g;
  Real *cappa = a.cappa, *zs = a.zs, *wsd = a.wsd, *delz = a.delz, *q_con = a.q_con, *delp = a.delp, *pt = a.pt, *zh = a.zh, *pe = a.pe, *ppe = a.ppe, *pk3 = a.pk3,
       *pk = a.pk, *peln = a.peln, *w = a.w;
  const Real dt = a.dt, ptop = a.ptop;
  const Real akap = (Real)(c->cst.rdgas / c->cst.cp_air);
  Real *PM = c->scratch[SC_A], *GAM = c->scratch[SC_E];
  const int nz = g.nz;
  {
    const Sim1W sw{g.sk, nz, (Real)c->cst.rdgas, (Real)1.0 / (Real)c->cst.grav, (Real)c->cfg.p_fac, ptop};
    const int i0 = 1, j0 = 1, ni = g.nx, ncol = ni * g.ny;
    const long st = g.st, st2 = g.st2, sk = g.sk;
    const int sj32 = g.sj32, go = g.o;
    const bool gl = plan.form.gam == GAM_LDS;
    // (two instantiations: the last sub-step also stores pe / peln / pk -- three more base pointers in a kernel that spills scalar
    //  registers as it is)
    const ColumnOrder ord{g.nx, g.ny, c->seq.frame_pass != 0 ? FV3_FRAME_W : 0};  // (the frame-first numbering of the columns: see riem_plan)
    const int w_lo = plan.w_lo, w_hi = plan.w_hi;  // waves [w_lo, w_hi)
    Real *const zn = a.zn;  // (update_dz_d left its scan to this call: see fv3_seq_hints::dz_scan)
    const bool store_delz = plan.store_delz;
    const Real dzm = a.dzm;
    auto go_ = [&](auto last_tag, auto ra_tag, auto pre_tag) {
    constexpr bool LAST = decltype(last_tag)::value;
    constexpr bool RA = decltype(ra_tag)::value;
    constexpr bool PRE = decltype(pre_tag)::value;
    launch_waves<1>(c, s, w_hi - w_lo, 1, g.nsub, sizeof(Real) * nz * FV3_WAVE * (gl ? 2 : 1), [=] FV3_HD(const Blk &blk, char *smem_) {
      const int t = blk.bz;
      const long tb = t * st;
      FV3_LANES(blk, lane, l) {
        const int cidx = (w_lo + blk.bx) * FV3_WAVE + lane;
        if (cidx >= ncol) continue;
        int ci, cj;
        ord.at(cidx, ci, cj);
        const unsigned pix = (unsigned)((cj + go) * sj32 + ci + go);
        struct Cl {
          long tb, sk;
          unsigned pix;
          Real pem, peg, pelng_k, z, akap;
          Real *pk3, *peln, *pk, *pe, *ppe, *zh, *delz;
          bool sdz;
          FV3_HD Real pm(int k, Real dm, Real qc) {
            pem = pem + dm;
            const Real peg_n = peg + dm * ((Real)1.0 - qc);
            const Real peln_n = fv3_log(pem), pelng_n = fv3_log(peg_n);
            const Real pk3v = fv3_exp(akap * peln_n);
            FV3_ST_NT(KW_(pk3, k + 1), pk3v);
            if constexpr (LAST) {
              FV3_ST_NT(KW_(peln, k + 1), peln_n);
              FV3_ST_NT(KW_(pk, k + 1), pk3v);
              FV3_ST_NT(KW_(pe, k + 1), pem);
            }
            const Real v = fv3_div(peg_n - peg, pelng_n - pelng_k);
            peg = peg_n;
            pelng_k = pelng_n;
            return v;
          }
          FV3_HD void out_pe(int k1, Real pev, Real) { FV3_ST_NT(KW_(ppe, k1), pev); }
          FV3_HD void finish(int k, Real dz) {
            z = z - dz;
            FV3_ST_NT(KW_(zh, k), z);
            if (sdz) FV3_ST_NT(KW_(delz, k), dz);  // (wave-uniform: see store_delz)
          }
        };
        const Real z_bot = zs[t * st2 + pix];
        const Real peln0 = fv3_log(ptop);
        Cl cl{tb, sk, pix, ptop, ptop, peln0, z_bot, akap, pk3, LAST ? peln : nullptr, LAST ? pk : nullptr, LAST ? pe : nullptr, ppe, zh, delz, store_delz};
        KW_(pk3, 0) = fv3_exp(akap * peln0);
        if constexpr (LAST) {
          KW_(peln, 0) = peln0;
          KW_(pk, 0) = KW_(pk3, 0);
          KW_(pe, 0) = ptop;
        }
        KW_(ppe, 0) = (Real)0;
        Real ws_v, z0 = (Real)0;
        if constexpr (PRE) {
          // update_dz_d's last kernel as a pre-sweep (bottom-up): interface k stays dz_min above interface k + 1; the limited heights go to the LDS line for
          // sweep 1 (z(k + 1) in slot k) and -- only where the limit changed them -- back into the marched field, which sweep 3 reads; the surface vertical
          // velocity from the lowest interface.  The scan kernel's expressions (fv3_update_dz_d_scan, fv3_dz_floor): bitwise the separate form.
          Real *A_ = (Real *)smem_ + lane;
          Real below = KW_(zn, nz);
          A_[(nz - 1) * FV3_WAVE] = below;
          ws_v = (z_bot - below) / dt;
          wsd[t * st2 + pix] = ws_v;
          auto ldz = [&](int k) {
            KRec<1> q;
            q.v[0] = KW_(zn, k);
            return q;
          };
          KWALK(1, FV3_RIEM_U1, false, ldz, {
            const Real zk = r.v[0];
            const Real v = fv3_dz_floor(zk, below, dzm);
            if (v != zk) KW_(zn, K) = v;
            if (K >= 1)
              A_[(K - 1) * FV3_WAVE] = v;
            else
              z0 = v;
            below = v;
          })
        } else {
          ws_v = wsd[t * st2 + pix];
        }
        sw.run<FV3_RIEM_GL != 0, RA, PRE>((Real *)smem_ + lane, (Real *)smem_ + nz * FV3_WAVE + lane, tb, pix, dt, delp, cappa, pt, q_con, PRE ? (const Real *)zn : (const Real *)zh, w, ws_v, PM, GAM, w, cl, z0);
        KW_(zh, nz) = z_bot;
      }
    });
    };
    riem3_tags(plan, go_);
  }
}

static void fv3_riem_solver3_columns(fv3_ctx *c, fv3_stream_t s, const RiemPlan &plan, const Riem3Args &a) {
  const Geo g = c->g;
  Real *cappa = a.cappa, *zs = a.zs, *wsd = a.wsd, *delz = a.delz, *q_con = a.q_con, *delp = a.delp, *pt = a.pt, *zh = a.zh, *pe = a.pe, *ppe = a.ppe, *pk3 = a.pk3,
       *pk = a.pk, *peln = a.peln, *w = a.w;
  const Real dt = a.dt, ptop = a.ptop;
  const Real akap = (Real)(c->cst.rdgas / c->cst.cp_air);
  Sim1 sim{g, (Real)c->cst.rdgas, (Real)1.0 / (Real)c->cst.grav, (Real)c->cfg.p_fac, ptop};
  Real *PM = c->scratch[SC_A], *W2 = c->scratch[SC_C], *PP = c->scratch[SC_D], *GAM = c->scratch[SC_E];
  const int nz = g.nz;
  const bool last = plan.last;
  launch2_pass(c, s, Box{1, g.nx, 1, g.ny, 0, 0}, c->seq.frame_pass, [=] FV3_HD(int t, int i, int j) {
    const long tb = t * g.st;
    const unsigned pix = IX(i, j);
    const long p = tb + pix;
    (void)p;
    Real pem = ptop, peg = ptop;
    Real peln_k = fv3_log(pem), pelng_k = fv3_log(peg);
    K_(pk3, 0) = fv3_exp(akap * peln_k);
    if (last) {
      K_(peln, 0) = peln_k;
      K_(pk, 0) = K_(pk3, 0);
      K_(pe, 0) = pem;
    }
    (void)peln_k;
    // setup (inside the solver's first sweep): interface pressures / Exner functions, layer-mean pressure, thickness
    auto setup = [&](int k, Real &pm, Real &dz) {
      const Real dm = K_(delp, k);
      pem = pem + dm;
      const Real peg_n = peg + dm * ((Real)1.0 - K_(q_con, k));
      const Real peln_n = fv3_log(pem), pelng_n = fv3_log(peg_n);
      const Real pk3v = fv3_exp(akap * peln_n);
      K_(pk3, k + 1) = pk3v;
      if (last) {
        K_(peln, k + 1) = peln_n;
        K_(pk, k + 1) = pk3v;
        K_(pe, k + 1) = pem;
      }
      pm = (peg_n - peg) / (pelng_n - pelng_k);
      dz = K_(zh, k + 1) - K_(zh, k);
      K_(PM, k) = pm;
      K_(delz, k) = dz;  // dz2 lives in the output array
      peg = peg_n;
      pelng_k = pelng_n;
    };
    // finish (inside the last sweep): interface heights from the new thickness
    Real z = zs[t * g.st2 + IX(i, j)];
    const Real z_bot = z;
    auto finish = [&](int k, Real dz) {
      z = z - dz;
      K_(zh, k) = z;
    };
    sim.run(tb, pix, dt, delp, cappa, pt, w, wsd[t * g.st2 + IX(i, j)], PM, delz, W2, PP, GAM, ppe, w, setup, finish);
    K_(zh, nz) = z_bot;
  });
}

extern "C" int fv3_riem_solver3(fv3_ctx *c, int last_call, double dtd, const fv3_field *cappa_, double ptopd, const fv3_field *zs_, const fv3_field *wsd_,
                                const fv3_field *delz_, const fv3_field *q_con_, const fv3_field *delp_, const fv3_field *pt_, const fv3_field *zh_,
                                const fv3_field *pe_, const fv3_field *ppe_, const fv3_field *pk3_, const fv3_field *pk_, const fv3_field *peln_,
                                const fv3_field *w_, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(cappa, cappa_) FV3_FIELD2D(zs, zs_) FV3_FIELD2D(wsd, wsd_) FV3_FIELD(delz, delz_) FV3_FIELD(q_con, q_con_) FV3_FIELD(delp, delp_)
  FV3_FIELD(pt, pt_) FV3_FIELD(zh, zh_) FV3_FIELD(pe, pe_) FV3_FIELD(ppe, ppe_) FV3_FIELD(pk3, pk3_) FV3_FIELD(pk, pk_) FV3_FIELD(peln, peln_)
  FV3_FIELD(w, w_)
  fv3_stream_t s = (fv3_stream_t)stream;
  Riem3Args a{cappa, zs, wsd, delz, q_con, delp, pt, zh, pe, ppe, pk3, pk, peln, w, (Real)dtd, (Real)ptopd, nullptr, (Real)0};
  // (frame-first passes: both take the pre-sweep, each on its own columns -- pass 1 leaves the heights for pass 2)
  a.zn = fv3_dz_scan_take(c, &a.dzm, c->seq.frame_pass == 1);
  RiemPlan plan;
  if (!riem_plan(c, true, last_call != 0, a.zn, plan))
    return fv3_fail(c, FV3_ERR_ARG, "riem_solver3: update_dz_d left its closing scan to a pre-sweep that this call's form does not have");
  if (plan.form.wave)
    fv3_riem_solver3_wave(c, s, plan, a);
  else
    fv3_riem_solver3_columns(c, s, plan, a);
  return fv3_post(c, s, "riem_solver3");
}


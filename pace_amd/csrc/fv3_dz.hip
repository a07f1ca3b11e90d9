// fv3_dz.hip -- the interface-height updates of the non-hydrostatic height chain: update_dz_c, update_dz_d with its edge_profile forms.
// CPU twin: oracle/fv3_oracle/nh.py.  [SURVEY A.5-A.12]
//
// update_dz_d is: field checks, dzd_plan() -- the edge_profile form, the del-n coefficient table, the interface the chain inside the march starts at, the
// fork of the sponge part, the hand-off of the closing scan, decided by the pure functions of fv3_col_plan.h -- then one function per stage.
//
// Column kernels: one thread per (i, j) column walks k; because i is the fastest index every
// per-level access of a wavefront is one coalesced row.
#include "fv3_ops.h"
#include "fv3_kwalk.h"
#include "fv3_col_plan.h"

// ---------------------------------------------------------------------------------------------
extern "C" int fv3_update_dz_c(fv3_ctx *c, const fv3_field *zs_, const fv3_field *ut_, const fv3_field *vt_, const fv3_field *gz_, const fv3_field *ws_,
                               double dtd, void *stream) {
  return fv3_update_dz_c_from(c, zs_, ut_, vt_, gz_, gz_, ws_, dtd, stream);
}

// gz_in -> gz: the sequencer passes zh as gz_in on the sub-steps where the reference first copies zh into gz
// (dyn_core: "gz = zh" before update_dz_c), which saves that full-field copy; only cells 0..n+1 of gz are written,
// and nothing downstream (riem_solver_c, p_grad_c) reads gz beyond them.
int fv3_update_dz_c_from(fv3_ctx *c, const fv3_field *zs_, const fv3_field *ut_, const fv3_field *vt_, const fv3_field *gzin_, const fv3_field *gz_,
                         const fv3_field *ws_, double dtd, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD2D(zs, zs_) FV3_FIELD(ut, ut_) FV3_FIELD(vt, vt_) FV3_FIELD(gz, gz_) FV3_FIELD(gzin, gzin_) FV3_FIELD2D(ws, ws_)
  const Geo g = c->g;
  fv3_stream_t s = (fv3_stream_t)stream;
  const Real dt = (Real)dtd;
  const int nz = g.nz;
  const Real dz_min = (Real)c->cst.dz_min;
  const std::vector<double> &dp = c->dp_ref_h;
  const Real top_ratio = (Real)(dp[0] / (dp[0] + dp[1]));
  const Real bot_ratio = (Real)(dp[nz - 1] / (dp[nz - 2] + dp[nz - 1]));
  Real *gzn = c->scratch[SC_A];
  if (gzin != gz && nz >= 3) {
    // Out of place (the sequencer's zh -> gz form): ONE column kernel walks the interfaces upward from the surface,
    // forms the advected height of interface k in registers and applies the monotonicity scan at once -- the
    // intermediate field is never stored (2 field passes less) and each wind layer is read once (it serves the
    // interface above and the one below).  In place (gz -> gz) the two-kernel form below is required: neighbours'
    // heights are read while columns are rewritten.
    launch2(c, s, Box{0, g.nx + 1, 0, g.ny + 1, 0, 0}, [=] FV3_HD(int t, int i, int j) {
      const int fl = g.flags[t];
      const long tb = t * g.st, m2 = t * g.st2;
      const unsigned pix = IX(i, j), qx1 = IX(i + 1, j), qy1 = IX(i, j + 1);
      const unsigned gw = f4_index<1>(g, fl, i - 1, j), gc1 = f4_index<1>(g, fl, i, j), ge = f4_index<1>(g, fl, i + 1, j);
      const unsigned gs = f4_index<2>(g, fl, i, j - 1), gc2 = f4_index<2>(g, fl, i, j), gn = f4_index<2>(g, fl, i, j + 1);
      const Real ar = (g.area + m2)[pix];
      // layer values at the four faces: a* = layer k-1 (above the interface), c* = layer k (below), p* = layer k+1
      Real ax0, ax1, ay0, ay1, cx0 = (Real)0, cx1 = (Real)0, cy0 = (Real)0, cy1 = (Real)0, px0 = (Real)0, px1 = (Real)0, py0 = (Real)0, py1 = (Real)0;
      {
        const Real *u1 = ut + tb + (long)(nz - 1) * g.sk, *v1 = vt + tb + (long)(nz - 1) * g.sk;
        ax0 = u1[pix];
        ax1 = u1[qx1];
        ay0 = v1[pix];
        ay1 = v1[qy1];
      }
      Real below = (Real)0;
#pragma unroll 1
      for (int k = nz; k >= 0; --k) {
        // layer k-2 (becomes "above" for the next interface); at the bottom it also enters the extrapolation
        Real nx0 = (Real)0, nx1 = (Real)0, ny0 = (Real)0, ny1 = (Real)0;
        if (k >= 2) {
          const Real *u2 = ut + tb + (long)(k - 2) * g.sk, *v2 = vt + tb + (long)(k - 2) * g.sk;
          nx0 = u2[pix];
          nx1 = u2[qx1];
          ny0 = v2[pix];
          ny1 = v2[qy1];
        }
        Real x0, x1, y0, y1;
        if (k == nz) {
          x0 = ax0 + (ax0 - nx0) * bot_ratio;
          x1 = ax1 + (ax1 - nx1) * bot_ratio;
          y0 = ay0 + (ay0 - ny0) * bot_ratio;
          y1 = ay1 + (ay1 - ny1) * bot_ratio;
        } else if (k == 0) {
          x0 = cx0 + (cx0 - px0) * top_ratio;
          x1 = cx1 + (cx1 - px1) * top_ratio;
          y0 = cy0 + (cy0 - py0) * top_ratio;
          y1 = cy1 + (cy1 - py1) * top_ratio;
        } else {
          const Real d1 = g.dp_ref[k], d0 = g.dp_ref[k - 1];
          const Real int_ratio = (Real)1.0 / (d0 + d1);
          x0 = (d1 * ax0 + d0 * cx0) * int_ratio;
          x1 = (d1 * ax1 + d0 * cx1) * int_ratio;
          y0 = (d1 * ay0 + d0 * cy0) * int_ratio;
          y1 = (d1 * ay1 + d0 * cy1) * int_ratio;
        }
        const Real *gg = gzin + tb + (long)k * g.sk;
        const Real fx0 = x0 * (x0 > (Real)0 ? gg[gw] : gg[gc1]);
        const Real fx1 = x1 * (x1 > (Real)0 ? gg[gc1] : gg[ge]);
        const Real fy0 = y0 * (y0 > (Real)0 ? gg[gs] : gg[gc2]);
        const Real fy1 = y1 * (y1 > (Real)0 ? gg[gc2] : gg[gn]);
        const Real zn = (gg[pix] * ar + fx0 - fx1 + fy0 - fy1) / (ar + x0 - x1 + y0 - y1);
        Real v = zn;
        if (k == nz) {
          ws[t * g.st2 + pix] = (zs[t * g.st2 + pix] - zn) / dt;
        } else {
          v = fv3_dz_floor(zn, below, dz_min);
        }
        (gz + tb + (long)k * g.sk)[pix] = v;
        below = v;
        // shift: the interface above sees this one's "above" layer as its "below" layer
        px0 = cx0;
        px1 = cx1;
        py0 = cy0;
        py1 = cy1;
        cx0 = ax0;
        cx1 = ax1;
        cy0 = ay0;
        cy1 = ay1;
        if (k == nz) {
          // (interface nz-1 keeps layer nz-1 below it and gets layer nz-2 above it)
        }
        ax0 = nx0;
        ax1 = nx1;
        ay0 = ny0;
        ay1 = ny1;
      }
    });
    return fv3_post(c, s, "update_dz_c");
  }
  launch3(c, s, Box{0, g.nx + 1, 0, g.ny + 1, 0, nz}, [=] FV3_HD(int t, int k, int i, int j) {
    const int fl = g.flags[t];
    const long bt = t * g.st, b = bt + k * g.sk, m2 = t * g.st2;
    auto XI = [&](const Real *f0, int ii, int jj) -> Real {
      const unsigned q = IX(ii, jj);
      const Real *f = f0 + bt;
      if (k == 0) return f[q] + (f[q] - (f + g.sk)[q]) * top_ratio;
      if (k == nz) return (f + (nz - 1) * g.sk)[q] + ((f + (nz - 1) * g.sk)[q] - (f + (nz - 2) * g.sk)[q]) * bot_ratio;
      const Real int_ratio = (Real)1.0 / (g.dp_ref[k - 1] + g.dp_ref[k]);
      return (g.dp_ref[k] * (f + (k - 1) * g.sk)[q] + g.dp_ref[k - 1] * (f + k * g.sk)[q]) * int_ratio;
    };
    const Real *gg = gzin + b;
    const Real x0 = XI(ut, i, j), x1 = XI(ut, i + 1, j), y0 = XI(vt, i, j), y1 = XI(vt, i, j + 1);
    const Real fx0 = x0 * (x0 > (Real)0 ? gg[f4_index<1>(g, fl, i - 1, j)] : gg[f4_index<1>(g, fl, i, j)]);
    const Real fx1 = x1 * (x1 > (Real)0 ? gg[f4_index<1>(g, fl, i, j)] : gg[f4_index<1>(g, fl, i + 1, j)]);
    const Real fy0 = y0 * (y0 > (Real)0 ? gg[f4_index<2>(g, fl, i, j - 1)] : gg[f4_index<2>(g, fl, i, j)]);
    const Real fy1 = y1 * (y1 > (Real)0 ? gg[f4_index<2>(g, fl, i, j)] : gg[f4_index<2>(g, fl, i, j + 1)]);
    const unsigned p = IX(i, j);
    const Real ar = (g.area + m2)[p];
    (gzn + b)[p] = (gg[p] * ar + fx0 - fx1 + fy0 - fy1) / (ar + x0 - x1 + y0 - y1);
  });
  launch2(c, s, Box{0, g.nx + 1, 0, g.ny + 1, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const long tb = t * g.st;
    const unsigned pix = IX(i, j);
    const long p = tb + pix;
    (void)p;
    Real below = gzn[p + (long)nz * g.sk];
    gz[p + (long)nz * g.sk] = below;
    ws[t * g.st2 + IX(i, j)] = (zs[t * g.st2 + IX(i, j)] - below) / dt;
    for (int k = nz - 1; k >= 0; --k) {
      const Real v = fv3_dz_floor(K_(gzn, k), below, dz_min);
      K_(gz, k) = v;
      below = v;
    }
  });
  return fv3_post(c, s, "update_dz_c");
}

// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// edge_profile with the whole column in registers (level count known at compile time): the NZ layer
// values are loaded up front (NZ independent loads in flight per lane), the forward elimination and the
// back substitution run in place on the register array and the NZ+1 interface values are stored once --
// one read and one write per field instead of the two column walks of the generic form below.
// ---------------------------------------------------------------------------------------------
template <int NZ>
static void edge_profile_reg(fv3_ctx *c, fv3_stream_t s, const Real *crx, const Real *xfx, const Real *cry, const Real *yfx, Real *crx_a, Real *xfx_a, Real *cry_a,
                             Real *yfx_a) {
  const Geo g = c->g;
  const int isd = 1 - g.nh, ied = g.nx + g.nh, jsd = 1 - g.nh, jed = g.ny + g.nh;
  const Real *gamd = g.ep_gam;
  launch2(c, s, Box{isd, ied, jsd, jed, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const long tb = t * g.st;
    const unsigned pix = IX(i, j);
    auto profile = [&](const Real *q, Real *qe) {
      const Real *dp0 = g.dp_ref;
      Real a[NZ + 1];
#pragma unroll
      for (int k = 0; k < NZ; ++k) a[k] = K_(q, k);
      const Real g0 = dp0[1] / dp0[0];
      Real xt1 = (Real)2.0 * g0 * (g0 + (Real)1.0);
      Real bet = g0 * (g0 + (Real)0.5);
      Real q_m = a[0], q_mm = a[0];  // q[k-1], q[k-2] (original layer values)
      a[0] = (xt1 * a[0] + a[1]) / bet;
      Real gam_prev = ((Real)1.0 + g0 * (g0 + (Real)1.5)) / bet;
      Real gk = g0;
#pragma unroll
      for (int k = 1; k < NZ; ++k) {
        gk = dp0[k - 1] / dp0[k];
        bet = (Real)2.0 + (Real)2.0 * gk - gam_prev;
        const Real qk = a[k];
        a[k] = ((Real)3.0 * (q_m + gk * qk) - a[k - 1]) / bet;
        gam_prev = gk / bet;
        q_mm = q_m;
        q_m = qk;
      }
      const Real a_bot = (Real)1.0 + gk * (gk + (Real)1.5);
      xt1 = (Real)2.0 * gk * (gk + (Real)1.0);
      const Real xt2 = gk * (gk + (Real)0.5) - a_bot * gam_prev;
      a[NZ] = (xt1 * q_m + q_mm - a_bot * a[NZ - 1]) / xt2;
#pragma unroll
      for (int k = NZ - 1; k >= 0; --k) a[k] = a[k] - gamd[k] * a[k + 1];
#pragma unroll
      for (int k = 0; k <= NZ; ++k) K_(qe, k) = a[k];
    };
    if (i >= 1 && i <= g.nx + 1) {
      profile(crx, crx_a);
      profile(xfx, xfx_a);
    }
    if (j >= 1 && j <= g.ny + 1) {
      profile(cry, cry_a);
      profile(yfx, yfx_a);
    }
  });
}

// Wave forms of edge_profile: a wave owns 64 columns of ONE of the four fields (flattened column index: no
// idle lanes on the face-field boxes).  The pivots / ratios are level-only tables built at context
// creation, so a level costs one division.
//   NZ > 0: the column lives in registers, all NZ loads in flight at once, code = one unrolled profile
//           (the older edge_profile_reg inlines four profiles with three divisions per level: ~130 KB of
//           code, 2.5 TB/s);
//   NZ = 0: any level count -- rolled loops, the forward-eliminated values sit in the lane's LDS line,
//           inputs prefetched 16 levels ahead (LDS-limited to 4 waves / CU at L79: latency-bound, 3.3 TB/s).
struct EpSet {  // the fields of one launch as element offsets from the first one's pointers
  long din[4], dout[4];
  int n;
};
template <int NZ>
static void edge_profile_wave1(fv3_ctx *c, fv3_stream_t s, const Real *q, Real *qe, bool xf, EpSet set = EpSet{{0, 0, 0, 0}, {0, 0, 0, 0}, 1});
template <int NZ>
static void edge_profile_wave(fv3_ctx *c, fv3_stream_t s, bool one, const Real *crx, const Real *xfx, const Real *cry, const Real *yfx, Real *crx_a, Real *xfx_a,
                              Real *cry_a, Real *yfx_a) {
  // one launch per field: the field pointers stay kernel arguments (selecting among them inside the kernel
  // turns every access into a flat load through a scratch copy of the argument block)
  // Round 5 (review item 2): the four solves as ONE launch -- the field of a wave is a wave-uniform ELEMENT OFFSET from the first field's pointer (four
  // integers among the kernel arguments), so every access stays a global load off one base.  Experiment R5-22 (update_dz_d -0.18 ms, but d_sw +0.5 ms in the
  // same processes: left off); re-measured in round 6 on the fused wind stage (R6-8: update_dz_d -0.11 / -0.20 ms, d_sw -0.0 / -0.4): the default now.
  // FV3_EP_ONE_LAUNCH=0 (one = false, EpPlan::one_launch): four launches (A/B; bitwise equal).
  if (one) {
    const EpSet set{{0, (long)(xfx - crx), (long)(cry - crx), (long)(yfx - crx)}, {0, (long)(xfx_a - crx_a), (long)(cry_a - crx_a), (long)(yfx_a - crx_a)}, 4};
    edge_profile_wave1<NZ>(c, s, crx, crx_a, true, set);
    return;
  }
  edge_profile_wave1<NZ>(c, s, crx, crx_a, true);
  edge_profile_wave1<NZ>(c, s, xfx, xfx_a, true);
  edge_profile_wave1<NZ>(c, s, cry, cry_a, false);
  edge_profile_wave1<NZ>(c, s, yfx, yfx_a, false);
}
template <int NZ>
static void edge_profile_wave1(fv3_ctx *c, fv3_stream_t s, const Real *q0, Real *qe0, bool xf0, EpSet set) {
  const Geo g = c->g;
  const int nz = g.nz;
  const int isd = 1 - g.nh, ied = g.nx + g.nh, jsd = 1 - g.nh, jed = g.ny + g.nh;
  const int nix = g.nx + 1, ncx = nix * (jed - jsd + 1);  // x-face fields: i in [1, nx+1], every j
  const int niy = ied - isd + 1, ncy = niy * (g.ny + 1);  // y-face fields: every i, j in [1, ny+1]
  const int nfield = set.n, nsub = g.nsub;
  const int ncmax = nfield > 1 ? (ncx > ncy ? ncx : ncy) : (xf0 ? ncx : ncy);
  const long st = g.st, sk = g.sk;
  const int sj32 = g.sj32, go = g.o;
  const Real *gkt = g.ep_gk, *bett = g.ep_bet, *gamd = g.ep_gam;
  constexpr int WPE = NZ == 0 ? 1 : (NZ > 100 ? 1 : 2);
  launch_waves<WPE>(c, s, (ncmax + FV3_WAVE - 1) / FV3_WAVE, 1, g.nsub * nfield, NZ == 0 ? sizeof(Real) * nz * FV3_WAVE : 0, [=] FV3_HD(const Blk &blk, char *smem_) {
    // (set of four: fields 0, 1 are x-face fields, 2, 3 y-face fields)
    const int f = nfield > 1 ? blk.bz / nsub : 0;
    const bool xf = nfield > 1 ? f < 2 : xf0;
    const long din = f == 0 ? set.din[0] : f == 1 ? set.din[1] : f == 2 ? set.din[2] : set.din[3];
    const long dout = f == 0 ? set.dout[0] : f == 1 ? set.dout[1] : f == 2 ? set.dout[2] : set.dout[3];
    const Real *const q = q0 + din;
    Real *const qe = qe0 + dout;
    const int ni = xf ? nix : niy, ncol = xf ? ncx : ncy, i0 = xf ? 1 : isd, j0 = xf ? jsd : 1;
    const long tb = (blk.bz - f * nsub) * st;
    FV3_LANES(blk, lane, l) {
      const int cidx = blk.bx * FV3_WAVE + lane;
      if (cidx >= ncol) continue;
      const int jr = cidx / ni;
      const unsigned pix = (unsigned)((j0 + jr + go) * sj32 + (i0 + cidx - jr * ni) + go);
      if constexpr (NZ > 0) {
        (void)smem_;
        Real a[NZ + 1];
#pragma unroll
        for (int k = 0; k < NZ; ++k) a[k] = KW_(q, k);
        const Real g0 = gkt[0];
        Real q_m = a[0], q_mm = a[0];
        a[0] = ((Real)2.0 * g0 * (g0 + (Real)1.0) * a[0] + a[1]) / bett[0];
#pragma unroll
        for (int k = 1; k < NZ; ++k) {
          const Real qk = a[k];
          a[k] = ((Real)3.0 * (q_m + gkt[k] * qk) - a[k - 1]) / bett[k];
          q_mm = q_m;
          q_m = qk;
        }
        const Real gk = gkt[NZ - 1], gam_prev = gamd[NZ - 1];
        const Real a_bot = (Real)1.0 + gk * (gk + (Real)1.5);
        const Real xt1 = (Real)2.0 * gk * (gk + (Real)1.0);
        const Real xt2 = gk * (gk + (Real)0.5) - a_bot * gam_prev;
        a[NZ] = (xt1 * q_m + q_mm - a_bot * a[NZ - 1]) / xt2;
#pragma unroll
        for (int k = NZ - 1; k >= 0; --k) a[k] = a[k] - gamd[k] * a[k + 1];
#pragma unroll
        for (int k = 0; k <= NZ; ++k) KW_(qe, k) = a[k];
      } else {
        Real *A = (Real *)smem_ + lane;
        Real q_m = (Real)0, q_mm = (Real)0, a_prev = (Real)0;
        k_walk<1, 16, true>(
            nz,
            [&](int k) {
              KRec<1> r;
              r.v[0] = KW_(q, k);
              return r;
            },
            [&](int k, const KRec<1> &r) {
              const Real qk = r.v[0];
              if (k == 0) {
                q_m = q_mm = qk;
                return;
              }
              if (k == 1) {
                const Real g0 = gkt[0];
                a_prev = ((Real)2.0 * g0 * (g0 + (Real)1.0) * q_m + qk) / bett[0];
                A[0] = a_prev;
              }
              const Real gk = gkt[k];
              a_prev = ((Real)3.0 * (q_m + gk * qk) - a_prev) / bett[k];
              A[k * FV3_WAVE] = a_prev;
              q_mm = q_m;
              q_m = qk;
            });
        const Real gk = gkt[nz - 1], gam_prev = gamd[nz - 1];
        const Real a_bot = (Real)1.0 + gk * (gk + (Real)1.5);
        const Real xt1 = (Real)2.0 * gk * (gk + (Real)1.0);
        const Real xt2 = gk * (gk + (Real)0.5) - a_bot * gam_prev;
        Real a_next = (xt1 * q_m + q_mm - a_bot * a_prev) / xt2;
        KW_(qe, nz) = a_next;
        for (int k = nz - 1; k >= 0; --k) {
          a_next = A[k * FV3_WAVE] - gamd[k] * a_next;
          KW_(qe, k) = a_next;
        }
      }
    }
  });
}

// The generic form: a thread per column, any level count; the forward elimination and the back substitution as two kernels, the
// interface values through memory between them.
static void edge_profile_generic(fv3_ctx *c, fv3_stream_t s, Real *crx, Real *xfx, Real *cry, Real *yfx, Real *crx_a, Real *xfx_a, Real *cry_a, Real *yfx_a) {
  const Geo g = c->g;
  const int nz = g.nz;
  const int isd = 1 - g.nh, ied = g.nx + g.nh, jsd = 1 - g.nh, jed = g.ny + g.nh;
  {
    launch2(c, s, Box{isd, ied, jsd, jed, 0, 0}, [=] FV3_HD(int t, int i, int j) {
      const long tb = t * g.st;
      const unsigned pix = IX(i, j);
      const long p = tb + pix;
      (void)p;
      auto profile = [&](const Real *q, Real *qe) {
        const Real *dp0 = g.dp_ref;
        const Real g0 = dp0[1] / dp0[0];
        Real xt1 = (Real)2.0 * g0 * (g0 + (Real)1.0);
        Real bet = g0 * (g0 + (Real)0.5);
        K_(qe, 0) = (xt1 * K_(q, 0) + K_(q, 1)) / bet;
        Real gam_prev = ((Real)1.0 + g0 * (g0 + (Real)1.5)) / bet;
        Real gk = g0;
        // gam[k] is level-only: recomputed in the backward sweep from the same recurrence
        for (int k = 1; k < nz; ++k) {
          gk = dp0[k - 1] / dp0[k];
          bet = (Real)2.0 + (Real)2.0 * gk - gam_prev;
          K_(qe, k) = ((Real)3.0 * (K_(q, k - 1) + gk * K_(q, k)) - K_(qe, k - 1)) / bet;
          gam_prev = gk / bet;
        }
        const Real a_bot = (Real)1.0 + gk * (gk + (Real)1.5);
        xt1 = (Real)2.0 * gk * (gk + (Real)1.0);
        const Real xt2 = gk * (gk + (Real)0.5) - a_bot * gam_prev;
        K_(qe, nz) = (xt1 * K_(q, nz - 1) + K_(q, nz - 2) - a_bot * K_(qe, nz - 1)) / xt2;
      };
      const bool inx = i >= 1 && i <= g.nx + 1, iny = j >= 1 && j <= g.ny + 1;
      if (inx) {
        profile(crx, crx_a);
        profile(xfx, xfx_a);
      }
      if (iny) {
        profile(cry, cry_a);
        profile(yfx, yfx_a);
      }
    });
    // backward sweep: gam[k] depends on dp_ref only (table built at context creation)
    {
      const Real *gamd = g.ep_gam;
      launch2(c, s, Box{isd, ied, jsd, jed, 0, 0}, [=] FV3_HD(int t, int i, int j) {
        const long tb = t * g.st;
      const unsigned pix = IX(i, j);
      const long p = tb + pix;
      (void)p;
        const bool inx = i >= 1 && i <= g.nx + 1, iny = j >= 1 && j <= g.ny + 1;
        for (int k = nz - 1; k >= 0; --k) {
          const Real gm = gamd[k];
          if (inx) {
            K_(crx_a, k) = K_(crx_a, k) - gm * K_(crx_a, k + 1);
            K_(xfx_a, k) = K_(xfx_a, k) - gm * K_(xfx_a, k + 1);
          }
          if (iny) {
            K_(cry_a, k) = K_(cry_a, k) - gm * K_(cry_a, k + 1);
            K_(yfx_a, k) = K_(yfx_a, k) - gm * K_(yfx_a, k + 1);
          }
        }
      });
    }
  }
}

// cubic-spline-like layer -> interface interpolation (FV3 edge_profile, limiter 0), in the form the plan chose
static void edge_profile(fv3_ctx *c, fv3_stream_t s, const EpPlan &ep, Real *crx, Real *xfx, Real *cry, Real *yfx, Real *crx_a, Real *xfx_a, Real *cry_a, Real *yfx_a) {
  const int nz = c->g.nz;
  switch (ep.form) {
    case EP_WAVE_NZ:
      if (nz == 79)
        edge_profile_wave<79>(c, s, ep.one_launch, crx, xfx, cry, yfx, crx_a, xfx_a, cry_a, yfx_a);
      else
        edge_profile_wave<127>(c, s, ep.one_launch, crx, xfx, cry, yfx, crx_a, xfx_a, cry_a, yfx_a);
      return;
    case EP_WAVE_RT:
      edge_profile_wave<0>(c, s, ep.one_launch, crx, xfx, cry, yfx, crx_a, xfx_a, cry_a, yfx_a);
      return;
    case EP_REG:
      if (nz == 79)
        edge_profile_reg<79>(c, s, crx, xfx, cry, yfx, crx_a, xfx_a, cry_a, yfx_a);
      else if (nz == 127)
        edge_profile_reg<127>(c, s, crx, xfx, cry, yfx, crx_a, xfx_a, cry_a, yfx_a);
      else  // 8: exercised by the parity tests
        edge_profile_reg<8>(c, s, crx, xfx, cry, yfx, crx_a, xfx_a, cry_a, yfx_a);
      return;
    default:
      edge_profile_generic(c, s, crx, xfx, cry, yfx, crx_a, xfx_a, cry_a, yfx_a);
  }
}

// What this call does: the ONLY function of this file that asks the switch table.  It reports the edge_profile form (FV3_DEBUG_FD); the closing scan's line
// follows the transports, where the stage prints it.
static DzdPlan dzd_plan(const fv3_ctx *c, fv3_stream_t s) {
  const Geo &g = c->g;
  const int nz = g.nz;
  DzdPlan p{};
  p.debug = fv3_sw(FV3SW_DEBUG_FD);
  p.ep = ep_form(nz, sizeof(Real), fv3_sw(FV3SW_EDGE_PROFILE_GENERIC), fv3_sw(FV3SW_EDGE_PROFILE_REG), fv3_sw(FV3SW_EDGE_PROFILE_LDS));  // A/B switches
  p.ep.one_launch = fv3_sw(FV3SW_EP_ONE_LAUNCH);
  if (p.debug)
    for (int n = 0; n < p.ep.n_lines; ++n) fprintf(stderr, "[update_dz_d] edge_profile: %s\n", p.ep.lines[n]);
  for (int k = 0; k <= nz; ++k) p.nord_max = std::max(p.nord_max, c->nord_v_h[k]);
  // (FV3_ALT=dz_damp_scaled -- DESIGN §2, uncertain restatement 1: the coefficient d_sw's vorticity damping uses,
  //  (damp_vt * da_min_c)^(nord_v + 1), instead of the raw column value; the on / off test stays the raw coefficient)
  p.coef_scaled = fv3_alt("dz_damp_scaled");
  // Interfaces from fd_k0 on (chain of order 2 and switched on: all but the sponge layers) run the chain INSIDE the transport march
  // on the strips away from the W / E tile edges (tp2d_stream_t, TF_FD); del6_stream then only serves the tile-edge strips and
  // the cube-corner patches there.  FV3_DZ_DELN=arrays: the chain of every interface as one del6_stream launch (A/B reference).
  const bool off = dzd_chain_off(fv3_sw_is(FV3SW_DZ_DELN, "arrays"), fv3_sw_is(FV3SW_TP2D_MODE, "staged"), fv3_sw_is(FV3SW_DEL6_MODE, "staged"));
  p.lev = dzd_levels(nz, c->nord_v_h.data(), c->damp_vt_h.data(), off, fv3_aux(c, s) != s);
  // Round 6: inside the sequencer (fv3_seq_hints::dz_scan) the scan at the end of this operator becomes the pre-sweep of riem_solver3's wave form, which reads the
  // marched heights where this call leaves them (the free slot SC_F: riem_solver3's scratch fields are SC_A / C / D / E).  FV3_DZ_SCAN=separate: the scan kernel (A/B).
  const RiemForm heavy = riem_form(nz, sizeof(Real), g.sk, true, fv3_sw(FV3SW_RIEM_MODE), fv3_sw(FV3SW_RIEM_REGS));
  p.defer = dz_scan_defers(c->seq.dz_scan, heavy, fv3_sw_is(FV3SW_DZ_SCAN, "separate"));
  return p;
}

// del-n damping fluxes of the interface heights, then their transport: the advective-form update and the
// damping term are the transport kernel's epilogue (znew; the height fluxes are never stored)
static void fv3_update_dz_d_transport(fv3_ctx *c, fv3_stream_t s, const DzdPlan &plan, Real *zh, Real *znew) {
  const Geo &g = c->g;
  const int nz = g.nz, fd_k0 = plan.lev.fd_k0;
  Real *crx_a = c->scratch[SC_A], *xfx_a = c->scratch[SC_B], *cry_a = c->scratch[SC_C], *yfx_a = c->scratch[SC_D];
  Real *fx2 = c->scratch[SC_G], *fy2 = c->scratch[SC_H], *d2 = c->scratch[SC_I];
  const Real *dz_coef = plan.coef_scaled ? c->tab.d6_vt : g.damp_vt;
  Deln dn{g.nord_v, dz_coef, g.damp_vt, 0, (Real)0, false, (Real)1.0e-5, plan.nord_max};
  // (the interfaces without the chain inside the march -- the sponge layers: their del-n launch and their small transport launch go
  //  to the auxiliary stream, beside the march of the others; EV_SUB_FORK / EV_SUB_JOIN)
  fv3_stream_t sa = plan.lev.fork ? fv3_aux(c, s) : s;
  if (sa != s) {
    fv3_signal(c, s, EV_SUB_FORK);
    fv3_wait(c, sa, EV_SUB_FORK);
  }
  del6_vt_flux(c, sa, zh, d2, fx2, fy2, dn, false, 0, fd_k0 - 1);
  if (tp2d_fd_lean(c, c->cfg.hord_tm, fd_k0, nz))  // (the round-5 march runs the chain on every strip: only the cube-corner patches come from the staged chain)
    del6_vt_flux_patches(c, s, zh, d2, fx2, fy2, dn, false, fd_k0, nz);
  else
    del6_vt_flux_edge_strips(c, s, zh, d2, fx2, fy2, dn, false, fd_k0, nz);
  TpEpi e{znew, nullptr, false, nullptr, nullptr, nullptr, nullptr, nullptr, true, fx2, fy2, g.damp_vt, nullptr, nullptr};
  tp2d(c, sa, zh, crx_a, cry_a, xfx_a, yfx_a, c->scratch[SC_J], c->scratch[SC_K], nullptr, nullptr, nullptr, c->cfg.hord_tm, nullptr, 0, fd_k0 - 1, &e);
  if (sa != s) fv3_signal(c, sa, EV_SUB_JOIN);
  e.fd = 1;
  e.fd_coef = dz_coef;
  tp2d(c, s, zh, crx_a, cry_a, xfx_a, yfx_a, c->scratch[SC_J], c->scratch[SC_K], nullptr, nullptr, nullptr, c->cfg.hord_tm, nullptr, fd_k0, nz, &e);
  if (sa != s) fv3_wait(c, s, EV_SUB_JOIN);
}

// the closing scan (bottom-up): interface k stays dz_min above interface k + 1; the surface vertical velocity from the lowest interface
static void fv3_update_dz_d_scan(fv3_ctx *c, fv3_stream_t s, Real *zs, Real *zh, Real *wsd, Real *znew, Real dt, Real dz_min) {
  const Geo g = c->g;
  const int nz = g.nz;
  launch2(c, s, Box{1, g.nx, 1, g.ny, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const long tb = t * g.st;
    const unsigned pix = IX(i, j);
    const long p = tb + pix;
    (void)p;
    Real below = K_(znew, nz);
    K_(zh, nz) = below;
    wsd[t * g.st2 + IX(i, j)] = (zs[t * g.st2 + IX(i, j)] - below) / dt;
    for (int k = nz - 1; k >= 0; --k) {
      const Real v = fv3_dz_floor(K_(znew, k), below, dz_min);
      K_(zh, k) = v;
      below = v;
    }
  });
}

extern "C" int fv3_update_dz_d(fv3_ctx *c, const fv3_field *zs_, const fv3_field *zh_, const fv3_field *crx_, const fv3_field *cry_, const fv3_field *xfx_,
                               const fv3_field *yfx_, const fv3_field *wsd_, double dtd, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD2D(zs, zs_) FV3_FIELD(zh, zh_) FV3_FIELD(crx, crx_) FV3_FIELD(cry, cry_) FV3_FIELD(xfx, xfx_) FV3_FIELD(yfx, yfx_) FV3_FIELD2D(wsd, wsd_)
  fv3_stream_t s = (fv3_stream_t)stream;
  const Real dz_min = (Real)c->cst.dz_min;
  const DzdPlan plan = dzd_plan(c, s);
  Real *znew = c->scratch[plan.defer ? SC_F : SC_E];
  edge_profile(c, s, plan.ep, crx, xfx, cry, yfx, c->scratch[SC_A], c->scratch[SC_B], c->scratch[SC_C], c->scratch[SC_D]);
  fv3_update_dz_d_transport(c, s, plan, zh, znew);
  if (plan.debug) fprintf(stderr, "[update_dz_d] closing scan: %s\n", plan.defer ? "left to riem_solver3's pre-sweep" : "own kernel");
  if (plan.defer)
    fv3_dz_scan_leave(c, znew, dz_min);
  else
    fv3_update_dz_d_scan(c, s, zs, zh, wsd, znew, (Real)dtd, dz_min);
  return fv3_post(c, s, "update_dz_d");
}


// fv3_fillz.hip -- vertical filling of negative tracer means after the Lagrangian-to-Eulerian remap (FV3 fv_fill.F90, subroutine
// fillz in its default form; pyFV3 FillNegativeTracerValues, the last tracer step of LagrangianToEulerian with `fill: true`
// [REF driver/examples/configs/baroclinic_c12.yaml:56]).  Column-local, in place, on the compute cells and levels 0 .. nz-1.
//
// Per column and tracer (0-based, km = nz, every product / quotient / sum rounded on its own):
//   1 top       q[0] < 0: q[1] += (q[0] * dp[0]) / dp[1], q[0] = 0                                          (does not set zfix)
//   2 interior  k = 1 .. km-2 in increasing order, q[k] < 0: zfix; borrow min(q[k-1] * dp[k-1], -q[k] * dp[k]) from above where
//               q[k-1] > 0, then, where q[k] is still < 0 and q[k+1] > 0, min(q[k+1] * dp[k+1], -q[k] * dp[k]) from below
//   3 bottom    q[km-1] < 0 and q[km-2] > 0: zfix; borrow min(-q[km-1] * dp[km-1], q[km-2] * dp[km-2]) from above
//   4 non-local where zfix: dm[k] = q[k] * dp[k] (k >= 1), sum0 = sum dm, sum1 = sum max(0, dm) (increasing k, from 0); where
//               sum0 > 0: q[k] = max(0, ((sum0 / sum1) * dm[k]) / dp[k]) for k >= 1
// Comparisons are plain IEEE (-0.0 and NaN take no branch); min(a, b) is `a < b ? a : b`, max(0, x) is `x < 0 ? 0 : x` in the
// quotient and `x > 0 ? x : 0` in sum1.  A column without a negative value is not written at all.
//
// A thread owns a column (i fastest: every level access of a wave is one coalesced row) and carries up to four tracers through it, so
// dp is read once per group.  ONE sweep down the column does steps 1 - 3 on a three-level register window (q[k-1], q[k], q[k+1]) per
// tracer + the dp window, with the loads of level k+2 issued a step ahead; a level is final when it leaves the window as k-1, and
// that is where it is added to sum0 / sum1 and -- only if a step changed it (one dirty bit per window slot) -- stored.  The columns
// with zfix and sum0 > 0 (rare on real data) then run the rescaling sweep, a divergent tail: read q, dp, write q where it differs.
// On data without negatives the kernel reads n_tracers + ceil(n_tracers / 4) fields and writes nothing.
#include "fv3_common.h"

namespace {

#define FZ_MAXG 4  // tracers a thread carries (fp64, 4: 96 VGPRs, nothing spilled -- four waves per SIMD need <= 128)

template <int NG>
struct FillGroup {
  Real *q[NG];
};

FV3_HD inline Real fz_min(Real a, Real b) { return a < b ? a : b; }

// level k of a field at the thread's column: wave-uniform plane base + 32-bit in-plane offset
#define FZ(ptr, k) FV3_EL((ptr) + tb + (long)(k)*sk, pix)

template <int NG>
void fillz_group(fv3_ctx *c, fv3_stream_t s, const FillGroup<NG> grp, const Real *dp) {
  const Geo g = c->g;
  launch2(c, s, Box{1, g.nx, 1, g.ny, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const int km = g.nz;
    const long tb = t * g.st, sk = g.sk;
    const unsigned pix = IX(i, j);
    // window: a / b / cq = q[k-1] / q[k] / q[k+1], nq = the prefetched q[k+2]; dirty bits 0 / 1 / 2 = slots a / b / cq
    Real a[NG], b[NG], cq[NG], nq[NG], s0[NG], s1[NG];
    unsigned dirty[NG];
    bool zfix[NG];
    const int k2 = km > 2 ? 2 : km - 1;  // (two levels: the third slot re-reads the last one and is never used)
    Real da = FZ(dp, 0), db = FZ(dp, 1), dc = FZ(dp, k2), dn;
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      a[n] = FZ(grp.q[n], 0);
      b[n] = FZ(grp.q[n], 1);
      cq[n] = FZ(grp.q[n], k2);
      s0[n] = (Real)0;
      s1[n] = (Real)0;
      dirty[n] = 0u;
      zfix[n] = false;
    }
    // ---- 1: top layer
#pragma unroll
    for (int n = 0; n < NG; ++n)
      if (a[n] < (Real)0) {
        b[n] = b[n] + (a[n] * da) / db;
        a[n] = (Real)0;
        dirty[n] |= 3u;
      }
    // ---- 2: interior
    for (int k = 1; k < km - 1; ++k) {
      const int kn = k + 2 < km ? k + 2 : km - 1;  // (the pad level is never read: the last level again)
      dn = FZ(dp, kn);
#pragma unroll
      for (int n = 0; n < NG; ++n) nq[n] = FZ(grp.q[n], kn);
#pragma unroll
      for (int n = 0; n < NG; ++n) {
        if (b[n] < (Real)0) {
          zfix[n] = true;
          if (a[n] > (Real)0) {  // borrow from above
            const Real dq = fz_min(a[n] * da, -b[n] * db);
            a[n] = a[n] - dq / da;
            b[n] = b[n] + dq / db;
            dirty[n] |= 3u;
          }
          if (b[n] < (Real)0 && cq[n] > (Real)0) {  // borrow from below
            const Real dq = fz_min(cq[n] * dc, -b[n] * db);
            cq[n] = cq[n] - dq / dc;
            b[n] = b[n] + dq / db;
            dirty[n] |= 6u;
          }
        }
        // level k-1 leaves the window: final
        if (dirty[n] & 1u) FZ(grp.q[n], k - 1) = a[n];
        if (k >= 2) {
          const Real dm = a[n] * da;
          s0[n] = s0[n] + dm;
          s1[n] = s1[n] + (dm > (Real)0 ? dm : (Real)0);
        }
        a[n] = b[n];
        b[n] = cq[n];
        cq[n] = nq[n];
        dirty[n] >>= 1;
      }
      da = db;
      db = dc;
      dc = dn;
    }
    // ---- 3: bottom layer (a / b = levels km-2 / km-1), the two last levels become final
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      if (b[n] < (Real)0 && a[n] > (Real)0) {
        zfix[n] = true;
        const Real dup = fz_min(-b[n] * db, a[n] * da);
        a[n] = a[n] - dup / da;
        b[n] = b[n] + dup / db;
        dirty[n] |= 3u;
      }
      if (dirty[n] & 1u) FZ(grp.q[n], km - 2) = a[n];
      if (dirty[n] & 2u) FZ(grp.q[n], km - 1) = b[n];
      if (km >= 3) {
        const Real dm = a[n] * da;
        s0[n] = s0[n] + dm;
        s1[n] = s1[n] + (dm > (Real)0 ? dm : (Real)0);
      }
      const Real dm = b[n] * db;
      s0[n] = s0[n] + dm;
      s1[n] = s1[n] + (dm > (Real)0 ? dm : (Real)0);
    }
    // ---- 4: non-local fix (level 0 is not touched)
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      if (zfix[n] && s0[n] > (Real)0) {
        const Real fac = s0[n] / s1[n];
        for (int k = 1; k < km; ++k) {
          const Real qv = FZ(grp.q[n], k), d = FZ(dp, k);
          Real v = (fac * (qv * d)) / d;
          if (v < (Real)0) v = (Real)0;
          if (v != qv) FZ(grp.q[n], k) = v;
        }
      }
    }
  });
}

template <int NG>
void fillz_launch(fv3_ctx *c, fv3_stream_t s, Real *const *q, const Real *dp) {
  FillGroup<NG> grp;
  for (int n = 0; n < NG; ++n) grp.q[n] = q[n];
  fillz_group<NG>(c, s, grp, dp);
}

}  // namespace

// the launches of fv3_fillz on checked pointers (n_tracers >= 1, nz >= 2, no field given twice): also the filling step of fv3_remap_moist
void fv3_fillz_launch(fv3_ctx *c, fv3_stream_t s, int n_tracers, Real *const *q, const Real *dp) {
  for (int n0 = 0; n0 < n_tracers; n0 += FZ_MAXG) {
    const int ng = n_tracers - n0 < FZ_MAXG ? n_tracers - n0 : FZ_MAXG;
    if (ng == 4)
      fillz_launch<4>(c, s, q + n0, dp);
    else if (ng == 3)
      fillz_launch<3>(c, s, q + n0, dp);
    else if (ng == 2)
      fillz_launch<2>(c, s, q + n0, dp);
    else
      fillz_launch<1>(c, s, q + n0, dp);
  }
}

extern "C" int fv3_fillz(fv3_ctx *c, int n_tracers, const fv3_field *const *tracers, const fv3_field *dp_, void *stream) {
  if (!c) return FV3_ERR_ARG;
  if (n_tracers < 0) return fv3_fail(c, FV3_ERR_ARG, "fillz: n_tracers = " + std::to_string(n_tracers) + " is negative");
  if (n_tracers > 0 && !tracers) return fv3_fail(c, FV3_ERR_ARG, "fillz: the tracer list is null with n_tracers = " + std::to_string(n_tracers));
  FV3_FIELD(dp, dp_)
  std::vector<Real *> q(n_tracers);
  for (int n = 0; n < n_tracers; ++n) {
    q[n] = fv3_chk(c, tracers[n], "tracer");
    if (!q[n]) return FV3_ERR_ARG;
    // the tracers of a group share a thread: a field given twice, or dp among them, would make the result depend on the grouping
    if (q[n] == dp) return fv3_fail(c, FV3_ERR_ARG, "fillz: tracer " + std::to_string(n) + " is the dp field (dp is only read)");
    for (int m = 0; m < n; ++m)
      if (q[m] == q[n]) return fv3_fail(c, FV3_ERR_ARG, "fillz: tracers " + std::to_string(m) + " and " + std::to_string(n) + " are the same field");
  }
  if (c->g.nz < 2) return fv3_fail(c, FV3_ERR_UNSUPPORTED, "fillz: needs at least 2 levels (nz = " + std::to_string(c->g.nz) + ")");
  if (n_tracers == 0) return FV3_OK;
  fv3_stream_t s = (fv3_stream_t)stream;
  fv3_fillz_launch(c, s, n_tracers, q.data(), dp);
  return fv3_post(c, s, "fillz");
}

// fv3_nh.hip -- non-hydrostatic pressure-gradient and column operators: p_grad_c, nh_p_grad (staged form), pk3_halo, edge_pe, Ray_fast,
// del2_cubed, apply_diffusive_heating, and the device self-tests of the hand-written arithmetic.  The height chain lives beside it: the
// Riemann solvers in fv3_riem.hip, update_dz_c / update_dz_d in fv3_dz.hip.  CPU twin: oracle/fv3_oracle/nh.py.  [SURVEY A.5-A.12]
//
// Column kernels: one thread per (i, j) column walks k; because i is the fastest index every
// per-level access of a wavefront is one coalesced row.
#include "fv3_ops.h"
#include "fv3_kwalk.h"
#include "fv3_math.h"
#include "fv3_agpr.h"

#ifndef PG_KC
#define PG_KC 16  // levels one thread of the pressure-gradient kernels walks
#endif

// ---------------------------------------------------------------------------------------------
extern "C" int fv3_p_grad_c(fv3_ctx *c, const fv3_field *uc_, const fv3_field *vc_, const fv3_field *delpc_, const fv3_field *pkc_, const fv3_field *gz_,
                            double dt2d, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(uc, uc_) FV3_FIELD(vc, vc_) FV3_FIELD(delpc, delpc_) FV3_FIELD(pkc, pkc_) FV3_FIELD(gz, gz_)
  const Geo g = c->g;
  const Real dt2 = (Real)dt2d;
  // A thread walks PG_KC levels keeping the lower-interface values (gz, pkc at k+1, three points each) in
  // registers for the next level: every interface plane is read once instead of twice (9 -> 7 field passes).
  // (rolled loop: an unrolled level loop lets the compiler hoist every level's loads at once)
  const int nz = g.nz, nchunk = (nz + PG_KC - 1) / PG_KC;
  launch3_pass(c, (fv3_stream_t)stream, Box{1, g.nx + 1, 1, g.ny + 1, 0, nchunk - 1}, c->seq.frame_pass, [=] FV3_HD(int t, int kc, int i, int j) {
    const long m2 = t * g.st2;
    const unsigned p = IX(i, j), px = IX(i - 1, j), py = IX(i, j - 1);
    const bool do_u = j <= g.ny, do_v = i <= g.nx;
    const Real rx = (g.rdxc + m2)[p], ry = (g.rdyc + m2)[p];
    const int ka = kc * PG_KC, kb = ka + PG_KC < nz ? ka + PG_KC : nz;
    long b = t * g.st + ka * g.sk;
    Real g0 = (gz + b)[p], gx0 = (gz + b)[px], gy0 = (gz + b)[py];
    Real k0 = (pkc + b)[p], kx0 = (pkc + b)[px], ky0 = (pkc + b)[py];
#pragma unroll 1
    for (int k = ka; k < kb; ++k) {
      const long b1 = b + g.sk;
      const Real g1 = (gz + b1)[p], gx1 = (gz + b1)[px], gy1 = (gz + b1)[py];
      const Real k1 = (pkc + b1)[p], kx1 = (pkc + b1)[px], ky1 = (pkc + b1)[py];
      const Real dpc = (delpc + b)[p];
      if (do_u) (uc + b)[p] = (uc + b)[p] + dt2 * rx / ((delpc + b)[px] + dpc) * ((gx1 - g0) * (k1 - kx0) + (gx0 - g1) * (kx1 - k0));
      if (do_v) (vc + b)[p] = (vc + b)[p] + dt2 * ry / ((delpc + b)[py] + dpc) * ((gy1 - g0) * (k1 - ky0) + (gy0 - g1) * (ky1 - k0));
      g0 = g1;
      gx0 = gx1;
      gy0 = gy1;
      k0 = k1;
      kx0 = kx1;
      ky0 = ky1;
      b = b1;
    }
  });
  return fv3_post(c, (fv3_stream_t)stream, "p_grad_c");
}

extern "C" int fv3_nh_p_grad(fv3_ctx *c, const fv3_field *u_, const fv3_field *v_, const fv3_field *pp_, const fv3_field *gz_, const fv3_field *pk3_,
                             const fv3_field *delp_, double dtd, double ptop, double akap, void *stream) {
  return fv3_nh_p_grad_scaled(c, u_, v_, pp_, gz_, pk3_, delp_, dtd, ptop, akap, 1.0, stream);
}

// gz_scale: the sequencer passes the interface heights zh with gz_scale = g instead of first storing
// gz = g * zh (compute_geopotential): the product is formed where a2b_ord4 reads its input (same bits).
int fv3_nh_p_grad_scaled(fv3_ctx *c, const fv3_field *u_, const fv3_field *v_, const fv3_field *pp_, const fv3_field *gz_, const fv3_field *pk3_,
                         const fv3_field *delp_, double dtd, double ptop, double akap, double gz_scale, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(u, u_) FV3_FIELD(v, v_) FV3_FIELD(pp, pp_) FV3_FIELD(gz, gz_) FV3_FIELD(pk3, pk3_) FV3_FIELD(delp, delp_)
  const Geo g = c->g;
  fv3_stream_t s = (fv3_stream_t)stream;
  const Real dt = (Real)dtd;
  const Real top = (Real)std::pow(ptop, akap);
  const int nz = g.nz;
  // corner-interpolated pp / pk3 / gz / delp go to scratch: the reference interpolates pp, pk3 and gz in
  // place, but nothing reads them afterwards (gz and pk3 are rebuilt every sub-step), so the three
  // copy-back passes are not spent; the inputs come back unchanged.
  // product form: the four corner interpolations and the wind update as one marching kernel (fv3_pgf.hip); FV3_NH_PGF=staged keeps
  // the four a2b_ord4 launches + the level-walking update below (A/B reference)
  if (!fv3_sw_is(FV3SW_NH_PGF, "staged")) {  // (read per call: the A/B parity test flips it in one process)
    nh_pgf_fused(c, s, pp, pk3, gz, delp, u, v, dt, top, (Real)gz_scale, c->seq.frame_pass);
    return fv3_post(c, s, "nh_p_grad");
  }
  Real *ppb = c->scratch[SC_B], *pk3b = c->scratch[SC_C], *gzb = c->scratch[SC_D], *wk1 = c->scratch[SC_A];
  if (c->seq.frame_pass != 2) {  // (interior pass of the frame-first form: the corner fields are in scratch already)
    launch2(c, s, Box{1, g.nx + 1, 1, g.ny + 1, 0, 0}, [=] FV3_HD(int t, int i, int j) {
      const long p = t * g.st + IX(i, j);
      ppb[p] = (Real)0;
      pk3b[p] = top;
    });
    a2b_ord4(c, s, pp, ppb, 1, 1, nz, false);
    a2b_ord4(c, s, pk3, pk3b, 1, 1, nz, false);
    a2b_ord4(c, s, gz, gzb, 0, 0, nz + 1, false, (Real)gz_scale);
    a2b_ord4(c, s, delp, wk1, 0, 0, nz, false);
  }
  // A thread walks PG_KC levels keeping the lower-interface corner values (pk3, gz, pp at k+1, three corners each)
  // in registers for the next level: every interface plane is read once instead of twice (11 -> 8 field passes).
  const int nchunk = (nz + PG_KC - 1) / PG_KC;
  launch3_pass(c, s, Box{1, g.nx + 1, 1, g.ny + 1, 0, nchunk - 1}, c->seq.frame_pass, [=] FV3_HD(int t, int kc, int i, int j) {
    const long m2 = t * g.st2;
    const unsigned p = IX(i, j), pe_ = IX(i + 1, j), pn = IX(i, j + 1);
    const bool do_u = i <= g.nx, do_v = j <= g.ny;
    const Real rx = (g.rdx + m2)[p], ry = (g.rdy + m2)[p];
    const int ka = kc * PG_KC, kb = ka + PG_KC < nz ? ka + PG_KC : nz;
    long b = t * g.st + ka * g.sk;
    Real k0 = (pk3b + b)[p], ke0 = (pk3b + b)[pe_], kn0 = (pk3b + b)[pn];
    Real g0 = (gzb + b)[p], ge0 = (gzb + b)[pe_], gn0 = (gzb + b)[pn];
    Real q0 = (ppb + b)[p], qe0 = (ppb + b)[pe_], qn0 = (ppb + b)[pn];
#pragma unroll 1
    for (int k = ka; k < kb; ++k) {
      const long b1 = b + g.sk;
      const Real k1 = (pk3b + b1)[p], ke1 = (pk3b + b1)[pe_], kn1 = (pk3b + b1)[pn];
      const Real g1 = (gzb + b1)[p], ge1 = (gzb + b1)[pe_], gn1 = (gzb + b1)[pn];
      const Real q1 = (ppb + b1)[p], qe1 = (ppb + b1)[pe_], qn1 = (ppb + b1)[pn];
      const Real wkp = k1 - k0, w1p = (wk1 + b)[p];
      if (do_u) {
        const Real du = dt / (wkp + (ke1 - ke0)) * ((g1 - ge0) * (ke1 - k0) + (g0 - ge1) * (k1 - ke0));
        (u + b)[p] = ((u + b)[p] + du + dt / (w1p + (wk1 + b)[pe_]) * ((g1 - ge0) * (qe1 - q0) + (g0 - ge1) * (q1 - qe0))) * rx;
      }
      if (do_v) {
        const Real dv = dt / (wkp + (kn1 - kn0)) * ((g1 - gn0) * (kn1 - k0) + (g0 - gn1) * (k1 - kn0));
        (v + b)[p] = ((v + b)[p] + dv + dt / (w1p + (wk1 + b)[pn]) * ((g1 - gn0) * (qn1 - q0) + (g0 - gn1) * (q1 - qn0))) * ry;
      }
      k0 = k1;
      ke0 = ke1;
      kn0 = kn1;
      g0 = g1;
      ge0 = ge1;
      gn0 = gn1;
      q0 = q1;
      qe0 = qe1;
      qn0 = qn1;
      b = b1;
    }
  });
  return fv3_post(c, s, "nh_p_grad");
}

// ---------------------------------------------------------------------------------------------
extern "C" int fv3_pk3_halo(fv3_ctx *c, const fv3_field *pk3_, const fv3_field *delp_, double ptopd, double akapd, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(pk3, pk3_) FV3_FIELD(delp, delp_)
  const Geo g = c->g;
  const Real ptop = (Real)ptopd, akap = (Real)akapd;
  // the two-cell ring around the compute domain only: S / N strips as they lie, W / E strips transposed (lanes along j)
  // -- a launch over the whole padded plane spends its time on threads that exit (0.49 -> 0.2 ms at C768)
  auto column = [=] FV3_HD(int t, int i, int j) {
    const long tb = t * g.st;
    const unsigned pix = IX(i, j);
    Real pei = ptop;
    for (int k = 0; k < g.nz; ++k) {
      pei = pei + K_(delp, k);
      K_(pk3, k + 1) = fv3_exp(akap * fv3_log(pei));
    }
  };
  fv3_stream_t s = (fv3_stream_t)stream;
  const int nx = g.nx, ny = g.ny;
  launch2(c, s, Box{-1, nx + 2, -1, 0, 0, 0}, column);
  launch2(c, s, Box{-1, nx + 2, ny + 1, ny + 2, 0, 0}, column);
  launch2(c, s, Box{1, ny, 0, 1, 0, 0}, [=] FV3_HD(int t, int a, int b_) { column(t, b_ - 1, a); });
  launch2(c, s, Box{1, ny, 0, 1, 0, 0}, [=] FV3_HD(int t, int a, int b_) { column(t, nx + 1 + b_, a); });
  return fv3_post(c, (fv3_stream_t)stream, "pk3_halo");
}

extern "C" int fv3_edge_pe(fv3_ctx *c, const fv3_field *pe_, const fv3_field *delp_, double ptopd, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(pe, pe_) FV3_FIELD(delp, delp_)
  const Geo g = c->g;
  const Real ptop = (Real)ptopd;
  launch2(c, (fv3_stream_t)stream, Box{0, g.nx + 1, 0, g.ny + 1, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    if (i >= 1 && i <= g.nx && j >= 1 && j <= g.ny) return;
    const long tb = t * g.st;
    const unsigned pix = IX(i, j);
    const long p = tb + pix;
    (void)p;
    Real pei = ptop;
    K_(pe, 0) = pei;
    for (int k = 0; k < g.nz; ++k) {
      pei = pei + K_(delp, k);
      K_(pe, k + 1) = pei;
    }
  });
  return fv3_post(c, (fv3_stream_t)stream, "edge_pe");
}

// ---------------------------------------------------------------------------------------------
extern "C" int fv3_ray_fast(fv3_ctx *c, const fv3_field *u_, const fv3_field *v_, const fv3_field *w_, double dt, double ptop, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(u, u_) FV3_FIELD(v, v_) FV3_FIELD(w, w_)
  const Geo g = c->g;
  const int nz = g.nz;
  const double rf_cutoff = c->cfg.rf_cutoff;
  const double nudge = rf_cutoff + std::fmin(100.0, 10.0 * ptop);
  const double tau0 = c->cfg.tau * c->cst.seconds_per_day;
  // rf table for this (dt, ptop): host libm, cached in the context
  if (!c->tab_rf || c->rf_dt != dt || c->rf_ptop != ptop) {
    std::vector<Real> rf(nz, (Real)1);
    int nd = 0, nn = 0;
    double dm = 0.0;
    for (int k = 0; k < nz; ++k) {
      const double pf = c->pfull_h[k];
      if (pf < rf_cutoff) {
        const double sn = std::sin(0.5 * c->cst.pi * std::log(rf_cutoff / pf) / std::log(rf_cutoff / ptop));
        rf[k] = (Real)(1.0 / (1.0 + dt / tau0 * (sn * sn)));
        nd = k + 1;
      }
      if (pf < nudge) {
        dm += c->dp_ref_h[k];
        nn = k + 1;
      }
    }
    if (!c->tab_rf) {
      c->tab_rf = fv3_dev_alloc(c, nz * sizeof(Real));
      if (!c->tab_rf) return fv3_fail(c, FV3_ERR_NOMEM, "rf table");
    }
    fv3_h2d(c->tab_rf, rf.data(), nz * sizeof(Real));
    c->rf_dt = dt;
    c->rf_ptop = ptop;
    c->rf_nd = nd;
    c->rf_nn = nn;
    c->rf_dm = dm;
  }
  const int nd = c->rf_nd, nn = c->rf_nn;
  if (nn == 0) return FV3_OK;
  const Real dm = (Real)c->rf_dm;
  const Real *rf = (const Real *)c->tab_rf;
  const bool momentum_fix = !fv3_alt("ray_fast_plain");  // (FV3_ALT: DESIGN §2, uncertain restatement 4)
  launch2_pass(c, (fv3_stream_t)stream, Box{1, g.nx + 1, 1, g.ny + 1, 0, 0}, c->seq.frame_pass, [=] FV3_HD(int t, int i, int j) {
    const long tb = t * g.st;
    const unsigned pix = IX(i, j);
    const long p = tb + pix;
    (void)p;
    auto wind = [&](Real *a) {
      Real dmdir = (Real)0;
      for (int k = 0; k < nd; ++k) {
        dmdir = dmdir + ((Real)1.0 - rf[k]) * g.dp_ref[k] * K_(a, k);
        K_(a, k) = K_(a, k) * rf[k];
      }
      const Real add = dmdir / dm;
      if (momentum_fix)
        for (int k = 0; k < nn; ++k) K_(a, k) = K_(a, k) + add;
    };
    if (i <= g.nx) wind(u);
    if (j <= g.ny) wind(v);
    if (i <= g.nx && j <= g.ny)
      for (int k = 0; k < nd; ++k) K_(w, k) = K_(w, k) * rf[k];
  });
  return fv3_post(c, (fv3_stream_t)stream, "ray_fast");
}

// the three cells at every cube corner of a sub-domain become their mean (del2_cubed, before each iteration), in place
void del2_fill_corners(fv3_ctx *c, fv3_stream_t s, Real *qin) {
  const Geo g = c->g;
  const int nz1 = g.nz - 1;
  launch3(c, s, Box{1, 1, 1, 1, 0, nz1}, [=] FV3_HD(int t, int k, int, int) {
    const int fl = g.flags[t];
    const bool W = fl & FV3_W, E = fl & FV3_E, S = fl & FV3_S, N = fl & FV3_N;
    Real *qq = qin + t * g.st + k * g.sk;
    const int npx = g.npx, npy = g.npy, ie = g.nx, je = g.ny;
    const Real r3 = (Real)(1.0 / 3.0);
    if (W && S) {
      const Real a = (qq[IX(1, 1)] + qq[IX(0, 1)] + qq[IX(1, 0)]) * r3;
      qq[IX(1, 1)] = a; qq[IX(0, 1)] = a; qq[IX(1, 0)] = a;
    }
    if (E && S) {
      const Real a = (qq[IX(ie, 1)] + qq[IX(npx, 1)] + qq[IX(ie, 0)]) * r3;
      qq[IX(ie, 1)] = a; qq[IX(npx, 1)] = a; qq[IX(ie, 0)] = a;
    }
    if (E && N) {
      const Real a = (qq[IX(ie, je)] + qq[IX(npx, je)] + qq[IX(ie, npy)]) * r3;
      qq[IX(ie, je)] = a; qq[IX(npx, je)] = a; qq[IX(ie, npy)] = a;
    }
    if (W && N) {
      const Real a = (qq[IX(1, je)] + qq[IX(0, je)] + qq[IX(1, npy)]) * r3;
      qq[IX(1, je)] = a; qq[IX(0, je)] = a; qq[IX(1, npy)] = a;
    }
  });
}

// ---------------------------------------------------------------------------------------------
extern "C" int fv3_del2_cubed(fv3_ctx *c, const fv3_field *q_, double cdd, int nmax, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(q, q_)
  const Geo g = c->g;
  fv3_stream_t s = (fv3_stream_t)stream;
  const Real cd = (Real)cdd;
  const int ntimes = nmax < 3 ? nmax : 3;
  const int nz1 = g.nz - 1;
  // One launch per iteration, out of place (q -> B -> A -> q for three iterations): the x / y fluxes of a cell's four
  // faces are formed in registers from the five neighbouring values instead of being stored and read back (7 -> 2
  // field passes per iteration), FV3_KC levels per thread with the five metric terms loaded once.  Every launch
  // covers the whole padded plane -- cells outside the iteration's update box are copied -- so each buffer is
  // complete, as the in-place reference field is.
  Real *bufA = c->scratch[SC_A], *bufB = c->scratch[SC_B];
  const int isd = 1 - g.nh, ied = g.nx + g.nh, jsd = 1 - g.nh, jed = g.ny + g.nh;
  const int nkc = (nz1 + FV3_KC) / FV3_KC;
  Real *in = q;
  for (int n = 1; n <= ntimes; ++n) {
    const int nt = ntimes - n;
    Real *out = nt == 0 ? (ntimes == 1 ? bufA : q) : (nt % 2 ? bufA : bufB);
    if (out == in) out = out == bufA ? bufB : bufA;
    Real *qin = in;
    del2_fill_corners(c, s, qin);
    launch3(c, s, Box{isd, ied, jsd, jed, 0, nkc - 1}, [=] FV3_HD(int t, int kp, int i_, int j_) {
      const int fl = g.flags[t];
      const long m2 = t * g.st2;
      int i = i_, j = j_;
      const bool upd = i >= 1 - nt && i <= g.nx + nt && j >= 1 - nt && j <= g.ny + nt;
      const unsigned p0 = IX(i, j);
      Real mvx0 = (Real)0, mvx1 = (Real)0, muy0 = (Real)0, muy1 = (Real)0, cra = (Real)0;
      // the six points of the stencil as in-plane offsets, formed ONCE (they do not depend on the level): the corner-halo remaps
      // (cc_index: a dozen compares and selects per point) were evaluated per level inside the loop -- the kernel ran at 2.8 TB/s on its
      // 5.5 GB because of that index arithmetic, not because of its bytes
      unsigned pxw = p0, pxc = p0, pxe = p0, pys = p0, pyc = p0, pyn = p0;
      if (upd) {
        mvx0 = (g.del6_v + m2)[p0];
        mvx1 = (g.del6_v + m2)[IX(i + 1, j)];
        muy0 = (g.del6_u + m2)[p0];
        muy1 = (g.del6_u + m2)[IX(i, j + 1)];
        cra = cd * (g.rarea + m2)[p0];
        if (nt > 0) {
          pxw = cc_index<1>(g, fl, i - 1, j);
          pxc = cc_index<1>(g, fl, i, j);
          pxe = cc_index<1>(g, fl, i + 1, j);
          pys = cc_index<2>(g, fl, i, j - 1);
          pyc = cc_index<2>(g, fl, i, j);
          pyn = cc_index<2>(g, fl, i, j + 1);
        } else {
          pxw = IX(i - 1, j);
          pxe = IX(i + 1, j);
          pys = IX(i, j - 1);
          pyn = IX(i, j + 1);
        }
      }
#ifndef FV3_DEL2_UNROLL
#define FV3_DEL2_UNROLL 2
#endif
      // (no early exit inside the loop: a level past the last one is clamped and its store masked, so that the unrolled body has the
      //  loads of several levels in flight -- with `break` every level waited for its own seven loads)
#pragma unroll FV3_DEL2_UNROLL
      for (int kk = 0; kk < FV3_KC; ++kk) {
        const int k_ = FV3_KC * kp + kk;
        const bool live = k_ <= nz1;
        const int k = live ? k_ : nz1;
        const long b = t * g.st + k * g.sk;
        const Real *qq = qin + b;
        Real v = qq[p0];
        if (upd) {
          const Real xw = qq[pxw], xc = qq[pxc], xe = qq[pxe], ys = qq[pys], yc = qq[pyc], yn = qq[pyn];
          v = v + cra * (mvx0 * (xw - xc) - mvx1 * (xc - xe) + muy0 * (ys - yc) - muy1 * (yc - yn));
        }
        if (live) (out + b)[p0] = v;
      }
    });
    in = out;
  }
  if (in != q) {
    Real *src = in;
    launch3<4>(c, s, Box{isd, ied, jsd, jed, 0, nz1}, [=] FV3_HD(int t, int k, int i, int j) {
      const long p = t * g.st + k * g.sk + IX(i, j);
      q[p] = src[p];
    });
  }
  return fv3_post(c, s, "del2_cubed");
}

extern "C" int fv3_apply_diffusive_heating(fv3_ctx *c, const fv3_field *delp_, const fv3_field *delz_, const fv3_field *cappa_, const fv3_field *hs_,
                                           const fv3_field *pt_, double delt, void *stream) {
  if (!c) return FV3_ERR_ARG;
  FV3_FIELD(delp, delp_) FV3_FIELD(delz, delz_) FV3_FIELD(cappa, cappa_) FV3_FIELD(hs, hs_) FV3_FIELD(pt, pt_)
  const Geo g = c->g;
  const Real rdg = (Real)(-c->cst.rdgas / c->cst.grav), cv_air = (Real)(c->cst.cp_air - c->cst.rdgas), lim0 = (Real)delt;
  launch3(c, (fv3_stream_t)stream, Box{1, g.nx, 1, g.ny, 0, g.nz - 1}, [=] FV3_HD(int t, int k, int i, int j) {
    const long p = t * g.st + k * g.sk + IX(i, j);
    const Real cp = cappa[p];
    const Real pkz = fv3_exp(cp / ((Real)1.0 - cp) * fv3_log(rdg * delp[p] / delz[p] * pt[p]));
    const Real dtmp = hs[p] / (cv_air * delp[p]);
    Real lim = lim0;
    if (k == 0) lim = lim * (Real)0.1;
    if (k == 1) lim = lim * (Real)0.5;
    const Real mag = fv3_min(lim, fabs(dtmp));
    const Real sg = dtmp > (Real)0 ? (Real)1 : (dtmp < (Real)0 ? (Real)-1 : (Real)0);
    pt[p] = pt[p] + sg * mag / pkz;
  });
  return fv3_post(c, (fv3_stream_t)stream, "apply_diffusive_heating");
}

// ---------------------------------------------------------------------------------------------
// Self-test of the hand-written arithmetic / register tables of the SIM1 solvers (fv3_math.h, fv3_agpr.h; fv3_riem.hip) ON THE DEVICE (tests/test_device_math.py): the claims "fv3_div
// is bit for bit `/`", "log / exp are the host emulation's" and "every slot of the accumulation-register column holds what was put
// there" are checked directly, not only through the solvers.  x, y, out: device pointers to n doubles.
//   which 0: out = fv3_div(x, y)    1: out = fv3_log(x)    2: out = fv3_exp(x)
//   which 3: n = 80 * 64: one wave puts x[k * 64 + lane] into slot k (k = 0 .. 79; slots 4g .. 4g+3 through the group table when
//            g is odd, one by one when even), then reads the slots back in descending order into out[k * 64 + lane]
// ---------------------------------------------------------------------------------------------
#ifndef FV3_HOST_EMU
__global__ void __launch_bounds__(256) fv3_selftest_math_kernel(int which, const double *x, const double *y, double *out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = which == 0 ? fv3_div(x[i], y[i]) : which == 1 ? fv3_log(x[i]) : fv3_exp(x[i]);
}
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) fv3_selftest_agpr_kernel(const double *x, double *out) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass parses kernel bodies too; the register tables exist in the device pass only)
  const int lane = threadIdx.x;
  for (int g = 0; g < FV3_AGPR_LEVELS / 4; ++g) {
    const double v0 = x[(4 * g + 0) * 64 + lane], v1 = x[(4 * g + 1) * 64 + lane], v2 = x[(4 * g + 2) * 64 + lane], v3 = x[(4 * g + 3) * 64 + lane];
    if (g & 1) {
      fv3_agpr_set4(g, v0, v1, v2, v3);
    } else {
      fv3_agpr_set(4 * g + 0, v0);
      fv3_agpr_set(4 * g + 1, v1);
      fv3_agpr_set(4 * g + 2, v2);
      fv3_agpr_set(4 * g + 3, v3);
    }
  }
  for (int k = FV3_AGPR_LEVELS - 1; k >= 0; --k) out[k * 64 + lane] = fv3_agpr_get(k);
#else
  (void)x;
  (void)out;
#endif
}
#endif
extern "C" int fv3_selftest_math(fv3_ctx *c, int which, const double *x, const double *y, double *out, int64_t n, void *stream) {
  if (!c || !x || !out || n < 0 || which < 0 || which > 3 || (which == 0 && !y)) return FV3_ERR_ARG;
  if (which == 3 && n != (int64_t)FV3_AGPR_LEVELS * 64) return fv3_fail(c, FV3_ERR_ARG, "fv3_selftest_math(3): n must be 80 * 64");
  if (n == 0) return FV3_OK;
#ifdef FV3_HOST_EMU
  (void)stream;
  for (int64_t i = 0; i < n; ++i) out[i] = which == 0 ? fv3_div(x[i], y[i]) : which == 1 ? fv3_log(x[i]) : which == 2 ? fv3_exp(x[i]) : x[i];
  return FV3_OK;
#else
  if (which == 3)
    hipLaunchKernelGGL(fv3_selftest_agpr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, x, out);
  else
    hipLaunchKernelGGL(fv3_selftest_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, which, x, y, out, n);
  return fv3_post(c, (fv3_stream_t)stream, "selftest_math");
#endif
}

#ifdef FV3_HOST_EMU
// test hook of the host-emulation library only (tests/test_fast_math.py): the solvers' log on an array
extern "C" void fv3_hostemu_log(const double *x, double *y, long n) {
  for (long i = 0; i < n; ++i) y[i] = fv3_log(x[i]);
}
extern "C" void fv3_hostemu_exp(const double *x, double *y, long n) {
  for (long i = 0; i < n; ++i) y[i] = fv3_exp(x[i]);
}
#endif

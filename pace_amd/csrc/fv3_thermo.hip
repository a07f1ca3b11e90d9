// fv3_thermo.hip -- the thermodynamic bookends of DynamicalCore.step_dynamics: state.pt is a temperature (K) before and after a
// model step, the acoustic loop transports T_v / pkz [REF driver/pace/driver/driver.py:494-504, 639-644; SURVEY §1, §3.1].
//
//   fv3_pt_from_temperature   the preamble of fv_dynamics: T -> the loop's form, pkz of the full (non-hydrostatic) pressure
//       tv = pt * fac;  pz = exp(cappa * log(rrg * delp / delz * tv));  pkz = pz;  pt = tv / pz
//   fv3_temperature_from_pt   the last-step conversion of the remap + the omga and ps diagnoses
//       recompute_pkz == 0:  tv = pt * pkz                                                    (valid right after a remap)
//       recompute_pkz == 1:  tv = pt * exp(cappa / (1 - cappa) * log(rrg * delp / delz * pt)),  pkz = exp(cappa * log(rrg * delp / delz * tv))
//       pt = tv / fac;  omga = delp / delz * w (where given);  ps = pe[.., nz] (where given; 2-D)
//   fac = (1 + zvir * qvapor) * (1 - q_con), zvir = rvgas / rdgas - 1 (qvapor absent: zvir * qvapor = 0), rrg = -rdgas / grav.
// Every product and quotient is rounded on its own, left to right (the build has no contraction); exp / log are the calls of
// fv3_remap.hip's T_v and closing kernels, so the entries agree with the remap to the last bits in both precisions.
//
// Compute cells and levels 0 .. nz-1 of every sub-domain; no halo cell, no pad level and no input field is written.
//
// Streaming cell kernels (the family of fv3_copy / fv3_diag_pack): lanes run along i, every access of a wave is one coalesced row,
// a thread walks four levels (launch3<4>), the outputs are written once and not read back by the kernel: streaming stores.  No LDS,
// no scratch.  qvapor present / absent, recompute_pkz and omga present / absent are template parameters: every form is straight-line
// code per cell.  ps is one row copy per sub-domain plane (launch2).
#include "fv3_common.h"

namespace {

struct ThermoIn {
  const Real *delp, *delz, *q_con, *cappa, *qv;
};

// (1 + zvir * qvapor) * (1 - q_con); without qvapor the first factor is (1 + 0) = 1 and the product is (1 - q_con) exactly:
// bitwise what a qvapor field of zeros gives
template <bool QV>
FV3_HD inline Real thermo_fac(const ThermoIn &in, long p, Real zvir) {
  const Real dry = (Real)1.0 - in.q_con[p];
  if constexpr (QV) {
    const Real zq = zvir * in.qv[p];
    return ((Real)1.0 + zq) * dry;
  } else {
    (void)zvir;
    return dry;
  }
}

template <bool QV>
void thermo_fwd(fv3_ctx *c, fv3_stream_t s, Real *pt, Real *pkz, const ThermoIn in) {
  const Geo g = c->g;
  const Real rrg = (Real)(-c->cst.rdgas / c->cst.grav), zvir = (Real)(c->cst.rvgas / c->cst.rdgas - 1.0);
  launch3<4>(c, s, Box{1, g.nx, 1, g.ny, 0, g.nz - 1}, [=] FV3_HD(int t, int k, int i, int j) {
    const long p = t * g.st + k * g.sk + IX(i, j);
    const Real fac = thermo_fac<QV>(in, p, zvir);
    const Real tv = pt[p] * fac;
    const Real pz = exp(in.cappa[p] * log(rrg * in.delp[p] / in.delz[p] * tv));
    FV3_ST_NT(pkz[p], pz);
    FV3_ST_NT(pt[p], tv / pz);
  });
}

template <bool QV, bool RECOMP, bool OMGA>
void thermo_bwd(fv3_ctx *c, fv3_stream_t s, Real *pt, Real *pkz, const ThermoIn in, const Real *w, Real *omga) {
  const Geo g = c->g;
  const Real rrg = (Real)(-c->cst.rdgas / c->cst.grav), zvir = (Real)(c->cst.rvgas / c->cst.rdgas - 1.0);
  launch3<4>(c, s, Box{1, g.nx, 1, g.ny, 0, g.nz - 1}, [=] FV3_HD(int t, int k, int i, int j) {
    const long p = t * g.st + k * g.sk + IX(i, j);
    const Real fac = thermo_fac<QV>(in, p, zvir);
    const Real ptv = pt[p];
    Real tv;
    if constexpr (RECOMP) {
      const Real cp = in.cappa[p];
      const Real r = rrg * in.delp[p] / in.delz[p];
      tv = ptv * exp(cp / ((Real)1.0 - cp) * log(r * ptv));
      FV3_ST_NT(pkz[p], exp(cp * log(r * tv)));
    } else {
      tv = ptv * pkz[p];
    }
    FV3_ST_NT(pt[p], tv / fac);
    if constexpr (OMGA) FV3_ST_NT(omga[p], in.delp[p] / in.delz[p] * w[p]);
  });
}

template <bool QV, bool RECOMP>
void thermo_bwd_o(fv3_ctx *c, fv3_stream_t s, Real *pt, Real *pkz, const ThermoIn &in, const Real *w, Real *omga) {
  if (omga)
    thermo_bwd<QV, RECOMP, true>(c, s, pt, pkz, in, w, omga);
  else
    thermo_bwd<QV, RECOMP, false>(c, s, pt, pkz, in, w, omga);
}

struct Named {
  const char *name;
  const void *ptr;
};

// the written fields may alias neither each other nor a field that is read: the result would depend on the order of the cells
int thermo_alias(fv3_ctx *c, const char *op, const Named *out, int n_out, const Named *in, int n_in) {
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

extern "C" int fv3_pt_from_temperature(fv3_ctx *c, const fv3_field *pt_, const fv3_field *pkz_, const fv3_field *delp_, const fv3_field *delz_, const fv3_field *q_con_,
                                       const fv3_field *cappa_, const fv3_field *qvapor_, void *stream) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "pt_from_temperature: the context is null");
  FV3_FIELD(pt, pt_) FV3_FIELD(pkz, pkz_) FV3_FIELD(delp, delp_) FV3_FIELD(delz, delz_) FV3_FIELD(q_con, q_con_) FV3_FIELD(cappa, cappa_)
  Real *qvapor = nullptr;
  if (qvapor_) {
    qvapor = fv3_chk(c, qvapor_, "qvapor_");
    if (!qvapor) return FV3_ERR_ARG;
  }
  const Named out[] = {{"pt", pt}, {"pkz", pkz}};
  const Named in[] = {{"delp", delp}, {"delz", delz}, {"q_con", q_con}, {"cappa", cappa}, {"qvapor", qvapor}};
  if (int st = thermo_alias(c, "pt_from_temperature", out, 2, in, qvapor ? 5 : 4)) return st;
  fv3_stream_t s = (fv3_stream_t)stream;
  const ThermoIn f{delp, delz, q_con, cappa, qvapor};
  if (qvapor)
    thermo_fwd<true>(c, s, pt, pkz, f);
  else
    thermo_fwd<false>(c, s, pt, pkz, f);
  return fv3_post(c, s, "pt_from_temperature");
}

extern "C" int fv3_temperature_from_pt(fv3_ctx *c, const fv3_field *pt_, const fv3_field *pkz_, const fv3_field *delp_, const fv3_field *delz_, const fv3_field *q_con_,
                                       const fv3_field *cappa_, const fv3_field *qvapor_, const fv3_field *w_, const fv3_field *omga_, const fv3_field *pe_,
                                       const fv3_field *ps_, int recompute_pkz, void *stream) {
  if (!c) return fv3_fail(c, FV3_ERR_ARG, "temperature_from_pt: the context is null");
  FV3_FIELD(pt, pt_) FV3_FIELD(pkz, pkz_) FV3_FIELD(delp, delp_) FV3_FIELD(delz, delz_) FV3_FIELD(q_con, q_con_) FV3_FIELD(cappa, cappa_) FV3_FIELD(w, w_) FV3_FIELD(pe, pe_)
  Real *qvapor = nullptr, *omga = nullptr, *ps = nullptr;
  if (qvapor_) {
    qvapor = fv3_chk(c, qvapor_, "qvapor_");
    if (!qvapor) return FV3_ERR_ARG;
  }
  if (omga_) {
    omga = fv3_chk(c, omga_, "omga_");
    if (!omga) return FV3_ERR_ARG;
  }
  if (ps_) {
    ps = fv3_chk(c, ps_, "ps_", true);
    if (!ps) return FV3_ERR_ARG;
  }
  if (recompute_pkz != 0 && recompute_pkz != 1)
    return fv3_fail(c, FV3_ERR_ARG, "temperature_from_pt: recompute_pkz = " + std::to_string(recompute_pkz) + " (0: tv = pt * pkz, 1: pkz is rebuilt)");
  const Named out[] = {{"pt", pt}, {"pkz", pkz}, {"omga", omga}, {"ps", ps}};
  const Named in[] = {{"delp", delp}, {"delz", delz}, {"q_con", q_con}, {"cappa", cappa}, {"w", w}, {"pe", pe}, {"qvapor", qvapor}};
  if (int st = thermo_alias(c, "temperature_from_pt", out, 4, in, qvapor ? 7 : 6)) return st;
  fv3_stream_t s = (fv3_stream_t)stream;
  const ThermoIn f{delp, delz, q_con, cappa, qvapor};
  if (qvapor) {
    if (recompute_pkz)
      thermo_bwd_o<true, true>(c, s, pt, pkz, f, w, omga);
    else
      thermo_bwd_o<true, false>(c, s, pt, pkz, f, w, omga);
  } else {
    if (recompute_pkz)
      thermo_bwd_o<false, true>(c, s, pt, pkz, f, w, omga);
    else
      thermo_bwd_o<false, false>(c, s, pt, pkz, f, w, omga);
  }
  if (ps) {
    const Geo g = c->g;
    launch2(c, s, Box{1, g.nx, 1, g.ny, 0, 0}, [=] FV3_HD(int t, int i, int j) {
      const unsigned pix = IX(i, j);
      FV3_ST_NT(ps[t * g.st2 + pix], pe[t * g.st + (long)g.nz * g.sk + pix]);
    });
  }
  return fv3_post(c, s, "temperature_from_pt");
}

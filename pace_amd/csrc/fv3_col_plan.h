// fv3_col_plan.h -- the decisions of the column height chain (update_dz_c, riem_solver_c, update_dz_d, riem_solver3) in one place: which form a Riemann
// solver runs and where its gam lives, whether update_dz_d leaves its closing scan to riem_solver3, which edge_profile form serves a level count, and from
// which interface on update_dz_d's del-n chain runs inside the transport march.  Pure functions of plain numbers (level count, sizeof(Real), level stride,
// switch values, the per-interface host tables, the sequencer's hints).  Plain C++ and fv3_switch.h only (no HIP, no fv3_common.h): fv3_riem.hip and
// fv3_dz.hip include it, and so does the stand-alone program of tests/test_column_plan.py, which compares every function with literals derived by hand
// from the predicates as they stood while they were spread over the operators.
#pragma once
#include <cstddef>
#include "fv3_switch.h"

#ifndef FV3_RIEM_GL
#define FV3_RIEM_GL 0  // 1: gam arrays in a second LDS line (experiment; halves the resident waves)
#endif
#define FV3_COL_WAVE 64  // lanes of a wave = columns per LDS line group (fv3_riem.hip asserts that it is FV3_WAVE)

// ---------------------------------------------------------------------------------------------
// Riemann solvers
// ---------------------------------------------------------------------------------------------
// where the tridiagonal gam of the wave form lives: the lane's accumulation registers (fv3_agpr.h), the scratch field, a second LDS line (FV3_RIEM_GL builds)
enum RiemGam { GAM_REGS = 0, GAM_SCRATCH, GAM_LDS };
struct RiemForm {
  bool wave;  // the LDS-line wave kernels; else the thread-per-column kernels
  int gam;    // RiemGam (wave form only)
};
// levels the accumulation registers of a lane hold: 80 in fp64 (two registers per level), 128 in fp32 (fv3_agpr.h; fv3_riem.hip asserts the two agree)
inline int riem_kreg_levels(size_t real_bytes) { return real_bytes == 8 ? 80 : 128; }

// mode: FV3_RIEM_MODE (0 default, 1 columns, 2 wave); regs_on: FV3_RIEM_REGS; sk: elements between two levels of a field; heavy: riem_solver3
inline RiemForm riem_form(int nz, size_t real_bytes, long sk, bool heavy, int mode, bool regs_on) {
  const bool gl = FV3_RIEM_GL != 0;
  // LDS line budget of the wave solver; above it (very deep columns) the callers fall back to the column kernels
  const size_t line = (size_t)nz * FV3_COL_WAVE * real_bytes * (gl ? 2 : 1);
  bool wave = line <= (size_t)(gl ? 160 : 64) * 1024 && nz >= 3;
  if (mode == 1) wave = false;
  // heavy = riem_solver3 (7 exp/log per level): below 4 waves per CU (line > 40 KB: 127 levels in fp64) the
  // bandwidth-bound column form is faster (25.7 vs 29.1 ms at C768 L127 fp64); riem_solver_c still gains (24.7 vs 29.2)
  if (heavy && mode != 2 && line > 40 * 1024) wave = false;
  if ((nz + 2) * sk * (long)real_bytes >= (1L << 32)) wave = false;  // (KW_: 32-bit byte offsets inside a sub-domain's field)
  // gam in the accumulation registers (level k sits in slot k + 1); FV3_RIEM_REGS=0: through the scratch field (A/B, same values).
  // (A first attempt let the COMPILER index a register-tuple array: riem_solver_c 9.64 -> 13.84 ms -- DESIGN §7.)
  const int gam = gl ? GAM_LDS : regs_on && nz < riem_kreg_levels(real_bytes) ? GAM_REGS : GAM_SCRATCH;
  return RiemForm{wave, gam};
}

// THE predicate of the hand-off of update_dz_d's closing scan: update_dz_d decides with it, riem_solver3 verifies with it when it finds the marched heights
// waiting.  seq_dz_scan: fv3_seq_hints::dz_scan; heavy: riem_solver3's form on this context; separate: FV3_DZ_SCAN=separate.  (The pre-sweep exists in the
// register forms of the wave kernel only.)
inline bool dz_scan_defers(bool seq_dz_scan, RiemForm heavy, bool separate) { return seq_dz_scan && heavy.wave && heavy.gam == GAM_REGS && !separate; }

// the waves [w_lo, w_hi) one call solves: all nwave of them, the nwave_frame that hold frame columns (frame pass 1), or the rest (pass 2)
inline void riem_wave_range(int nwave, int nwave_frame, int frame_pass, int &w_lo, int &w_hi) {
  w_lo = frame_pass == 2 ? nwave_frame : 0;
  w_hi = frame_pass == 1 ? nwave_frame : nwave;
}

// What one call of a solver does.  Built by riem_plan() (fv3_riem.hip), the only function there that asks the switch table.
struct RiemPlan {
  RiemForm form;
  bool last;        // riem_solver3: the last sub-step also stores pe / peln / pk
  bool pre;         // riem_solver3: update_dz_d left its closing scan to this call's pre-sweep
  bool store_delz;  // riem_solver3: the layer thickness is stored (inside the sequencer only by the last sub-step of a call; FV3_SEQ_DELZ=every: A/B)
  int w_lo, w_hi;   // wave form: the waves of this (frame) pass
};

// ---------------------------------------------------------------------------------------------
// update_dz_d
// ---------------------------------------------------------------------------------------------
// edge_profile: generic thread-per-column form (two kernels) | the column in registers, three divisions per level (nz 8, 79, 127) | wave form with the
// column in registers (nz 79, 127) | wave form with the level count at run time (the column in the lane's LDS line)
enum EpForm { EP_GENERIC = 0, EP_REG, EP_WAVE_NZ, EP_WAVE_RT };
struct EpPlan {
  int form;
  int n_lines;           // FV3_DEBUG_FD: "[update_dz_d] edge_profile: <line>" for each
  const char *lines[2];
  bool one_launch;       // wave forms: the four solves as one launch (FV3_EP_ONE_LAUNCH; set by dzd_plan)
};
// generic / reg / lds: FV3_EDGE_PROFILE_GENERIC / _REG / _LDS
inline EpPlan ep_form(int nz, size_t real_bytes, bool generic, bool reg, bool lds) {
  EpPlan p{EP_GENERIC, 0, {nullptr, nullptr}, false};
  auto say = [&](const char *line) { p.lines[p.n_lines++] = line; };
  if (generic) {
    say("generic thread-per-column form");
    return p;
  }
  if (!reg && nz >= 2) {
    const bool own = (nz == 79 || nz == 127) && !lds;  // the level counts with an instantiation of their own
    if (own) {
      say(nz == 79 ? "wave form, 79 levels" : "wave form, 127 levels");
      p.form = EP_WAVE_NZ;
      return p;
    }
    if (real_bytes * nz * FV3_COL_WAVE <= 64 * 1024) {
      say("wave form, level count at run time");
      p.form = EP_WAVE_RT;
      return p;
    }
    say("no wave form");  // (the LDS line of a column this deep does not fit: the thread-per-column forms below)
  }
  const bool inst = nz == 79 || nz == 127 || nz == 8;  // (8: exercised by the parity tests)
  say(inst ? "register-resident column form" : "generic thread-per-column form");
  p.form = inst ? EP_REG : EP_GENERIC;
  return p;
}

// Interfaces from fd_k0 on (chain of order 2 and switched on: all but the sponge layers) run the del-n chain INSIDE the transport march; nz + 1: none
// (off: dzd_chain_off).  The interfaces without it -- the sponge layers -- go to the auxiliary stream beside the march of the others when there are some
// of both and such a stream exists (aux).
struct DzdLevels {
  int fd_k0;
  bool fork;
};
// FV3_DZ_DELN=arrays, FV3_TP2D_MODE=staged, FV3_DEL6_MODE=staged: each keeps the chain of every interface out of the march
inline bool dzd_chain_off(bool deln_arrays, bool tp2d_staged, bool del6_staged) { return deln_arrays || tp2d_staged || del6_staged; }
inline DzdLevels dzd_levels(int nz, const int *nord_v_h, const double *damp_vt_h, bool off, bool aux) {
  int fd_k0 = nz + 1;
  if (!off)
    for (int k = nz; k >= 0; --k) {
      if (!(nord_v_h[k] == 2 && damp_vt_h[k] > 1.0e-5)) break;
      fd_k0 = k;
    }
  return DzdLevels{fd_k0, fd_k0 > 0 && fd_k0 <= nz && aux};
}

// What one call of update_dz_d does.  Built by dzd_plan() (fv3_dz.hip), the only function there that asks the switch table.
struct DzdPlan {
  EpPlan ep;
  bool coef_scaled;  // the del-n coefficient table: d_sw's scaled one (FV3_ALT=dz_damp_scaled) instead of the raw column value
  int nord_max;      // highest del-n order over the interfaces
  DzdLevels lev;
  bool defer;        // the closing scan is left to riem_solver3's pre-sweep (dz_scan_defers): the marched heights then go to the slot riem_solver3 leaves free
  bool debug;        // FV3_DEBUG_FD
};

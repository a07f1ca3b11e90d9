// fv3_switch.h -- the kernel-form switches of the library: the ONLY place that reads the environment.
//
// The library keeps alternative forms of its kernels (the A/B twins that let one form check another, and a few tuning
// numbers) and chooses between them through FV3_* environment variables.  Every such variable is one row of the table
// below; operator code asks fv3_sw() / fv3_sw_is() / fv3_alt() and never calls getenv itself.  A new experiment adds a row.
//
// Plain C++ and the standard library only (no HIP, no fv3_common.h): a stand-alone host program can include this header
// (tests/test_switches.py does).  INTEGRATION.md §2 lists the same rows in the same order.
#pragma once
#include <atomic>
#include <cstdlib>
#include <cstring>

// Read policy.  ONCE: read at the first query and kept for the process.  LIVE: read again at every query (the parity tests flip
// these between two calls of one process; an operator queries them once per call, or where it sets a context field).
#define FV3_SW_ONCE true
#define FV3_SW_LIVE false

// Kind = how the value is parsed; fv3_sw() returns:
//   present   1 when the variable is set at all (empty and "0" included), else 0
//   off_if_0  0 when the value starts with '0', else 1 (unset: 1)
//   on_if_1   1 when the value starts with '1', else 0 (unset: 0)
//   tri       -1 unset, 0 / 1 when the value starts with '0' / '1', 2 set to anything else
//   word      i >= 1 when the value IS the i-th of the row's '|'-separated words, else 0 (unset, unknown: the default form); ask with fv3_sw_is()
//   integer   atoi of the value; the row's default when unset
//   names     comma-separated list of names, asked with fv3_alt(name); fv3_sw() says whether the variable is set
// Unknown values are silent.
enum fv3_sw_kind { FV3_SW_present, FV3_SW_off_if_0, FV3_SW_on_if_1, FV3_SW_tri, FV3_SW_word, FV3_SW_integer, FV3_SW_names };

// X(identifier, environment name, read policy, kind, words, integer default, what it selects) -- ONE ROW PER LINE (tests/test_switches.py parses them)
// clang-format off
#define FV3_SWITCH_TABLE(X) \
  X(SEG, "FV3_SEG", LIVE, integer, "", 0, "rows a marching wave owns; unset or <= 0 (default): automatic, 96 where that still fills the chip eight times over, else 64") \
  X(GRID_SPLIT, "FV3_GRID_SPLIT", ONCE, off_if_0, "", 0, "0: whole planes per XCD also for launches of few planes; default: such launches map sub-planes to the XCDs") \
  X(FRAME_LAUNCH, "FV3_FRAME_LAUNCH", ONCE, word, "split", 0, "split: one launch per boundary window; default: the four windows of a frame in one launch") \
  X(Q4_KB, "FV3_Q4_KB", ONCE, integer, "", 16, "levels of one tile an XCD walks back to back in the transport marches (level-major launches; default 16); 0: plane-major launches") \
  X(KE_KB, "FV3_KE_KB", ONCE, integer, "", 16, "the same for the corner-KE, divergence-damping and fused wind-stage marches (default 16); 0: plane-major launches") \
  X(GATHER_BATCH, "FV3_GATHER_BATCH", ONCE, off_if_0, "", 0, "0: one launch per halo gather; default: up to twelve gathers per launch") \
  X(AUX_STREAM, "FV3_AUX_STREAM", LIVE, off_if_0, "", 0, "0: everything in program order on the caller's stream; default: small launches on an auxiliary stream beside the marches (read when a context is created)") \
  X(ALT, "FV3_ALT", LIVE, names, "", 0, "named alternatives of the uncertain restatements (DESIGN section 2; the oracle reads the same variable), e.g. dz_damp_scaled,heat_dt_full; default: none") \
  X(DEBUG_FD, "FV3_DEBUG_FD", LIVE, present, "", 0, "set: the operators report on stderr which forms and level ranges they chose; default: silent") \
  X(DEBUG_DEL2, "FV3_DEBUG_DEL2", LIVE, present, "", 0, "set: the fused del2_cubed + heating reports its calls on stderr; default: silent") \
  X(TP2D_MODE, "FV3_TP2D_MODE", ONCE, word, "staged", 0, "staged: fv_tp_2d as one launch per stage (reference path, no auxiliary stream); default: the marching kernels") \
  X(DEL6_MODE, "FV3_DEL6_MODE", ONCE, word, "staged", 0, "staged: the del-n damping fluxes as one launch per stage (reference path); default: the streaming kernel") \
  X(TP2D_MARCH, "FV3_TP2D_MARCH", LIVE, word, "old", 0, "old: the round-4 single-tracer march with the del-n chain inside; default: the round-5 march that serves every tile") \
  X(TP2D_FA, "FV3_TP2D_FA", ONCE, off_if_0, "", 0, "0: the general form of the single-tracer marches with the chain inside; default: the form that takes 'order 2, on at every level' as a constant") \
  X(HORD_CONST, "FV3_HORD_CONST", ONCE, tri, "", 0, "0: PPM order at run time in every march; 1: as a constant (6) also in the two-tracer marches; default: constant in the single-tracer and wind-stage marches only") \
  X(CSW_B_GENERIC, "FV3_CSW_B_GENERIC", LIVE, present, "", 0, "set: c_sw computes every point with the generic per-point stage kernels; default: interior kernels + boundary windows") \
  X(CSW_MARCH, "FV3_CSW_MARCH", LIVE, word, "0|abc", 0, "0: c_sw's round-1 stage kernels; abc: stages A - C as a march, D and E as stage kernels; default: the whole interior as one march") \
  X(CSW_WIN_KC, "FV3_CSW_WIN_KC", ONCE, integer, "", 2, "levels one thread of c_sw's boundary-window kernels walks beside the interior march (default 2)") \
  X(CSW_WIN_OVERLAP, "FV3_CSW_WIN_OVERLAP", ONCE, off_if_0, "", 0, "0: c_sw's stage A / B windows in program order; default: on the auxiliary stream beside the march") \
  X(CSW_DEFER, "FV3_CSW_DEFER", ONCE, on_if_1, "", 0, "1: the sequencer joins c_sw's stage D / E windows only before riem_solver_c; default: c_sw waits for them") \
  X(SEQ_UAVA, "FV3_SEQ_UAVA", LIVE, word, "every", 0, "every: c_sw stores ua / va in full in every sub-step of the sequencer; default: only where a later operator reads them") \
  X(FXADV_FULL_UT, "FV3_FXADV_FULL_UT", ONCE, present, "", 0, "set: fxadv stores ut / vt everywhere inside d_sw too; default: only within 4 cells of a cube-tile edge") \
  X(DSW_SCALARS, "FV3_DSW_SCALARS", LIVE, word, "separate|quad", 0, "separate: d_sw's four scalar transports as four launches + the division kernel; quad: one four-tracer wave; default: two two-tracer marches") \
  X(DSW_DELN, "FV3_DSW_DELN", LIVE, word, "arrays", 0, "arrays: the scalars' del-n fluxes of every level from staged launches; default: the chains inside the marches above the sponge layers") \
  X(DSW_MARCH, "FV3_DSW_MARCH", LIVE, word, "old|coupled", 0, "old: the round-4 two-tracer marches; coupled: the two roles as coupled wave pairs; default: the round-5 march, one launch per role") \
  X(DSW_SPONGE_SERIAL, "FV3_DSW_SPONGE_SERIAL", ONCE, on_if_1, "", 0, "1: the sponge levels' scalar marches in program order; default: on the auxiliary stream beside the other levels") \
  X(DSW_HEAT, "FV3_DSW_HEAT", LIVE, word, "separate", 0, "separate: the damping heat in its own kernel; default: as the epilogue of the vorticity march") \
  X(DSW_VORT_DELN, "FV3_DSW_VORT_DELN", LIVE, word, "arrays", 0, "arrays: the vorticity's del-n fluxes of every level from staged launches; default: the chain inside the vorticity march") \
  X(DSW_VORT_IN_KE, "FV3_DSW_VORT_IN_KE", LIVE, on_if_1, "", 0, "1: the corner-KE march also forms the cell vorticity under its corners; default: the vorticity kernel forms all of it") \
  X(DSW_WINDSTAGE, "FV3_DSW_WINDSTAGE", LIVE, word, "staged", 0, "staged: every level of d_sw's wind stage through the staged kernels; default: the fused wind-stage march above the sponge layers") \
  X(KE_STAGED, "FV3_KE_STAGED", ONCE, present, "", 0, "set: the corner kinetic energy as stage kernels (profiling; switches the fused wind stage off); default: the marching kernel") \
  X(DIVDAMP_STAGED, "FV3_DIVDAMP_STAGED", ONCE, present, "", 0, "set: the divergence damping as one launch per iteration (profiling; switches the fused wind stage off); default: the marching iteration") \
  X(DSW_SPONGE_WIND, "FV3_DSW_SPONGE_WIND", LIVE, word, "serial", 0, "serial: the sponge levels' wind chain in program order; default: on the auxiliary stream beside the fused wind stage") \
  X(DSW_SIDE, "FV3_DSW_SIDE", LIVE, word, "copy", 0, "copy: separate copies of the winds on the segment / strip boundaries for the damping heat; default: the wind stage stores them") \
  X(DSW_WIND_OVERLAP, "FV3_DSW_WIND_OVERLAP", ONCE, on_if_1, "", 0, "1: d_sw's wind branch on the auxiliary stream beside the scalar marches; default: in program order behind them") \
  X(RIEM_MODE, "FV3_RIEM_MODE", ONCE, word, "columns|wave", 0, "columns: thread-per-column Riemann solvers; wave: the LDS-line wave form also for deep columns; default: wave form unless riem_solver3's line exceeds 40 KB") \
  X(RIEM_REGS, "FV3_RIEM_REGS", ONCE, off_if_0, "", 0, "0: the wave solvers' gam through the scratch field; default: in the accumulation registers") \
  X(SEQ_DELZ, "FV3_SEQ_DELZ", LIVE, word, "every", 0, "every: riem_solver3 stores delz in every sub-step of the sequencer; default: only in the last one of a call") \
  X(NH_PGF, "FV3_NH_PGF", LIVE, word, "staged", 0, "staged: nh_p_grad as four a2b_ord4 launches + the level-walking update; default: one marching kernel") \
  X(EP_ONE_LAUNCH, "FV3_EP_ONE_LAUNCH", ONCE, off_if_0, "", 0, "0: edge_profile's four solves as four launches; default: one launch") \
  X(EDGE_PROFILE_GENERIC, "FV3_EDGE_PROFILE_GENERIC", ONCE, present, "", 0, "set: edge_profile's generic thread-per-column form; default: the wave forms") \
  X(EDGE_PROFILE_REG, "FV3_EDGE_PROFILE_REG", ONCE, present, "", 0, "set: edge_profile's register-resident column form; default: the wave forms") \
  X(EDGE_PROFILE_LDS, "FV3_EDGE_PROFILE_LDS", ONCE, present, "", 0, "set: edge_profile's wave form with the level count at run time also for 79 / 127 levels; default: their own instantiations") \
  X(DZ_DELN, "FV3_DZ_DELN", LIVE, word, "arrays", 0, "arrays: update_dz_d's del-n fluxes of every interface from one staged launch; default: the chain inside the transport march") \
  X(DZ_SCAN, "FV3_DZ_SCAN", LIVE, word, "separate", 0, "separate: update_dz_d's closing scan as its own kernel also inside the sequencer; default: left to riem_solver3's pre-sweep there") \
  X(DEL2_FUSED, "FV3_DEL2_FUSED", LIVE, off_if_0, "", 0, "0: del2_cubed and the diffusive heating as the two staged operators; default: one fused pass") \
  X(DEL2_HEAT, "FV3_DEL2_HEAT", LIVE, word, "fused", 0, "fused: the heating as the epilogue of the third del2 iteration; default: its own launch on the smoothed field") \
  X(FRAME_FIRST, "FV3_FRAME_FIRST", LIVE, tri, "", 0, "1: operators that feed a halo update compute the frame first; set to anything else: never; default: only with a message transport") \
  X(ACC_STORE, "FV3_ACC_STORE", LIVE, off_if_0, "", 0, "0: flux accumulators zeroed, then read-modify-write in every sub-step; default: the first sub-step of a call stores") \
  X(ACC_DEFER, "FV3_ACC_DEFER", LIVE, off_if_0, "", 0, "0: cx / cy read-modify-write in every sub-step; default: summed once per call (read when a context first allocates the slots)") \
  X(PINGPONG, "FV3_PINGPONG", LIVE, off_if_0, "", 0, "0: d_sw copies its new scalars back in place; default: the sequencer alternates two buffer sets (read when a context first allocates them)") \
  X(GZ_FIRST, "FV3_GZ_FIRST", LIVE, word, "copy", 0, "copy: the reference's order at the start of a call (gz filled, copied to zh, updated in place); default: heights straight into zh") \
  X(SEQ_KEEP_DIVGD, "FV3_SEQ_KEEP_DIVGD", LIVE, present, "", 0, "set: d_sw leaves the iterated divergence in divgd inside the sequencer; default: not stored there (nothing reads it)")
// clang-format on

#define FV3_SW_ENUM_(id, env, policy, kind, words, dflt, what) FV3SW_##id,
enum fv3_sw_id { FV3_SWITCH_TABLE(FV3_SW_ENUM_) FV3SW_COUNT };
#undef FV3_SW_ENUM_

struct fv3_sw_row {
  const char *env;
  bool once;
  fv3_sw_kind kind;
  const char *words;
  int dflt;
  const char *what;
};
#define FV3_SW_ROW_(id, env, policy, kind, words, dflt, what) {env, FV3_SW_##policy, FV3_SW_##kind, words, dflt, what},
inline constexpr fv3_sw_row fv3_sw_rows[FV3SW_COUNT] = {FV3_SWITCH_TABLE(FV3_SW_ROW_)};
#undef FV3_SW_ROW_

// 1-based position of w among the '|'-separated words, 0 when it is none of them
inline int fv3_sw_word(const char *words, const char *w) {
  const size_t n = strlen(w);
  int i = 1;
  for (const char *p = words; *p; ++i) {
    const char *q = strchr(p, '|');
    const size_t len = q ? (size_t)(q - p) : strlen(p);
    if (len == n && !strncmp(p, w, n)) return i;
    p += len + (q ? 1 : 0);
  }
  return 0;
}

// the value v of row r (v == nullptr: unset), by the row's kind
inline int fv3_sw_parse(const fv3_sw_row &r, const char *v) {
  switch (r.kind) {
    case FV3_SW_present:
    case FV3_SW_names: return v != nullptr;
    case FV3_SW_off_if_0: return !(v && v[0] == '0');
    case FV3_SW_on_if_1: return v && v[0] == '1';
    case FV3_SW_tri: return !v ? -1 : v[0] == '0' ? 0 : v[0] == '1' ? 1 : 2;
    case FV3_SW_word: return v ? fv3_sw_word(r.words, v) : 0;
    case FV3_SW_integer: return v ? atoi(v) : r.dflt;
  }
  return 0;
}

// ONCE rows: 0 = not read yet, else bit 32 and the value in the low word.  The first reader's answer stays (as with a function-local static).
inline std::atomic<long long> fv3_sw_cache[FV3SW_COUNT];

inline int fv3_sw(fv3_sw_id id) {
  const fv3_sw_row &r = fv3_sw_rows[id];
  if (!r.once) return fv3_sw_parse(r, getenv(r.env));
  long long seen = fv3_sw_cache[id].load(std::memory_order_acquire);
  if (!seen) {
    const long long mine = (1LL << 32) | (long long)(unsigned)fv3_sw_parse(r, getenv(r.env));
    if (fv3_sw_cache[id].compare_exchange_strong(seen, mine)) seen = mine;
  }
  return (int)(unsigned)(seen & 0xffffffffLL);
}

// word rows: is the switch set to this one of its words?  (a word the row does not list is never selected)
inline bool fv3_sw_is(fv3_sw_id id, const char *word) {
  const int w = fv3_sw_word(fv3_sw_rows[id].words, word);
  return w > 0 && fv3_sw(id) == w;
}

// FV3_ALT="name[,name...]": the named alternatives of the restatements DESIGN §2 lists as uncertain -- the same variable and names the
// oracle reads (oracle/fv3_oracle/util.py: alt), so that one run against reference savepoints can try them.  Read per call.
inline bool fv3_alt(const char *name) {
  const char *e = getenv(fv3_sw_rows[FV3SW_ALT].env);
  if (!e) return false;
  const size_t n = strlen(name);
  for (const char *p = e; (p = strstr(p, name)) != nullptr; p += n)
    if ((p == e || p[-1] == ',' || p[-1] == ' ') && (p[n] == 0 || p[n] == ',' || p[n] == ' ')) return true;
  return false;
}

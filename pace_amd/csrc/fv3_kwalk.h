// fv3_kwalk.h -- how the column kernels of fv3_riem.hip, fv3_dz.hip and fv3_nh.hip walk the levels of a column: the two addressing forms (K_, KW_), the
// prefetching level walk (k_walk, KWALK) and the one expression of the height scans (fv3_dz_floor).
#pragma once
#include "fv3_common.h"

// column access: uniform (sub-domain, level) base + 32-bit in-plane offset
#define K_(arr, k) ((arr) + tb + (long)(k)*g.sk)[pix]

// The bottom-up scans of the interface heights (update_dz_c's, update_dz_d's closing scan and the pre-sweep of riem_solver3 that stands in for it):
// interface k stays dz_min above the limited interface k + 1.
FV3_HD inline Real fv3_dz_floor(Real z, Real below, Real dz_min) { return fv3_max(z, below + dz_min); }

namespace {

template <int N>
struct KRec {
  Real v[N];
};

template <int N, int U, bool UP, class Load, class Body>
FV3_HD inline void k_walk(int nz, Load load, Body body) {
  KRec<N> buf[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int kk = u < nz ? u : nz - 1;
    buf[u] = load(UP ? kk : nz - 1 - kk);
  }
  for (int c = 0; c < nz; c += U) {
    KRec<N> nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int kk = c + U + u;
      kk = kk < nz ? kk : nz - 1;
      nxt[u] = load(UP ? kk : nz - 1 - kk);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c + u < nz) body(UP ? c + u : nz - 1 - (c + u), buf[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) buf[u] = nxt[u];
  }
}

}  // namespace

// k_walk as a statement macro: the body (the trailing block, which sees the level K and the record r) is expanded INSIDE the function
// that owns the register arrays -- a lambda that captures them by reference sends them to scratch memory (the element store turns into a
// scalar store through a pointer before the closure is dissolved, and nothing promotes the array afterwards).  `load` may be a lambda:
// it touches no register array.
#define KWALK(N, U, UP, load, ...) KWALK_E(N, U, UP, load, , __VA_ARGS__)
// ... with a statement EPI that runs after the U bodies of a loop iteration (sees c_: the first level index of the group)
#define KWALK_E(N, U, UP, load, EPI, ...)                                    \
  {                                                                          \
    KRec<N> buf_[U];                                                         \
    _Pragma("unroll") for (int u_ = 0; u_ < U; ++u_) {                       \
      const int kk_ = u_ < nz ? u_ : nz - 1;                                 \
      buf_[u_] = load(UP ? kk_ : nz - 1 - kk_);                              \
    }                                                                        \
    for (int c_ = 0; c_ < nz; c_ += U) {                                     \
      KRec<N> nxt_[U];                                                       \
      _Pragma("unroll") for (int u_ = 0; u_ < U; ++u_) {                     \
        int kk_ = c_ + U + u_;                                               \
        kk_ = kk_ < nz ? kk_ : nz - 1;                                       \
        nxt_[u_] = load(UP ? kk_ : nz - 1 - kk_);                            \
      }                                                                      \
      _Pragma("unroll") for (int u_ = 0; u_ < U; ++u_) if (c_ + u_ < nz) {   \
        const int K = UP ? c_ + u_ : nz - 1 - (c_ + u_);                     \
        const KRec<N> &r = buf_[u_];                                         \
        __VA_ARGS__                                                          \
      }                                                                      \
      EPI;                                                                   \
      _Pragma("unroll") for (int u_ = 0; u_ < U; ++u_) buf_[u_] = nxt_[u_];  \
    }                                                                        \
  }

// Scalar-base addressing: a wave-uniform 64-bit base (the field of the sub-domain) + a 32-bit BYTE offset per lane that carries the level too.
// With the plain `(arr + tb + k * sk)[pix]` the compiler forms a 64-bit address per access with a vector instruction (it cannot prove that
// pix * 8 fits 32 bits, and `global_load v, v_off, s[base]` is only selected when the zero-extension of the offset is in the same basic
// block as the access: a loop-invariant offset never is); here the offset changes with the level, so one 32-bit add per level serves every
// field of that level.  riem_form() (fv3_col_plan.h) checks that a sub-domain's field stays below 4 GB.  -DFV3_RIEM_ADDR64: the plain form (A/B).
#ifdef FV3_RIEM_ADDR64
#define KW_(arr, k) ((arr) + tb + (long)(k)*sk)[pix]
#else
#define KW_(arr, k) (*fv3_at((arr) + tb, pix * (unsigned)sizeof(Real) + (unsigned)(k) * (unsigned)(sk * (long)sizeof(Real))))
#endif
#ifndef FV3_RIEM_U
#define FV3_RIEM_U 4   // levels in flight in the sweeps with 4-5 inputs
#endif
#ifndef FV3_RIEM_U1
#define FV3_RIEM_U1 8  // ... in the sweeps with 1-2 inputs
#endif

// fv3_diag.hip -- driver diagnostics: what leaves the device when the driver stores its state.
//
//   fv3_diag_pack             the compute box (1..ni, 1..nj) of levels k0 .. k0+nk-1 of every sub-domain of a field, packed into a
//                             contiguous out[t][k][j][i] (i fastest) -- whole fields (nk = nz or nz+1), level slices (nk = 1) and 2-D
//                             fields (k0 = 0, nk = 1).  ni is nx or nx+1, nj is ny or ny+1: the staggered end belongs to the variable.
//   fv3_diag_column_integral  out[t][j][i] = rgrav * sum_k q * delp on the compute cells (the reference driver's
//                             column_integrated_<tracer>: RGRAV * np.sum(q * delp, axis=2), kg/m^2).
//
// Neither reads a halo cell or the pad level (what a host copy of the padded storage moves and then throws away: 2.35 GB per field at
// C768 L79), neither allocates: the caller owns `out`.
//
// Memory-bound copies: lanes run along i, a wavefront reads one row of the box (512 B of fp64 per 64 lanes, starting nh elements into the
// padded row) and writes 64 consecutive elements of the packed array; the packed row of ni elements is contiguous with the next one, so the
// stores of a workgroup (4 rows) form one contiguous run.  The output is not read back by any kernel: streaming stores.
#include "fv3_common.h"

extern "C" int fv3_diag_pack(fv3_ctx *c, const fv3_field *src_, int ni, int nj, int k0, int nk, void *out_, long out_elems, void *stream) {
  const bool two_d = src_ && src_->shape[2] == 1;
  Real *src = fv3_chk(c, src_, "src", two_d);
  if (!src) return FV3_ERR_ARG;
  const Geo g = c->g;
  if (!out_) return fv3_fail(c, FV3_ERR_ARG, "diag_pack: out is null");
  if ((ni != g.nx && ni != g.nx + 1) || (nj != g.ny && nj != g.ny + 1))
    return fv3_fail(c, FV3_ERR_ARG, "diag_pack: ni must be nx or nx+1 and nj must be ny or ny+1 (got ni = " + std::to_string(ni) + ", nj = " + std::to_string(nj) +
                                        " for nx = " + std::to_string(g.nx) + ", ny = " + std::to_string(g.ny) + ")");
  const int ktop = two_d ? 1 : g.nz + 1;  // (levels 0 .. nz of a 3-D field: the interface fields use the last one)
  if (k0 < 0 || nk < 1 || (long)k0 + nk > ktop)
    return fv3_fail(c, FV3_ERR_ARG, "diag_pack: level range k0 = " + std::to_string(k0) + ", nk = " + std::to_string(nk) + " outside the field's " + std::to_string(ktop) + " level(s)");
  const long want = (long)g.nsub * nk * nj * ni;
  if (out_elems != want)
    return fv3_fail(c, FV3_ERR_ARG, "diag_pack: out_elems = " + std::to_string(out_elems) + ", the packed box has n_sub * nk * nj * ni = " + std::to_string(want) + " elements");
  Real *out = (Real *)out_;
  const long st = two_d ? g.st2 : g.st, sk = two_d ? 0 : g.sk;
  const long pj = ni, pk = (long)ni * nj, pt = pk * nk;
  launch3<4>(c, (fv3_stream_t)stream, Box{1, ni, 1, nj, k0, k0 + nk - 1}, [=] FV3_HD(int t, int k, int i, int j) {
    FV3_ST_NT(out[t * pt + (k - k0) * pk + (j - 1) * pj + (i - 1)], src[t * st + k * sk + IX(i, j)]);
  });
  return fv3_post(c, (fv3_stream_t)stream, "diag_pack");
}

extern "C" int fv3_diag_column_integral(fv3_ctx *c, const fv3_field *q_, const fv3_field *delp_, void *out_, long out_elems, void *stream) {
  FV3_FIELD(q, q_) FV3_FIELD(delp, delp_)
  const Geo g = c->g;
  if (!out_) return fv3_fail(c, FV3_ERR_ARG, "diag_column_integral: out is null");
  const long want = (long)g.nsub * g.ny * g.nx;
  if (out_elems != want)
    return fv3_fail(c, FV3_ERR_ARG, "diag_column_integral: out_elems = " + std::to_string(out_elems) + ", the compute cells are n_sub * ny * nx = " + std::to_string(want));
  Real *out = (Real *)out_;
  const Real rgrav = (Real)(1.0 / c->cst.grav);
  // one thread per column, the levels in a loop: products rounded, then added in increasing k (the build has no contraction), the
  // finished sum scaled once -- the result is fixed bitwise
  launch2(c, (fv3_stream_t)stream, Box{1, g.nx, 1, g.ny, 0, 0}, [=] FV3_HD(int t, int i, int j) {
    const Real *qk = q + t * g.st + IX(i, j), *dk = delp + t * g.st + IX(i, j);
    Real s = (Real)0;
    for (int k = 0; k < g.nz; ++k, qk += g.sk, dk += g.sk) {
      const Real p = qk[0] * dk[0];
      s = s + p;
    }
    FV3_ST_NT(out[((long)t * g.ny + (j - 1)) * g.nx + (i - 1)], s * rgrav);
  });
  return fv3_post(c, (fv3_stream_t)stream, "diag_column_integral");
}

// fv3_box.h -- index boxes, the frame of four boundary windows and the tile-edge flags of a sub-domain.  Plain C++ (no HIP): fv3_common.h includes
// it, and so do the stand-alone programs that check an operator's window geometry on the host (tests/test_c_sw_plan.py).
#pragma once

#define FV3_W 1
#define FV3_E 2
#define FV3_S 4
#define FV3_N 8

struct Box {
  int i0, i1, j0, j1, k0, k1;  // inclusive; i, j Fortran-local; k 0-based
};

// the windows along a sub-domain's W / E / S / N boundary (launch_frame, fv3_common.h); k runs over the range of w[0]
struct Frame {
  Box w[4];
};

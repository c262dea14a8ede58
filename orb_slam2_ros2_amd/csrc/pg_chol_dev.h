// pg_chol_dev.h -- the 6x6 block arithmetic of the pose graph's block-sparse Cholesky (k_pgsparse.hip), shared with the host: the
// stand-alone program tests/cpp/test_pg_symbolic.cpp runs a whole factorisation over the symbolic structure with these lines.  Rules
// F2 .. F4 of DESIGN 4.26.  fp64, contraction off; every loop has constant bounds and is unrolled: no array here is indexed at run time.
// A block is 36 doubles, row-major.
#pragma once
#include "se3_dev.h"

namespace orbfe {

// F2: the Cholesky factor of a 6x6 block in place, lower triangle (the entries above the diagonal are left as they are and never
// read).  false where a pivot is not positive and finite; the block is then partly overwritten.
ORBFE_HD inline bool pg_chol6(double* Lk) {
  ORBFE_FP_STRICT
  bool good = true;
  ORBFE_UNROLL
  for (int j = 0; j < 6; ++j) {
    double d = Lk[7 * j];
    ORBFE_UNROLL
    for (int k = 0; k < j; ++k) d -= Lk[6 * j + k] * Lk[6 * j + k];
    good = good && d > 0 && isfinite(d);
    d = sqrt(d);
    Lk[7 * j] = d;
    ORBFE_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      double v = Lk[6 * i + j];
      ORBFE_UNROLL
      for (int k = 0; k < j; ++k) v -= Lk[6 * i + k] * Lk[6 * j + k];
      Lk[6 * i + j] = v / d;
    }
  }
  return good;
}

// F3: one row (6 entries, stride 1) of a block below the diagonal, or the right-hand side of the column's own block row:
// out = in * Lk^-T, entry by entry from the left
ORBFE_HD inline void pg_row_solve6(const double* Lk, const double* in, double* out) {
  ORBFE_FP_STRICT
  double v[6];
  ORBFE_UNROLL
  for (int c = 0; c < 6; ++c) {
    double s = in[c];
    ORBFE_UNROLL
    for (int m = 0; m < c; ++m) s -= v[m] * Lk[6 * c + m];
    v[c] = s / Lk[7 * c];
  }
  ORBFE_UNROLL
  for (int c = 0; c < 6; ++c) out[c] = v[c];
}

// F4: what one entry of a rank-6 update subtracts: the products of two rows of 6 added from the left
ORBFE_HD inline double pg_dot6(const double* a, const double* b) {
  ORBFE_FP_STRICT
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}

// F6: the column's own block of the backward substitution, x = Lk^-T v in place, from the bottom
ORBFE_HD inline void pg_back6(const double* Lk, double* v) {
  ORBFE_FP_STRICT
  ORBFE_UNROLL
  for (int a = 5; a >= 0; --a) {
    double s = v[a];
    ORBFE_UNROLL
    for (int m = a + 1; m < 6; ++m) s -= Lk[6 * m + a] * v[m];
    v[a] = s / Lk[7 * a];
  }
}

}  // namespace orbfe

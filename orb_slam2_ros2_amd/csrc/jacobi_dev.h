// jacobi_dev.h -- cyclic trig-free Jacobi for small symmetric matrices in fp64 on one lane (registers).  Restated bit for bit by
// tests/pnp_restatement.py (jacobi); shared by k_pnp.hip, k_tri.hip and k_sim3.hip.  Include inside the including file's namespace, with contraction off.
#pragma once

#define JAC_SWEEPS 50      // Jacobi sweeps at most
#define JAC_NEGL_SWEEP 4   // from this sweep on, negligible off-diagonals are set to 0

// ---- one-lane symmetric eigen-problems (n = 3, 4), registers ----------------------------------------------------------------------
template <int n>
__device__ void jacobi_small(double (&a)[n][n], double (&V)[n][n]) {
#pragma unroll
  for (int i = 0; i < n; ++i)
#pragma unroll
    for (int j = 0; j < n; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < JAC_SWEEPS; ++sweep) {
    bool off = false;
#pragma unroll
    for (int p = 0; p < n - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < n; ++q) off |= a[p][q] != 0;
    if (!off) break;
#pragma unroll
    for (int p = 0; p < n - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[p][q];
        if (apq == 0) continue;
        const double app = a[p][p], aqq = a[q][q];
        if (sweep >= JAC_NEGL_SWEEP) {
          const double g = 100.0 * fabs(apq);
          if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
            a[p][q] = 0.0;
            a[q][p] = 0.0;
            continue;
          }
        }
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c), h = t * apq;
        a[p][p] = app - h;
        a[q][q] = aqq + h;
        a[p][q] = 0.0;
        a[q][p] = 0.0;
#pragma unroll
        for (int r = 0; r < n; ++r) {
          if (r == p || r == q) continue;
          const double g = a[r][p], hh = a[r][q];
          const double np = g - s * (hh + g * tau), nq = hh + s * (g - hh * tau);
          a[r][p] = np;
          a[p][r] = np;
          a[r][q] = nq;
          a[q][r] = nq;
        }
#pragma unroll
        for (int r = 0; r < n; ++r) {
          const double g = V[r][p], hh = V[r][q];
          V[r][p] = g - s * (hh + g * tau);
          V[r][q] = hh + s * (g - hh * tau);
        }
      }
  }
}


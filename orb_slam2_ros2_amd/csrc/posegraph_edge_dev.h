// posegraph_edge_dev.h -- the edge model of Optimizer::optimizeEssentialGraph (src/Optimizer.cc:746-920): g2o's EdgeSim3 between two
// VertexSim3Expmap with the scale fixed (types/sim3/types_seven_dof_expmap.h), Sim3::log (types/sim3/sim3.h) and the NUMERIC Jacobians
// of both vertices -- EdgeSim3 is taken to define no linearizeOplus (decision D3 of DESIGN 4.24), so g2o differentiates it by central
// differences and the rounding noise of that is part of what is computed.  Rules G1 .. G5 of DESIGN 4.24;
// tests/essential_graph_restatement.py spells the same operations in the same order.  The group (Sim3Dev, product, inverse, exp, oplus,
// the twelve perturbed estimates) is sim3_edge_dev.h's.  fp64, contraction off.
// Host + device like sim3_edge_dev.h: tests/cpp/test_posegraph_edge.cpp compiles this header with the host compiler alone.
#pragma once
#include "sim3_edge_dev.h"

namespace orbfe {

#define PG_LOG_EPS 1e-5  // g2o's Sim3::log: eps of the small-angle switch
#define PG_N_EVAL 25     // evaluations of one linearisation: the estimate, 12 perturbed of vertex 0, 12 perturbed of vertex 1

// x = W^-1 t by partial-pivot LU of the 3x3 W (rows r0, r1, r2, the right-hand side carried as a fourth column: the forward substitution
// is part of the elimination).  The pivot of a column is the first entry of the largest magnitude; rows move by selects, so nothing here
// is an array indexed at run time.
ORBFE_HD inline void pg_lu3_solve(double (*M)[4], double* x) {
  ORBFE_FP_STRICT
  double a[4], b[4], c[4];
  ORBFE_UNROLL
  for (int j = 0; j < 4; ++j) a[j] = M[0][j], b[j] = M[1][j], c[j] = M[2][j];
  // column 0: pivot among a, b, c
  {
    const bool pb = fabs(b[0]) > fabs(a[0]);
    const double big = pb ? fabs(b[0]) : fabs(a[0]);
    const bool pc = fabs(c[0]) > big;
    ORBFE_UNROLL
    for (int j = 0; j < 4; ++j) {
      const double aj = a[j], bj = b[j], cj = c[j];
      a[j] = pc ? cj : (pb ? bj : aj);
      b[j] = pc ? bj : (pb ? aj : bj);
      c[j] = pc ? aj : cj;
    }
  }
  const double l1 = b[0] / a[0], l2 = c[0] / a[0];
  ORBFE_UNROLL
  for (int j = 1; j < 4; ++j) {
    b[j] = b[j] - l1 * a[j];
    c[j] = c[j] - l2 * a[j];
  }
  // column 1: pivot among b, c
  {
    const bool pc = fabs(c[1]) > fabs(b[1]);
    ORBFE_UNROLL
    for (int j = 1; j < 4; ++j) {
      const double bj = b[j], cj = c[j];
      b[j] = pc ? cj : bj;
      c[j] = pc ? bj : cj;
    }
  }
  const double l3 = c[1] / b[1];
  ORBFE_UNROLL
  for (int j = 2; j < 4; ++j) c[j] = c[j] - l3 * b[j];
  // U x = y, a column at a time
  x[2] = c[3] / c[2];
  double y1 = b[3] - b[2] * x[2];
  double y0 = a[3] - a[2] * x[2];
  x[1] = y1 / b[1];
  y0 = y0 - a[1] * x[1];
  x[0] = y0 / a[0];
}

// Sim3::log with sigma = log(s) = 0 (G1: every scale is 1): out = (omega, upsilon); the seventh entry is 0 and is not stored (G4)
ORBFE_HD inline void sim3_log(const Sim3Dev& S, double* out) {
  ORBFE_FP_STRICT
  double R[9];
  quat_to_rot(S.q, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  double w[3], A, B;
  if (d > 1 - PG_LOG_EPS) {
    w[0] = 0.5 * dR[0], w[1] = 0.5 * dR[1], w[2] = 0.5 * dR[2];
    A = 0.5, B = 1. / 6.;
  } else {
    const double theta = acos(d);
    const double theta2 = theta * theta;
    const double k = theta / (2 * sqrt(1 - d * d));
    w[0] = k * dR[0], w[1] = k * dR[1], w[2] = k * dR[2];
    A = (1 - cos(theta)) / theta2;
    B = (theta - sin(theta)) / (theta2 * theta);
  }
  const double Om[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
  double M[3][4];
  ORBFE_UNROLL
  for (int i = 0; i < 3; ++i) {
    ORBFE_UNROLL
    for (int j = 0; j < 3; ++j) {
      double o2 = 0;
      ORBFE_UNROLL
      for (int k = 0; k < 3; ++k) o2 = o2 + Om[i][k] * Om[k][j];
      M[i][j] = A * Om[i][j] + B * o2 + ((i == j) ? 1.0 : 0.0);
    }
    M[i][3] = S.t[i];
  }
  out[0] = w[0], out[1] = w[1], out[2] = w[2];
  pg_lu3_solve(M, out + 3);
}

// EdgeSim3::computeError (G3): e = log(C * S_v0 * S_v1^-1), C the measurement; the information is the identity
ORBFE_HD inline void pg_edge_error(const Sim3Dev& C, const Sim3Dev& S0, const Sim3Dev& S1, double* e) {
  Sim3Dev S1i, A, B;
  sim3_inverse(S1, S1i);
  sim3_mul(C, S0, A);
  sim3_mul(A, S1i, B);
  sim3_log(B, e);
}

// chi2 = e . e in index order
ORBFE_HD_INLINE double pg_edge_chi2(const double* e) {
  ORBFE_FP_STRICT
  return e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3] + e[4] * e[4] + e[5] * e[5];
}

// Evaluation k of a linearisation (G5): k = 0 at the estimates; k = 1 + m, m = 0 .. 11, with vertex 0 at sim3_perturbed(S0, m);
// k = 13 + m with vertex 1 at sim3_perturbed(S1, m).  Column d of J_v0 is sim3_num_diff(e[1 + 2 d], e[2 + 2 d]), of J_v1
// sim3_num_diff(e[13 + 2 d], e[14 + 2 d]).
ORBFE_HD inline void pg_edge_eval(const Sim3Dev& C, const Sim3Dev& S0, const Sim3Dev& S1, int k, double* e) {
  Sim3Dev P0 = S0, P1 = S1;
  if (k >= 1 && k <= 12) sim3_perturbed(S0, k - 1, P0);
  if (k >= 13) sim3_perturbed(S1, k - 13, P1);
  pg_edge_error(C, P0, P1, e);
}

// linearizeOplus of one edge for both vertices: J0[r][d], J1[r][d], r the error row, d = omega, upsilon
ORBFE_HD inline void pg_edge_jacobians(const Sim3Dev& C, const Sim3Dev& S0, const Sim3Dev& S1, double (*J0)[6], double (*J1)[6]) {
  for (int d = 0; d < 6; ++d) {
    double ep[6], em[6];
    pg_edge_eval(C, S0, S1, 1 + 2 * d, ep);
    pg_edge_eval(C, S0, S1, 2 + 2 * d, em);
    for (int r = 0; r < 6; ++r) J0[r][d] = sim3_num_diff(ep[r], em[r]);
    pg_edge_eval(C, S0, S1, 13 + 2 * d, ep);
    pg_edge_eval(C, S0, S1, 14 + 2 * d, em);
    for (int r = 0; r < 6; ++r) J1[r][d] = sim3_num_diff(ep[r], em[r]);
  }
}

}  // namespace orbfe

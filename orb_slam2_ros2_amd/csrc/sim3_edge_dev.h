// sim3_edge_dev.h -- the edge model of Optimizer::OptimizeSim3 (src/Optimizer.cc:464-619): g2o's Sim3 (types/sim3/sim3.h) with the scale
// update fixed at 0, EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ (types_seven_dof_expmap) and their NUMERIC Jacobians -- these two
// edge types define no linearizeOplus, so g2o differentiates them by central differences, and the rounding noise of that is part of what
// the reference computes.  Rules O1 .. O5 of DESIGN 4.22; tests/sim3_opt_restatement.py spells the same operations in the same order.
// Estimate = (qx, qy, qz, qw, tx, ty, tz, s), map(X) = s * (q * X) + t.  fp64, contraction off.
// Host + device like ba_edge_dev.h: tests/cpp/test_sim3_edge.cpp compiles this header with the host compiler alone.
#pragma once
#include "ba_edge_dev.h"

namespace orbfe {

struct Sim3Dev {
  double q[4], t[3], s;
};

#define SIM3_NUM_DELTA 1e-9                        // g2o's BaseBinaryEdge::linearizeOplus: delta of the central difference
#define SIM3_NUM_SCALE (1.0 / (2 * SIM3_NUM_DELTA))
#define SIM3_CHI2_TH 9.210                         // Optimizer.cc:574, :599
#define SIM3_MIN_PAIRS 20                          // Optimizer.cc:584

// Sim3::map: s * (r * X) + t
ORBFE_HD_INLINE void sim3_map(const Sim3Dev& S, const double* X, double* p) {
  ORBFE_FP_STRICT
  double r[3];
  quat_rotate(S.q, X, r);
  p[0] = S.s * r[0] + S.t[0];
  p[1] = S.s * r[1] + S.t[1];
  p[2] = S.s * r[2] + S.t[2];
}

// Sim3::inverse: (r*, r* * ((-1 / s) * t), 1 / s)
ORBFE_HD_INLINE void sim3_inverse(const Sim3Dev& S, Sim3Dev& out) {
  ORBFE_FP_STRICT
  out.q[0] = -S.q[0], out.q[1] = -S.q[1], out.q[2] = -S.q[2], out.q[3] = S.q[3];
  const double k = -1.0 / S.s;
  const double kt[3] = {k * S.t[0], k * S.t[1], k * S.t[2]};
  quat_rotate(out.q, kt, out.t);
  out.s = 1.0 / S.s;
}

// Sim3::operator*: r = rA rB, t = sA (rA * tB) + tA, s = sA sB.  The rotation is NOT renormalised (decision D2 of DESIGN 4.22).
ORBFE_HD_INLINE void sim3_mul(const Sim3Dev& A, const Sim3Dev& B, Sim3Dev& out) {
  ORBFE_FP_STRICT
  const double ax = A.q[0], ay = A.q[1], az = A.q[2], aw = A.q[3];
  const double bx = B.q[0], by = B.q[1], bz = B.q[2], bw = B.q[3];
  out.q[3] = aw * bw - ax * bx - ay * by - az * bz;
  out.q[0] = aw * bx + ax * bw + ay * bz - az * by;
  out.q[1] = aw * by + ay * bw + az * bx - ax * bz;
  out.q[2] = aw * bz + az * bw + ax * by - ay * bx;
  double rt[3];
  quat_rotate(A.q, B.t, rt);
  out.t[0] = A.s * rt[0] + A.t[0];
  out.t[1] = A.s * rt[1] + A.t[1];
  out.t[2] = A.s * rt[2] + A.t[2];
  out.s = A.s * B.s;
}

// g2o's Sim3(Vector7) with sigma = 0 (O1: VertexSim3Expmap::oplusImpl zeroes update[6] when the scale is fixed): upd = (omega, upsilon),
// eps = 1e-5.  Small angles: A = 1/2, B = 1/6, R = I + Omega + Omega^2 / 2 (decision D1).
ORBFE_HD inline void sim3_exp(const double* upd, Sim3Dev& out) {
  ORBFE_FP_STRICT
  const double wx = upd[0], wy = upd[1], wz = upd[2];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  const double Om[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
  double Om2[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double a = 0;
      for (int k = 0; k < 3; ++k) a = a + Om[i][k] * Om[k][j];
      Om2[i][j] = a;
    }
  double R[3][3], A, B;
  if (theta < 0.00001) {
    A = 0.5, B = 1. / 6.;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i][j] = ((i == j) ? 1.0 : 0.0) + Om[i][j] + 0.5 * Om2[i][j];
  } else {
    const double st = sin(theta), ct = cos(theta);
    A = (1 - ct) / (theta * theta);
    B = (theta - st) / (theta * theta * theta);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i][j] = ((i == j) ? 1.0 : 0.0) + st / theta * Om[i][j] + A * Om2[i][j];
  }
  for (int i = 0; i < 3; ++i) {
    double W[3];
    for (int j = 0; j < 3; ++j) W[j] = A * Om[i][j] + B * Om2[i][j] + ((i == j) ? 1.0 : 0.0);
    out.t[i] = W[0] * upd[3] + W[1] * upd[4] + W[2] * upd[5];
  }
  rot_to_quat(R, out.q);
  out.s = 1.0;
}

// VertexSim3Expmap::oplusImpl: exp(update) * estimate
ORBFE_HD inline void sim3_oplus(const Sim3Dev& est, const double* upd, Sim3Dev& out) {
  Sim3Dev e;
  sim3_exp(upd, e);
  sim3_mul(e, est, out);
}

// The estimate the numeric Jacobian evaluates for k = 0 .. 11: oplus(+delta e_d) for k = 2 d, oplus(-delta e_d) for k = 2 d + 1 (O4; column
// 6 is exactly 0 by O1 and is never evaluated).  The same twelve estimates serve every edge of a linearisation.
ORBFE_HD inline void sim3_perturbed(const Sim3Dev& est, int k, Sim3Dev& out) {
  double u[6];
  for (int j = 0; j < 6; ++j) u[j] = (j == (k >> 1)) ? ((k & 1) ? -SIM3_NUM_DELTA : SIM3_NUM_DELTA) : 0.0;
  sim3_oplus(est, u, out);
}

// ConvertSim3G2o (O2): float R (row-major), t -> double, Eigen's Quaternion(R), g2o's Sim3(r, t, s) constructor (w < 0 negates, then
// divide by the norm); s = 1
ORBFE_HD inline void sim3_from_model(const float* model, Sim3Dev& out) {
  ORBFE_FP_STRICT
  double R[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = (double)model[3 * i + j];
  rot_to_quat(R, out.q);
  if (out.q[3] < 0)
    for (int i = 0; i < 4; ++i) out.q[i] = -out.q[i];
  const double n = sqrt(out.q[0] * out.q[0] + out.q[1] * out.q[1] + out.q[2] * out.q[2] + out.q[3] * out.q[3]);
  for (int i = 0; i < 4; ++i) out.q[i] = out.q[i] / n;
  for (int i = 0; i < 3; ++i) out.t[i] = (double)model[9 + i];
  out.s = 1.0;
}

// ConvertG2o2Sim3 (O2): Eigen's toRotationMatrix in double, every entry cast to float
ORBFE_HD inline void sim3_to_model(const Sim3Dev& S, float* model) {
  double R[9];
  quat_to_rot(S.q, R);
  for (int i = 0; i < 9; ++i) model[i] = (float)R[i];
  for (int i = 0; i < 3; ++i) model[9 + i] = (float)S.t[i];
}

// one match of OptimizeSim3: cPc and mPc (the two map points in their own keyframe's camera frame), the key points they were seen at
// and the information of the two edges
struct Sim3Pair {
  double pc[3], pm[3], uvc[2], uvm[2], wc, wm;
};

// computeError of both edges of a pair at the estimate S with inverse Si: e[0..1] = EdgeSim3ProjectXYZ (mPc mapped into pCurr, against
// uv_c), e[2..3] = EdgeInverseSim3ProjectXYZ (cPc mapped into pMatch, against uv_m); both cameras are the one Camera (prm.bf unused)
ORBFE_HD_INLINE void sim3_pair_errors(const Sim3Dev& S, const Sim3Dev& Si, const Sim3Pair& P, const BaParamsDev& prm, double* e) {
  double p[3], e3[3];
  sim3_map(S, P.pm, p);
  ba_edge_error(p, P.uvc, false, prm, e3);
  e[0] = e3[0], e[1] = e3[1];
  sim3_map(Si, P.pc, p);
  ba_edge_error(p, P.uvm, false, prm, e3);
  e[2] = e3[0], e[3] = e3[1];
}

// chi2 of the two edges from the pair's four errors
ORBFE_HD_INLINE void sim3_pair_chi2(const double* e, const Sim3Pair& P, double* chi2) {
  chi2[0] = ba_edge_chi2(e, P.wc, false);
  chi2[1] = ba_edge_chi2(e + 2, P.wm, false);
}

// column d of both edges' Jacobians from the errors at oplus(+delta e_d) and oplus(-delta e_d)
ORBFE_HD_INLINE double sim3_num_diff(double e_plus, double e_minus) {
  ORBFE_FP_STRICT
  return SIM3_NUM_SCALE * (e_plus - e_minus);
}

// linearizeOplus of both edges of a pair: J[r][d], r = e1.u, e1.v, e2.u, e2.v, d = omega, upsilon
ORBFE_HD inline void sim3_pair_jacobian(const Sim3Dev& est, const Sim3Pair& P, const BaParamsDev& prm, double (*J)[6]) {
  for (int d = 0; d < 6; ++d) {
    Sim3Dev S, Si;
    double ep[4], em[4];
    sim3_perturbed(est, 2 * d, S);
    sim3_inverse(S, Si);
    sim3_pair_errors(S, Si, P, prm, ep);
    sim3_perturbed(est, 2 * d + 1, S);
    sim3_inverse(S, Si);
    sim3_pair_errors(S, Si, P, prm, em);
    for (int r = 0; r < 4; ++r) J[r][d] = sim3_num_diff(ep[r], em[r]);
  }
}

}  // namespace orbfe

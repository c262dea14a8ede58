// ba_edge_dev.h -- the ONE edge model of the bundle-adjustment and pose-only kernels: what g2o's EdgeSE3ProjectXYZ /
// EdgeStereoSE3ProjectXYZ (types_six_dof_expmap) and their OnlyPose variants compute per edge -- map, projection error, chi2,
// RobustKernelHuber, both Jacobians -- plus the outlier test of Optimizer.cc and the damped point-block inverse of BlockSolver_6_3.
// Pose vertex = SE3Quat (qx, qy, qz, qw, tx, ty, tz), map(X) = q * X + t.  Every expression is spelled in g2o's evaluation order (as
// the CPU checker of the test suite spells it): fp64, contraction off, so every kernel that uses an edge gets the same bits for it.
// Host + device like se3_dev.h: tests/cpp/test_ba_edge.cpp compiles this header with the host compiler alone and checks it against
// the 40-digit references of tests/se3_reference.py.
#pragma once
#include "se3_dev.h"

struct BaParamsDev {
  double fx, fy, cx, cy, bf;
};

namespace orbfe {

// T * X (SE3Quat::map): the Eigen quaternion-vector product, then + t
ORBFE_HD_INLINE void se3_map(const double* q, const double* t, const double* X, double* p) {
  ORBFE_FP_STRICT
  quat_rotate(q, X, p);
  p[0] = p[0] + t[0];
  p[1] = p[1] + t[1];
  p[2] = p[2] + t[2];
}

// computeError of both edge types at the camera-frame point p = T * X: m - cam_project(p); e[2] = 0 for a mono edge
ORBFE_HD_INLINE void ba_edge_error(const double* p, const double* m, bool stereo, const BaParamsDev& prm, double* e) {
  ORBFE_FP_STRICT
  const double u = p[0] / p[2] * prm.fx + prm.cx, v = p[1] / p[2] * prm.fy + prm.cy;
  e[0] = m[0] - u;
  e[1] = m[1] - v;
  e[2] = stereo ? (m[2] - (u - prm.bf / p[2])) : 0.0;
}

// isDepthPositive: (T * X).z > 0
ORBFE_HD_INLINE bool ba_depth_positive(const double* p) { return p[2] > 0.0; }

// chi2 = e^T (w I) e the way Eigen evaluates it: dot(e, (w * I) * e)
ORBFE_HD_INLINE double ba_edge_chi2(const double* e, double w, bool stereo) {
  ORBFE_FP_STRICT
  return stereo ? (e[0] * (w * e[0]) + e[1] * (w * e[1]) + e[2] * (w * e[2])) : (e[0] * (w * e[0]) + e[1] * (w * e[1]));
}

// RobustKernelHuber::robustify: rho(chi2) and rho'(chi2)
ORBFE_HD_INLINE void huber_robustify(double c2, double delta, double& rho, double& drho) {
  ORBFE_FP_STRICT
  const double dsqr = delta * delta;
  rho = c2, drho = 1.0;
  if (c2 > dsqr) {
    const double sq = sqrt(c2);
    rho = 2 * sq * delta - dsqr;
    drho = delta / sq;
  }
}
// an edge's robust kernel as the problems carry it: delta <= 0 means no kernel, rho = (chi2, 1)
ORBFE_HD_INLINE void ba_edge_robustify(double c2, double delta, double& rho, double& drho) {
  rho = c2, drho = 1.0;
  if (delta > 0.0) huber_robustify(c2, delta, rho, drho);
}

// rotation matrix of the unit quaternion (Eigen toRotationMatrix), row-major
ORBFE_HD_INLINE void quat_to_rot(const double* q, double* R) {
  ORBFE_FP_STRICT
  const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
  const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
  const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}

// linearizeOplus, d e / d point (3x3 row-major, row 2 zero for mono).  Stereo: EdgeStereoSE3ProjectXYZ; mono: EdgeSE3ProjectXYZ's
// -1/z * tmp * R with tmp = [[fx, 0, -x/z*fx], [0, fy, -y/z*fy]], scalar * matrix first as Eigen evaluates it
ORBFE_HD_INLINE void ba_edge_jpoint(const double* q, const double* p, bool stereo, const BaParamsDev& prm, double* A_out) {
  ORBFE_FP_STRICT
  const double x = p[0], y = p[1], z = p[2], z_2 = z * z;
  const double fx = prm.fx, fy = prm.fy, bf = prm.bf;
  double R[9], A[9];
  quat_to_rot(q, R);
  if (stereo) {
    ORBFE_UNROLL
    for (int k = 0; k < 3; ++k) {
      A[k] = -fx * R[k] / z + fx * x * R[6 + k] / z_2;
      A[3 + k] = -fy * R[3 + k] / z + fy * y * R[6 + k] / z_2;
      A[6 + k] = A[k] - bf * R[6 + k] / z_2;
    }
  } else {
    const double t02 = -x / z * fx, t12 = -y / z * fy, s = -1. / z;
    ORBFE_UNROLL
    for (int k = 0; k < 3; ++k) {
      A[k] = (s * fx) * R[k] + (s * t02) * R[6 + k];
      A[3 + k] = (s * fy) * R[3 + k] + (s * t12) * R[6 + k];
      A[6 + k] = 0.0;
    }
  }
  // (all nine entries leave in one place: written branch by branch into the caller's array, k_lm_linpoints carried that array around
  //  its edge loop as a vector -- 18 registers more and an occupancy step less)
  ORBFE_UNROLL
  for (int k = 0; k < 9; ++k) A_out[k] = A[k];
}

// linearizeOplus, d e / d pose (3x6 row-major: omega, upsilon; row 2 zero for mono)
ORBFE_HD_INLINE void ba_edge_jpose(const double* p, bool stereo, const BaParamsDev& prm, double* B) {
  ORBFE_FP_STRICT
  const double x = p[0], y = p[1], z = p[2], z_2 = z * z;
  const double fx = prm.fx, fy = prm.fy, bf = prm.bf;
  B[0] = x * y / z_2 * fx;
  B[1] = -(1 + (x * x / z_2)) * fx;
  B[2] = y / z * fx;
  B[3] = -1. / z * fx;
  B[4] = 0;
  B[5] = x / z_2 * fx;
  B[6] = (1 + y * y / z_2) * fy;
  B[7] = -x * y / z_2 * fy;
  B[8] = -x / z * fy;
  B[9] = 0;
  B[10] = -1. / z * fy;
  B[11] = y / z_2 * fy;
  if (stereo) {
    B[12] = B[0] - bf * y / z_2;
    B[13] = B[1] + bf * x / z_2;
    B[14] = B[2];
    B[15] = B[3];
    B[16] = 0;
    B[17] = B[5] - bf / z_2;
  } else {
    ORBFE_UNROLL
    for (int k = 12; k < 18; ++k) B[k] = 0.0;
  }
}

// The same Jacobian as Edge(Stereo)SE3ProjectXYZOnlyPose spells it, with invz: it rounds differently from ba_edge_jpose and stays separate.
ORBFE_HD_INLINE void pose_edge_jpose(const double* p, bool stereo, const BaParamsDev& prm, double* J) {
  ORBFE_FP_STRICT
  const double x = p[0], y = p[1], z = p[2];
  const double invz = 1.0 / z, invz_2 = invz * invz;
  J[0] = x * y * invz_2 * prm.fx;
  J[1] = -(1 + (x * x * invz_2)) * prm.fx;
  J[2] = y * invz * prm.fx;
  J[3] = -invz * prm.fx;
  J[4] = 0;
  J[5] = x * invz_2 * prm.fx;
  J[6] = (1 + y * y * invz_2) * prm.fy;
  J[7] = -x * y * invz_2 * prm.fy;
  J[8] = -x * invz * prm.fy;
  J[9] = 0;
  J[10] = -invz * prm.fy;
  J[11] = y * invz_2 * prm.fy;
  J[12] = stereo ? J[0] - prm.bf * y * invz_2 : 0.0;
  J[13] = stereo ? J[1] + prm.bf * x * invz_2 : 0.0;
  J[14] = stereo ? J[2] : 0.0;
  J[15] = stereo ? J[3] : 0.0;
  J[16] = 0;
  J[17] = stereo ? J[5] - prm.bf * invz_2 : 0.0;
}

// Optimizer.cc:338-359 / :364-391: an edge is an outlier when chi2 > 7.815 (stereo, 3 dof) / 5.991 (mono, 2 dof) or its depth is not positive
ORBFE_HD_INLINE double ba_chi2_threshold(bool stereo) { return stereo ? 7.815 : 5.991; }
ORBFE_HD_INLINE bool ba_edge_outlier(double chi2, bool stereo, bool depth_positive) {
  return chi2 > ba_chi2_threshold(stereo) || !depth_positive;
}

// D = (H + lambda I)^-1 of a point block (Eigen's 3x3 inverse: cofactors / determinant); false (D untouched) when the determinant is
// zero or not finite
ORBFE_HD_INLINE bool inv3_damped(const double* H, double lambda, double* D) {
  ORBFE_FP_STRICT
  double M[9];
  ORBFE_UNROLL
  for (int i = 0; i < 9; ++i) M[i] = H[i];
  M[0] += lambda, M[4] += lambda, M[8] += lambda;
  const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
  if (det == 0 || !isfinite(det)) return false;
  const double id = 1.0 / det;
  D[0] = c00 * id;
  D[1] = (M[2] * M[7] - M[1] * M[8]) * id;
  D[2] = (M[1] * M[5] - M[2] * M[4]) * id;
  D[3] = c01 * id;
  D[4] = (M[0] * M[8] - M[2] * M[6]) * id;
  D[5] = (M[2] * M[3] - M[0] * M[5]) * id;
  D[6] = c02 * id;
  D[7] = (M[1] * M[6] - M[0] * M[7]) * id;
  D[8] = (M[0] * M[4] - M[1] * M[3]) * id;
  return true;
}

}  // namespace orbfe

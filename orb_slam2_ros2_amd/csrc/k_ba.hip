// k_ba.hip -- local-BA reprojection error / Jacobian / Huber evaluation, one lane per edge, fp64.
//
// Replaces the per-edge arithmetic g2o runs for the graph Optimizer::OptimizeLocalMap builds
// (src/ORB_SLAM2/src/Optimizer.cc:296-330): EdgeStereoSE3ProjectXYZ / EdgeSE3ProjectXYZ computeError,
// linearizeOplus, chi2, isDepthPositive, and RobustKernelHuber::robustify (g2o 20241228 types_sba,
// core/robust_kernel_impl).  The arithmetic is ba_edge_dev.h's, the edge model every optimiser kernel shares: this entry point
// (orbfe_ba_eval_edges, and the chi2 of the host-driven loop) shows an edge exactly as k_lm.hip's system builder sees it.
// HBM-bound gather/scatter: 304 B per edge + the vertices; nothing here is a dense
// contraction, so no MFMA.
#include <hip/hip_runtime.h>

#include "ba_edge_dev.h"
#include "orbfe_internal.h"

namespace orbfe {

__global__ __launch_bounds__(256) void k_ba_edges(int n_edges, const double* __restrict__ poses, const double* __restrict__ points,
                                                  const int32_t* __restrict__ edge_pose, const int32_t* __restrict__ edge_point,
                                                  const double* __restrict__ meas, const uint8_t* __restrict__ is_stereo,
                                                  const double* __restrict__ info, const double* __restrict__ delta, BaParamsDev prm,
                                                  double* __restrict__ error, double* __restrict__ chi2, double* __restrict__ rho,
                                                  double* __restrict__ jpoint, double* __restrict__ jpose,
                                                  uint8_t* __restrict__ depth_pos) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  const double* T = poses + (size_t)edge_pose[e] * 7;
  double p[3], err[3], r0, r1;
  se3_map(T, T + 4, points + (size_t)edge_point[e] * 3, p);
  const bool st = is_stereo[e] != 0;
  ba_edge_error(p, meas + (size_t)e * 3, st, prm, err);
#pragma unroll
  for (int k = 0; k < 3; ++k) error[(size_t)e * 3 + k] = err[k];
  const double c2 = ba_edge_chi2(err, info[e], st);
  chi2[e] = c2;
  ba_edge_robustify(c2, delta[e], r0, r1);
  rho[(size_t)e * 2 + 0] = r0;
  rho[(size_t)e * 2 + 1] = r1;
  if (depth_pos) depth_pos[e] = ba_depth_positive(p);
  if (jpoint) {
    double A[9];
    ba_edge_jpoint(T, p, st, prm, A);
#pragma unroll
    for (int k = 0; k < 9; ++k) jpoint[(size_t)e * 9 + k] = A[k];
  }
  if (jpose) {
    double B[18];
    ba_edge_jpose(p, st, prm, B);
#pragma unroll
    for (int k = 0; k < 18; ++k) jpose[(size_t)e * 18 + k] = B[k];
  }
}

void launch_ba_edges(hipStream_t s, int n_edges, const double* d_poses, const double* d_points, const int32_t* d_edge_pose,
                     const int32_t* d_edge_point, const double* d_meas, const uint8_t* d_is_stereo, const double* d_info,
                     const double* d_delta, BaParamsDev prm, double* d_error, double* d_chi2, double* d_rho, double* d_jpoint,
                     double* d_jpose, uint8_t* d_depth_pos) {
  if (n_edges <= 0) return;
  hipLaunchKernelGGL(k_ba_edges, dim3((n_edges + 255) / 256), dim3(256), 0, s, n_edges, d_poses, d_points, d_edge_pose,
                     d_edge_point, d_meas, d_is_stereo, d_info, d_delta, prm, d_error, d_chi2, d_rho, d_jpoint, d_jpose, d_depth_pos);
}

}  // namespace orbfe

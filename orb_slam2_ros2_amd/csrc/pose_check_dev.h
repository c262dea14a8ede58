// pose_check_dev.h -- what surrounds a pose-only optimisation inside a Tracking step, shared by k_guided.hip (k_track_edges), k_reloc.hip
// (DESIGN 4.28), k_trackref.hip and k_motion.hip: the edge list of Optimizer::OptimizePoseOnly in feature
// order (src/Optimizer.cc:58-117), its two pose conversions (:119, :201) in fp64, its projection post-check (:179-199) and the write-back
// of the estimate, as the 1024 threads of one workgroup run them over orbfe_internal.h's PoseFrameDev / PoseEdgesDev.  The callers differ
// only in where a feature's point comes from and in what a feature that is no inlier loses; both are parameters here, so the edge
// builder and the post-check have one text each.  Beside them the motion direction and the octave window of
// searchByProjection(frame, other frame), which the relocalisation refine and the motion model share.
// Float arithmetic: map_point_dev.h's rows and `A x + t`; the includer switches contraction off.
#pragma once
#include <hip/hip_runtime.h>

#include "map_point_dev.h"
#include "orbfe_internal.h"

namespace orbfe {

// the largest-diagonal branch of Eigen::Quaterniond(Matrix3d) with the largest element at I (constant indices: the arrays stay registers)
template <int I>
__device__ __forceinline__ void quat_diag(const double (&m)[3][3], double (&q)[4]) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  double tr = sqrt(m[I][I] - m[J][J] - m[K][K] + 1.0);
  q[I] = 0.5 * tr;
  tr = 0.5 / tr;
  q[3] = (m[K][J] - m[J][K]) * tr;
  q[J] = (m[J][I] + m[I][J]) * tr;
  q[K] = (m[K][I] + m[I][K]) * tr;
}

// Converter::ConvertTcw2SE3 (src/Optimizer.cc:630-645): host/map_pb.hpp's tcw_to_se3
__device__ __forceinline__ void tcw_to_se3_dev(const float* R, const float* t, double* out) {
  double m[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) m[i][j] = (double)R[i * 3 + j];
  double q[4];
  double tr = m[0][0] + m[1][1] + m[2][2];
  if (tr > 0.0) {
    tr = sqrt(tr + 1.0);
    q[3] = 0.5 * tr;
    tr = 0.5 / tr;
    q[0] = (m[2][1] - m[1][2]) * tr, q[1] = (m[0][2] - m[2][0]) * tr, q[2] = (m[1][0] - m[0][1]) * tr;
  } else if (m[2][2] > (m[1][1] > m[0][0] ? m[1][1] : m[0][0]))
    quat_diag<2>(m, q);
  else if (m[1][1] > m[0][0])
    quat_diag<1>(m, q);
  else
    quat_diag<0>(m, q);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {  // Quaterniond::normalize(), then SE3Quat::normalizeRotation()
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (n > 0.0) q[0] /= n, q[1] /= n, q[2] /= n, q[3] /= n;
  }
  if (q[3] < 0.0) q[0] = -q[0], q[1] = -q[1], q[2] = -q[2], q[3] = -q[3];
  out[0] = q[0], out[1] = q[1], out[2] = q[2], out[3] = q[3];
  out[4] = (double)t[0], out[5] = (double)t[1], out[6] = (double)t[2];
}

// Converter::ConvertSE32Tcw (src/Optimizer.cc:653-675): host/map_pb.hpp's se3_to_tcw
__device__ __forceinline__ void se3_to_tcw_dev(const double* p, float* R, float* t) {
  const double x = p[0], y = p[1], z = p[2], w = p[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = (float)(1.0 - (tyy + tzz)), R[1] = (float)(txy - twz), R[2] = (float)(txz + twy);
  R[3] = (float)(txy + twz), R[4] = (float)(1.0 - (txx + tzz)), R[5] = (float)(tyz - twx);
  R[6] = (float)(txz - twy), R[7] = (float)(tyz + twx), R[8] = (float)(1.0 - (txx + tyy));
  t[0] = (float)p[4], t[1] = (float)p[5], t[2] = (float)p[6];
}

// The motion direction of ORBMatcher::searchByProjection(frame, other frame) (src/ORBMatcher.cc:274-276): twc = -Rcw^T tcw of the searching
// frame, tlc = R2 twc + t2 with the other frame's pose; returns tlc.z
__device__ __forceinline__ float tlc_z_dev(const float* R, const float* tc, const float* R2, const float* t2) {
  float twc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) twc[r] = -(R[r] * tc[0] + R[3 + r] * tc[1] + R[6 + r] * tc[2]);
  float tlc[3];
  affine(1.0f, R2, twc, t2, tlc);
  return tlc[2];
}

// the octave window of a query of octave o under that direction (:279-280, :300-313)
__device__ __forceinline__ void motion_window(int o, float z, float baseline, int& lo, int& hi) {
  if (fabsf(z) > baseline) {
    if (z > 0.f) lo = o, hi = 7;
    else lo = 0, hi = o;
  } else
    lo = max(0, o - 1), hi = min(o + 1, 7);
}

// The edge list of Optimizer::OptimizePoseOnly (src/Optimizer.cc:58-117) over the features of F, in feature order, by the 1024 threads of
// one workgroup (all of them call it): a ballot per wave, the waves' counts summed in wave order, the base carried across the trips.
// point_of(f), called once for every f < F.nf by the thread that owns f, returns the position of the point the feature's edge goes to, or
// nullptr when the feature has no edge; what else the caller does per feature (its assignment, its counts) it does in there.  Writes
// E.edge_of[f] for every feature and Xw, meas, info, sig per edge; the octave that indexes the level tables is clamped into them.
// Returns the edge count to every thread.  s_wave[16], s_base: LDS of the caller.
template <class PointOf>
__device__ __forceinline__ int pose_edges_1024(const PoseFrameDev& F, const PoseEdgesDev& E, int* s_wave, int* s_base, PointOf point_of) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) *s_base = 0;
  __syncthreads();
  for (int f0 = 0; f0 < F.nf; f0 += 1024) {
    const int f = f0 + t;
    const float* X = f < F.nf ? point_of(f) : nullptr;
    const bool edge = X != nullptr;
    const unsigned long long me = __ballot(edge);
    if (lane == 0) s_wave[wv] = __popcll(me);
    __syncthreads();
    int before = *s_base, chunk = 0;
    for (int w = 0; w < 16; ++w) {
      if (w < wv) before += s_wave[w];
      chunk += s_wave[w];
    }
    const int e = before + __popcll(me & ((1ull << lane) - 1ull));
    if (f < F.nf) E.edge_of[f] = edge ? e : -1;
    if (edge) {
      const orbfe_keypoint k = F.kps[f];
      E.Xw[3 * e] = (double)X[0], E.Xw[3 * e + 1] = (double)X[1], E.Xw[3 * e + 2] = (double)X[2];
      const double ru = F.right_u[f];
      E.meas[3 * e] = (double)k.x, E.meas[3 * e + 1] = (double)k.y, E.meas[3 * e + 2] = ru < 0 ? -1.0 : ru;
      const int oc = min(max(k.octave, 0), F.n_levels - 1);
      E.info[e] = (double)F.inv_sigma2[oc];
      E.sig[e] = F.sigma2[oc];
    }
    __syncthreads();
    if (t == 0) *s_base += chunk;
    __syncthreads();
  }
  return *s_base;
}

// The post-check over the features of F by the 1024 threads of one workgroup (all of them call it): feature f is an inlier when its edge
// is one of the optimiser's and its point projects into the image under (Rf, tf), the pose the frame still has -- setPose comes last
// (Optimizer.cc:201).  pos_of(f, X) gives the position of the point feature f holds (called for the optimiser's inliers only), drop(f)
// takes the point from a feature that is no inlier (`if (!inLier[idx]) mvpMapPoints[idx] = nullptr`, :191-194).  Writes inlier[f];
// returns edges - nBad to every thread.
template <class PosOf, class Drop>
__device__ __forceinline__ int post_check_1024(const PoseFrameDev& F, const float* Rf, const float* tf, const PoseEdgesDev& E,
                                               uint8_t* __restrict__ inlier, int* s_wave, PosOf pos_of, Drop drop) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float Rb[9], tb[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rb[k] = Rf[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tb[k] = tf[k];
  int mine = 0;
  for (int f0 = 0; f0 < F.nf; f0 += 1024) {
    const int f = f0 + t;
    bool inl = false;
    if (f < F.nf) {
      const int e = E.edge_of[f];
      inl = e >= 0 && E.e_inl[e] != 0;
      if (inl) {  // VirtualFrame::project2UV (src/Frame.cc:320-333) and the test of Optimizer.cc:185: 0, not mfMinU / mfMinV
        float X[3];
        pos_of(f, X);
        float pc[3];
        affine(1.0f, Rb, X, tb, pc);
        const float z = pc[2];
        const float u = pc[0] / z * F.fx + F.cx, v = pc[1] / z * F.fy + F.cy;
        if (!(z > 0.f) || u > F.max_u || u < 0.f || v > F.max_v || v < 0.f) inl = false;
      }
      inlier[f] = inl ? 1 : 0;
      if (!inl) drop(f);
    }
    mine += __popcll(__ballot(inl));
  }
  if (lane == 0) s_wave[wv] = mine;
  __syncthreads();
  int n_in = 0;
  for (int w = 0; w < 16; ++w) n_in += s_wave[w];
  return n_in;
}

// The close of a check, by one thread: the estimate and its float pose (Converter::ConvertSE32Tcw's R, tc) into the downloaded block.
__device__ __forceinline__ void pose_write_back(const double* est, const float* R, const float* tc, double* pose_out, float* tcw_out) {
  for (int k = 0; k < 7; ++k) pose_out[k] = est[k];
  for (int k = 0; k < 9; ++k) tcw_out[k] = R[k];
  for (int k = 0; k < 3; ++k) tcw_out[9 + k] = tc[k];
}

}  // namespace orbfe

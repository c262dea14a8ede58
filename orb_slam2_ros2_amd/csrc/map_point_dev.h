// map_point_dev.h -- MapPoint::isInVision and MapPoint::predictLevel (src/MapPoint.cc:141-201) as the guided matchers evaluate them per
// map point before the area search, in the float / double mix of the reference's cv::Mat expressions:
//   A * x            3x3 * 3x1 gemm: float products summed left to right
//   alpha A x + t    (float)((double)alpha * sum + t) (cv::gemm's alpha / beta; alpha = 1 multiplies exactly)
//   cv::norm, Mat::dot  double accumulation of float elements
// The one copy: k_guided.hip's k_project_map_points, k_fuse.hip's k_fuse_visible, k_sim3search.hip, k_fusepoints.hip's
// k_fusepts_project.  Every translation unit is built
// without floating-point contraction (Makefile), which these expressions need.
#pragma once
#include <hip/hip_runtime.h>

namespace orbfe {

__device__ __forceinline__ float mat3_row(const float* A, int r, const float* x) { return A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2]; }

__device__ __forceinline__ void affine(float alpha, const float* A, const float* x, const float* t, float* out) {
#pragma unroll
  for (int r = 0; r < 3; ++r) out[r] = (float)((double)alpha * (double)mat3_row(A, r, x) + (double)t[r]);
}

// what isInVision computed as far as its tests got; the rest stays 0
struct MapPointView {
  float pc[3];  // Rcw * X + tcw
  float u, v, distance, cos_theta;
};

// X, D: the point's world position and mean viewing direction (D is read only by a point that passes the first three tests);
// bounds = {min_u, max_u, min_v, max_v}.  The tests keep the reference's order: z < 0, isGoodDistance, VirtualFrame::isInImage, cos < 0.5.
__device__ __forceinline__ bool is_in_vision(const float* R, const float* t, const float* X, const float* D, float max_dist, float min_dist,
                                             float fx, float fy, float cx, float cy, const float* bounds, MapPointView& o) {
  const float Xw[3] = {X[0], X[1], X[2]};
  affine(1.0f, R, Xw, t, o.pc);
  o.u = 0.f, o.v = 0.f, o.distance = 0.f, o.cos_theta = 0.f;
  const float x = o.pc[0], y = o.pc[1], z = o.pc[2];
  if (z < 0.f) return false;
  o.distance = sqrtf(x * x + y * y + z * z);  // (correctly rounded; __fsqrt_rn maps to the native approximation)
  if (!(o.distance < max_dist && o.distance > min_dist)) return false;
  o.u = x / z * fx + cx;
  o.v = y / z * fy + cy;
  if (!(o.u < bounds[1] && o.v < bounds[3] && o.u > bounds[0] && o.v > bounds[2])) return false;
  const float Dw[3] = {D[0], D[1], D[2]};
  const float vd[3] = {mat3_row(R, 0, Dw), mat3_row(R, 1, Dw), mat3_row(R, 2, Dw)};
  const double nn = (double)vd[0] * (double)vd[0] + (double)vd[1] * (double)vd[1] + (double)vd[2] * (double)vd[2];
  const float vabs = (float)sqrt(nn);
  const double dot = (double)vd[0] * (double)x + (double)vd[1] * (double)y + (double)vd[2] * (double)z;
  o.cos_theta = (float)(dot / (double)(o.distance * vabs));
  return !(o.cos_theta < 0.5f);
}

// cvRound(std::log(nMaxDis / distance) / std::log(mfScaledFactor)) clamped to [0, max_level]; log_sf: the float of the denominator
__device__ __forceinline__ int predict_level(float max_dist, float distance, float log_sf, int max_level) {
  const float lr = (float)log((double)(max_dist / distance));
  const int level = __float2int_rn(lr / log_sf);
  return level < 0 ? 0 : (level > max_level ? max_level : level);
}

}  // namespace orbfe

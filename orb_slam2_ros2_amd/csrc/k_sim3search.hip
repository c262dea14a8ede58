// k_sim3search.hip -- both overloads of ORBMatcher::searchBySim3 (src/ORBMatcher.cc:370-559) over stored keyframes.
//
// k_sim3_search_pair    one wave per source feature, n_c + n_m waves: waves [0, n_c) are direction A (C's map points into M, :446-461),
//                       waves [n_c, n_c + n_m) direction B (M's into C, :463-475).  SIM3Project (:370-414): world -> source camera ->
//                       target camera through the similarity -> pixel, isInImage on the SOURCE keyframe's bounds, the distance range of
//                       the map point, predictLevel, then findFeaturesInArea over the target's stored grid with the window
//                       [octave - 1, octave + 1], the vGoodIndices filter, getBestMatch and the acceptance test.
// k_sim3_search_points  one wave per loop-group map point (:501-549) against one stored keyframe: the same with the similarity applied to
//                       the world position, cv::norm in double, the viewing-angle test, no filter on the target's features.
// The projection is wave-uniform and every lane computes it; a point that fails a test writes -1 and its wave leaves.  No wave waits on
// another; every loop is bounded by a grid size or a feature count (area_search_body.h); a wave owns its point, so the results do not
// depend on the launch geometry.  Float arithmetic: map_point_dev.h's rows and `alpha A x + t`, its predictLevel; no contraction.
#include <hip/hip_runtime.h>

#include "area_search_body.h"
#include "map_point_dev.h"

#pragma clang fp contract(off)

namespace {

using namespace orbfe;

__device__ __forceinline__ AreaTarget target_of(const Sim3Kf& K) {
  return {K.desc, K.cell_off, K.cell_feat, K.rows, K.cols, K.clip_w, K.clip_h};
}

// the acceptance of :408-414: a non-empty list, best <= threshold and (float)best / (float)second <= ratio (0 / 0 is NaN: rejected)
__device__ __forceinline__ bool accepted(int total, const Best2& b, const Sim3SearchParams& P) {
  return total > 0 && b.min_d <= P.dist_threshold && (float)b.min_d / (float)b.second <= P.ratio;
}

__global__ __launch_bounds__(256) void k_sim3_search_pair(const uint8_t* __restrict__ up, Sim3Kf C, Sim3Kf M, Sim3SearchParams P,
                                                          int32_t* __restrict__ best_idx) {
  __shared__ int32_t stage_all[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long q = (long long)blockIdx.x * 4 + wv;
  if (q >= (long long)C.n + M.n) return;
  const bool dir_b = q >= C.n;
  const Sim3Kf& S = dir_b ? M : C;  // source
  const Sim3Kf& T = dir_b ? C : M;  // target
  const int i = (int)(dir_b ? q - C.n : q);
  int best = -1;
  do {
    // the source: named by no input match; A: a good point in the map (:448-452), B: a good point (:465-468)
    const int st = up[S.o_state + i];
    const int need = dir_b ? ORBFE_TRI_GOOD : (ORBFE_TRI_GOOD | ORBFE_TRI_INMAP);
    if ((st & SIM3S_NAMED) || (st & need) != need) break;
    const float* pos = (const float*)(up + S.o_pos) + 3 * (size_t)i;
    const float pw[3] = {pos[0], pos[1], pos[2]};
    float pc[3], pm[3];
    affine(1.0f, S.Rcw, pw, S.tcw, pc);
    affine(S.s, S.R, pc, S.t, pm);
    if (pm[2] <= 0.f) break;
    const float u = P.fx * (pm[0] / pm[2]) + P.cx, v = P.fy * (pm[1] / pm[2]) + P.cy;  // Camera::project (src/Camera.cc:14-22)
    if (!(u < S.bounds[1] && v < S.bounds[3] && u > S.bounds[0] && v > S.bounds[2])) break;  // mpCurr->isInImage: the SOURCE's bounds
    const float d = sqrtf(pm[0] * pm[0] + pm[1] * pm[1] + pm[2] * pm[2]) / S.s;
    const float mx = ((const float*)(up + S.o_max))[i], mn = ((const float*)(up + S.o_min))[i];
    if (!(d < mx && d > mn)) break;  // isGoodDistance
    const int o = predict_level(mx, d, P.log_sf, P.max_level);
    const float sf = ((const float*)(up + P.o_sf))[o];
    const uint4 a0 = *(const uint4*)(S.desc + (size_t)i * 32);
    const uint4 a1 = *(const uint4*)(S.desc + (size_t)i * 32 + 16);
    const uint8_t* __restrict__ t_state = up + T.o_state;
    Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
    const orbfe_keypoint* __restrict__ t_kps = T.kps;
    const int total = area_fold(target_of(T), u, v, P.th * (sf * sf), a0, a1, stage_all[wv], lane, b, [&](int id) {
      const int oc = t_kps[id].octave;
      return oc <= o + 1 && oc >= o - 1 &&
             (t_state[id] & (ORBFE_TRI_GOOD | ORBFE_TRI_INMAP)) == (ORBFE_TRI_GOOD | ORBFE_TRI_INMAP);  // vGoodIndices (:396-405)
    });
    if (accepted(total, b, P)) best = b.min_idx;
  } while (false);
  if (lane == 0) best_idx[q] = best;
}

__global__ __launch_bounds__(256) void k_sim3_search_points(const uint8_t* __restrict__ up, Sim3Kf T, Sim3Points L, Sim3SearchParams P,
                                                            int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist) {
  __shared__ int32_t stage_all[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long q = (long long)blockIdx.x * 4 + wv;
  if (q >= L.m) return;
  const size_t j = (size_t)q;
  int best = -1, dist = 0;
  do {
    if (!up[L.o_usable + j]) break;
    const float* pos = (const float*)(up + L.o_pos) + 3 * j;
    const float pw[3] = {pos[0], pos[1], pos[2]};
    float pc[3];
    affine(L.s, L.R, pw, L.t, pc);
    if (pc[2] <= 0.f) break;
    const float u = P.fx * (pc[0] / pc[2]) + P.cx, v = P.fy * (pc[1] / pc[2]) + P.cy;
    if (!(u < T.bounds[1] && v < T.bounds[3] && u > T.bounds[0] && v > T.bounds[2])) break;  // pCurr->isInImage
    const float d_with_s = (float)sqrt((double)pc[0] * (double)pc[0] + (double)pc[1] * (double)pc[1] + (double)pc[2] * (double)pc[2]);  // cv::norm
    const float d = d_with_s / L.s;
    const float mx = ((const float*)(up + L.o_max))[j], mn = ((const float*)(up + L.o_min))[j];
    if (!(d < mx && d > mn)) break;
    // the viewing angle (:534-536): (R * viewDirection) . p3dC >= 0.5 * |p3dC|, Mat::dot in double
    const float* vd = (const float*)(up + L.o_vdir) + 3 * j;
    const float vw[3] = {vd[0], vd[1], vd[2]};
    const float rv[3] = {mat3_row(L.R, 0, vw), mat3_row(L.R, 1, vw), mat3_row(L.R, 2, vw)};
    const double dot = (double)rv[0] * (double)pc[0] + (double)rv[1] * (double)pc[1] + (double)rv[2] * (double)pc[2];
    if (dot < 0.5 * (double)d_with_s) break;
    const int o = predict_level(mx, d, P.log_sf, P.max_level);
    const float sf = ((const float*)(up + P.o_sf))[o];
    const uint8_t* qd = up + L.o_desc + j * 32;
    const uint4 a0 = *(const uint4*)qd;
    const uint4 a1 = *(const uint4*)(qd + 16);
    Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
    const orbfe_keypoint* __restrict__ t_kps = T.kps;
    const int total = area_fold(target_of(T), u, v, P.th * (sf * sf), a0, a1, stage_all[wv], lane, b, [&](int id) {
      const int oc = t_kps[id].octave;
      return oc <= o + 1 && oc >= o - 1;
    });
    if (accepted(total, b, P)) best = b.min_idx, dist = b.min_d;
  } while (false);
  if (lane == 0) best_idx[q] = best, best_dist[q] = dist;
}

}  // namespace

void launch_sim3_search_pair(hipStream_t st, const uint8_t* up, const Sim3Kf& C, const Sim3Kf& M, const Sim3SearchParams& P, int32_t* best_idx) {
  const long long nq = (long long)C.n + M.n;
  if (nq <= 0) return;
  hipLaunchKernelGGL(k_sim3_search_pair, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, up, C, M, P, best_idx);
}

void launch_sim3_search_points(hipStream_t st, const uint8_t* up, const Sim3Kf& T, const Sim3Points& L, const Sim3SearchParams& P,
                               int32_t* best_idx, int32_t* best_dist) {
  if (L.m <= 0) return;
  hipLaunchKernelGGL(k_sim3_search_points, dim3((unsigned)(((long long)L.m + 3) / 4)), dim3(256), 0, st, up, T, L, P, best_idx, best_dist);
}

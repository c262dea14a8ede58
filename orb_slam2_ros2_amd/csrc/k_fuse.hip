// k_fuse.hip -- the inverse fuses of LocalMapping::fuseMapPoints (src/LocalMapping.cc:352-405) as one batch: for every target keyframe k
// and every feature i of the current keyframe, what ORBMatcher::fuse(pkf_k, cur, map) (src/ORBMatcher.cc:716-724) needs before its
// processFuseMps (:623-663).  searchByProjection(pkf_k, cur, matches, 3.0f, bFuse = true) (:265-347) projects nothing into pkf_k: it
// searches around cur's feature position with cur's descriptor, so (k, i) is a function of keyframe data alone; only
// MapPoint::isInVision(pkf_k) (src/MapPoint.cc:141-171) reads the map point of slot i.
//
// k_fuse_grid     one workgroup per target: VirtualFrame::initGrid (src/Frame.cc:53-69), the one grid build (area_grid_body.h) with the
//                 grid sized from the target's own bounds.
// k_fuse_visible  one thread per (k, i): isInVision (map_point_dev.h).
// k_fuse_search   one wave per (k, i): findFeaturesInArea (src/Frame.cc:286-311) + getBestMatch over the target's cell lists, the one
//                 area search (area_search_body.h) filtered by the octave window of the target's motion case, then the acceptance
//                 test of ORBMatcher.cc:339.
// No kernel waits on another workgroup; every loop is bounded by a feature count or a grid size; results do not depend on the launch
// geometry (a wave owns a query, a workgroup owns a target's grid, and the per-cell lists end up sorted).
#include <hip/hip_runtime.h>

#include "area_search_body.h"
#include "map_point_dev.h"
#include "orbfe_internal.h"

#pragma clang fp contract(off)

namespace {

using namespace orbfe;

// array `off` of a target: bytes behind `base`.  The stored form (orbfe_fuse_into_keyframes_stored) passes base = nullptr and the arrays'
// device addresses as offsets: a stored keyframe lies wherever its slab is (orbfe_kfstore.hip), and the kernels below are the same.
template <class T>
__device__ __forceinline__ T* at(const uint8_t* base, uint64_t off) {
  return (T*)((uintptr_t)base + off);
}

// cell_off[ncells + 1], cell_feat[n] (a cell's features in ascending index) of target blockIdx.x
__global__ __launch_bounds__(AREA_GRID_NT) void k_fuse_grid(uint8_t* __restrict__ base, const FuseKf* __restrict__ kfs) {
  extern __shared__ __attribute__((aligned(16))) int32_t l_grid[];  // (area_grid_body.h)
  __shared__ int32_t l_scan[AREA_GRID_NT];
  const FuseKf& K = kfs[blockIdx.x];
  area_grid_build(at<const orbfe_keypoint>(base, K.o_kps), K.n, K.rows, K.cols, K.in_lds, at<int32_t>(base, K.o_coff), at<int32_t>(base, K.o_cfeat),
                  l_grid, l_scan);
}

// MapPoint::isInVision(target k) for the point of slot i
__global__ __launch_bounds__(256) void k_fuse_visible(const FuseKf* __restrict__ kfs, FuseParams P, const uint8_t* __restrict__ has_point,
                                                      const float* __restrict__ pos, const float* __restrict__ vdir,
                                                      const float* __restrict__ max_dist, const float* __restrict__ min_dist,
                                                      uint8_t* __restrict__ visible) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long long)P.n_kf * P.n_cur) return;
  const int k = (int)(q / P.n_cur), i = (int)(q - (long long)k * P.n_cur);
  bool vis = false;
  if (has_point[i]) {
    const FuseKf& K = kfs[k];
    MapPointView w;
    vis = is_in_vision(K.R, K.t, pos + 3 * i, vdir + 3 * i, max_dist[i], min_dist[i], P.fx, P.fy, P.cx, P.cy, K.bounds, w);
  }
  visible[q] = vis ? 1 : 0;
}

// one wave per (k, i)
__global__ __launch_bounds__(256) void k_fuse_search(const uint8_t* __restrict__ base, const FuseKf* __restrict__ kfs, FuseParams P,
                                                     const orbfe_keypoint* __restrict__ q_kps, const uint8_t* __restrict__ q_desc,
                                                     const float* __restrict__ sf, int32_t* __restrict__ best_idx,
                                                     int32_t* __restrict__ best_dist) {
  __shared__ int32_t stage_all[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long q = (long long)blockIdx.x * 4 + wv;
  if (q >= (long long)P.n_kf * P.n_cur) return;
  const int k = (int)(q / P.n_cur), i = (int)(q - (long long)k * P.n_cur);
  const FuseKf& K = kfs[k];
  const orbfe_keypoint* __restrict__ kps = at<const orbfe_keypoint>(base, K.o_kps);
  const AreaTarget T = {at<const uint8_t>(base, K.o_desc), at<const int32_t>(base, K.o_coff), at<const int32_t>(base, K.o_cfeat), K.rows, K.cols,
                        K.clip_w, K.clip_h};
  const int mode = K.mode;
  const float x = q_kps[i].x, y = q_kps[i].y;
  const int oct = q_kps[i].octave;
  const float s = sf[oct];
  const float rad = P.th * (s * s);  // findFeaturesInArea: radius * getScaledFactor2(octave) (Frame.cc:289)
  const int lo = mode == 1 ? oct : (mode == 2 ? 0 : max(0, oct - 1));
  const int hi = mode == 1 ? 7 : (mode == 2 ? oct : min(oct + 1, 7));
  const uint4 a0 = *(const uint4*)(q_desc + (size_t)i * 32);
  const uint4 a1 = *(const uint4*)(q_desc + (size_t)i * 32 + 16);
  Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
  const int total = area_fold(T, x, y, rad, a0, a1, stage_all[wv], lane, b, [&](int id) {
    const int oc = kps[id].octave;
    return oc <= hi && oc >= lo;
  });
  if (lane == 0) {
    // ORBMatcher.cc:314-341: candidates, getBestMatch's ratio (float)best / (float)second (second = INT_MAX: ~0), the two thresholds
    const bool ok = total > 0 && (float)b.min_d / (float)b.second < P.ratio && b.min_d < P.dist_threshold;
    best_idx[q] = ok ? b.min_idx : -1;
    best_dist[q] = ok ? b.min_d : 0;
  }
}

}  // namespace

// build_grids false: the targets' grids are already there (stored keyframes)
void launch_fuse(hipStream_t st, uint8_t* base, const FuseKf* kfs, const FuseParams& P, size_t grid_lds, const orbfe_keypoint* q_kps,
                 const uint8_t* q_desc, const float* sf, const uint8_t* has_point, const float* pos, const float* vdir, const float* max_dist,
                 const float* min_dist, int32_t* best_idx, int32_t* best_dist, uint8_t* visible, bool build_grids) {
  const long long nq = (long long)P.n_kf * P.n_cur;
  if (nq <= 0) return;
  if (build_grids) hipLaunchKernelGGL(k_fuse_grid, dim3(P.n_kf), dim3(AREA_GRID_NT), grid_lds, st, base, kfs);
  hipLaunchKernelGGL(k_fuse_visible, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, kfs, P, has_point, pos, vdir, max_dist, min_dist, visible);
  hipLaunchKernelGGL(k_fuse_search, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, base, kfs, P, q_kps, q_desc, sf, best_idx, best_dist);
}

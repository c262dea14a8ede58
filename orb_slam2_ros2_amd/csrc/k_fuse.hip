// k_fuse.hip -- the inverse fuses of LocalMapping::fuseMapPoints (src/LocalMapping.cc:352-405) as one batch: for every target keyframe k
// and every feature i of the current keyframe, what ORBMatcher::fuse(pkf_k, cur, map) (src/ORBMatcher.cc:716-724) needs before its
// processFuseMps (:623-663).  searchByProjection(pkf_k, cur, matches, 3.0f, bFuse = true) (:265-347) projects nothing into pkf_k: it
// searches around cur's feature position with cur's descriptor, so (k, i) is a function of keyframe data alone; only
// MapPoint::isInVision(pkf_k) (src/MapPoint.cc:141-171) reads the map point of slot i.
//
// k_fuse_grid     one workgroup per target: VirtualFrame::initGrid (src/Frame.cc:53-69) -- the logic of k_guided.hip's k_grid_build with the
//                 grid sized from the target's own bounds.
// k_fuse_visible  one thread per (k, i): isInVision in the float / double mix of k_guided.hip's k_project_map_points.
// k_fuse_search   one wave per (k, i): findFeaturesInArea (src/Frame.cc:286-311) over the target's cell lists, rows outer / columns inner /
//                 index order inside a cell, the octave window of the target's motion case, getBestMatch's order-dependent fold
//                 (match_fold.h) 64 candidates at a time, then the acceptance test of ORBMatcher.cc:339.
// No kernel waits on another workgroup; every loop is bounded by a feature count or a grid size; results do not depend on the launch
// geometry (a wave owns a query, a workgroup owns a target's grid, and the per-cell lists end up sorted).
#include <hip/hip_runtime.h>

#include "fuse_grid_body.h"
#include "match_fold.h"
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
__global__ __launch_bounds__(FUSE_GRID_NT) void k_fuse_grid(uint8_t* __restrict__ base, const FuseKf* __restrict__ kfs) {
  extern __shared__ __attribute__((aligned(16))) int32_t l_grid[];  // (fuse_grid_body.h)
  __shared__ int32_t l_scan[FUSE_GRID_NT];
  const FuseKf& K = kfs[blockIdx.x];
  fuse_grid_build(at<const orbfe_keypoint>(base, K.o_kps), K.n, K.rows, K.cols, K.in_lds, at<int32_t>(base, K.o_coff), at<int32_t>(base, K.o_cfeat),
                  l_grid, l_scan);
}

// MapPoint::isInVision(target k) for the point of slot i: Rcw * X + tcw as float products summed left to right, then
// (float)((double)s + (double)t); cv::norm and Mat::dot accumulate in double.  The early exits keep the reference's order.
__global__ __launch_bounds__(256) void k_fuse_visible(const FuseKf* __restrict__ kfs, FuseParams P, const uint8_t* __restrict__ has_point,
                                                      const float* __restrict__ pos, const float* __restrict__ vdir,
                                                      const float* __restrict__ max_dist, const float* __restrict__ min_dist,
                                                      uint8_t* __restrict__ visible) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long long)P.n_kf * P.n_cur) return;
  const int k = (int)(q / P.n_cur), i = (int)(q - (long long)k * P.n_cur);
  uint8_t vis = 0;
  if (has_point[i]) {
    const FuseKf& K = kfs[k];
    const float X0 = pos[3 * i], X1 = pos[3 * i + 1], X2 = pos[3 * i + 2];
    const float s0 = K.R[0] * X0 + K.R[1] * X1 + K.R[2] * X2;
    const float s1 = K.R[3] * X0 + K.R[4] * X1 + K.R[5] * X2;
    const float s2 = K.R[6] * X0 + K.R[7] * X1 + K.R[8] * X2;
    const float x = (float)((double)s0 + (double)K.t[0]), y = (float)((double)s1 + (double)K.t[1]), zc = (float)((double)s2 + (double)K.t[2]);
    do {
      if (zc < 0.f) break;
      const float distance = sqrtf(x * x + y * y + zc * zc);
      if (!(distance < max_dist[i] && distance > min_dist[i])) break;  // isGoodDistance
      const float u = x / zc * P.fx + P.cx;
      const float v = y / zc * P.fy + P.cy;
      if (!(u < K.bounds[1] && v < K.bounds[3] && u > K.bounds[0] && v > K.bounds[2])) break;  // VirtualFrame::isInImage
      const float D0 = vdir[3 * i], D1 = vdir[3 * i + 1], D2 = vdir[3 * i + 2];
      const float v0 = K.R[0] * D0 + K.R[1] * D1 + K.R[2] * D2;
      const float v1 = K.R[3] * D0 + K.R[4] * D1 + K.R[5] * D2;
      const float v2 = K.R[6] * D0 + K.R[7] * D1 + K.R[8] * D2;
      const double nn = (double)v0 * (double)v0 + (double)v1 * (double)v1 + (double)v2 * (double)v2;
      const float vabs = (float)sqrt(nn);
      const double dot = (double)v0 * (double)x + (double)v1 * (double)y + (double)v2 * (double)zc;
      const float cos_theta = (float)(dot / (double)(distance * vabs));
      if (cos_theta < 0.5f) break;
      vis = 1;
    } while (false);
  }
  visible[q] = vis;
}

// one wave per (k, i); the candidates that pass the octave window wait in LDS until 64 of them make a chunk (order preserved)
__global__ __launch_bounds__(256) void k_fuse_search(const uint8_t* __restrict__ base, const FuseKf* __restrict__ kfs, FuseParams P,
                                                     const orbfe_keypoint* __restrict__ q_kps, const uint8_t* __restrict__ q_desc,
                                                     const float* __restrict__ sf, int32_t* __restrict__ best_idx,
                                                     int32_t* __restrict__ best_dist) {
  __shared__ int32_t stage_all[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int32_t* stage = stage_all[wv];
  const long long q = (long long)blockIdx.x * 4 + wv;
  if (q >= (long long)P.n_kf * P.n_cur) return;
  const int k = (int)(q / P.n_cur), i = (int)(q - (long long)k * P.n_cur);
  const FuseKf& K = kfs[k];
  const orbfe_keypoint* __restrict__ kps = at<const orbfe_keypoint>(base, K.o_kps);
  const uint8_t* __restrict__ desc = at<const uint8_t>(base, K.o_desc);
  const int32_t* __restrict__ cell_off = at<const int32_t>(base, K.o_coff);
  const int32_t* __restrict__ cell_feat = at<const int32_t>(base, K.o_cfeat);
  const int rows = K.rows, cols = K.cols, width = K.clip_w, height = K.clip_h, mode = K.mode;
  const float x = q_kps[i].x, y = q_kps[i].y;
  const int oct = q_kps[i].octave;
  const float s = sf[oct];
  const float rad = P.th * (s * s);  // findFeaturesInArea: radius * getScaledFactor2(octave) (Frame.cc:289)
  const int lo = mode == 1 ? oct : (mode == 2 ? 0 : max(0, oct - 1));
  const int hi = mode == 1 ? 7 : (mode == 2 ? oct : min(oct + 1, 7));
  const int min_x = max(0, __float2int_rn(x - rad)), max_x = min(width, __float2int_rn(x + rad));
  const int min_y = max(0, __float2int_rn(y - rad)), max_y = min(height, __float2int_rn(y + rad));
  const int c0 = max(0, min(cols - 1, cvfloor_f((float)min_x / (float)FUSE_GRID_W))), c1 = min(cols - 1, cvfloor_f((float)max_x / (float)FUSE_GRID_W));
  const int r0 = max(0, min(rows - 1, cvfloor_f((float)min_y / (float)FUSE_GRID_H))), r1 = min(rows - 1, cvfloor_f((float)max_y / (float)FUSE_GRID_H));
  const uint4 a0 = *(const uint4*)(q_desc + (size_t)i * 32);
  const uint4 a1 = *(const uint4*)(q_desc + (size_t)i * 32 + 16);
  Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
  int staged = 0, total = 0;
  auto flush = [&](int count) {  // stage[0 .. count) (count <= 64) as one chunk
    const int idx = (lane < count) ? stage[lane] : 0;
    const int d = (lane < count) ? hamming256(a0, a1, desc + (size_t)idx * 32) : ORB_INT_MAX;
    fold_chunk(b, d, idx, lane);
  };
  for (int r = r0; r <= r1; ++r)
    for (int c = c0; c <= c1; ++c) {
      const int beg = cell_off[r * cols + c], end = cell_off[r * cols + c + 1];
      for (int j0 = beg; j0 < end; j0 += 64) {
        const int j = j0 + lane;
        int id = 0;
        bool pass = false;
        if (j < end) {
          id = cell_feat[j];
          const int oc = kps[id].octave;
          pass = oc <= hi && oc >= lo;
        }
        const unsigned long long m = __ballot(pass);
        if (pass) stage[staged + __popcll(m & ((1ull << lane) - 1ull))] = id;
        staged += __popcll(m);
        total += __popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (staged >= 64) {
          flush(64);
          const int keep = (lane < staged - 64) ? stage[64 + lane] : 0;
          __builtin_amdgcn_wave_barrier();
          if (lane < staged - 64) stage[lane] = keep;
          staged -= 64;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  if (staged > 0) flush(staged);
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
  if (build_grids) hipLaunchKernelGGL(k_fuse_grid, dim3(P.n_kf), dim3(FUSE_GRID_NT), grid_lds, st, base, kfs);
  hipLaunchKernelGGL(k_fuse_visible, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, kfs, P, has_point, pos, vdir, max_dist, min_dist, visible);
  hipLaunchKernelGGL(k_fuse_search, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, base, kfs, P, q_kps, q_desc, sf, best_idx, best_dist);
}

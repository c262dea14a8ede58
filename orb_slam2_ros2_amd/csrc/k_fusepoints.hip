// k_fusepoints.hip -- the forward fuse ORBMatcher::fuse(pkf, mapPoints, map, bLoop, th) (src/ORBMatcher.cc:682-707) of m map points into
// n_kf stored keyframes: for every pair (k, j) what searchByProjection(pkf_k, {point j}, th, matches, bFuse = true)
// (:573-609) would put in its DMatch.  A loop group is visible to a given keyframe only in part, so the pairs are projected by threads
// and only the survivors get a wave:
//
// k_fusepts_project  one thread per (k, j): usable, MapPoint::isInVision on keyframe k's pose and STORED bounds, predictLevel
//                    (map_point_dev.h).  A failing pair writes its own (-1, 0).  A surviving pair is appended to the work list with what
//                    the projection found (u, v, level, cosTheta): ballot and prefix within the wave, ONE atomic add per wave.  The list
//                    holds n_kf * m entries, so it cannot overflow.
// k_fusepts_search   one wave per list entry, a fixed grid striding over min(count, capacity): radius and octave window (:579-582),
//                    findFeaturesInArea over the keyframe's stored grid + getBestMatch (area_search_body.h), the acceptance test of :591.
//                    Lane 0 writes the pair's (best_idx, best_dist).
// Every output element is written exactly once, by exactly one of the two kernels.  The list's order varies between runs; an entry names
// its pair and its wave writes only that pair's element, so the order shows in no output.  No wave waits on another; every loop is bounded
// by the count, the grid size or a cell's feature count.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "area_search_body.h"
#include "map_point_dev.h"
#include "orbfe_internal.h"

#pragma clang fp contract(off)

namespace {

using namespace orbfe;

__global__ __launch_bounds__(256) void k_fusepts_project(const FusePtsKf* __restrict__ kfs, FusePtsParams P, FusePtsEntry* __restrict__ list,
                                                         uint32_t* __restrict__ count, int32_t* __restrict__ best_idx,
                                                         int32_t* __restrict__ best_dist) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)P.n_kf * P.m;
  const int lane = threadIdx.x & 63;
  bool keep = false;
  FusePtsEntry e = {0, 0, 0, 0.f, 0.f, 0.f};
  if (q < total) {
    const int k = (int)(q / P.m), j = (int)(q - (long long)k * P.m);
    if (P.usable[j]) {
      const FusePtsKf& K = kfs[k];
      const float mx = P.max_dist[j], mn = P.min_dist[j];
      MapPointView w;
      if (is_in_vision(K.R, K.t, P.pos + 3 * (size_t)j, P.vdir + 3 * (size_t)j, mx, mn, P.fx, P.fy, P.cx, P.cy, K.bounds, w)) {
        keep = true;
        e.k = k, e.j = j, e.o = predict_level(mx, w.distance, P.log_sf, P.max_level);
        e.u = w.u, e.v = w.v, e.cos_theta = w.cos_theta;
      }
    }
    if (!keep) best_idx[q] = -1, best_dist[q] = 0;
  }
  // every lane of the wave is here (none has left): the survivors' slots are one reservation
  const unsigned long long mask = __ballot(keep);
  const int n_keep = __popcll(mask);
  if (n_keep == 0) return;
  uint32_t first = 0;
  if (lane == 0) first = atomicAdd(count, (uint32_t)n_keep);
  first = __shfl(first, 0);
  if (keep) list[(size_t)first + (size_t)__popcll(mask & ((1ull << lane) - 1ull))] = e;
}

__global__ __launch_bounds__(256) void k_fusepts_search(const FusePtsKf* __restrict__ kfs, FusePtsParams P, const FusePtsEntry* __restrict__ list,
                                                        const uint32_t* __restrict__ count, int32_t* __restrict__ best_idx,
                                                        int32_t* __restrict__ best_dist) {
  __shared__ int32_t stage_all[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long capacity = (long long)P.n_kf * P.m;
  const long long n = min((long long)*count, capacity);  // read once; the launch before this one has finished
  const long long n_waves = (long long)gridDim.x * 4;
  for (long long w = (long long)blockIdx.x * 4 + wv; w < n; w += n_waves) {
    const FusePtsEntry e = list[w];
    // (an entry the projection cannot have written is skipped: no address is formed from it)
    if (e.k < 0 || e.k >= P.n_kf || e.j < 0 || e.j >= P.m || e.o < 0 || e.o > P.max_level) continue;
    const FusePtsKf& K = kfs[e.k];
    const int o = e.o;
    const float s = P.sf[o];
    const float rad = ((e.cos_theta > 0.998f ? 2.5f : 4.0f) * P.th) * (s * s);  // :579-581 and findFeaturesInArea's getScaledFactor2
    const int lo = max(0, o - 1), hi = min(P.n_levels - 1, o + 1);               // :582
    const uint8_t* qd = P.desc + (size_t)e.j * 32;
    const uint4 a0 = *(const uint4*)qd;
    const uint4 a1 = *(const uint4*)(qd + 16);
    const AreaTarget T = {K.desc, K.cell_off, K.cell_feat, K.rows, K.cols, K.clip_w, K.clip_h};
    const orbfe_keypoint* __restrict__ kps = K.kps;
    Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
    const int total = area_fold(T, e.u, e.v, rad, a0, a1, stage_all[wv], lane, b, [&](int id) {
      const int oc = kps[id].octave;
      return oc <= hi && oc >= lo;
    });
    if (lane == 0) {
      // :591: bestMatch.first != -1 && best < threshold && ratio < mfRatio, getBestMatch's ratio (float)best / (float)second
      const bool ok = total > 0 && b.min_d < P.dist_threshold && (float)b.min_d / (float)b.second < P.ratio;
      const size_t at = (size_t)e.k * (size_t)P.m + (size_t)e.j;
      best_idx[at] = ok ? b.min_idx : -1;
      best_dist[at] = ok ? b.min_d : 0;
    }
    __builtin_amdgcn_wave_barrier();  // the next entry's candidates go into the same LDS words
  }
}

}  // namespace

void launch_fuse_points(hipStream_t st, const FusePtsKf* kfs, const FusePtsParams& P, FusePtsEntry* list, uint32_t* count, int32_t* best_idx,
                        int32_t* best_dist, hipEvent_t between) {
  const long long nq = (long long)P.n_kf * P.m;
  if (nq <= 0) return;
  hipLaunchKernelGGL(k_fusepts_project, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, kfs, P, list, count, best_idx, best_dist);
  if (between) (void)hipEventRecord(between, st);  // (a profiled call times the two kernels apart)
  const long long blocks = std::min<long long>((nq + 3) / 4, FUSEPTS_SEARCH_BLOCKS);
  hipLaunchKernelGGL(k_fusepts_search, dim3((unsigned)blocks), dim3(256), 0, st, kfs, P, list, count, best_idx, best_dist);
}

// k_guided.hip -- grid-guided descriptor matching against the device-resident features of one image slot.
//
// Replaces VirtualFrame::initGrid (src/ORB_SLAM2/src/Frame.cc:53-69) + VirtualFrame::findFeaturesInArea (:286-311) +
// ORBMatcher::getBestMatch (src/ORBMatcher.cc:967-990) as used by the guided searches (searchByProjection frame-to-frame
// ORBMatcher.cc:265-347, map points to frame :561-612): candidates of a query = the features of the 64x48-px grid cells that
// overlap its search box, rows outer / columns inner / index order inside a cell, filtered by octave range and an exclusion
// mask, scanned with the reference's order-dependent best / second-best rule.  SURVEY 8f, row f1.
// The kernels here are thin: the grid build is area_grid_body.h, the area loop and the fold area_search_body.h (this file's filter: the
// octave of the packed record, then the exclusion mask and its hit counts), isInVision / predictLevel map_point_dev.h, the pose-only
// edge list of the tracking chain pose_check_dev.h (k_track_edges says what a feature holds and counts the matches).
#include <hip/hip_runtime.h>

#include "area_search_body.h"
#include "map_point_dev.h"
#include "orbfe_internal.h"
#include "pose_check_dev.h"
#include "search_area_layout.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace orbfe {

// grid build: one workgroup per call (area_grid_body.h).  cell_off[ncells+1], cell_feat[n] (features of a cell in ascending index).
__global__ __launch_bounds__(AREA_GRID_NT) void k_grid_build(const orbfe_keypoint* __restrict__ kps, const int32_t* __restrict__ n_kp_ptr,
                                                             int rows, int cols, int feat_in_lds, int32_t* __restrict__ cell_off,
                                                             int32_t* __restrict__ cell_feat) {
  extern __shared__ int32_t l_grid[];
  __shared__ int32_t l_scan[AREA_GRID_NT];
  area_grid_build(kps, *n_kp_ptr, rows, cols, feat_in_lds, cell_off, cell_feat, l_grid, l_scan);
}

// search: one wave per query (area_search_body.h).  A candidate's octave is byte 0 of word 1 of its packed record.
__global__ __launch_bounds__(256) void k_search_area(const uint4* __restrict__ kpl, const uint8_t* __restrict__ desc, int width,
                                                     int height, int rows, int cols, const int32_t* __restrict__ cell_off,
                                                     const int32_t* __restrict__ cell_feat, int nq, const float* __restrict__ qxy,
                                                     const float* __restrict__ radius, const int8_t* __restrict__ min_level,
                                                     const int8_t* __restrict__ max_level, const uint8_t* __restrict__ q_desc,
                                                     const uint8_t* __restrict__ exclude, int32_t* __restrict__ best_idx,
                                                     int32_t* __restrict__ best_dist, int32_t* __restrict__ second_dist,
                                                     int32_t* __restrict__ n_cand, int32_t* __restrict__ excluded_hits) {
  __shared__ int32_t stage_all[4][128];  // per wave: filtered candidates waiting to fill a 64-lane chunk (order preserved)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wv;
  if (q >= nq) return;
  const float x = qxy[2 * q], y = qxy[2 * q + 1], rad = radius[q];
  if (rad < 0.f) {  // (the tracking chain marks a map point that takes no part in the search this way)
    if (lane == 0) n_cand[q] = 0, best_idx[q] = -1, best_dist[q] = ORB_INT_MAX, second_dist[q] = ORB_INT_MAX;
    return;
  }
  const int lo = min_level[q], hi = max_level[q];
  const uint4 a0 = *(const uint4*)(q_desc + (size_t)q * 32);
  const uint4 a1 = *(const uint4*)(q_desc + (size_t)q * 32 + 16);
  Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
  const AreaTarget T = {desc, cell_off, cell_feat, rows, cols, width, height};
  const int total = area_fold(T, x, y, rad, a0, a1, stage_all[wv], lane, b, [&](int id) {
    const int oc = (int)(kpl[id].y & 0xFFu);
    if (!(oc <= hi && oc >= lo)) return false;
    if (exclude && exclude[id]) {
      // a feature the caller excluded WAS in this query's window: searchByProjection bumps MapPoint::addMatchInTrack once per such
      // (query, feature) occurrence while it filters the candidates (src/ORBMatcher.cc:321-331) -- the counts let the caller do the same
      if (excluded_hits) atomicAdd(&excluded_hits[id], 1);
      return false;
    }
    return true;
  });
  if (lane == 0) {
    n_cand[q] = total;
    best_idx[q] = total ? b.min_idx : -1;
    best_dist[q] = b.min_d;
    second_dist[q] = b.second;
  }
}

// ---------------------------------------------------------------------------------------------
// MapPoint::isInVision + MapPoint::predictLevel (src/MapPoint.cc:141-201) for n map points against one frame: what
// ORBMatcher::searchByProjection(frame, mapPoints) evaluates per point before the area search (src/ORBMatcher.cc:575-580).
// One thread per map point over map_point_dev.h (the float / double mix and the order of the tests are stated there); a point that
// fails leaves visible = 0, level = 0 and the values its tests got to.
// ---------------------------------------------------------------------------------------------
struct ProjectParams {
  float R[9], t[3];
  float fx, fy, cx, cy;
  float bounds[4];  // min_u, max_u, min_v, max_v
  float log_sf;     // std::log(ORBExtractor::mfScaledFactor) as float
  int max_level;
};

__global__ __launch_bounds__(256) void k_project_map_points(int n, const float* __restrict__ pos, const float* __restrict__ vdir,
                                                            const float* __restrict__ max_dist, const float* __restrict__ min_dist,
                                                            ProjectParams P, float* __restrict__ uv, float* __restrict__ dist_out,
                                                            float* __restrict__ cos_out, int8_t* __restrict__ level_out,
                                                            uint8_t* __restrict__ visible) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  MapPointView w;
  const bool vis = is_in_vision(P.R, P.t, pos + 3 * i, vdir + 3 * i, max_dist[i], min_dist[i], P.fx, P.fy, P.cx, P.cy, P.bounds, w);
  uv[2 * i] = w.u, uv[2 * i + 1] = w.v;
  dist_out[i] = w.distance, cos_out[i] = w.cos_theta;
  level_out[i] = (int8_t)(vis ? predict_level(max_dist[i], w.distance, P.log_sf, P.max_level) : 0);  // ([0, 7] in the reference)
  visible[i] = vis ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// The tracking chain (Tracking::trackLocalMap, src/Tracking.cc:641-675): ORBMatcher::searchByProjection(frame, map points, th)
// (src/ORBMatcher.cc:561-612) -> Optimizer::OptimizePoseOnly(frame) (src/Optimizer.cc:33-178) with every intermediate on the device.
// k_track_queries: per map point, the search window the reference derives from isInVision / predictLevel (:575-582).
// k_track_claim / k_track_edges: the reference assigns in map-point order -- a feature that holds a (good) map point keeps it, a free
// feature goes to the FIRST map point whose best match it is (later ones find it taken): the minimum map-point index per feature,
// an atomicMin.  The pose-only edges are the features that hold a good map point afterwards, in feature order (Optimizer.cc:59-118).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_track_queries(int n, const uint8_t* __restrict__ mp_flags, const uint8_t* __restrict__ visible,
                                                       const float* __restrict__ cos_theta, const int8_t* __restrict__ level, float th,
                                                       const float* __restrict__ level_sigma2, int n_levels, float* __restrict__ radius,
                                                       int8_t* __restrict__ min_level, int8_t* __restrict__ max_level) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r = -1.f;
  int lo = 0, hi = 0;
  if ((mp_flags[i] & 5) == 5 && visible[i]) {  // in the search list, !isBad, isInMap (ORBMatcher.cc:575-576)
    const int oc = level[i];
    const float base = cos_theta[i] > 0.998f ? 2.5f : 4.0f;
    r = (base * th) * level_sigma2[oc];  // findFeaturesInArea(kp, radius * th, ..): radius * getScaledFactor2(octave) (Frame.cc:289)
    lo = max(0, oc - 1), hi = min(n_levels - 1, oc + 1);
  }
  radius[i] = r;
  min_level[i] = (int8_t)lo, max_level[i] = (int8_t)hi;
}

__global__ __launch_bounds__(256) void k_track_claim(int n, const int32_t* __restrict__ n_cand, const int32_t* __restrict__ best_idx,
                                                     const int32_t* __restrict__ best_dist, const int32_t* __restrict__ second_dist,
                                                     int min_threshold, float ratio, int32_t* __restrict__ claim, int last_wins,
                                                     int32_t* __restrict__ n_accept, uint8_t* __restrict__ accepted) {
  // last_wins (the frame <- frame search, ORBMatcher.cc:265-347): every accepted query is a match and setMapPoints assigns them in query
  // order (:815-830) -- the LAST query that picked a feature keeps it (atomicMax over claims that start at -1), and the return value counts
  // the accepted queries (n_accept), not the features
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || n_cand[i] <= 0) return;
  const float fr = (float)best_dist[i] / (float)second_dist[i];  // getBestMatch's ratio (ORBMatcher.cc:988); second = INT_MAX -> ~0
  if (best_dist[i] < min_threshold && fr < ratio) {
    if (last_wins) {
      atomicMax(&claim[best_idx[i]], i);
      atomicAdd(n_accept, 1);
      if (accepted) accepted[i] = 1;  // (setMapPoints calls addMatchInTrack for every match, kept or overwritten: the caller needs them all)
    } else
      atomicMin(&claim[best_idx[i]], i);
  }
}

// One workgroup: final assignment per feature, the reference's match count, and the pose-only edge list in feature order.
// held[f]: map point the feature holds on entry (-1 none); mp_flags bit 0: !isBad && isInMap (the occupancy test, ORBMatcher.cc:595, and
// the search loop's own filter, :575), bit 1: !isBad (the initial count, :566-571, and the edge test, Optimizer.cc:64), bit 2: member of
// the list searchByProjection walks.
// The edge list itself is pose_check_dev.h's pose_edges_1024 (of F only the frame view is read: no pose, no camera).
__global__ __launch_bounds__(1024) void k_track_edges(PoseFrameDev F, PoseEdgesDev E, const int32_t* __restrict__ held,
                                                      const int32_t* __restrict__ claim, const uint8_t* __restrict__ mp_flags,
                                                      const float* __restrict__ mp_pos, int min_matches, int32_t* __restrict__ assigned,
                                                      int32_t* __restrict__ counts /*[0] n_matches, [1] n_edges (-1: below min_matches)*/,
                                                      int32_t unclaimed, const int32_t* __restrict__ n_accept, int base_matches) {
  // unclaimed: the value a claim starts with (0x7F7F7F7F under atomicMin, -1 under atomicMax).  n_accept (nullable, the frame <- frame
  // search): the matches of this pass are the accepted queries counted there, on top of base_matches from an earlier pass
  __shared__ int s_wave[16], s_match[16];
  __shared__ int s_base;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n_kp = min(*F.n_kp, F.nf);
  int my_matches = 0;  // this thread's features: one for a good point held on entry, one for a claim taken
  const int edges = pose_edges_1024(F, E, s_wave, &s_base, [&](int f) -> const float* {
    int mp = -1;
    if (f < n_kp) {
      const int h = held ? held[f] : -1;
      if (h >= 0 && (mp_flags[h] & 2)) ++my_matches;  // `if (pMp && !pMp->isBad()) ++nMatches` (ORBMatcher.cc:566-571)
      mp = h;
      const int cl = claim[f];
      if (cl != unclaimed && !(h >= 0 && (mp_flags[h] & 1))) mp = cl, ++my_matches;  // setMapPoint + ++nMatches (:595-599)
    }
    assigned[f] = mp;
    return mp >= 0 && (mp_flags[mp] & 2) ? mp_pos + 3 * mp : nullptr;
  });
  my_matches = wave_reduce_dpp<OpAddI>(my_matches);
  if (lane == 0) s_match[wv] = my_matches;
  __syncthreads();
  if (t == 0) {
    int total_matches = 0;
    for (int w = 0; w < 16; ++w) total_matches += s_match[w];
    if (n_accept) total_matches = base_matches + *n_accept;
    counts[0] = total_matches;
    counts[1] = total_matches < min_matches ? -1 : edges;  // Tracking::trackLocalMap returns before the optimisation (Tracking.cc:656-657)
  }
}

void launch_track_queries(hipStream_t s, int n, const uint8_t* d_flags, const uint8_t* d_visible, const float* d_cos, const int8_t* d_level, float th,
                          const float* d_sigma2, int n_levels, float* d_radius, int8_t* d_min_level, int8_t* d_max_level) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_track_queries, dim3((n + 255) / 256), dim3(256), 0, s, n, d_flags, d_visible, d_cos, d_level, th, d_sigma2, n_levels, d_radius,
                     d_min_level, d_max_level);
}
void launch_track_claim(hipStream_t s, int n, const int32_t* d_n_cand, const int32_t* d_best_idx, const int32_t* d_best_dist, const int32_t* d_second,
                        int min_threshold, float ratio, int32_t* d_claim, int last_wins, int32_t* d_n_accept, uint8_t* d_accepted) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_track_claim, dim3((n + 255) / 256), dim3(256), 0, s, n, d_n_cand, d_best_idx, d_best_dist, d_second, min_threshold, ratio, d_claim,
                     last_wins, d_n_accept, d_accepted);
}
void launch_track_edges(hipStream_t s, const PoseFrameDev& F, const PoseEdgesDev& E, const int32_t* d_held, const int32_t* d_claim,
                        const uint8_t* d_mp_flags, const float* d_mp_pos, int min_matches, int32_t* d_assigned, int32_t* d_counts, int32_t unclaimed,
                        const int32_t* d_n_accept, int base_matches) {
  hipLaunchKernelGGL(k_track_edges, dim3(1), dim3(1024), 0, s, F, E, d_held, d_claim, d_mp_flags, d_mp_pos, min_matches, d_assigned, d_counts,
                     unclaimed, d_n_accept, base_matches);
}

void launch_project_map_points(hipStream_t s, int n, const float* d_pos, const float* d_vdir, const float* d_max, const float* d_min,
                               const float* R, const float* t, const float* cam4, const float* bounds4, float log_sf, int max_level,
                               float* d_uv, float* d_dist, float* d_cos, int8_t* d_level, uint8_t* d_vis) {
  if (n <= 0) return;
  ProjectParams P;
  for (int k = 0; k < 9; ++k) P.R[k] = R[k];
  for (int k = 0; k < 3; ++k) P.t[k] = t[k];
  P.fx = cam4[0], P.fy = cam4[1], P.cx = cam4[2], P.cy = cam4[3];
  for (int k = 0; k < 4; ++k) P.bounds[k] = bounds4[k];
  P.log_sf = log_sf, P.max_level = max_level;
  hipLaunchKernelGGL(k_project_map_points, dim3((n + 255) / 256), dim3(256), 0, s, n, d_pos, d_vdir, d_max, d_min, P, d_uv, d_dist, d_cos,
                     d_level, d_vis);
}

void launch_grid_build(hipStream_t s, const orbfe_keypoint* d_kps, const int32_t* d_n_kp, int n_cap, int rows, int cols,
                       int32_t* d_cell_off, int32_t* d_cell_feat) {
  // n_cap: upper bound of *d_n_kp; the cells' lists are filled and ordered in LDS when they fit there (the callers refuse a grid
  // whose counters do not)
  const AreaGridLds g = area_grid_lds((size_t)rows * cols, (size_t)n_cap);
  hipLaunchKernelGGL(k_grid_build, dim3(1), dim3(AREA_GRID_NT), g.bytes, s, d_kps, d_n_kp, rows, cols, g.in_lds, d_cell_off, d_cell_feat);
}

void launch_search_area(hipStream_t s, const uint4* d_kpl, const uint8_t* d_desc, int width, int height, int rows, int cols,
                        const int32_t* d_cell_off, const int32_t* d_cell_feat, int nq, const float* d_qxy, const float* d_radius,
                        const int8_t* d_min_level, const int8_t* d_max_level, const uint8_t* d_q_desc, const uint8_t* d_exclude,
                        int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second, int32_t* d_n_cand, int32_t* d_excluded_hits) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(k_search_area, dim3((nq + 3) / 4), dim3(256), 0, s, d_kpl, d_desc, width, height, rows, cols, d_cell_off,
                     d_cell_feat, nq, d_qxy, d_radius, d_min_level, d_max_level, d_q_desc, d_exclude, d_best_idx, d_best_dist, d_second,
                     d_n_cand, d_excluded_hits);
}

}  // namespace orbfe

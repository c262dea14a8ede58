// k_motion.hip -- the glue of orbfe_track_motion_model_slots (include/orbfe.h): what Tracking::trackMotionModel
// (src/Tracking.cc:381-406) does around its two ORBMatcher::searchByProjection(frame, lastFrame) calls and Optimizer::OptimizePoseOnly, on
// the device.  The searches are k_guided.hip's launch_search_area / launch_track_claim, the edge list its launch_track_edges, the
// optimisation k_pose.hip's launch_pose_only; this file prepares their inputs from the two slots and closes the call.
//
// k_motion_prep    one thread per last-frame feature: Frame::unProject (src/Frame.cc:179-202, :262-275) where the feature holds no good
//                  point and has depth -- a temporary point --, the position of a good point from the map-point store's row (or the
//                  uploaded array), the motion direction and the octave window (ORBMatcher.cc:270-313: pose_check_dev.h's form, the
//                  relocalisation refine's), the query of the feature for the first search.  A feature that is no query gets radius -1.
//                  Thread 0: Converter::ConvertTcw2SE3 of the predicted pose, the optimisation's seed.
// k_motion_between one workgroup, between the searches: the decision of Tracking.cc:388 on the accepted-query counter; the radii of the
//                  second search (-1 for every query when it is not wanted: its kernels then leave at once) and the features the first
//                  search assigned, which the second drops as candidates and counts (ORBMatcher.cc:321-331).
// k_motion_check   one workgroup: query_matches, the :392 decision as k_track_edges left it (edge count -1), pose_check_dev.h's
//                  post-check with the pose the frame still has, Converter::ConvertSE32Tcw and the write-back, the isInMap count of
//                  :397-404, the verdict.
// No kernel waits on another; every loop is bounded by the feature capacity.  Float arithmetic: map_point_dev.h's rows and `A x + t`, no
// contraction; the conversions in fp64.
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"
#include "orbfe_mpstore.h"
#include "pose_check_dev.h"

#pragma clang fp contract(off)

namespace orbfe {
namespace {

__global__ __launch_bounds__(256) void k_motion_prep(MotionDev P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) tcw_to_se3_dev(P.F.R0, P.F.t0, P.p_init);
  if (i >= P.F.nf) return;
  const int n_last = min(max(*P.l_n_kp, 0), P.F.nf);
  const bool valid = i < n_last;
  orbfe_keypoint kp = {};
  if (valid) kp = P.l_kps[i];
  float X[3] = {0.f, 0.f, 0.f};
  bool good = valid && (P.l_flags[i] & 1);
  bool temp = false;
  if (good) {  // `pMp && !pMp->isBad()`: the point stays (Frame.cc:187-191)
    if (P.table) {
      const MpTable T = {(uint8_t* const*)P.table, P.rows_per_page, P.max_pages};
      uint8_t* pres = nullptr;
      const uint8_t* row = mp_row(T, P.l_ids[i], &pres);
      if (row && *pres) {
        const float* p = (const float*)row;
        X[0] = p[0], X[1] = p[1], X[2] = p[2];
      } else {
        good = false;  // no query; the host names the id after the download
        *P.bad = 1u;   // (every thread that finds one stores the same value)
      }
    } else
      X[0] = P.l_pos[3 * i], X[1] = P.l_pos[3 * i + 1], X[2] = P.l_pos[3 * i + 2];
  } else if (valid && P.l_depth) {
    const double depth = P.l_depth[i];
    if (depth >= 0) {  // VirtualFrame::unProject (Frame.cc:262-275), then mRwc * p3dC + mtwc (:195)
      const float x = (kp.x - P.F.cx) / P.F.fx, y = (kp.y - P.F.cy) / P.F.fy;
      const float pc[3] = {(float)(depth * (double)x), (float)(depth * (double)y), (float)depth};
      affine(1.0f, P.lRwc, pc, P.ltwc, X);
      temp = true;
    }
  }
  const bool query = good || temp;
  const int o = min(max(kp.octave, 0), P.F.n_levels - 1);
  int lo, hi;
  motion_window(o, tlc_z_dev(P.F.R0, P.F.t0, P.lR, P.lt), P.baseline, lo, hi);
  P.qxy[2 * i] = kp.x, P.qxy[2 * i + 1] = kp.y;
  P.rad1[i] = query ? P.th * P.F.sigma2[o] : -1.f;  // findFeaturesInArea: radius * getScaledFactor2(octave) (Frame.cc:289)
  P.lo[i] = (int8_t)lo, P.hi[i] = (int8_t)hi;
  P.q_pos[3 * i] = X[0], P.q_pos[3 * i + 1] = X[1], P.q_pos[3 * i + 2] = X[2];
  P.q_flags[i] = query ? 3 : 0;  // k_track_edges' flags: every query is a good point
  P.temp[i] = temp ? 1 : 0;
  P.temp_pos[3 * i] = temp ? X[0] : 0.f, P.temp_pos[3 * i + 1] = temp ? X[1] : 0.f, P.temp_pos[3 * i + 2] = temp ? X[2] : 0.f;
}

__global__ __launch_bounds__(1024) void k_motion_between(MotionDev P) {
  const int t = threadIdx.x;
  const bool second = *P.n_accept < P.min_matches && P.th_second > 0.f;  // Tracking.cc:388 (uniform over the workgroup)
  for (int i = t; i < P.F.nf; i += 1024) {
    float r = -1.f;
    if (second && P.q_flags[i]) {
      const int o = min(max(P.l_kps[i].octave, 0), P.F.n_levels - 1);
      r = P.th_second * P.F.sigma2[o];
    }
    P.rad2[i] = r;
    P.ex2[i] = P.claim1[i] >= 0 ? 1 : 0;  // the feature holds a point of the first search: no candidate of the second (:321-331)
  }
  if (t == 0) P.hdr[MOTION_H_PASSES] = second ? 2 : 1;
}

__global__ __launch_bounds__(1024) void k_motion_check(MotionDev P) {
  __shared__ int s_wave[16], s_map[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int edges = P.cnt[1];
  for (int f = t; f < P.F.nf; f += 1024) {
    P.qm[f] = (int)P.qa1[f] + (int)P.qa2[f];  // setMapPoints' addMatchInTrack: once per accepted query and search
    P.cur[f] = P.assigned[f];
  }
  if (edges < 0) {  // Tracking.cc:392: both frames are written, nothing is optimised
    if (t == 0) P.hdr[MOTION_H_MATCHES] = P.cnt[0], P.hdr[MOTION_H_VERDICT] = ORBFE_MOTION_REJECT_MATCHES;
    return;
  }
  float R[9], tc[3];
  se3_to_tcw_dev(P.p_opt, R, tc);
  const int n_in = post_check_1024(  // (the pose the frame still has is the predicted one)
      P.F, P.F.R0, P.F.t0, P.E, P.inlier, s_wave,
      [&](int f, float (&X)[3]) {
        const int a = P.assigned[f];
        X[0] = P.q_pos[3 * a], X[1] = P.q_pos[3 * a + 1], X[2] = P.q_pos[3 * a + 2];
      },
      [&](int f) { P.cur[f] = -1; });  // (a thread drops the cur[f] it wrote above)
  // `if (pMp && pMp->isInMap()) ++inLiers` over what the frame holds now (Tracking.cc:397-404); a temporary point is not in the map
  int mine = 0;
  for (int f0 = 0; f0 < P.F.nf; f0 += 1024) {
    const int f = f0 + t;
    bool in_map = false;
    if (f < P.F.nf) {
      const int a = P.cur[f];
      in_map = a >= 0 && (P.l_flags[a] & 3) == 3;
    }
    mine += __popcll(__ballot(in_map));
  }
  if (lane == 0) s_map[wv] = mine;
  __syncthreads();
  if (t != 0) return;
  int n_map = 0;
  for (int w = 0; w < 16; ++w) n_map += s_map[w];
  P.hdr[MOTION_H_MATCHES] = P.cnt[0];
  P.hdr[MOTION_H_EDGES] = edges;
  P.hdr[MOTION_H_INLIERS] = n_in;
  P.hdr[MOTION_H_INMAP] = n_map;
  pose_write_back(P.p_opt, R, tc, P.pose_out, P.tcw_out);
  P.hdr[MOTION_H_VERDICT] = n_map >= P.min_inliers ? ORBFE_MOTION_ACCEPT : ORBFE_MOTION_REJECT_INLIERS;  // Tracking.cc:405
}

}  // namespace

void launch_motion_prep(hipStream_t st, const MotionDev& P) {
  hipLaunchKernelGGL(k_motion_prep, dim3((unsigned)((P.F.nf + 255) / 256)), dim3(256), 0, st, P);
}
void launch_motion_between(hipStream_t st, const MotionDev& P) { hipLaunchKernelGGL(k_motion_between, dim3(1), dim3(1024), 0, st, P); }
void launch_motion_check(hipStream_t st, const MotionDev& P) { hipLaunchKernelGGL(k_motion_check, dim3(1), dim3(1024), 0, st, P); }

}  // namespace orbfe

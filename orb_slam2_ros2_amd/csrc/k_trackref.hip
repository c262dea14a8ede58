// k_trackref.hip -- the glue of orbfe_track_reference_stored (include/orbfe.h): what Tracking::trackReference
// (src/Tracking.cc:360-371) does between ORBMatcher::searchByBow's match list and its verdict, on the device.  The list is k_bowsearch.hip's
// (k_bow_match on the slot, k_bow_select for one candidate), the optimisation k_pose.hip's launch_pose_only on the edge list built here.
//
// k_trackref_seed    one workgroup: setMapPoints over the list in match order (ORBMatcher.cc:815-830; in TRACK mode a train is always good,
//                    so the nulling branch cannot fire) as a maximum of the match index per frame feature -- the last match that names a
//                    feature keeps it --, the :365 decision, the edge list of Optimizer::OptimizePoseOnly in feature order
//                    (Optimizer.cc:58-117) over the points the frame came with and the assigned ones, Converter::ConvertTcw2SE3 of the
//                    frame's pose (:119).  The edge list is pose_check_dev.h's pose_edges_1024; this kernel says what a feature holds.
// k_trackref_check   one workgroup: pose_check_dev.h's post-check with the pose the frame still has (:179-199),
//                    Converter::ConvertSE32Tcw of the estimate (:201) and its write-back, edges - nBad, the :370 decision.
// The check reads the verdict word first and leaves when the seed has rejected; the pose kernel between them sees no edge list through its
// device count.  No kernel waits on another; every loop is bounded by the feature count or the match count (at most one per keyframe
// feature).  Float arithmetic: map_point_dev.h's rows and `A x + t`, no contraction; the conversions in fp64.
#include <hip/hip_runtime.h>

#include "orbfe_internal.h"
#include "pose_check_dev.h"

#pragma clang fp contract(off)

namespace orbfe {
namespace {

__global__ __launch_bounds__(1024) void k_trackref_seed(TrackRefDev P) {
  __shared__ int s_claim[POSE_REG_EDGES];  // (the host refuses a frame of more features: the claims fit the LDS)
  __shared__ int s_wave[16], s_base;
  const int t = threadIdx.x;
  const int n_kp = min(*P.F.n_kp, P.F.nf);
  const int nm = min(max(*P.n_list, 0), P.n);
  for (int f = t; f < P.F.nf; f += 1024) s_claim[f] = -1;
  __syncthreads();
  for (int m = t; m < nm; m += 1024) {
    const BowMatch x = P.list[m];
    P.matches[m] = x;
    // `pFrame->setMapPoint(queryIdx, ..)` in match order: the last one stays.  (A host FeatureVector that names a feature past the slot's
    // count is not the frame's own: such a match is listed but gives no point, so no edge is built from a stale keypoint.)
    if (x.q >= 0 && x.q < n_kp) atomicMax(&s_claim[x.q], m);
  }
  __syncthreads();
  for (int f = t; f < P.F.nf; f += 1024) {  // what the frame holds now: the claim's point, else the one it came with
    int a = -1;
    const int cl = s_claim[f];
    if (cl >= 0) a = P.list[cl].t;
    else if (f < n_kp && P.f_good[f]) a = ORBFE_TRACKREF_OWN;
    P.assigned[f] = a;
    P.cur[f] = a;
  }
  if (nm < P.min_matches) {  // Tracking.cc:365, after the frame was written (ORBMatcher.cc:251)
    if (t != 0) return;
    P.hdr[TRACKREF_H_MATCHES] = nm;
    P.hdr[TRACKREF_H_VERDICT] = ORBFE_TRACKREF_REJECT_MATCHES;
    P.cnt[0] = -1;  // no optimisation
    return;
  }
  // the edges: every feature that holds a point (a thread reads the cur[f] it wrote)
  const int edges = pose_edges_1024(P.F, P.E, s_wave, &s_base, [&](int f) -> const float* {
    const int a = P.cur[f];
    return a == -1 ? nullptr : a >= 0 ? P.pos + 3 * (size_t)a : P.f_pos + 3 * (size_t)f;
  });
  if (t != 0) return;
  P.hdr[TRACKREF_H_MATCHES] = nm;
  P.hdr[TRACKREF_H_EDGES] = edges;
  P.cnt[0] = edges > 0 ? edges : -1;  // no edge: the estimate stays, nothing is an inlier
  tcw_to_se3_dev(P.F.R0, P.F.t0, P.p_init);
}

__global__ __launch_bounds__(1024) void k_trackref_check(TrackRefDev P) {
  __shared__ int s_wave[16];
  const int t = threadIdx.x;
  if (P.hdr[TRACKREF_H_VERDICT] != 0) return;  // (written by the seed only: every thread reads the same word)
  float R[9], tc[3];
  se3_to_tcw_dev(P.p_opt, R, tc);
  const int n_in = post_check_1024(
      P.F, P.F.R0, P.F.t0, P.E, P.inlier, s_wave,
      [&](int f, float (&X)[3]) {
        const int a = P.assigned[f];
        const float* src = a >= 0 ? P.pos + 3 * (size_t)a : P.f_pos + 3 * (size_t)f;
        X[0] = src[0], X[1] = src[1], X[2] = src[2];
      },
      [&](int f) { P.cur[f] = -1; });
  if (t != 0) return;
  P.hdr[TRACKREF_H_INLIERS] = n_in;
  pose_write_back(P.p_opt, R, tc, P.pose_out, P.tcw_out);
  P.hdr[TRACKREF_H_VERDICT] = n_in >= P.min_inliers ? ORBFE_TRACKREF_ACCEPT : ORBFE_TRACKREF_REJECT_INLIERS;  // Tracking.cc:370
}

}  // namespace

void launch_trackref_seed(hipStream_t st, const TrackRefDev& P) { hipLaunchKernelGGL(k_trackref_seed, dim3(1), dim3(1024), 0, st, P); }
void launch_trackref_check(hipStream_t st, const TrackRefDev& P) { hipLaunchKernelGGL(k_trackref_check, dim3(1), dim3(1024), 0, st, P); }

}  // namespace orbfe

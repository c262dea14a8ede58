// k_reloc.hip -- the glue of orbfe_reloc_refine_stored (include/orbfe.h): what Tracking::trackReLocalize does with one PnP
// hypothesis between its two Optimizer::OptimizePoseOnly calls and its two ORBMatcher::searchByProjection calls (src/Tracking.cc:565-584,
// :612-629), on the device.  The optimisations themselves are k_pose.hip's launch_pose_only on the edge lists built here.
//
// k_reloc_seed    one workgroup: setCurrFrameAttrib's map points (Tracking.cc:503-512) as cur[f], the edge list of the first
//                 optimisation in feature order (Optimizer.cc:58-117: pose_check_dev.h's pose_edges_1024), Converter::ConvertTcw2SE3 of
//                 the PnP pose (:119).
// k_reloc_check   one workgroup: the projection post-check with the pose the frame still has (:179-190), the nulling (:191-199),
//                 Converter::ConvertSE32Tcw of the estimate (:201) and its write-back, edges - nBad, the verdict of Tracking.cc:567-584 / :622, and for
//                 a search that follows tlc.z (ORBMatcher.cc:274-276) and the next optimisation's initial estimate.
// k_reloc_search  one wave per feature of the stored keyframe (ORBMatcher.cc:283-343, bFuse == false) over the slot's grid through
//                 area_search_body.h; its filter: the octave window by the motion direction, then "holds no point", with one hit
//                 counted per occurrence of a feature that does (:321-331); its acceptance (:339) claims the feature for the LAST
//                 query that picked it (setMapPoints, :344-345: an atomicMax over claims that start at -1).
// k_reloc_after   one workgroup: the claims become what the frame holds, the sum test of Tracking.cc:619 / :625, and after the first
//                 search the edge list of the second optimisation.
// Every kernel after the seed reads the verdict word first and leaves when it has fallen; no kernel waits on another; every loop is
// bounded by the feature count, the grid size or a cell's feature count.  Float arithmetic: map_point_dev.h's rows and `A x + t`, no
// contraction; the two pose conversions are host/map_pb.hpp's tcw_to_se3 / se3_to_tcw operation for operation, in fp64.
#include <hip/hip_runtime.h>

#include "area_search_body.h"
#include "map_point_dev.h"
#include "orbfe_internal.h"
#include "pose_check_dev.h"

#pragma clang fp contract(off)

namespace orbfe {
namespace {

// The pose-only edges of what the frame holds (cur), in feature order: pose_check_dev.h's list.  Returns the count to every thread.
__device__ __forceinline__ int build_edges(const RelocDev& P, int* s_wave, int* s_base) {
  return pose_edges_1024(P.F, P.E, s_wave, s_base, [&](int f) -> const float* {
    const int mp = P.cur[f];
    return mp >= 0 ? P.pos + 3 * mp : nullptr;
  });
}

__global__ __launch_bounds__(1024) void k_reloc_seed(RelocDev P) {
  __shared__ int s_wave[16], s_base;
  const int t = threadIdx.x;
  const int n_kp = min(*P.F.n_kp, P.F.nf);
  for (int f = t; f < P.F.nf; f += 1024) {
    const int h = f < n_kp ? P.held[f] : -1;
    P.cur[f] = (h >= 0 && P.good[h]) ? h : -1;  // `if (pMp && !pMp->isBad()) setMapPoint` (Tracking.cc:510-511)
  }
  const int edges = build_edges(P, s_wave, &s_base);  // (a thread reads the cur[f] it wrote)
  if (t == 0) {
    P.hdr[RELOC_H_EDGES] = edges;
    P.cnt[0] = edges > 0 ? edges : -1;  // no edge: the estimate stays, nothing is an inlier
    tcw_to_se3_dev(P.F.R0, P.F.t0, P.p_init);
  }
}

__global__ __launch_bounds__(1024) void k_reloc_check(RelocDev P, int s) {
  __shared__ int s_wave[16];
  const int t = threadIdx.x;
  const int verdict = P.hdr[RELOC_H_VERDICT];
  __syncthreads();  // (every thread has read the word before thread 0 may write it)
  if (verdict != 0) return;
  const double* est = P.p_opt + 7 * s;
  float R[9], tc[3], Rf[9], tf[3];
  se3_to_tcw_dev(est, R, tc);
  // the pose the frame still has: the PnP pose, then the first float pose
#pragma unroll
  for (int k = 0; k < 9; ++k) Rf[k] = s == 0 ? P.F.R0[k] : P.tcw_out[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tf[k] = s == 0 ? P.F.t0[k] : P.tcw_out[9 + k];
  const int n_in = post_check_1024(
      P.F, Rf, tf, P.E, P.inlier + (size_t)s * P.F.nf, s_wave,
      [&](int f, float (&X)[3]) {
        const int mp = P.cur[f];
        X[0] = P.pos[3 * mp], X[1] = P.pos[3 * mp + 1], X[2] = P.pos[3 * mp + 2];
      },
      [&](int f) { P.cur[f] = -1; });
  if (t != 0) return;
  P.hdr[RELOC_H_INLIERS + s] = n_in;
  pose_write_back(est, R, tc, P.pose_out + 7 * s, P.tcw_out + 12 * s);
  if (s == 0 && n_in < P.min_inliers) {
    P.hdr[RELOC_H_VERDICT] = ORBFE_RELOC_REJECT_1;
    return;
  }
  if (n_in >= P.enough) {
    P.hdr[RELOC_H_VERDICT] = s == 0 ? ORBFE_RELOC_ACCEPT_1 : ORBFE_RELOC_ACCEPT_2;
    return;
  }
  // a search follows: twc = -Rcw^T tcw, tlc = Rkf twc + tkf (ORBMatcher.cc:274-276)
  P.hdr[RELOC_H_TLCZ + s] = __float_as_int(tlc_z_dev(R, tc, P.kf_R, P.kf_t));
  if (s == 0) tcw_to_se3_dev(R, tc, P.p_init + 7);  // the frame's pose is the float one now (setPose, Optimizer.cc:201)
}

__global__ __launch_bounds__(256) void k_reloc_search(RelocDev P, int s) {
  __shared__ int32_t stage_all[4][128];
  if (P.hdr[RELOC_H_VERDICT] != 0) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wv;
  if (q >= P.n || !P.good[q]) return;  // `if (!pMp2 || pMp2->isBad()) continue` (:286-287)
  const orbfe_keypoint kp = P.k_kps[q];
  const int o = min(max(kp.octave, 0), P.F.n_levels - 1);
  const float z = __int_as_float(P.hdr[RELOC_H_TLCZ + s]);
  int lo, hi;
  motion_window(o, z, P.baseline, lo, hi);
  const float rad = P.th[s] * P.F.sigma2[o];  // findFeaturesInArea: radius * getScaledFactor2(octave) (Frame.cc:289)
  const uint4 a0 = *(const uint4*)(P.k_desc + (size_t)q * 32);
  const uint4 a1 = *(const uint4*)(P.k_desc + (size_t)q * 32 + 16);
  Best2 b = {ORB_INT_MAX, ORB_INT_MAX, 0};
  const AreaTarget T = {P.f_desc, P.cell_off, P.cell_feat, P.rows, P.cols, P.clip_w, P.clip_h};
  const uint4* __restrict__ kpl = P.f_kpl;
  const int32_t* __restrict__ cur = P.cur;
  int32_t* hits = P.hits + (size_t)s * P.F.nf;
  const int total = area_fold(T, kp.x, kp.y, rad, a0, a1, stage_all[wv], lane, b, [&](int id) {
    const int oc = (int)(kpl[id].y & 0xFFu);
    if (!(oc <= hi && oc >= lo)) return false;
    if (cur[id] >= 0) {  // the feature holds a point: addMatchInTrack, no candidate (:321-331)
      atomicAdd(&hits[id], 1);
      return false;
    }
    return true;
  });
  if (lane != 0 || total <= 0) return;
  const float fr = (float)b.min_d / (float)b.second;  // getBestMatch's ratio (:988)
  if (fr < P.ratio && b.min_d < P.min_threshold) {
    atomicMax(&P.claim[(size_t)s * P.F.nf + b.min_idx], q);
    atomicAdd(&P.hdr[RELOC_H_ADDED + s], 1);
    P.qa[(size_t)s * P.n + q] = 1;
  }
}

__global__ __launch_bounds__(1024) void k_reloc_after(RelocDev P, int s) {
  __shared__ int s_wave[16], s_base;
  const int t = threadIdx.x;
  const int verdict = P.hdr[RELOC_H_VERDICT];
  __syncthreads();
  if (verdict != 0) {
    if (s == 0 && t == 0) P.cnt[1] = -1;  // no second optimisation
    return;
  }
  for (int f = t; f < P.F.nf; f += 1024) {
    const int cl = P.claim[(size_t)s * P.F.nf + f];
    int c = P.cur[f];
    if (cl >= 0) c = cl, P.cur[f] = cl;
    P.assigned[(size_t)s * P.F.nf + f] = c;
  }
  const bool too_few = P.hdr[RELOC_H_ADDED + s] + P.hdr[RELOC_H_INLIERS + s] < P.enough;  // Tracking.cc:619, :625
  if (too_few || s == 1) {
    if (t == 0) {
      P.hdr[RELOC_H_VERDICT] = too_few ? (s == 0 ? ORBFE_RELOC_REJECT_2 : ORBFE_RELOC_REJECT_3) : ORBFE_RELOC_ACCEPT_3;
      if (s == 0) P.cnt[1] = -1;
    }
    return;
  }
  const int edges = build_edges(P, s_wave, &s_base);
  if (t == 0) {
    P.hdr[RELOC_H_EDGES + 1] = edges;
    P.cnt[1] = edges > 0 ? edges : -1;
  }
}

}  // namespace

void launch_reloc_seed(hipStream_t st, const RelocDev& P) { hipLaunchKernelGGL(k_reloc_seed, dim3(1), dim3(1024), 0, st, P); }
void launch_reloc_check(hipStream_t st, const RelocDev& P, int s) { hipLaunchKernelGGL(k_reloc_check, dim3(1), dim3(1024), 0, st, P, s); }
void launch_reloc_search(hipStream_t st, const RelocDev& P, int s) {
  if (P.n <= 0) return;
  hipLaunchKernelGGL(k_reloc_search, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0, st, P, s);
}
void launch_reloc_after(hipStream_t st, const RelocDev& P, int s) { hipLaunchKernelGGL(k_reloc_after, dim3(1), dim3(1024), 0, st, P, s); }

}  // namespace orbfe

// pose_call.h -- the host side of the pose-only step that the six tracking calls share (orbfe_guided.hip: the two track_local_map calls and
// the array motion model; orbfe_reloc.hip, orbfe_trackref.hip, orbfe_motion.hip): the scratch of the step, the frame's side of an upload,
// the launch of the optimisation and the argument checks the calls repeat.  The device side is pose_check_dev.h.
// The first part is host only, like search_area_layout.h (tests/cpp/test_scratch_layout.cpp compiles it with the host compiler alone);
// the second part is for the .hip files and needs orbfe_ctx.h in front of it.
#pragma once
#include <cstdint>

#include "scratch_layout.h"

// The scratch of k pose-only optimisations (1, or the relocalisation refine's 2) over a frame of NF features, in three takes: the caller
// says which of its regions (uploaded, zero-filled, downloaded, device-only) each lies in by opening and closing them around the takes.
struct PoseWorkspace {
  size_t NF, k;
  size_t o_p0 = 0;                                // seed: p_init[k][7], uploaded by the chains, written by a kernel in the fused calls
  size_t o_xw = 0, o_ms = 0, o_info = 0, o_sig = 0;  // list: Xw[NF][3], meas[NF][3], info[NF], sigma2[NF] -- device-only everywhere
  size_t o_p1 = 0, o_ng = 0, o_eo = 0, o_ei = 0;  // results: p_opt[k][7], n_good, edge_of[NF], the optimiser's inlier flag per edge
  PoseWorkspace(size_t n_features, size_t n_opt = 1) : NF(n_features), k(n_opt) {}
  ScratchLayout& take_seed(ScratchLayout& L) { return o_p0 = L.take<double>(7 * k), L; }
  ScratchLayout& take_list(ScratchLayout& L) {
    return o_xw = L.take<double>(NF * 3), o_ms = L.take<double>(NF * 3), o_info = L.take<double>(NF), o_sig = L.take<float>(NF), L;
  }
  ScratchLayout& take_results(ScratchLayout& L) {
    return o_p1 = L.take<double>(7 * k), o_ng = L.take(8), o_eo = L.take<int32_t>(NF), o_ei = L.take(NF), L;
  }
};

// The frame's side of an upload: right_u[NF] and the two level tables.
struct FrameUpload {
  size_t o_ru = 0, o_s2 = 0, o_is2 = 0;
  ScratchLayout& take(ScratchLayout& L, size_t NF, size_t nl) { return o_ru = L.take<double>(NF), o_s2 = L.take<float>(nl), o_is2 = L.take<float>(nl), L; }
};

#ifdef __HIPCC__
// ---- the bound: a frame of more features than the register kernels of k_pose.hip take edges is refused ----
static inline orbfe_status pose_check_features(orbfe_ctx* c, const char* fn, size_t NF) {
  static_assert(POSE_REG_EDGES == 2048, "the message names the bound");
  if (NF > POSE_REG_EDGES)
    return fail(c, ORBFE_EBADSIZE, "%s: %zu features per frame (the fused pose kernel keeps up to 2048 edges in registers)", fn, NF);
  return ORBFE_OK;
}

// ---- the checks ----
struct FloatSpan {
  const float* p;
  size_t n;
};
// every entry of these spans -- camera, bounds, scalars, rotations, translations -- is finite
static inline orbfe_status check_finite(orbfe_ctx* c, const char* fn, std::initializer_list<FloatSpan> spans) {
  for (const FloatSpan& s : spans)
    for (size_t i = 0; i < s.n; ++i)
      if (!std::isfinite(s.p[i])) return fail(c, ORBFE_EBADARG, "%s: a camera entry, a bound, a scalar, a rotation or a translation entry is not finite", fn);
  return ORBFE_OK;
}
// the frame's grid (bounds NULL: the image itself) and the LDS rule of its build over n_target features
static inline orbfe_status check_area_grid(orbfe_ctx* c, const char* fn, const float* bounds, size_t n_target, AreaGrid* ag) {
  if (!area_grid(c->cfg.width, c->cfg.height, bounds, ag)) return fail(c, ORBFE_EBADARG, "%s: bad frame bounds", fn);
  const size_t ncells = (size_t)ag->rows * ag->cols;
  if (area_grid_lds(ncells, n_target).refused) return fail(c, ORBFE_EBADSIZE, "%s: %zu grid cells exceed the LDS counters", fn, ncells);
  return ORBFE_OK;
}
// what the features hold on entry: -1 or a point of the call's n
static inline orbfe_status check_held(orbfe_ctx* c, const char* fn, const int32_t* held, size_t NF, int n) {
  for (size_t f = 0; f < NF; ++f)
    if (held[f] < -1 || held[f] >= n) return fail(c, ORBFE_EBADARG, "%s: held[%zu] = %d out of range", fn, f, held[f]);
  return ORBFE_OK;
}

// ---- the frame ----
// right_u (NULL: -1.0 everywhere, every edge mono) and the level tables into the staging buffer
static inline void put_frame(StagedIo& io, const FrameUpload& U, size_t NF, size_t nl, const double* right_u, const float* sigma2,
                             const float* inv_sigma2) {
  if (right_u) io.put(U.o_ru, right_u, NF * 8);
  else
    for (size_t f = 0; f < NF; ++f) io.host<double>(U.o_ru)[f] = -1.0;
  io.put(U.o_s2, sigma2, nl * 4);
  io.put(U.o_is2, inv_sigma2, nl * 4);
}
// the frame view of `slot`; pose and camera stay zero (the chains) until pose_frame_camera
static inline PoseFrameDev pose_frame(const orbfe_ctx* c, int slot, const double* d_right_u, const float* d_sigma2, const float* d_inv_sigma2) {
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1);
  PoseFrameDev F = {};
  F.kps = c->d_kps + (size_t)slot * NF, F.n_kp = c->d_n_kp + slot, F.nf = (int32_t)NF, F.n_levels = c->cfg.n_levels;
  F.right_u = d_right_u, F.sigma2 = d_sigma2, F.inv_sigma2 = d_inv_sigma2;
  return F;
}
static inline PoseFrameDev pose_frame(const orbfe_ctx* c, int slot, const uint8_t* b, const FrameUpload& U) {
  return pose_frame(c, slot, (const double*)(b + U.o_ru), (const float*)(b + U.o_s2), (const float*)(b + U.o_is2));
}
static inline void pose_frame_camera(PoseFrameDev& F, const float* Rcw, const float* tcw, const orbfe_camera* cam, const float* bounds) {
  std::memcpy(F.R0, Rcw, sizeof F.R0), std::memcpy(F.t0, tcw, sizeof F.t0);
  F.fx = cam->fx, F.fy = cam->fy, F.cx = cam->cx, F.cy = cam->cy, F.max_u = bounds[1], F.max_v = bounds[3];
}

// ---- the workspace on the device: b is the call's scratch block ----
static inline PoseEdgesDev pose_edges(const PoseWorkspace& W, uint8_t* b) {
  return {(int32_t*)(b + W.o_eo), (double*)(b + W.o_xw), (double*)(b + W.o_ms), (double*)(b + W.o_info), (float*)(b + W.o_sig), b + W.o_ei};
}
// optimisation s on the edge list, from p_init[s] to p_opt[s]; d_count: the edge count in device memory (negative: no optimisation)
static inline void pose_optimise(orbfe_ctx* c, hipStream_t st, const PoseWorkspace& W, uint8_t* b, const orbfe_camera* cam, int s,
                                 const int32_t* d_count) {
  StageTimer tm(c, ORBFE_STAGE_BA, st);
  const BaParamsDev prm = {(double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy, (double)cam->bf};
  const PoseEdgesDev E = pose_edges(W, b);
  launch_pose_only_reg(st, (int)W.NF, E.Xw, E.meas, E.info, E.sig, (const double*)(b + W.o_p0) + 7 * s, prm, (double)(float)std::sqrt(5.991),
                       (double)(float)std::sqrt(7.815), b + W.o_ei, (double*)(b + W.o_p1) + 7 * s, (int32_t*)(b + W.o_ng), d_count);
}
#endif

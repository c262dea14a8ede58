// orbfe_fuse.hip -- host side of orbfe_fuse_into_keyframes (include/orbfe.h): the inverse fuses of LocalMapping::fuseMapPoints
// (src/LocalMapping.cc:352-405; ORBMatcher::fuse(pkf, cur), searchByProjection with bFuse and processFuseMps, src/ORBMatcher.cc:265-347,
// 623-724) as one batch.  Argument checks, one upload into the context's scratch, the three launches of k_fuse.hip, one download.
#include "orbfe_ctx.h"

void launch_fuse(hipStream_t st, uint8_t* base, const FuseKf* kfs, const FuseParams& P, size_t grid_lds, const orbfe_keypoint* q_kps,
                 const uint8_t* q_desc, const float* sf, const uint8_t* has_point, const float* pos, const float* vdir, const float* max_dist,
                 const float* min_dist, int32_t* best_idx, int32_t* best_dist, uint8_t* visible);

namespace {

orbfe_status check_fuse_kf(orbfe_ctx* c, const orbfe_fuse_kf* k, int32_t n_levels, const char* who, int idx) {
  if (k->n < 0 || k->n > ORBFE_BOW_MAX_FEATURES) return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: %s %d: %d features", who, idx, k->n);
  if (k->n > 0 && (!k->kps || !k->desc)) return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: %s %d: NULL array", who, idx);
  for (int32_t i = 0; i < k->n; ++i)
    if (k->kps[i].octave < 0 || k->kps[i].octave >= n_levels)
      return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: %s %d: feature %d has octave %d outside 0..%d", who, idx, i, k->kps[i].octave, n_levels - 1);
  return ORBFE_OK;
}

}  // namespace

extern "C" {

orbfe_status orbfe_fuse_into_keyframes(orbfe_ctx* c, const orbfe_fuse_kf* cur, const orbfe_fuse_points* pts, int32_t n_kf,
                                       const orbfe_fuse_kf* targets, const float* z, const orbfe_camera* cam, float bl, const float* scale_factors,
                                       int32_t n_levels, float th, float ratio, int32_t dist_threshold, int32_t* best_idx, int32_t* best_dist,
                                       uint8_t* visible) {
  ApiLock api_lk(c);
  if (!c || !cur || !pts || !cam || !scale_factors || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS)
    return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: bad arguments");
  if (n_kf < 0 || n_kf > ORBFE_FUSE_MAX_KF) return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: %d target keyframes, 0..%d allowed", n_kf, ORBFE_FUSE_MAX_KF);
  TRY(check_fuse_kf(c, cur, n_levels, "current keyframe", 0));
  if (n_kf == 0 || cur->n == 0) return ORBFE_OK;
  if (!targets || !z || !best_idx || !best_dist || !visible || !pts->has_point || !pts->pos || !pts->view_dir || !pts->max_dist || !pts->min_dist)
    return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: NULL array");
  for (int32_t k = 0; k < n_kf; ++k) TRY(check_fuse_kf(c, targets + k, n_levels, "target", k));

  const size_t K = (size_t)n_kf, N = (size_t)cur->n, NQ = K * N;
  std::vector<FuseKf> kf(K);
  // [ upload: FuseKf x K | scale factors | cur's features and slot points | every target's features ] [ the grids ] [ download ]
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_kf = L.open(up).take<FuseKf>(K), o_sf = L.take<float>((size_t)n_levels), o_qk = L.take<orbfe_keypoint>(N), o_qd = L.take(N * 32),
               o_hp = L.take(N), o_pos = L.take<float>(N * 3), o_vd = L.take<float>(N * 3), o_mx = L.take<float>(N), o_mn = L.take<float>(N);
  for (size_t k = 0; k < K; ++k) {
    kf[k].o_kps = L.take<orbfe_keypoint>((size_t)targets[k].n);
    kf[k].o_desc = L.take((size_t)targets[k].n * 32);
  }
  L.close(up);
  size_t grid_lds = 0;
  for (size_t k = 0; k < K; ++k) {
    const orbfe_fuse_kf& t = targets[k];
    FuseKf& d = kf[k];
    AreaGrid ag;
    if (!area_grid(c->cfg.width, c->cfg.height, t.bounds, &ag)) return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: target %zu: bad frame bounds", k);
    const size_t ncells = (size_t)ag.rows * ag.cols, lds_base = (2 * ncells + 1) * sizeof(int32_t), lds_lists = (size_t)t.n * 2 * sizeof(int32_t);
    if (lds_base > 60 * 1024) return fail(c, ORBFE_EBADSIZE, "fuse_into_keyframes: target %zu: %zu grid cells exceed the LDS counters", k, ncells);
    d.n = t.n, d.rows = ag.rows, d.cols = ag.cols, d.clip_w = ag.clip_w, d.clip_h = ag.clip_h;
    // ORBMatcher.cc:277-280: zabs > mfBl ? (z > 0 ? up : down) : neither
    d.mode = std::abs(z[k]) > bl ? (z[k] > 0 ? 1 : 2) : 0;
    d.in_lds = lds_base + lds_lists <= 56 * 1024 ? 1 : 0;
    d.pad = 0;
    grid_lds = std::max(grid_lds, d.in_lds ? lds_base + lds_lists : lds_base);
    std::memcpy(d.R, t.Rcw, sizeof d.R);
    std::memcpy(d.t, t.tcw, sizeof d.t);
    std::memcpy(d.bounds, t.bounds, sizeof d.bounds);
    d.o_coff = L.take<int32_t>(ncells + 1);  // k_fuse_grid writes cell_off[0 .. ncells], k_fuse_search reads cell_off[cell + 1]
    d.o_cfeat = L.take<int32_t>((size_t)t.n);
  }
  const size_t o_bi = L.open(down).take<int32_t>(NQ), o_bd = L.take<int32_t>(NQ), o_vis = L.take(NQ);
  L.close(down);

  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  // up to 8 MB: one upload and one download through the page-locked staging buffer; beyond, the arrays are copied directly
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes()), L.end() <= ((size_t)8 << 20)));
  io.put(o_kf, kf.data(), K * sizeof(FuseKf));
  io.put(o_sf, scale_factors, (size_t)n_levels * 4);
  io.put(o_qk, cur->kps, N * sizeof(orbfe_keypoint));
  io.put(o_qd, cur->desc, N * 32);
  io.put(o_hp, pts->has_point, N);
  io.put(o_pos, pts->pos, N * 12);
  io.put(o_vd, pts->view_dir, N * 12);
  io.put(o_mx, pts->max_dist, N * 4);
  io.put(o_mn, pts->min_dist, N * 4);
  for (size_t k = 0; k < K; ++k) {
    io.put(kf[k].o_kps, targets[k].kps, (size_t)targets[k].n * sizeof(orbfe_keypoint));
    io.put(kf[k].o_desc, targets[k].desc, (size_t)targets[k].n * 32);
  }
  HIP_TRY(c, io.upload(up));
  FuseParams P = {};
  P.fx = cam->fx, P.fy = cam->fy, P.cx = cam->cx, P.cy = cam->cy;
  P.th = th, P.ratio = ratio, P.dist_threshold = dist_threshold;
  P.n_kf = n_kf, P.n_cur = cur->n;
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    launch_fuse(c->stream, io.d, io.dev<FuseKf>(o_kf), P, grid_lds, io.dev<orbfe_keypoint>(o_qk), io.dev<uint8_t>(o_qd), io.dev<float>(o_sf),
                io.dev<uint8_t>(o_hp), io.dev<float>(o_pos), io.dev<float>(o_vd), io.dev<float>(o_mx), io.dev<float>(o_mn), io.dev<int32_t>(o_bi),
                io.dev<int32_t>(o_bd), io.dev<uint8_t>(o_vis));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.download(down));
  if (io.staged) HIP_TRY(c, io.wait());  // (staged: get reads the downloaded block; unstaged: get is the copy, waited for below)
  io.get(best_idx, o_bi, NQ * 4);
  io.get(best_dist, o_bd, NQ * 4);
  io.get(visible, o_vis, NQ);
  if (!io.staged) HIP_TRY(c, io.wait());
  drain_timers(c);
  return ORBFE_OK;
}

}  // extern "C"

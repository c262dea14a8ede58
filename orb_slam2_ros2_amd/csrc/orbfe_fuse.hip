// orbfe_fuse.hip -- host side of orbfe_fuse_into_keyframes (include/orbfe.h): the inverse fuses of LocalMapping::fuseMapPoints
// (src/LocalMapping.cc:352-405; ORBMatcher::fuse(pkf, cur), searchByProjection with bFuse and processFuseMps, src/ORBMatcher.cc:265-347,
// 623-724) as one batch.  Argument checks, one upload into the context's scratch, the three launches of k_fuse.hip, one download.
// orbfe_fuse_into_keyframes_stored names the keyframes by their id in a keyframe store (orbfe_kfstore.h): only the target records and
// cur's slot points go up, the grids are the store's, and everything from the upload on (fuse_run) is one text for both forms.
#include "orbfe_kfstore.h"

void launch_fuse(hipStream_t st, uint8_t* base, const FuseKf* kfs, const FuseParams& P, size_t grid_lds, const orbfe_keypoint* q_kps,
                 const uint8_t* q_desc, const float* sf, const uint8_t* has_point, const float* pos, const float* vdir, const float* max_dist,
                 const float* min_dist, int32_t* best_idx, int32_t* best_dist, uint8_t* visible, bool build_grids);

namespace {

orbfe_status check_fuse_kf(orbfe_ctx* c, const orbfe_fuse_kf* k, int32_t n_levels, const char* who, int idx) {
  if (k->n < 0 || k->n > ORBFE_BOW_MAX_FEATURES) return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: %s %d: %d features", who, idx, k->n);
  if (k->n > 0 && (!k->kps || !k->desc)) return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: %s %d: NULL array", who, idx);
  for (int32_t i = 0; i < k->n; ++i)
    if (k->kps[i].octave < 0 || k->kps[i].octave >= n_levels)
      return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: %s %d: feature %d has octave %d outside 0..%d", who, idx, i, k->kps[i].octave, n_levels - 1);
  return ORBFE_OK;
}

// what both forms lay out first: the target records, the scale factors and the rows of cur's slot points
struct FuseLayout {
  ScratchLayout L;
  ScratchRegion up, down;
  size_t o_kf, o_sf, o_hp, o_pos, o_vd, o_mx, o_mn, o_bi, o_bd, o_vis;
  void open(size_t K, size_t N, size_t n_levels) {
    o_kf = L.open(up).take<FuseKf>(K), o_sf = L.take<float>(n_levels);
    o_hp = L.take(N), o_pos = L.take<float>(N * 3), o_vd = L.take<float>(N * 3), o_mx = L.take<float>(N), o_mn = L.take<float>(N);
  }
  void results(size_t NQ) {
    o_bi = L.open(down).take<int32_t>(NQ), o_bd = L.take<int32_t>(NQ), o_vis = L.take(NQ);
    L.close(down);
  }
};

// the octave-window case and the pose of target k (ORBMatcher.cc:277-280: zabs > mfBl ? (z > 0 ? up : down) : neither)
void fuse_pose(FuseKf& d, float z, float bl, const float* Rcw, const float* tcw) {
  d.mode = std::abs(z) > bl ? (z > 0 ? 1 : 2) : 0;
  std::memcpy(d.R, Rcw, sizeof d.R);
  std::memcpy(d.t, tcw, sizeof d.t);
}

// From the reservation on.  put_features(io): the form's own inputs into the upload; base / q_kps / q_desc: where the targets' offsets
// count from and where cur's features are -- the upload (nullptr: filled in from the reserved block at q_off) or the store.
template <class Put>
orbfe_status fuse_run(orbfe_ctx* c, FuseLayout& F, const std::vector<FuseKf>& kf, size_t N, const orbfe_fuse_points* pts, const float* scale_factors,
                      int32_t n_levels, const orbfe_camera* cam, float th, float ratio, int32_t dist_threshold, size_t grid_lds, bool in_upload,
                      size_t o_qk, size_t o_qd, const orbfe_keypoint* q_kps, const uint8_t* q_desc, Put put_features, int32_t* best_idx,
                      int32_t* best_dist, uint8_t* visible) {
  const size_t K = kf.size(), NQ = K * N;
  // up to 8 MB: one upload and one download through the page-locked staging buffer; beyond, the arrays are copied directly
  StagedIo io;
  TRY(io.reserve(c, F.L.end(), std::max(F.up.end, F.down.bytes()), F.L.end() <= ((size_t)8 << 20)));
  io.put(F.o_kf, kf.data(), K * sizeof(FuseKf));
  io.put(F.o_sf, scale_factors, (size_t)n_levels * 4);
  io.put(F.o_hp, pts->has_point, N);
  io.put(F.o_pos, pts->pos, N * 12);
  io.put(F.o_vd, pts->view_dir, N * 12);
  io.put(F.o_mx, pts->max_dist, N * 4);
  io.put(F.o_mn, pts->min_dist, N * 4);
  put_features(io);
  HIP_TRY(c, io.upload(F.up));
  FuseParams P = {};
  P.fx = cam->fx, P.fy = cam->fy, P.cx = cam->cx, P.cy = cam->cy;
  P.th = th, P.ratio = ratio, P.dist_threshold = dist_threshold;
  P.n_kf = (int32_t)K, P.n_cur = (int32_t)N;
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    launch_fuse(c->stream, in_upload ? io.d : nullptr, io.dev<FuseKf>(F.o_kf), P, grid_lds, in_upload ? io.dev<orbfe_keypoint>(o_qk) : q_kps,
                in_upload ? io.dev<uint8_t>(o_qd) : q_desc, io.dev<float>(F.o_sf), io.dev<uint8_t>(F.o_hp), io.dev<float>(F.o_pos),
                io.dev<float>(F.o_vd), io.dev<float>(F.o_mx), io.dev<float>(F.o_mn), io.dev<int32_t>(F.o_bi), io.dev<int32_t>(F.o_bd),
                io.dev<uint8_t>(F.o_vis), in_upload);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.download(F.down));
  if (io.staged) HIP_TRY(c, io.wait());  // (staged: get reads the downloaded block; unstaged: get is the copy, waited for below)
  io.get(best_idx, F.o_bi, NQ * 4);
  io.get(best_dist, F.o_bd, NQ * 4);
  io.get(visible, F.o_vis, NQ);
  if (!io.staged) HIP_TRY(c, io.wait());
  drain_timers(c);
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

  const size_t K = (size_t)n_kf, N = (size_t)cur->n;
  std::vector<FuseKf> kf(K);
  // [ upload: FuseKf x K | scale factors | cur's slot points | cur's features | every target's features ] [ the grids ] [ download ]
  FuseLayout F;
  F.open(K, N, (size_t)n_levels);
  ScratchLayout& L = F.L;
  const size_t o_qk = L.take<orbfe_keypoint>(N), o_qd = L.take(N * 32);
  for (size_t k = 0; k < K; ++k) {
    kf[k].o_kps = L.take<orbfe_keypoint>((size_t)targets[k].n);
    kf[k].o_desc = L.take((size_t)targets[k].n * 32);
  }
  L.close(F.up);
  size_t grid_lds = 0;
  for (size_t k = 0; k < K; ++k) {
    const orbfe_fuse_kf& t = targets[k];
    FuseKf& d = kf[k];
    AreaGrid ag;
    if (!area_grid(c->cfg.width, c->cfg.height, t.bounds, &ag)) return fail(c, ORBFE_EBADARG, "fuse_into_keyframes: target %zu: bad frame bounds", k);
    const size_t ncells = (size_t)ag.rows * ag.cols;
    const AreaGridLds g = area_grid_lds(ncells, (size_t)t.n);
    if (g.refused) return fail(c, ORBFE_EBADSIZE, "fuse_into_keyframes: target %zu: %zu grid cells exceed the LDS counters", k, ncells);
    d.n = t.n, d.rows = ag.rows, d.cols = ag.cols, d.clip_w = ag.clip_w, d.clip_h = ag.clip_h;
    fuse_pose(d, z[k], bl, t.Rcw, t.tcw);
    d.in_lds = g.in_lds;
    d.pad = 0;
    grid_lds = std::max(grid_lds, g.bytes);
    std::memcpy(d.bounds, t.bounds, sizeof d.bounds);
    d.o_coff = L.take<int32_t>(ncells + 1);  // k_fuse_grid writes cell_off[0 .. ncells], k_fuse_search reads cell_off[cell + 1]
    d.o_cfeat = L.take<int32_t>((size_t)t.n);
  }
  F.results(K * N);

  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  auto put_features = [&](StagedIo& io) {
    io.put(o_qk, cur->kps, N * sizeof(orbfe_keypoint));
    io.put(o_qd, cur->desc, N * 32);
    for (size_t k = 0; k < K; ++k) {
      io.put(kf[k].o_kps, targets[k].kps, (size_t)targets[k].n * sizeof(orbfe_keypoint));
      io.put(kf[k].o_desc, targets[k].desc, (size_t)targets[k].n * 32);
    }
  };
  return fuse_run(c, F, kf, N, pts, scale_factors, n_levels, cam, th, ratio, dist_threshold, grid_lds, true, o_qk, o_qd, nullptr, nullptr, put_features,
                  best_idx, best_dist, visible);
}

orbfe_status orbfe_fuse_into_keyframes_stored(orbfe_ctx* c, orbfe_kfstore* store, uint64_t cur_id, int32_t n_cur, const orbfe_fuse_points* pts,
                                              int32_t n_kf, const uint64_t* target_ids, const orbfe_fuse_pose* poses, const float* z,
                                              const orbfe_camera* cam, float bl, const float* scale_factors, int32_t n_levels, float th,
                                              float ratio, int32_t dist_threshold, int32_t* best_idx, int32_t* best_dist, uint8_t* visible) {
  ApiLock api_lk(c);
  const char* fn = "fuse_into_keyframes_stored";
  if (!c || !store || !pts || !cam || !scale_factors || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS) return fail(c, ORBFE_EBADARG, "%s: bad arguments", fn);
  if (n_kf < 0 || n_kf > ORBFE_FUSE_MAX_KF) return fail(c, ORBFE_EBADARG, "%s: %d target keyframes, 0..%d allowed", fn, n_kf, ORBFE_FUSE_MAX_KF);
  TRY(kfstore_check_ctx(c, store, fn));
  if (n_levels < store->n_levels) return fail(c, ORBFE_EBADARG, "%s: %d scale factors, the store's octaves go up to %d", fn, n_levels, store->n_levels - 1);
  if (n_kf > 0 && !target_ids) return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
  std::shared_lock<std::shared_timed_mutex> store_lk(store->mu);  // held until the results are down: no erase frees memory under the kernels
  const KfEntry* cur = store->map.find(cur_id);
  if (!cur) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)cur_id);
  if (cur->n != n_cur) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu has %d features, the call says %d", fn, (unsigned long long)cur_id, cur->n, n_cur);
  const size_t K = (size_t)n_kf, N = (size_t)cur->n;
  std::vector<FuseKf> kf(K);
  for (size_t k = 0; k < K; ++k) {
    const KfEntry* e = store->map.find(target_ids[k]);
    if (!e) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)target_ids[k]);
    FuseKf& d = kf[k];
    // (base nullptr: the offsets are the arrays' addresses)
    d.o_kps = (uint64_t)(uintptr_t)e->at<uint8_t>(e->o_kps), d.o_desc = (uint64_t)(uintptr_t)e->at<uint8_t>(e->o_desc);
    d.o_coff = (uint64_t)(uintptr_t)e->at<uint8_t>(e->o_coff), d.o_cfeat = (uint64_t)(uintptr_t)e->at<uint8_t>(e->o_cfeat);
    d.n = e->n, d.rows = e->ag.rows, d.cols = e->ag.cols, d.clip_w = e->ag.clip_w, d.clip_h = e->ag.clip_h;
    d.in_lds = 0, d.pad = 0;
    std::memcpy(d.bounds, e->bounds, sizeof d.bounds);
  }
  if (n_kf == 0 || N == 0) return ORBFE_OK;
  if (!poses || !z || !best_idx || !best_dist || !visible || !pts->has_point || !pts->pos || !pts->view_dir || !pts->max_dist || !pts->min_dist)
    return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
  for (size_t k = 0; k < K; ++k) fuse_pose(kf[k], z[k], bl, poses[k].Rcw, poses[k].tcw);
  // [ upload: FuseKf x K | scale factors | cur's slot points ] [ download ]: the features and the grids are the store's
  FuseLayout F;
  F.open(K, N, (size_t)n_levels);
  F.L.close(F.up);
  F.results(K * N);
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  return fuse_run(c, F, kf, N, pts, scale_factors, n_levels, cam, th, ratio, dist_threshold, 0, false, 0, 0, cur->at<orbfe_keypoint>(cur->o_kps),
                  cur->at<uint8_t>(cur->o_desc), [](StagedIo&) {}, best_idx, best_dist, visible);
}

}  // extern "C"

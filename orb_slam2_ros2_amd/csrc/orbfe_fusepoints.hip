// orbfe_fusepoints.hip -- host side of orbfe_fuse_points_into_keyframes_stored (include/orbfe.h): the forward fuse
// ORBMatcher::fuse(pkf, mapPoints, map, bLoop, th) (src/ORBMatcher.cc:682-707) of one list of map points into n_kf stored keyframes.
// Argument checks, one upload into the context's scratch (map state only: the keyframes' poses, the points' arrays, the scale factors,
// and the zero of the work list's counter), the two launches of k_fusepoints.hip, one download.  The keyframes' features, descriptors,
// bounds and area grids are read where the keyframe store keeps them.
#include "orbfe_kfstore.h"

void launch_fuse_points(hipStream_t st, const FusePtsKf* kfs, const FusePtsParams& P, FusePtsEntry* list, uint32_t* count, int32_t* best_idx,
                        int32_t* best_dist, hipEvent_t between);

namespace {
// device milliseconds of the two kernels in the last call made with the MATCH stage timed (orbfe_debug_fuse_points_kernels)
double g_kernel_ms[2] = {0.0, 0.0};
}  // namespace

extern "C" {

orbfe_status orbfe_fuse_points_into_keyframes_stored(orbfe_ctx* c, orbfe_kfstore* store, int32_t n_kf, const uint64_t* kf_ids,
                                                     const orbfe_fuse_pose* poses, const orbfe_sim3_points* pts, const orbfe_camera* cam,
                                                     const float* scale_factors, int32_t n_levels, float th, float ratio, int32_t dist_threshold,
                                                     int32_t* best_idx, int32_t* best_dist) {
  ApiLock api_lk(c);
  const char* fn = "fuse_points_into_keyframes_stored";
  if (!c || !store || !pts || !cam || !scale_factors || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS || pts->m < 0 || pts->m > (1 << 20))
    return fail(c, ORBFE_EBADARG, "%s: bad arguments", fn);
  if (n_kf < 0 || n_kf > ORBFE_FUSE_MAX_KF) return fail(c, ORBFE_EBADARG, "%s: %d keyframes, 0..%d allowed", fn, n_kf, ORBFE_FUSE_MAX_KF);
  TRY(kfstore_check_ctx(c, store, fn));
  if (n_levels < store->n_levels) return fail(c, ORBFE_EBADARG, "%s: %d scale factors, the store's octaves go up to %d", fn, n_levels, store->n_levels - 1);
  if (!std::isfinite(th) || !std::isfinite(ratio)) return fail(c, ORBFE_EBADARG, "%s: th %g, ratio %g", fn, (double)th, (double)ratio);
  if (n_kf > 0 && !kf_ids) return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
  const size_t K = (size_t)n_kf, m = (size_t)pts->m;
  if (K * m > (size_t)ORBFE_FUSE_POINTS_MAX_PAIRS)
    return fail(c, ORBFE_EBADSIZE, "%s: %zu keyframes x %zu points exceed %d pairs", fn, K, m, ORBFE_FUSE_POINTS_MAX_PAIRS);
  std::shared_lock<std::shared_timed_mutex> store_lk(store->mu);  // held until the results are down: no erase frees memory under the kernels
  std::vector<FusePtsKf> kf(K);
  int32_t n_max = 0;
  for (size_t k = 0; k < K; ++k) {
    const KfEntry* e = store->map.find(kf_ids[k]);
    if (!e) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)kf_ids[k]);
    FusePtsKf& d = kf[k];
    d.kps = e->at<orbfe_keypoint>(e->o_kps), d.desc = e->at<uint8_t>(e->o_desc);
    d.cell_off = e->at<int32_t>(e->o_coff), d.cell_feat = e->at<int32_t>(e->o_cfeat);
    d.n = e->n, d.rows = e->ag.rows, d.cols = e->ag.cols, d.clip_w = e->ag.clip_w, d.clip_h = e->ag.clip_h, d.pad = 0;
    std::memcpy(d.bounds, e->bounds, sizeof d.bounds);
    n_max = std::max(n_max, e->n);
  }
  if (K == 0 || m == 0) return ORBFE_OK;
  if (!poses || !pts->usable || !pts->pos || !pts->view_dir || !pts->max_dist || !pts->min_dist || !pts->desc || !best_idx || !best_dist)
    return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
  for (size_t k = 0; k < K; ++k) {
    for (int q = 0; q < 9; ++q)
      if (!std::isfinite(poses[k].Rcw[q])) return fail(c, ORBFE_EBADARG, "%s: pose %zu is not finite", fn, k);
    for (int q = 0; q < 3; ++q)
      if (!std::isfinite(poses[k].tcw[q])) return fail(c, ORBFE_EBADARG, "%s: pose %zu is not finite", fn, k);
    std::memcpy(kf[k].R, poses[k].Rcw, sizeof kf[k].R);
    std::memcpy(kf[k].t, poses[k].tcw, sizeof kf[k].t);
  }
  // [ upload: counter = 0 | FusePtsKf x K | scale factors | usable | positions | view directions | ranges | descriptors ]
  // [ the work list, K * m entries ] [ download: best_idx | best_dist ]
  const size_t NQ = K * m;
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_cnt = L.open(up).take<uint32_t>(1), o_kf = L.take<FusePtsKf>(K), o_sf = L.take<float>((size_t)n_levels);
  const size_t o_us = L.take(m), o_pos = L.take<float>(m * 3), o_vd = L.take<float>(m * 3), o_mx = L.take<float>(m), o_mn = L.take<float>(m),
               o_d = L.take(m * 32);
  const size_t o_list = L.close(up).take<FusePtsEntry>(NQ);
  const size_t o_bi = L.open(down).take<int32_t>(NQ), o_bd = L.take<int32_t>(NQ);
  L.close(down);
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  // up to 8 MB of upload and download: one copy each through the page-locked staging buffer; beyond, the arrays are copied directly
  StagedIo io;
  const uint32_t zero = 0;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes()), up.bytes() + down.bytes() <= ((size_t)8 << 20)));
  io.put(o_cnt, &zero, sizeof zero);
  io.put(o_kf, kf.data(), K * sizeof(FusePtsKf));
  io.put(o_sf, scale_factors, (size_t)n_levels * 4);
  io.put(o_us, pts->usable, m);
  io.put(o_pos, pts->pos, m * 12);
  io.put(o_vd, pts->view_dir, m * 12);
  io.put(o_mx, pts->max_dist, m * 4);
  io.put(o_mn, pts->min_dist, m * 4);
  io.put(o_d, pts->desc, m * 32);
  HIP_TRY(c, io.upload(up));
  FusePtsParams P = {};
  P.fx = cam->fx, P.fy = cam->fy, P.cx = cam->cx, P.cy = cam->cy;
  P.th = th, P.ratio = ratio, P.dist_threshold = dist_threshold;
  P.log_sf = std::log(n_levels > 1 ? scale_factors[1] : 1.2f);
  P.max_level = std::min(7, n_levels - 1), P.n_levels = n_levels;
  P.n_kf = n_kf, P.m = pts->m;
  P.usable = io.dev<uint8_t>(o_us), P.desc = io.dev<uint8_t>(o_d);
  P.pos = io.dev<float>(o_pos), P.vdir = io.dev<float>(o_vd), P.max_dist = io.dev<float>(o_mx), P.min_dist = io.dev<float>(o_mn);
  P.sf = io.dev<float>(o_sf);
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  if (timed(c, ORBFE_STAGE_MATCH))
    for (hipEvent_t& e : ev)
      if (hipEventCreate(&e) != hipSuccess) e = nullptr;
  const bool split = ev[0] && ev[1] && ev[2];
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    if (split) (void)hipEventRecord(ev[0], c->stream);
    launch_fuse_points(c->stream, io.dev<FusePtsKf>(o_kf), P, io.dev<FusePtsEntry>(o_list), io.dev<uint32_t>(o_cnt), io.dev<int32_t>(o_bi),
                       io.dev<int32_t>(o_bd), split ? ev[1] : nullptr);
    if (split) (void)hipEventRecord(ev[2], c->stream);
  }
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = io.download(down);
  if (err == hipSuccess && io.staged) err = io.wait();  // (staged: get reads the downloaded block; unstaged: get is the copy, waited for below)
  bool corrupt = false;
  if (err == hipSuccess && io.staged) {
    const int32_t* bi = (const int32_t*)io.got(o_bi);
    for (size_t q = 0; q < NQ && !corrupt; ++q) corrupt = bi[q] < -1 || bi[q] >= n_max;
  }
  if (err == hipSuccess && !corrupt) {
    io.get(best_idx, o_bi, NQ * 4);
    io.get(best_dist, o_bd, NQ * 4);
    if (!io.staged) err = io.wait();
  }
  if (split && err == hipSuccess) {
    float a = 0.f, b = 0.f;
    if (hipEventElapsedTime(&a, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev[1], ev[2]) == hipSuccess)
      g_kernel_ms[0] = a, g_kernel_ms[1] = b;
  }
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  HIP_TRY(c, err);
  if (corrupt) return fail(c, ORBFE_EDEVICE, "%s: corrupt result", fn);
  drain_timers(c);
  return ORBFE_OK;
}

orbfe_status orbfe_debug_fuse_points_kernels(double* ms) {
  if (!ms) return ORBFE_EBADARG;
  ms[0] = g_kernel_ms[0], ms[1] = g_kernel_ms[1];
  return ORBFE_OK;
}

}  // extern "C"

// orbfe_sim3search.hip -- host side of orbfe_search_by_sim3_stored and orbfe_search_by_sim3_points_stored (include/orbfe.h, DESIGN
// 4.23): argument checks, one upload into the context's scratch (map state only: flags, positions, distance ranges, for the points
// overload their descriptors), one launch of k_sim3search.hip, one download, and for the pair the std::map merge of the two directions.
// The keyframes' features, descriptors and area grids are read where the keyframe store keeps them.
#include "orbfe_kfstore.h"

void launch_sim3_search_pair(hipStream_t st, const uint8_t* up, const Sim3Kf& C, const Sim3Kf& M, const Sim3SearchParams& P, int32_t* best_idx);
void launch_sim3_search_points(hipStream_t st, const uint8_t* up, const Sim3Kf& T, const Sim3Points& L, const Sim3SearchParams& P,
                               int32_t* best_idx, int32_t* best_dist);

namespace {

// what both calls check of the similarity, the camera and the scale factors
orbfe_status check_common(orbfe_ctx* c, const orbfe_kfstore* store, const char* fn, const float* model, float s, const orbfe_camera* cam,
                          const float* scale_factors, int32_t n_levels) {
  if (!model || !cam || !scale_factors || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS) return fail(c, ORBFE_EBADARG, "%s: bad arguments", fn);
  TRY(kfstore_check_ctx(c, store, fn));
  if (n_levels < store->n_levels) return fail(c, ORBFE_EBADARG, "%s: %d scale factors, the store's octaves go up to %d", fn, n_levels, store->n_levels - 1);
  if (!std::isfinite(s) || !(s > 0.f)) return fail(c, ORBFE_EBADARG, "%s: scale %g", fn, (double)s);
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(model[k])) return fail(c, ORBFE_EBADARG, "%s: model entry %d is not finite", fn, k);
  return ORBFE_OK;
}

void kf_arrays(Sim3Kf& d, const KfEntry* e) {
  d.kps = e->at<orbfe_keypoint>(e->o_kps), d.desc = e->at<uint8_t>(e->o_desc);
  d.cell_off = e->at<int32_t>(e->o_coff), d.cell_feat = e->at<int32_t>(e->o_cfeat);
  d.n = e->n, d.rows = e->ag.rows, d.cols = e->ag.cols, d.clip_w = e->ag.clip_w, d.clip_h = e->ag.clip_h;
  std::memcpy(d.bounds, e->bounds, sizeof d.bounds);
}

Sim3SearchParams search_params(const orbfe_camera* cam, const float* scale_factors, int32_t n_levels, float th, float ratio, int32_t dist_threshold,
                               size_t o_sf) {
  Sim3SearchParams P = {};
  P.fx = cam->fx, P.fy = cam->fy, P.cx = cam->cx, P.cy = cam->cy;
  P.th = th, P.ratio = ratio, P.dist_threshold = dist_threshold;
  P.log_sf = std::log(n_levels > 1 ? scale_factors[1] : 1.2f);
  P.max_level = std::min(7, n_levels - 1);
  P.o_sf = (uint32_t)o_sf;
  return P;
}

// the map state of one side in the upload
struct SideLayout {
  size_t o_state, o_pos, o_max, o_min;
  void take(ScratchLayout& L, size_t n) { o_state = L.take(n), o_pos = L.take<float>(n * 3), o_max = L.take<float>(n), o_min = L.take<float>(n); }
};

void put_side(StagedIo& io, const SideLayout& o, const orbfe_sim3_side* s, const std::vector<uint8_t>& state, Sim3Kf& d) {
  const size_t n = (size_t)s->n;
  io.put(o.o_state, state.data(), n);
  if (s->flags) {  // (without flags no row of the three arrays is read)
    io.put(o.o_pos, s->pos, n * 12);
    io.put(o.o_max, s->max_dist, n * 4);
    io.put(o.o_min, s->min_dist, n * 4);
  }
  d.o_state = (uint32_t)o.o_state, d.o_pos = (uint32_t)o.o_pos, d.o_max = (uint32_t)o.o_max, d.o_min = (uint32_t)o.o_min;
  std::memcpy(d.Rcw, s->Rcw, sizeof d.Rcw);
  std::memcpy(d.tcw, s->tcw, sizeof d.tcw);
}

}  // namespace

extern "C" {

orbfe_status orbfe_search_by_sim3_stored(orbfe_ctx* c, orbfe_kfstore* store, const orbfe_sim3_side* cur, const orbfe_sim3_side* match,
                                         const float* model, float s, int32_t n_matches, const orbfe_bow_match* matches, const orbfe_camera* cam,
                                         const float* scale_factors, int32_t n_levels, float th, float ratio, int32_t dist_threshold,
                                         orbfe_bow_match* new_matches, int32_t cap, int32_t* n_new) {
  ApiLock api_lk(c);
  const char* fn = "search_by_sim3_stored";
  if (!c || !store || !cur || !match || !n_new || cap < 0 || (cap > 0 && !new_matches) || n_matches < 0 || (n_matches > 0 && !matches))
    return fail(c, ORBFE_EBADARG, "%s: bad arguments", fn);
  TRY(check_common(c, store, fn, model, s, cam, scale_factors, n_levels));
  std::shared_lock<std::shared_timed_mutex> store_lk(store->mu);  // held until the results are down: no erase frees memory under the kernel
  const orbfe_sim3_side* side[2] = {cur, match};
  Sim3Kf kf[2] = {};
  for (int k = 0; k < 2; ++k) {
    const KfEntry* e = store->map.find(side[k]->id);
    if (!e) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)side[k]->id);
    if (e->n != side[k]->n) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu has %d features, the call says %d", fn, (unsigned long long)side[k]->id, e->n, side[k]->n);
    if (e->n > 0 && side[k]->flags && (!side[k]->pos || !side[k]->max_dist || !side[k]->min_dist)) return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
    kf_arrays(kf[k], e);
  }
  const size_t nc = (size_t)cur->n, nm = (size_t)match->n;
  for (int32_t k = 0; k < n_matches; ++k)
    if (matches[k].query < 0 || (size_t)matches[k].query >= nc || matches[k].train < 0 || (size_t)matches[k].train >= nm)
      return fail(c, ORBFE_EBADARG, "%s: match %d names (%d, %d), the keyframes have %zu and %zu features", fn, k, matches[k].query, matches[k].train, nc, nm);
  if (nc == 0 || nm == 0) {  // nothing to project, or nothing to find
    *n_new = 0;
    return ORBFE_OK;
  }
  // state = flags | SIM3S_NAMED: the reference's flagC / flagM (:433-440) and the map point's state in one byte per feature
  std::vector<uint8_t> state[2] = {std::vector<uint8_t>(nc, 0), std::vector<uint8_t>(nm, 0)};
  for (int k = 0; k < 2; ++k)
    if (side[k]->flags)
      for (size_t i = 0; i < state[k].size(); ++i) state[k][i] = side[k]->flags[i] & (ORBFE_TRI_GOOD | ORBFE_TRI_INMAP);
  for (int32_t k = 0; k < n_matches; ++k) state[0][(size_t)matches[k].query] |= SIM3S_NAMED, state[1][(size_t)matches[k].train] |= SIM3S_NAMED;

  // [ upload: scale factors | C's state, positions, ranges | M's ] [ download: best[n_c + n_m] ]
  ScratchLayout L;
  ScratchRegion up, down;
  SideLayout o[2];
  const size_t o_sf = L.open(up).take<float>((size_t)n_levels);
  o[0].take(L, nc), o[1].take(L, nm);
  const size_t o_best = L.close(up).open(down).take<int32_t>(nc + nm);
  L.close(down);
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  StagedIo io;
  TRY(io.reserve(c, L.end(), up.end + down.bytes()));
  io.put(o_sf, scale_factors, (size_t)n_levels * 4);
  for (int k = 0; k < 2; ++k) put_side(io, o[k], side[k], state[k], kf[k]);
  // direction A takes C's camera points into M through Scm.inv() (Sim3Ret::inv, Sim3Solver.h:36-43), direction B M's into C through Scm
  const float s_inv = 1.0f / s;
  kf[0].s = s_inv;
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) kf[0].R[3 * r + q] = model[3 * q + r];
  for (int r = 0; r < 3; ++r) {
    const float rt = kf[0].R[3 * r] * model[9] + kf[0].R[3 * r + 1] * model[10] + kf[0].R[3 * r + 2] * model[11];
    kf[0].t[r] = -s_inv * rt;
  }
  kf[1].s = s;
  std::memcpy(kf[1].R, model, sizeof kf[1].R);
  std::memcpy(kf[1].t, model + 9, sizeof kf[1].t);
  HIP_TRY(c, io.upload(up));
  const Sim3SearchParams P = search_params(cam, scale_factors, n_levels, th, ratio, dist_threshold, o_sf);
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    launch_sim3_search_pair(c->stream, io.d, kf[0], kf[1], P, io.dev<int32_t>(o_best));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down, up.end));  // (behind the staged inputs)
  drain_timers(c);
  // std::map::insert, first wins: A's (ic, best), then B's (best, im) in ascending im where the key is absent; out in ascending key
  const int32_t* best = (const int32_t*)io.got(o_best);
  std::vector<int32_t> fresh(nc, -1);
  int32_t total = 0;
  for (size_t ic = 0; ic < nc; ++ic) {
    if (best[ic] < -1 || best[ic] >= (int32_t)nm) return fail(c, ORBFE_EDEVICE, "%s: corrupt result", fn);
    if (best[ic] >= 0) fresh[ic] = best[ic], ++total;
  }
  for (size_t im = 0; im < nm; ++im) {
    const int32_t key = best[nc + im];
    if (key < -1 || key >= (int32_t)nc) return fail(c, ORBFE_EDEVICE, "%s: corrupt result", fn);
    if (key >= 0 && fresh[(size_t)key] < 0) fresh[(size_t)key] = (int32_t)im, ++total;
  }
  *n_new = total;
  if (total > cap) return fail(c, ORBFE_ECAPACITY, "%s: %d new matches, room for %d", fn, total, cap);
  int32_t w = 0;
  for (size_t ic = 0; ic < nc; ++ic)
    if (fresh[ic] >= 0) new_matches[w++] = {(int32_t)ic, fresh[ic], 0};
  return ORBFE_OK;
}

orbfe_status orbfe_search_by_sim3_points_stored(orbfe_ctx* c, orbfe_kfstore* store, uint64_t id, const orbfe_sim3_points* pts, const float* model,
                                                float s, const orbfe_camera* cam, const float* scale_factors, int32_t n_levels, float th,
                                                float ratio, int32_t dist_threshold, int32_t* best_idx, int32_t* best_dist) {
  ApiLock api_lk(c);
  const char* fn = "search_by_sim3_points_stored";
  if (!c || !store || !pts || pts->m < 0 || pts->m > (1 << 20)) return fail(c, ORBFE_EBADARG, "%s: bad arguments", fn);
  TRY(check_common(c, store, fn, model, s, cam, scale_factors, n_levels));
  std::shared_lock<std::shared_timed_mutex> store_lk(store->mu);
  const KfEntry* e = store->map.find(id);
  if (!e) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)id);
  const size_t m = (size_t)pts->m;
  if (m == 0) return ORBFE_OK;
  if (!pts->usable || !pts->pos || !pts->view_dir || !pts->max_dist || !pts->min_dist || !pts->desc || !best_idx || !best_dist)
    return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
  Sim3Kf T = {};
  kf_arrays(T, e);
  // [ upload: scale factors | usable | positions | view directions | ranges | descriptors ] [ download: best_idx | best_dist ]
  ScratchLayout L;
  ScratchRegion up, down;
  Sim3Points Q = {};
  const size_t o_sf = L.open(up).take<float>((size_t)n_levels);
  const size_t o_us = L.take(m), o_pos = L.take<float>(m * 3), o_vd = L.take<float>(m * 3), o_mx = L.take<float>(m), o_mn = L.take<float>(m),
               o_d = L.take(m * 32);
  const size_t o_bi = L.close(up).open(down).take<int32_t>(m), o_bd = L.take<int32_t>(m);
  L.close(down);
  Q.o_usable = (uint32_t)o_us, Q.o_pos = (uint32_t)o_pos, Q.o_vdir = (uint32_t)o_vd, Q.o_max = (uint32_t)o_mx, Q.o_min = (uint32_t)o_mn;
  Q.o_desc = (uint32_t)o_d, Q.m = pts->m, Q.s = s;
  std::memcpy(Q.R, model, sizeof Q.R);
  std::memcpy(Q.t, model + 9, sizeof Q.t);
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  // up to 8 MB: one upload and one download through the page-locked staging buffer; beyond, the arrays are copied directly
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes()), L.end() <= ((size_t)8 << 20)));
  io.put(o_sf, scale_factors, (size_t)n_levels * 4);
  io.put(o_us, pts->usable, m);
  io.put(o_pos, pts->pos, m * 12);
  io.put(o_vd, pts->view_dir, m * 12);
  io.put(o_mx, pts->max_dist, m * 4);
  io.put(o_mn, pts->min_dist, m * 4);
  io.put(o_d, pts->desc, m * 32);
  HIP_TRY(c, io.upload(up));
  const Sim3SearchParams P = search_params(cam, scale_factors, n_levels, th, ratio, dist_threshold, o_sf);
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    launch_sim3_search_points(c->stream, io.d, T, Q, P, io.dev<int32_t>(o_bi), io.dev<int32_t>(o_bd));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.download(down));
  if (io.staged) HIP_TRY(c, io.wait());  // (staged: get reads the downloaded block; unstaged: get is the copy, waited for below)
  if (io.staged) {
    const int32_t* bi = (const int32_t*)io.got(o_bi);
    for (size_t j = 0; j < m; ++j)
      if (bi[j] < -1 || bi[j] >= e->n) return fail(c, ORBFE_EDEVICE, "%s: corrupt result", fn);
  }
  io.get(best_idx, o_bi, m * 4);
  io.get(best_dist, o_bd, m * 4);
  if (!io.staged) HIP_TRY(c, io.wait());
  drain_timers(c);
  return ORBFE_OK;
}

}  // extern "C"

// orbfe_guided.hip -- the matchers beside the stereo match: brute-force getBestMatch loops, the grid-guided searches (findFeaturesInArea +
// getBestMatch, ORBMatcher.cc:265-347, 561-612), MapPoint::isInVision / predictLevel, and the fused tracking chains
// (orbfe_track_local_map / orbfe_track_motion_model).  (Split from orbfe_api.hip in r5, no change of behaviour.)
#include "orbfe_ctx.h"
#include "orbfe_mpstore.h"
#include "pose_call.h"

// the grid of `slot` for the geometry ag on stream st: the one kept from the last search if the slot's keypoints are still the same
orbfe_status slot_grid(orbfe_ctx* c, hipStream_t st, int slot, const AreaGrid& ag, const int32_t** d_off, const int32_t** d_feat) {
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1), M = (size_t)c->cfg.max_images, ncells = (size_t)ag.rows * ag.cols;
  if (ncells + 1 > c->grid_cells) {  // first use, or a larger grid than any before: (re)allocate, nothing cached survives
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->d_grid_off) (void)hipFree(c->d_grid_off);
    if (!c->d_grid_feat) HIP_TRY(c, hipMalloc((void**)&c->d_grid_feat, M * NF * sizeof(int32_t)));
    c->d_grid_off = nullptr;
    HIP_TRY(c, hipMalloc((void**)&c->d_grid_off, M * (ncells + 1) * sizeof(int32_t)));
    c->grid_cells = ncells + 1;
    for (size_t k = 0; k < M; ++k) grid_invalidate(c, (int)k);
  }
  int32_t* off = c->d_grid_off + (size_t)slot * c->grid_cells;
  int32_t* feat = c->d_grid_feat + (size_t)slot * NF;
  const uint32_t key = ((uint32_t)ag.rows << 16) | (uint32_t)ag.cols;
  uint64_t seen = c->grid_key[(size_t)slot].load();
  if ((uint32_t)seen != key) {
    launch_grid_build(st, c->d_kps + (size_t)slot * NF, c->d_n_kp + slot, (int)NF, ag.rows, ag.cols, off, feat);
    // kept for the next search only if no extraction touched the slot since `seen` (its generation is part of the compared value); on
    // failure nothing is cached: this call still uses what it built, the next one builds again
    (void)c->grid_key[(size_t)slot].compare_exchange_strong(seen, (seen & 0xFFFFFFFF00000000ull) | key);
  }
  *d_off = off, *d_feat = feat;
  return ORBFE_OK;
}

extern "C" {

orbfe_status orbfe_match_bruteforce(orbfe_ctx* c, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, const uint32_t* cand_offsets,
                                    const uint32_t* cand_idx, int32_t* best_idx, int32_t* best_dist, int32_t* second_dist) {
  ApiLock api_lk(c);
  if (!c || nq < 0 || nt < 0 || (nq && !q) || (nt && !t) || !best_idx || !best_dist || !second_dist)
    return fail(c, ORBFE_EBADARG, "match_bruteforce: NULL argument");
  if (cand_offsets && !cand_idx && cand_offsets[nq] > 0) return fail(c, ORBFE_EBADARG, "match_bruteforce: cand_idx is NULL");
  if (nq == 0) return ORBFE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t n_cand = cand_offsets ? cand_offsets[nq] : 0, NQ = (size_t)nq;
  if (cand_offsets)
    for (size_t i = 0; i < n_cand; ++i)
      if (cand_idx[i] >= (uint32_t)nt) return fail(c, ORBFE_EBADARG, "match_bruteforce: candidate %u >= nt %d", cand_idx[i], nt);
  ScratchLayout L;
  ScratchRegion up, out;
  const size_t o_q = L.open(up).take(NQ * 32), o_t = L.take((size_t)nt * 32),
               o_off = L.take<uint32_t>(NQ + 1),  // k_match_bruteforce reads off[i + 1] of the last query
               o_cand = L.take<uint32_t>(n_cand), o_bi = L.close(up).open(out).take<int32_t>(NQ), o_bd = L.take<int32_t>(NQ),
               o_sd = L.take<int32_t>(NQ);
  L.close(out);
  // up to 8 MB: one upload and one download through the page-locked staging buffer (seven copies from / to pageable memory otherwise)
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, out.bytes()), L.end() <= ((size_t)8 << 20)));
  io.put(o_q, q, NQ * 32);
  io.put(o_t, t, (size_t)nt * 32);
  if (cand_offsets) {
    io.put(o_off, cand_offsets, (NQ + 1) * 4);
    io.put(o_cand, cand_idx, n_cand * 4);
  }
  HIP_TRY(c, io.upload(up));
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    launch_match_bruteforce(c->stream, io.dev<uint8_t>(o_q), nq, io.dev<uint8_t>(o_t), nt, cand_offsets ? io.dev<uint32_t>(o_off) : nullptr,
                            io.dev<uint32_t>(o_cand), io.dev<int32_t>(o_bi), io.dev<int32_t>(o_bd), io.dev<int32_t>(o_sd));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.download(out));
  if (io.staged) HIP_TRY(c, io.wait());  // (staged: get reads the downloaded block; unstaged: get is the copy, waited for below)
  io.get(best_idx, o_bi, NQ * 4);
  io.get(best_dist, o_bd, NQ * 4);
  io.get(second_dist, o_sd, NQ * 4);
  if (!io.staged) HIP_TRY(c, io.wait());
  drain_timers(c);
  return ORBFE_OK;
}

// The grid-guided search against a feature set on the device: the features of an image slot (orbfe_search_in_area) or a set the caller
// uploaded (orbfe_search_in_area_features: a KeyFrame's keypoints and descriptors -- keyframes are not resident in a slot).
// (AreaGrid, area_grid and the search's scratch layout: search_area_layout.h)
// the grid and the scratch layout of a search behind `start` bytes of the caller's own: the callers size their reservation from l->end()
static orbfe_status search_area_plan(orbfe_ctx* c, const char* who, const float* bounds, size_t start, size_t n_target, int32_t nq,
                                     SearchAreaLayout* l) {
  AreaGrid ag;
  TRY(check_area_grid(c, who, bounds, n_target, &ag));
  *l = search_area_layout(start, ag, n_target, (size_t)nq);
  return ORBFE_OK;
}

static orbfe_status search_area_core(orbfe_ctx* c, const char* who, StagedIo& io, const SearchAreaLayout& l,
                                     const orbfe_keypoint* d_kps, const int32_t* d_n_kp, const uint4* d_kpl, const uint8_t* d_desc,
                                     size_t n_target, int32_t nq, const float* qxy, const float* radius, const int8_t* min_level,
                                     const int8_t* max_level, const uint8_t* q_desc, const uint8_t* exclude, int32_t* best_idx,
                                     int32_t* best_dist, int32_t* second_dist, int32_t* n_cand, int32_t* excluded_hits = nullptr,
                                     bool staged_prefix = false, int cache_slot = -1) {
  // staged_prefix: the caller has written the bytes in front of the layout into the staging buffer (same offsets): they go up
  // with the queries.  cache_slot >= 0: the target is that slot -- its grid is kept between searches (slot_grid)
  if (l.end() > c->tmp_bytes) return fail(c, ORBFE_ENOMEM, "%s: scratch not reserved", who);  // (the callers reserve before they upload)
  const size_t NQ = (size_t)nq;
  const AreaGrid& ag = l.grid;
  const bool hits = exclude && excluded_hits;
  io.put(l.o_q, qxy, NQ * 8);
  io.put(l.o_r, radius, NQ * 4);
  io.put(l.o_lo, min_level, NQ);
  io.put(l.o_hi, max_level, NQ);
  io.put(l.o_d, q_desc, NQ * 32);
  if (exclude) io.put(l.o_ex, exclude, n_target);
  HIP_TRY(c, io.upload(staged_prefix ? ScratchRegion{0, l.in.end} : l.in));
  if (hits && n_target) HIP_TRY(c, hipMemsetAsync(io.dev<uint8_t>(l.o_eh), 0, n_target * 4, c->stream));
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    const int32_t *g_off = io.dev<int32_t>(l.o_co), *g_feat = io.dev<int32_t>(l.o_cf);
    if (cache_slot >= 0)
      TRY(slot_grid(c, c->stream, cache_slot, ag, &g_off, &g_feat));
    else
      launch_grid_build(c->stream, d_kps, d_n_kp, (int)std::max<size_t>(n_target, 1), ag.rows, ag.cols, io.dev<int32_t>(l.o_co),
                        io.dev<int32_t>(l.o_cf));
    launch_search_area(c->stream, d_kpl, d_desc, ag.clip_w, ag.clip_h, ag.rows, ag.cols, g_off, g_feat, nq, io.dev<float>(l.o_q),
                       io.dev<float>(l.o_r), io.dev<int8_t>(l.o_lo), io.dev<int8_t>(l.o_hi), io.dev<uint8_t>(l.o_d),
                       exclude ? io.dev<uint8_t>(l.o_ex) : nullptr, io.dev<int32_t>(l.o_bi), io.dev<int32_t>(l.o_bd), io.dev<int32_t>(l.o_sd),
                       io.dev<int32_t>(l.o_nc), hits ? io.dev<int32_t>(l.o_eh) : nullptr);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(hits ? l.out : l.out.upto(l.o_eh)));
  drain_timers(c);
  io.get(best_idx, l.o_bi, NQ * 4);
  io.get(best_dist, l.o_bd, NQ * 4);
  io.get(second_dist, l.o_sd, NQ * 4);
  io.get(n_cand, l.o_nc, NQ * 4);
  if (hits) io.get(excluded_hits, l.o_eh, n_target * 4);
  else if (excluded_hits && n_target) std::memset(excluded_hits, 0, n_target * 4);
  return ORBFE_OK;
}

orbfe_status orbfe_search_in_area(orbfe_ctx* c, int32_t slot, int32_t nq, const float* qxy, const float* radius, const int8_t* min_level,
                                  const int8_t* max_level, const uint8_t* q_desc, const uint8_t* exclude, int32_t* best_idx,
                                  int32_t* best_dist, int32_t* second_dist, int32_t* n_cand) {
  ApiLock api_lk(c);
  if (!c || slot < 0 || slot >= c->cfg.max_images || nq < 0) return fail(c, ORBFE_EBADARG, "search_in_area: bad slot / count");
  if (nq && (!qxy || !radius || !min_level || !max_level || !q_desc || !best_idx || !best_dist || !second_dist || !n_cand))
    return fail(c, ORBFE_EBADARG, "search_in_area: NULL argument");
  if (nq == 0) return ORBFE_OK;
  TRY(slots_idle(c, slot, 1, "search_in_area"));
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1);
  SearchAreaLayout l;
  TRY(search_area_plan(c, "search_in_area", nullptr, 0, NF, nq, &l));
  StagedIo io;
  TRY(io.reserve(c, l.end(), std::max(l.in.end, l.out.bytes())));
  return search_area_core(c, "search_in_area", io, l, c->d_kps + (size_t)slot * NF, c->d_n_kp + slot, c->d_kpl + (size_t)slot * NF,
                          c->d_desc + (size_t)slot * NF * 32, NF, nq, qxy, radius, min_level, max_level, q_desc, exclude, best_idx, best_dist,
                          second_dist, n_cand, nullptr, false, slot);
}

orbfe_status orbfe_search_in_area_features(orbfe_ctx* c, int32_t nt, const orbfe_keypoint* t_kps, const uint8_t* t_desc, int32_t nq,
                                           const float* qxy, const float* radius, const int8_t* min_level, const int8_t* max_level,
                                           const uint8_t* q_desc, const uint8_t* exclude, int32_t* best_idx, int32_t* best_dist,
                                           int32_t* second_dist, int32_t* n_cand) {
  return orbfe_search_in_area_features_ex(c, nt, t_kps, t_desc, nullptr, nq, qxy, radius, min_level, max_level, q_desc, exclude, best_idx,
                                          best_dist, second_dist, n_cand, nullptr);
}

orbfe_status orbfe_search_in_area_features_ex(orbfe_ctx* c, int32_t nt, const orbfe_keypoint* t_kps, const uint8_t* t_desc,
                                              const float* bounds, int32_t nq, const float* qxy, const float* radius,
                                              const int8_t* min_level, const int8_t* max_level, const uint8_t* q_desc, const uint8_t* exclude,
                                              int32_t* best_idx, int32_t* best_dist, int32_t* second_dist, int32_t* n_cand,
                                              int32_t* excluded_hits) {
  ApiLock api_lk(c);
  if (!c || nt < 0 || nq < 0 || (nt && (!t_kps || !t_desc))) return fail(c, ORBFE_EBADARG, "search_in_area_features: bad count / NULL features");
  if (nq && (!qxy || !radius || !min_level || !max_level || !q_desc || !best_idx || !best_dist || !second_dist || !n_cand))
    return fail(c, ORBFE_EBADARG, "search_in_area_features: NULL argument");
  if (excluded_hits && nt) std::memset(excluded_hits, 0, (size_t)nt * 4);
  if (nq == 0) return ORBFE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t NT = (size_t)nt;
  // the uploaded feature set at the front of the scratch: keypoints | octave list in the layout of the slot arrays | descriptors | count
  ScratchLayout L;
  const size_t o_k = L.take<orbfe_keypoint>(NT), o_l = L.take<uint4>(NT), o_d = L.take(NT * 32), o_n = L.take<int32_t>(1);
  SearchAreaLayout l;
  TRY(search_area_plan(c, "search_in_area_features", bounds, L.end(), NT, nq, &l));
  StagedIo io;
  TRY(io.reserve(c, l.end(), std::max(l.in.end, l.out.bytes())));
  uint4* kpl = io.host<uint4>(o_l);  // (built in the staging buffer: it goes up with everything else)
  std::memset(kpl, 0, NT * sizeof(uint4));
  for (int i = 0; i < nt; ++i) {
    // caller-supplied features (a KeyFrame's undistorted mvFeatsLeft): coordinates may lie outside the image or be non-finite -- the grid
    // kernel clamps them into the border cells; the octave must be one a pyramid can have (it is compared as an unsigned byte)
    if (t_kps[i].octave < 0 || t_kps[i].octave >= ORBFE_MAX_LEVELS)
      return fail(c, ORBFE_EBADARG, "search_in_area_features: feature %d has octave %d (0..%d expected)", i, t_kps[i].octave, ORBFE_MAX_LEVELS - 1);
    kpl[(size_t)i].y = (uint32_t)t_kps[i].octave;  // the search reads the octave from here
  }
  io.put(o_k, t_kps, NT * sizeof(orbfe_keypoint));
  io.put(o_d, t_desc, NT * 32);
  io.put(o_n, &nt, 4);
  return search_area_core(c, "search_in_area_features", io, l, io.dev<orbfe_keypoint>(o_k), io.dev<int32_t>(o_n), io.dev<uint4>(o_l),
                          io.dev<uint8_t>(o_d), NT, nq, qxy, radius, min_level, max_level, q_desc, exclude, best_idx, best_dist, second_dist,
                          n_cand, excluded_hits, true);
}

orbfe_status orbfe_project_map_points(orbfe_ctx* c, int32_t n, const float* pos, const float* view_dir, const float* max_dist,
                                      const float* min_dist, const orbfe_frame_pose* pose, const orbfe_camera* cam, float* uv,
                                      float* distance, float* cos_theta, int8_t* level, uint8_t* visible) {
  ApiLock api_lk(c);
  if (!c || n < 0 || !pose || !cam) return fail(c, ORBFE_EBADARG, "project_map_points: NULL argument");
  if (n && (!pos || !view_dir || !max_dist || !min_dist || !uv || !distance || !cos_theta || !level || !visible))
    return fail(c, ORBFE_EBADARG, "project_map_points: NULL argument");
  if (n == 0) return ORBFE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t N = (size_t)n;
  ScratchLayout L;
  ScratchRegion up, out;
  const size_t o_p = L.open(up).take<float>(N * 3), o_v = L.take<float>(N * 3), o_mx = L.take<float>(N), o_mn = L.take<float>(N),
               o_uv = L.close(up).open(out).take<float>(N * 2), o_d = L.take<float>(N), o_c = L.take<float>(N), o_l = L.take(N), o_s = L.take(N);
  L.close(out);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, out.bytes())));  // one copy up, one down, through the page-locked staging buffer
  io.put(o_p, pos, N * 12);
  io.put(o_v, view_dir, N * 12);
  io.put(o_mx, max_dist, N * 4);
  io.put(o_mn, min_dist, N * 4);
  HIP_TRY(c, io.upload(up));
  const float cam4[4] = {cam->fx, cam->fy, cam->cx, cam->cy};
  const float bounds4[4] = {pose->min_u, pose->max_u, pose->min_v, pose->max_v};
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    // std::log(ORBExtractor::mfScaledFactor): float argument, float result
    launch_project_map_points(c->stream, n, io.dev<float>(o_p), io.dev<float>(o_v), io.dev<float>(o_mx), io.dev<float>(o_mn), pose->Rcw,
                              pose->tcw, cam4, bounds4, std::log(c->cfg.scale_factor), 7, io.dev<float>(o_uv), io.dev<float>(o_d),
                              io.dev<float>(o_c), io.dev<int8_t>(o_l), io.dev<uint8_t>(o_s));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(out));
  drain_timers(c);
  io.get(uv, o_uv, N * 8);
  io.get(distance, o_d, N * 4);
  io.get(cos_theta, o_c, N * 4);
  io.get(level, o_l, N);
  io.get(visible, o_s, N);
  return ORBFE_OK;
}
// what both tracking chains hand back from their downloaded block: the counts, the pose, the assignment and the inlier flag of every feature
static void track_results(StagedIo& io, size_t o_cnt, const PoseWorkspace& W, size_t o_asg, const orbfe_track_output* out) {
  const int32_t *cnt = (const int32_t*)io.got(o_cnt), *eo = (const int32_t*)io.got(W.o_eo);
  const uint8_t* ein = io.got(W.o_ei);
  *out->n_matches = cnt[0];
  *out->n_edges = cnt[1];
  io.get(out->n_good, W.o_ng, 4);
  io.get(out->pose_out, W.o_p1, 56);
  io.get(out->assigned, o_asg, W.NF * 4);
  for (size_t f = 0; f < W.NF; ++f) out->inlier[f] = (cnt[1] >= 0 && eo[f] >= 0) ? ein[eo[f]] : 0;
  io.get(out->edge_of, W.o_eo, W.NF * 4);
}

// ---- orbfe_track_local_map and orbfe_track_local_map_stored: their own first step (the point arrays onto the device), one shared rest ----
// The scratch of either call.  Array call: [ upload: point arrays, flags, frame | claim (0x7F fill) | device-only | download ], as ever.
// Stored call: [ download | bad | upload: ids, flags, frame | claim | device-only, the gathered point arrays among it ] -- `bad`, the word
// the gather sets for an id without a row, is the LAST take of the download and the FIRST of the upload: it goes up as 0 with the
// inputs and comes down with the results, so no fill of its own and no second synchronisation.
struct TrackLayout {
  size_t o_pos, o_vd, o_mx, o_mn, o_desc, o_ids = 0, o_bad = 0, o_fl, o_held, o_claim, o_uv, o_dist, o_cos, o_lvl, o_vis, o_rad, o_lo, o_hi, o_bi,
      o_bd, o_sd, o_nc, o_cnt, o_asg, end;
  PoseWorkspace W;  // the seed goes up with the frame, the results come down
  FrameUpload U;
  ScratchRegion up, claim, down;
  TrackLayout(size_t N, size_t NF, size_t nl, bool stored) : W(NF) {
    ScratchLayout L;
    auto points = [&] { o_pos = L.take<float>(N * 3), o_vd = L.take<float>(N * 3), o_mx = L.take<float>(N), o_mn = L.take<float>(N), o_desc = L.take(N * 32); };
    auto frame = [&] { o_fl = L.take(N), o_held = L.take<int32_t>(NF), U.take(L, NF, nl), W.take_seed(L); };
    auto results = [&] { o_cnt = L.take(16), W.take_results(L), o_asg = L.take<int32_t>(NF); };
    if (stored) {
      L.open(down), results(), o_bad = L.open(up).take(8), L.close(down);
      o_ids = L.take<uint64_t>(N), frame(), L.close(up);
    } else {
      L.open(up), points(), frame(), L.close(up);
    }
    o_claim = L.open(claim).take<int32_t>(NF), L.close(claim);
    if (stored) points();
    o_uv = L.take<float>(N * 2), o_dist = L.take<float>(N), o_cos = L.take<float>(N), o_lvl = L.take(N), o_vis = L.take(N), o_rad = L.take<float>(N),
    o_lo = L.take(N), o_hi = L.take(N), o_bi = L.take<int32_t>(N), o_bd = L.take<int32_t>(N), o_sd = L.take<int32_t>(N), o_nc = L.take<int32_t>(N);
    W.take_list(L);
    if (!stored) L.open(down), results(), L.close(down);
    end = L.end();
  }
};

// what both calls check alike and do before they touch the device.  have_points: the caller's own point arrays (or ids) are there --
// reported with the other NULL arrays, behind the NULL-argument / bad-slot check, as orbfe_track_local_map always did
static orbfe_status track_begin(orbfe_ctx* c, const char* who, int32_t slot, const orbfe_frame_pose* pose, const orbfe_camera* cam,
                                const orbfe_track_input* in, bool have_points, const orbfe_track_output* out, AreaGrid* ag) {
  if (!c || !pose || !cam || !in || !out || slot < 0 || slot >= c->cfg.max_images) return fail(c, ORBFE_EBADARG, "%s: NULL argument / bad slot", who);
  const int n = in->n_mp;
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1);
  if (n < 0 || !in->pose_se3 || !in->level_sigma2 || !in->level_inv_sigma2 || !out->assigned || !out->n_matches || !out->n_edges || !out->n_good ||
      !out->pose_out || !out->inlier || (n && (!have_points || !in->flags)))
    return fail(c, ORBFE_EBADARG, "%s: NULL array", who);
  TRY(pose_check_features(c, who, NF));
  if (in->held) TRY(check_held(c, who, in->held, NF, n));
  const float bounds[4] = {pose->min_u, pose->max_u, pose->min_v, pose->max_v};
  TRY(check_area_grid(c, who, bounds, NF, ag));
  TRY(slots_idle(c, slot, 1, who));
  HIP_TRY(c, hipSetDevice(c->device));
  return join_stereo(c);
}

// the flags and the frame's side of the upload into the staging buffer
static void track_put_frame(StagedIo& io, const TrackLayout& T, size_t N, size_t NF, size_t nl, const orbfe_track_input* in) {
  io.put(T.o_fl, in->flags, N);
  if (in->held) io.put(T.o_held, in->held, NF * 4);
  else std::memset(io.host<uint8_t>(T.o_held), 0xFF, NF * 4);
  put_frame(io, T.U, NF, nl, in->right_u, in->level_sigma2, in->level_inv_sigma2);
  io.put(T.W.o_p0, in->pose_se3, 56);
}

// The rest, with the point arrays, the flags and the frame's inputs on the device: the claim fill, the six launches from
// launch_project_map_points to launch_pose_only, the one download.  The caller reads the results (track_results).
static orbfe_status track_chain(orbfe_ctx* c, StagedIo& io, const TrackLayout& T, int32_t slot, const AreaGrid& ag, const orbfe_frame_pose* pose,
                                const orbfe_camera* cam, const orbfe_track_input* in) {
  const int n = in->n_mp, nl = c->cfg.n_levels;
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1);
  hipStream_t st = c->stream;
  uint8_t* b = io.d;
  HIP_TRY(c, hipMemsetAsync(b + T.claim.begin, 0x7F, T.claim.bytes(), st));
  const float cam4[4] = {cam->fx, cam->fy, cam->cx, cam->cy};
  const float bounds[4] = {pose->min_u, pose->max_u, pose->min_v, pose->max_v};
  const PoseFrameDev F = pose_frame(c, slot, b, T.U);
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, st);
    launch_project_map_points(st, n, (const float*)(b + T.o_pos), (const float*)(b + T.o_vd), (const float*)(b + T.o_mx), (const float*)(b + T.o_mn),
                              pose->Rcw, pose->tcw, cam4, bounds, std::log(c->cfg.scale_factor), 7, (float*)(b + T.o_uv), (float*)(b + T.o_dist),
                              (float*)(b + T.o_cos), (int8_t*)(b + T.o_lvl), b + T.o_vis);
    launch_track_queries(st, n, b + T.o_fl, b + T.o_vis, (const float*)(b + T.o_cos), (const int8_t*)(b + T.o_lvl), in->th, F.sigma2,
                         nl, (float*)(b + T.o_rad), (int8_t*)(b + T.o_lo), (int8_t*)(b + T.o_hi));
    const int32_t *g_off = nullptr, *g_feat = nullptr;
    TRY(slot_grid(c, st, slot, ag, &g_off, &g_feat));
    launch_search_area(st, c->d_kpl + (size_t)slot * NF, c->d_desc + (size_t)slot * NF * 32, ag.clip_w, ag.clip_h, ag.rows, ag.cols,
                       g_off, g_feat, n, (const float*)(b + T.o_uv), (const float*)(b + T.o_rad),
                       (const int8_t*)(b + T.o_lo), (const int8_t*)(b + T.o_hi), b + T.o_desc, nullptr, (int32_t*)(b + T.o_bi), (int32_t*)(b + T.o_bd),
                       (int32_t*)(b + T.o_sd), (int32_t*)(b + T.o_nc), nullptr);
    launch_track_claim(st, n, (const int32_t*)(b + T.o_nc), (const int32_t*)(b + T.o_bi), (const int32_t*)(b + T.o_bd), (const int32_t*)(b + T.o_sd),
                       in->min_threshold, in->ratio, (int32_t*)(b + T.o_claim));
    launch_track_edges(st, F, pose_edges(T.W, b), (const int32_t*)(b + T.o_held), (const int32_t*)(b + T.o_claim), b + T.o_fl,
                       (const float*)(b + T.o_pos), in->min_matches, (int32_t*)(b + T.o_asg), (int32_t*)(b + T.o_cnt));
  }
  pose_optimise(c, st, T.W, b, cam, 0, (const int32_t*)(b + T.o_cnt) + 1);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(T.down));
  drain_timers(c);
  return ORBFE_OK;
}

// Tracking::trackLocalMap's device work as ONE call (src/Tracking.cc:641-675): isInVision / predictLevel per map point
// (MapPoint.cc:141-201), ORBMatcher::searchByProjection(frame, map points, th) (ORBMatcher.cc:561-612) against the features of `slot`,
// and Optimizer::OptimizePoseOnly (Optimizer.cc:33-178) on what the frame holds afterwards -- one upload, seven launches, one download;
// the projections, the windows, the candidate lists, the assignment and the edge list never leave the device.
orbfe_status orbfe_track_local_map(orbfe_ctx* c, int32_t slot, const orbfe_frame_pose* pose, const orbfe_camera* cam, const orbfe_track_input* in,
                                   const orbfe_track_output* out) {
  ApiLock api_lk(c);
  AreaGrid ag;
  TRY(track_begin(c, "track_local_map", slot, pose, cam, in, in && in->pos && in->view_dir && in->max_dist && in->min_dist && in->desc, out, &ag));
  const size_t N = (size_t)in->n_mp, NF = (size_t)std::max(c->cfg.n_features, 1), nl = (size_t)c->cfg.n_levels;
  const TrackLayout T(N, NF, nl, false);
  StagedIo io;
  TRY(io.reserve(c, T.end, std::max(T.up.end, T.down.bytes())));
  io.put(T.o_pos, in->pos, N * 12);
  io.put(T.o_vd, in->view_dir, N * 12);
  io.put(T.o_mx, in->max_dist, N * 4);
  io.put(T.o_mn, in->min_dist, N * 4);
  io.put(T.o_desc, in->desc, N * 32);
  track_put_frame(io, T, N, NF, nl, in);
  HIP_TRY(c, io.upload(T.up));
  TRY(track_chain(c, io, T, slot, ag, pose, cam, in));
  track_results(io, T.o_cnt, T.W, T.o_asg, out);
  return ORBFE_OK;
}

// orbfe_track_local_map with the map points named by id in a map-point store (include/orbfe.h): 8 bytes of id and the flag
// go up per point instead of 73; k_mpstore_gather fills the point arrays in front of the same chain.  The store's lock is held shared
// until the results are down: no upsert or erase touches a row or a page under the running kernels.
orbfe_status orbfe_track_local_map_stored(orbfe_ctx* c, int32_t slot, orbfe_mpstore* store, const orbfe_frame_pose* pose, const orbfe_camera* cam,
                                          const orbfe_track_stored_input* sin, const orbfe_track_output* out) {
  ApiLock api_lk(c);
  const char* who = "track_local_map_stored";
  if (!c || !store || !sin) return fail(c, ORBFE_EBADARG, "%s: NULL argument", who);
  if (sin->n_mp > (1 << 24)) return fail(c, ORBFE_EBADARG, "%s: more than 2^24 ids", who);
  TRY(mpstore_check_ctx(c, store, who));
  const orbfe_track_input in_v = {sin->n_mp, nullptr, nullptr, nullptr, nullptr, nullptr, sin->flags, sin->held, sin->right_u, sin->level_sigma2,
                                  sin->level_inv_sigma2, sin->pose_se3, sin->th, sin->ratio, sin->min_threshold, sin->min_matches};
  const orbfe_track_input* in = &in_v;
  AreaGrid ag;
  TRY(track_begin(c, who, slot, pose, cam, in, sin->ids != nullptr, out, &ag));
  const int n = in->n_mp;
  const size_t N = (size_t)n, NF = (size_t)std::max(c->cfg.n_features, 1), nl = (size_t)c->cfg.n_levels;
  const TrackLayout T(N, NF, nl, true);
  StagedIo io;
  TRY(io.reserve(c, T.end, std::max(T.up.end, T.down.bytes())));
  io.put(T.o_ids, sin->ids, N * 8);
  *io.host<uint32_t>(T.o_bad) = 0;
  track_put_frame(io, T, N, NF, nl, in);
  std::shared_lock<std::shared_timed_mutex> lk(store->mu);
  HIP_TRY(c, io.upload(T.up));
  uint8_t* b = io.d;
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    launch_mpstore_gather(c->stream, store->table(), n, (const uint64_t*)(b + T.o_ids),
                          MpArrays{(float*)(b + T.o_pos), (float*)(b + T.o_vd), (float*)(b + T.o_mx), (float*)(b + T.o_mn), b + T.o_desc}, b + T.o_fl,
                          (uint32_t*)(b + T.o_bad));
  }
  TRY(track_chain(c, io, T, slot, ag, pose, cam, in));
  if (*(const uint32_t*)io.got(T.o_bad)) {
    for (int i = 0; i < n; ++i)
      if (!store->idx.has(sin->ids[i]))
        return fail(c, ORBFE_EBADARG, "%s: map point %llu (ids[%d]) is not in the store", who, (unsigned long long)sin->ids[i], i);
    return fail(c, ORBFE_EDEVICE, "%s: the device holds no row for an id the store's index lists", who);
  }
  track_results(io, T.o_cnt, T.W, T.o_asg, out);
  return ORBFE_OK;
}

// The middle of Tracking::trackMotionModel (src/Tracking.cc:382-396) as one call: ORBMatcher::searchByProjection(frame, lastFrame, matches, th)
// -- in this reference a search around the LAST frame's feature positions, no projection (src/ORBMatcher.cc:265-347) -- then, with fewer than
// min_matches matches, the same search again with th_second among the features still free, then Optimizer::OptimizePoseOnly(frame).  The
// second search is decided on the host (one more synchronisation in the rare frame that needs it).
orbfe_status orbfe_track_motion_model(orbfe_ctx* c, int32_t slot, const float* bounds4, const orbfe_camera* cam, const orbfe_motion_input* in,
                                      const orbfe_track_output* out, int32_t* excluded_hits, int32_t* query_matches, int32_t* passes) {
  ApiLock api_lk(c);
  if (!c || !bounds4 || !cam || !in || !out || slot < 0 || slot >= c->cfg.max_images) return fail(c, ORBFE_EBADARG, "track_motion_model: NULL argument / bad slot");
  const int n = in->n, nl = c->cfg.n_levels;
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1);
  if (n < 0 || !in->pose_se3 || !in->level_sigma2 || !in->level_inv_sigma2 || !out->assigned || !out->n_matches || !out->n_edges || !out->n_good ||
      !out->pose_out || !out->inlier || (n && (!in->qxy || !in->q_octave || !in->q_min_level || !in->q_max_level || !in->desc || !in->pos)))
    return fail(c, ORBFE_EBADARG, "track_motion_model: NULL array");
  for (int i = 0; i < n; ++i)
    if (in->q_octave[i] < 0 || in->q_octave[i] >= nl) return fail(c, ORBFE_EBADARG, "track_motion_model: q_octave[%d] = %d", i, (int)in->q_octave[i]);
  const char* fn = "track_motion_model";
  TRY(pose_check_features(c, fn, NF));
  if (in->held) TRY(check_held(c, fn, in->held, NF, n));
  AreaGrid ag;
  TRY(check_area_grid(c, fn, bounds4, NF, &ag));
  TRY(slots_idle(c, slot, 1, fn));
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t N = (size_t)n;
  // [ upload once | upload per pass | claim (-1 fill) | hits and counter (0 fill) | device-only | download ]
  ScratchLayout L;
  ScratchRegion up, up_pass, claim, zero, down;
  PoseWorkspace W(NF);
  FrameUpload U;
  const size_t o_qxy = L.open(up).take<float>(N * 2), o_lo = L.take(N), o_hi = L.take(N), o_desc = L.take(N * 32), o_pos = L.take<float>(N * 3),
               o_fl = L.take(N), o_rad = W.take_seed(U.take(L, NF, (size_t)nl)).open(up_pass).take<float>(N), o_held = L.take<int32_t>(NF),
               o_ex = L.take(NF),
               o_claim = L.close(up_pass).close(up).open(claim).take<int32_t>(NF), o_eh = L.close(claim).open(zero).take<int32_t>(NF),
               o_acc = L.take(16), o_qa = L.take(N), o_bi = L.close(zero).take<int32_t>(N), o_bd = L.take<int32_t>(N), o_sd = L.take<int32_t>(N),
               o_nc = L.take<int32_t>(N), o_cnt = W.take_list(L).open(down).take(16), o_asg = W.take_results(L).take<int32_t>(NF),
               o_ehd = L.take<int32_t>(NF), o_qad = L.take(N);
  L.close(down);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  uint8_t* b = io.d;
  io.put(o_qxy, in->qxy, N * 8);
  io.put(o_lo, in->q_min_level, N);
  io.put(o_hi, in->q_max_level, N);
  io.put(o_desc, in->desc, N * 32);
  io.put(o_pos, in->pos, N * 12);
  std::memset(io.host<uint8_t>(o_fl), 3, N);  // every query is a good map point in the map (the caller's filter, ORBMatcher.cc:286-289)
  put_frame(io, U, NF, (size_t)nl, in->right_u, in->level_sigma2, in->level_inv_sigma2);
  io.put(W.o_p0, in->pose_se3, 56);
  std::vector<int32_t> held(NF, -1);
  if (in->held) std::memcpy(held.data(), in->held, NF * 4);
  std::vector<int32_t> hits_total(excluded_hits ? NF : 0, 0), qm_total(query_matches ? N : 0, 0);
  hipStream_t st = c->stream;
  const PoseFrameDev F = pose_frame(c, slot, b, U);
  int base_matches = 0, n_pass = 0;
  const int32_t* cnt = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    const float th = pass == 0 ? in->th : in->th_second;
    if (pass == 1 && !(th > 0)) break;
    // the per-pass upload: radius, what the features hold, and the candidates that are excluded (a feature that holds a map point: :322-331)
    for (int i = 0; i < n; ++i) io.host<float>(o_rad)[i] = th * in->level_sigma2[in->q_octave[i]];  // findFeaturesInArea: radius * getScaledFactor2(octave)
    io.put(o_held, held.data(), NF * 4);
    for (size_t f = 0; f < NF; ++f) io.host<uint8_t>(o_ex)[f] = held[f] >= 0 ? 1 : 0;
    HIP_TRY(c, io.upload(pass == 0 ? up : up_pass));
    HIP_TRY(c, hipMemsetAsync(b + claim.begin, 0xFF, claim.bytes(), st));
    HIP_TRY(c, hipMemsetAsync(b + zero.begin, 0, zero.bytes(), st));
    {
      StageTimer tm(c, ORBFE_STAGE_MATCH, st);
      const int32_t *g_off = nullptr, *g_feat = nullptr;
      TRY(slot_grid(c, st, slot, ag, &g_off, &g_feat));
      launch_search_area(st, c->d_kpl + (size_t)slot * NF, c->d_desc + (size_t)slot * NF * 32, ag.clip_w, ag.clip_h, ag.rows, ag.cols,
                         g_off, g_feat, n, (const float*)(b + o_qxy), (const float*)(b + o_rad),
                         (const int8_t*)(b + o_lo), (const int8_t*)(b + o_hi), b + o_desc, b + o_ex, (int32_t*)(b + o_bi), (int32_t*)(b + o_bd),
                         (int32_t*)(b + o_sd), (int32_t*)(b + o_nc), (int32_t*)(b + o_eh));
      launch_track_claim(st, n, (const int32_t*)(b + o_nc), (const int32_t*)(b + o_bi), (const int32_t*)(b + o_bd), (const int32_t*)(b + o_sd),
                         in->min_threshold, in->ratio, (int32_t*)(b + o_claim), 1, (int32_t*)(b + o_acc), b + o_qa);
      launch_track_edges(st, F, pose_edges(W, b), (const int32_t*)(b + o_held), (const int32_t*)(b + o_claim), b + o_fl, (const float*)(b + o_pos),
                         in->min_matches, (int32_t*)(b + o_asg), (int32_t*)(b + o_cnt), -1, (const int32_t*)(b + o_acc), base_matches);
    }
    pose_optimise(c, st, W, b, cam, 0, (const int32_t*)(b + o_cnt) + 1);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(b + o_ehd, b + o_eh, NF * 4, hipMemcpyDeviceToDevice, st));  // (the hits sit in front of the downloaded block)
    HIP_TRY(c, hipMemcpyAsync(b + o_qad, b + o_qa, N, hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, io.fetch(down));
    cnt = (const int32_t*)io.got(o_cnt);
    ++n_pass;
    if (excluded_hits) {
      const int32_t* eh = (const int32_t*)io.got(o_ehd);
      for (size_t f = 0; f < NF; ++f) hits_total[f] += eh[f];
    }
    if (query_matches)
      for (int i = 0; i < n; ++i) qm_total[(size_t)i] += io.got(o_qad)[i];
    if (cnt[1] >= 0 || pass == 1 || !(in->th_second > 0)) break;
    // fewer than min_matches: the matches of this pass stay (setMapPoints, :344-345) and are excluded from the next one
    base_matches = cnt[0];
    io.get(held.data(), o_asg, NF * 4);
  }
  drain_timers(c);
  track_results(io, o_cnt, W, o_asg, out);
  if (excluded_hits) std::memcpy(excluded_hits, hits_total.data(), NF * 4);
  if (query_matches && n) std::memcpy(query_matches, qm_total.data(), (size_t)n * 4);
  if (passes) *passes = n_pass;
  return ORBFE_OK;
}

}  // extern "C"

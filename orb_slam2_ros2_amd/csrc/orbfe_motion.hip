// orbfe_motion.hip -- host side of orbfe_track_motion_model_slots (include/orbfe.h): argument checks, one upload of the map
// state (a flag byte per last-frame feature, the ids or positions of its points, the level tables), one launch sequence -- prepare,
// search, claim, between, search, claim, edges, optimise, check --, one download.  Both frames' features, the current frame's right_u and
// the last frame's depth are read in the slots and pairs their extraction left them in; whether the second search runs is decided on the
// device (k_motion.hip), so nothing is synchronised between the upload and the download.
#include "orbfe_ctx.h"
#include "orbfe_mpstore.h"
#include "pose_call.h"

namespace orbfe {
void launch_motion_prep(hipStream_t st, const MotionDev& P);
void launch_motion_between(hipStream_t st, const MotionDev& P);
void launch_motion_check(hipStream_t st, const MotionDev& P);
}  // namespace orbfe

extern "C" {

orbfe_status orbfe_track_motion_model_slots(orbfe_ctx* c, int32_t slot, int32_t pair, int32_t last_slot, int32_t last_pair, orbfe_mpstore* store,
                                            const orbfe_motion_slots_input* in, const orbfe_motion_slots_output* out) {
  ApiLock api_lk(c);
  const char* fn = "track_motion_model_slots";
  if (!c || !in || !out) return fail(c, ORBFE_EBADARG, "%s: NULL argument", fn);
  const int M = c->cfg.max_images, n_pairs = (M + 1) / 2;
  if (slot < 0 || slot >= M || last_slot < 0 || last_slot >= M || slot == last_slot || pair >= n_pairs || last_pair >= n_pairs)
    return fail(c, ORBFE_EBADARG, "%s: bad slots or pairs (slot %d pair %d, last slot %d pair %d; two different slots below %d, pairs below %d)", fn,
                slot, pair, last_slot, last_pair, M, n_pairs);
  if (!in->last_flags || !in->cam || !in->level_sigma2 || !in->level_inv_sigma2 || !out->verdict || !out->passes || !out->n_matches || !out->n_edges ||
      !out->n_inliers || !out->n_in_map || !out->assigned || !out->final_assigned || !out->inlier || !out->excluded_hits || !out->query_matches ||
      !out->temp || !out->temp_pos || !out->pose_se3 || !out->Tcw)
    return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
  if (!((store && in->last_ids && !in->last_pos) || (!store && !in->last_ids && in->last_pos)))
    return fail(c, ORBFE_EBADARG, "%s: exactly one of a store with last_ids and last_pos without a store must be given", fn);
  const int nl = c->cfg.n_levels;
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1);
  TRY(pose_check_features(c, fn, NF));
  if (store) TRY(mpstore_check_ctx(c, store, fn));
  const orbfe_camera* cam = in->cam;
  const float scalars[] = {cam->fx,       cam->fy,       cam->cx,       cam->cy,       cam->bf,  in->baseline, in->th,
                           in->th_second, in->ratio,     in->bounds[0], in->bounds[1], in->bounds[2], in->bounds[3]};
  TRY(check_finite(c, fn, {{scalars, 13}, {in->Rcw, 9}, {in->last_Rcw, 9}, {in->last_Rwc, 9}, {in->tcw, 3}, {in->last_tcw, 3}, {in->last_twc, 3}}));
  AreaGrid ag;
  TRY(check_area_grid(c, fn, in->bounds, NF, &ag));
  TRY(slots_idle(c, slot, 1, fn));
  TRY(slots_idle(c, last_slot, 1, fn));
  // held until the results are down: no upsert or erase touches a row or a page under the running kernels
  std::shared_lock<std::shared_timed_mutex> store_lk;
  if (store) store_lk = std::shared_lock<std::shared_timed_mutex>(store->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  // [ upload | claims (-1 fill) | header, results (0 fill; downloaded), accepted flags, counters (0 fill) | device-only ]
  ScratchLayout L;
  ScratchRegion up, claim, zero, down;
  PoseWorkspace W(NF);
  const size_t o_fl = L.open(up).take(NF), o_ids = L.take<uint64_t>(store ? NF : 0), o_lp = L.take<float>(store ? 0 : NF * 3),
               o_s2 = L.take<float>((size_t)nl), o_is2 = L.take<float>((size_t)nl), o_c1 = L.close(up).open(claim).take<int32_t>(NF),
               o_c2 = L.take<int32_t>(NF), o_hdr = L.close(claim).open(zero).open(down).take<int32_t>(8), o_bad = L.take(8),
               o_eh = L.take<int32_t>(NF), o_qm = L.take<int32_t>(NF), o_asg = L.take<int32_t>(NF), o_cur = L.take<int32_t>(NF), o_in = L.take(NF),
               o_tmp = L.take(NF), o_tpos = L.take<float>(NF * 3), o_po = L.take<double>(7), o_tc = L.take<float>(12),
               o_qa1 = L.close(down).take(NF), o_qa2 = L.take(NF), o_acc = L.take(16), o_cnt = L.take(16),
               o_qxy = W.take_results(L).close(zero).take<float>(NF * 2), o_r1 = L.take<float>(NF), o_r2 = L.take<float>(NF), o_lo = L.take(NF), o_hi = L.take(NF),
               o_qp = L.take<float>(NF * 3), o_qf = L.take(NF), o_ex = L.take(NF), o_bi = L.take<int32_t>(NF), o_bd = L.take<int32_t>(NF),
               o_sd = L.take<int32_t>(NF), o_nc = L.take<int32_t>(NF), o_ru = W.take_list(W.take_seed(L)).take<double>(pair < 0 ? NF : 0);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  uint8_t* b = io.d;
  io.put(o_fl, in->last_flags, NF);
  if (store) io.put(o_ids, in->last_ids, NF * 8);
  else io.put(o_lp, in->last_pos, NF * 12);
  io.put(o_s2, in->level_sigma2, (size_t)nl * 4);
  io.put(o_is2, in->level_inv_sigma2, (size_t)nl * 4);
  hipStream_t st = c->stream;
  HIP_TRY(c, io.upload(up));
  HIP_TRY(c, hipMemsetAsync(b + claim.begin, 0xFF, claim.bytes(), st));
  HIP_TRY(c, hipMemsetAsync(b + zero.begin, 0, zero.bytes(), st));
  // the current frame's right_u: its pair's, or -1 everywhere (the byte pattern 0xBF is a negative double: every edge mono)
  const double* d_ru = pair >= 0 ? c->d_right_u + (size_t)pair * NF : (const double*)(b + o_ru);
  if (pair < 0) HIP_TRY(c, hipMemsetAsync(b + o_ru, 0xBF, NF * 8, st));
  MotionDev P = {};
  P.F = pose_frame(c, slot, d_ru, (const float*)(b + o_s2), (const float*)(b + o_is2));
  pose_frame_camera(P.F, in->Rcw, in->tcw, cam, in->bounds);
  P.E = pose_edges(W, b);
  P.l_kps = c->d_kps + (size_t)last_slot * NF, P.l_n_kp = c->d_n_kp + last_slot;
  P.l_depth = last_pair >= 0 ? c->d_depth + (size_t)last_pair * NF : nullptr;
  P.l_flags = b + o_fl, P.l_ids = (const uint64_t*)(b + o_ids), P.l_pos = (const float*)(b + o_lp);
  if (store) {
    const MpTable T = store->table();
    P.table = T.table, P.rows_per_page = T.rows_per_page, P.max_pages = T.max_pages;
  }
  std::memcpy(P.lR, in->last_Rcw, sizeof P.lR), std::memcpy(P.lt, in->last_tcw, sizeof P.lt);
  std::memcpy(P.lRwc, in->last_Rwc, sizeof P.lRwc), std::memcpy(P.ltwc, in->last_twc, sizeof P.ltwc);
  P.baseline = in->baseline, P.th = in->th, P.th_second = in->th_second;
  P.min_matches = in->min_matches, P.min_inliers = in->min_inliers;
  P.qxy = (float*)(b + o_qxy), P.rad1 = (float*)(b + o_r1), P.rad2 = (float*)(b + o_r2), P.q_pos = (float*)(b + o_qp);
  P.lo = (int8_t*)(b + o_lo), P.hi = (int8_t*)(b + o_hi), P.q_flags = b + o_qf, P.ex2 = b + o_ex;
  P.claim1 = (const int32_t*)(b + o_c1), P.n_accept = (const int32_t*)(b + o_acc), P.qa1 = b + o_qa1, P.qa2 = b + o_qa2;
  P.cnt = (const int32_t*)(b + o_cnt), P.p_init = (double*)(b + W.o_p0), P.p_opt = (const double*)(b + W.o_p1);
  P.hdr = (int32_t*)(b + o_hdr), P.bad = (uint32_t*)(b + o_bad), P.assigned = (const int32_t*)(b + o_asg);
  P.cur = (int32_t*)(b + o_cur), P.qm = (int32_t*)(b + o_qm), P.inlier = b + o_in, P.temp = b + o_tmp, P.temp_pos = (float*)(b + o_tpos);
  P.pose_out = (double*)(b + o_po), P.tcw_out = (float*)(b + o_tc);
  const uint4* f_kpl = c->d_kpl + (size_t)slot * NF;
  const uint8_t *f_desc = c->d_desc + (size_t)slot * NF * 32, *l_desc = c->d_desc + (size_t)last_slot * NF * 32;
  int32_t *bi = (int32_t*)(b + o_bi), *bd = (int32_t*)(b + o_bd), *sd = (int32_t*)(b + o_sd), *nc = (int32_t*)(b + o_nc);
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, st);
    const int32_t *g_off = nullptr, *g_feat = nullptr;
    TRY(slot_grid(c, st, slot, ag, &g_off, &g_feat));
    launch_motion_prep(st, P);
    // one accepted-query counter for both searches: the between kernel reads search 1's count, the edges kernel the sum
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1) launch_motion_between(st, P);
      launch_search_area(st, f_kpl, f_desc, ag.clip_w, ag.clip_h, ag.rows, ag.cols, g_off, g_feat, (int)NF, P.qxy, pass == 0 ? P.rad1 : P.rad2, P.lo,
                         P.hi, l_desc, pass == 0 ? nullptr : P.ex2, bi, bd, sd, nc, pass == 0 ? nullptr : (int32_t*)(b + o_eh));
      launch_track_claim(st, (int)NF, nc, bi, bd, sd, in->min_threshold, in->ratio, (int32_t*)(b + (pass == 0 ? o_c1 : o_c2)), 1,
                         (int32_t*)(b + o_acc), b + (pass == 0 ? o_qa1 : o_qa2));
    }
    // what search 1 assigned is held, what search 2 claims is new: a feature of search 1 was no candidate of search 2
    launch_track_edges(st, P.F, P.E, P.claim1, (const int32_t*)(b + o_c2), P.q_flags, P.q_pos, in->min_matches, (int32_t*)(b + o_asg),
                       (int32_t*)(b + o_cnt), -1, (const int32_t*)(b + o_acc), 0);
  }
  pose_optimise(c, st, W, b, cam, 0, P.cnt + 1);
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, st);
    launch_motion_check(st, P);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down));
  drain_timers(c);
  if (*(const uint32_t*)io.got(o_bad)) {
    for (size_t i = 0; i < NF; ++i)
      if ((in->last_flags[i] & 1) && !store->idx.has(in->last_ids[i]))
        return fail(c, ORBFE_EBADARG, "%s: map point %llu (last_ids[%zu]) is not in the store", fn, (unsigned long long)in->last_ids[i], i);
    return fail(c, ORBFE_EDEVICE, "%s: the device holds no row for an id the store's index lists", fn);
  }
  const int32_t* hdr = (const int32_t*)io.got(o_hdr);
  const int v = hdr[MOTION_H_VERDICT], np = hdr[MOTION_H_PASSES];
  if (v < ORBFE_MOTION_REJECT_MATCHES || v > ORBFE_MOTION_ACCEPT || np < 1 || np > 2) return fail(c, ORBFE_EDEVICE, "%s: corrupt result", fn);
  *out->verdict = v;
  *out->passes = np;
  *out->n_matches = hdr[MOTION_H_MATCHES];
  *out->n_edges = hdr[MOTION_H_EDGES];
  *out->n_inliers = hdr[MOTION_H_INLIERS];
  *out->n_in_map = hdr[MOTION_H_INMAP];
  io.get(out->assigned, o_asg, NF * 4);
  io.get(out->final_assigned, o_cur, NF * 4);
  io.get(out->inlier, o_in, NF);
  io.get(out->excluded_hits, o_eh, NF * 4);
  io.get(out->query_matches, o_qm, NF * 4);
  io.get(out->temp, o_tmp, NF);
  io.get(out->temp_pos, o_tpos, NF * 12);
  io.get(out->pose_se3, o_po, 56);
  io.get(out->Tcw, o_tc, 48);
  return ORBFE_OK;
}

}  // extern "C"

// orbfe_reloc.hip -- host side of orbfe_reloc_refine_stored (include/orbfe.h): argument checks, one upload of the map state
// (good flags, positions, held, right_u, the level tables), one launch sequence -- seed, optimise, check, search, after, optimise, check,
// search, after -- whose kernels leave at once when the verdict has fallen (k_reloc.hip), one download.  The frame's features and grid
// are the slot's, the keyframe's features the store's; nothing is synchronised between the upload and the download.
#include "orbfe_kfstore.h"
#include "pose_call.h"

namespace orbfe {
void launch_reloc_seed(hipStream_t st, const RelocDev& P);
void launch_reloc_check(hipStream_t st, const RelocDev& P, int s);
void launch_reloc_search(hipStream_t st, const RelocDev& P, int s);
void launch_reloc_after(hipStream_t st, const RelocDev& P, int s);
}  // namespace orbfe

extern "C" {

orbfe_status orbfe_reloc_refine_stored(orbfe_ctx* c, int32_t slot, orbfe_kfstore* store, const orbfe_reloc_input* in,
                                       const orbfe_reloc_output* out) {
  ApiLock api_lk(c);
  const char* fn = "reloc_refine_stored";
  if (!c || !store || !in || !out || slot < 0 || slot >= c->cfg.max_images) return fail(c, ORBFE_EBADARG, "%s: NULL argument / bad slot", fn);
  const int n = in->n, nl = c->cfg.n_levels;
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1);
  if (n < 0 || !in->held || !in->level_sigma2 || !in->level_inv_sigma2 || !in->cam || (n && (!in->good || !in->pos)) || !out->verdict ||
      !out->n_edges || !out->n_inliers || !out->n_added || !out->tlc_z || !out->pose_se3 || !out->Tcw || !out->inlier || !out->assigned ||
      !out->final_assigned || !out->excluded_hits || (n && !out->query_accepted))
    return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
  TRY(pose_check_features(c, fn, NF));
  TRY(kfstore_check_ctx(c, store, fn));
  if (nl < store->n_levels) return fail(c, ORBFE_EBADARG, "%s: the context has %d levels, the store's octaves go up to %d", fn, nl, store->n_levels - 1);
  const orbfe_camera* cam = in->cam;
  const float scalars[] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, in->baseline, in->th_first, in->th_second, in->ratio};
  TRY(check_finite(c, fn, {{scalars, 9}, {in->Rcw, 9}, {in->kf_Rcw, 9}, {in->tcw, 3}, {in->kf_tcw, 3}}));
  TRY(check_held(c, fn, in->held, NF, n));
  AreaGrid ag;
  TRY(check_area_grid(c, fn, in->bounds, NF, &ag));
  std::shared_lock<std::shared_timed_mutex> store_lk(store->mu);  // held until the results are down: no erase frees memory under the kernels
  const KfEntry* e = store->map.find(in->kf_id);
  if (!e) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)in->kf_id);
  if (e->n != n) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu has %d features, the call says %d", fn, (unsigned long long)in->kf_id, e->n, n);
  TRY(slots_idle(c, slot, 1, fn));
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  const size_t N = (size_t)n;
  // [ upload | claims, assignments, held now (0xFF fill) | header, results, counts, estimates (0 fill) | edge list ]; the download runs
  // from the assignments to the accepted queries
  ScratchLayout L;
  ScratchRegion up, ones, zero, down;
  PoseWorkspace W(NF, 2);
  FrameUpload U;
  const size_t o_good = L.open(up).take(N), o_pos = L.take<float>(N * 3), o_held = L.take<int32_t>(NF),
               o_claim = U.take(L, NF, (size_t)nl).close(up).open(ones).take<int32_t>(2 * NF), o_asg = L.open(down).take<int32_t>(2 * NF),
               o_cur = L.take<int32_t>(NF), o_hdr = L.close(ones).open(zero).take<int32_t>(16), o_po = L.take<double>(14),
               o_tc = L.take<float>(24), o_in = L.take(2 * NF), o_eh = L.take<int32_t>(2 * NF), o_qa = L.take(2 * N),
               o_cnt = L.close(down).take<int32_t>(2);
  W.take_seed(L), W.take_results(L), L.close(zero), W.take_list(L);
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, down.bytes())));
  io.put(o_good, in->good, N);
  io.put(o_pos, in->pos, N * 12);
  io.put(o_held, in->held, NF * 4);
  put_frame(io, U, NF, (size_t)nl, in->right_u, in->level_sigma2, in->level_inv_sigma2);
  hipStream_t st = c->stream;
  uint8_t* b = io.d;
  HIP_TRY(c, io.upload(up));
  HIP_TRY(c, hipMemsetAsync(b + ones.begin, 0xFF, ones.bytes(), st));
  HIP_TRY(c, hipMemsetAsync(b + zero.begin, 0, zero.bytes(), st));
  RelocDev P = {};
  P.F = pose_frame(c, slot, b, U);
  pose_frame_camera(P.F, in->Rcw, in->tcw, cam, in->bounds);
  P.E = pose_edges(W, b);
  P.f_kpl = c->d_kpl + (size_t)slot * NF, P.f_desc = c->d_desc + (size_t)slot * NF * 32;
  P.rows = ag.rows, P.cols = ag.cols, P.clip_w = ag.clip_w, P.clip_h = ag.clip_h;
  P.k_kps = e->at<orbfe_keypoint>(e->o_kps), P.k_desc = e->at<uint8_t>(e->o_desc);
  P.good = b + o_good, P.pos = (const float*)(b + o_pos), P.n = n;
  std::memcpy(P.kf_R, in->kf_Rcw, sizeof P.kf_R), std::memcpy(P.kf_t, in->kf_tcw, sizeof P.kf_t);
  P.held = (const int32_t*)(b + o_held);
  P.baseline = in->baseline, P.th[0] = in->th_first, P.th[1] = in->th_second, P.ratio = in->ratio;
  P.min_threshold = in->min_threshold, P.min_inliers = in->min_inliers, P.enough = in->enough;
  P.cur = (int32_t*)(b + o_cur), P.claim = (int32_t*)(b + o_claim), P.cnt = (int32_t*)(b + o_cnt);
  P.p_init = (double*)(b + W.o_p0), P.p_opt = (double*)(b + W.o_p1);
  P.hdr = (int32_t*)(b + o_hdr), P.pose_out = (double*)(b + o_po), P.tcw_out = (float*)(b + o_tc), P.inlier = b + o_in;
  P.assigned = (int32_t*)(b + o_asg), P.hits = (int32_t*)(b + o_eh), P.qa = b + o_qa;
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, st);
    TRY(slot_grid(c, st, slot, ag, &P.cell_off, &P.cell_feat));
    launch_reloc_seed(st, P);
  }
  for (int s = 0; s < 2; ++s) {
    pose_optimise(c, st, W, b, cam, s, P.cnt + s);
    StageTimer tm(c, ORBFE_STAGE_MATCH, st);
    launch_reloc_check(st, P, s);
    launch_reloc_search(st, P, s);
    launch_reloc_after(st, P, s);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down));
  drain_timers(c);
  const int32_t* hdr = (const int32_t*)io.got(o_hdr);
  if (hdr[RELOC_H_VERDICT] < ORBFE_RELOC_REJECT_1 || hdr[RELOC_H_VERDICT] > ORBFE_RELOC_ACCEPT_3) return fail(c, ORBFE_EDEVICE, "%s: corrupt result", fn);
  *out->verdict = hdr[RELOC_H_VERDICT];
  std::memcpy(out->n_edges, hdr + RELOC_H_EDGES, 8);
  std::memcpy(out->n_inliers, hdr + RELOC_H_INLIERS, 8);
  std::memcpy(out->n_added, hdr + RELOC_H_ADDED, 8);
  std::memcpy(out->tlc_z, hdr + RELOC_H_TLCZ, 8);
  io.get(out->pose_se3, o_po, 112);
  io.get(out->Tcw, o_tc, 96);
  io.get(out->inlier, o_in, 2 * NF);
  io.get(out->assigned, o_asg, 2 * NF * 4);
  io.get(out->final_assigned, o_cur, NF * 4);
  io.get(out->excluded_hits, o_eh, 2 * NF * 4);
  io.get(out->query_accepted, o_qa, 2 * N);
  return ORBFE_OK;
}

}  // extern "C"

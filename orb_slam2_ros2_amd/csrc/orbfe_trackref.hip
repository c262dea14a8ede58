// orbfe_trackref.hip -- host side of orbfe_track_reference_stored (include/orbfe.h): argument checks, one upload of the map
// state (the keyframe's flags and positions, what the frame came with, right_u, the level tables and, for a frame whose computeBow has
// run, its FeatureVector), one launch sequence -- transform, match, select, seed, optimise, check -- whose kernels after the seed leave at
// once when the verdict has fallen (k_trackref.hip), one download.  The frame's features are the slot's, the keyframe's features and
// FeatureVector the store's; nothing is synchronised between the upload and the download.
#include "orbfe_kfstore.h"
#include "pose_call.h"

void launch_bow(hipStream_t s, const uint8_t* d_desc, size_t desc_img_stride, const int32_t* d_counts, int count_step, int n_fixed, int n_img, int cap,
                const BowVocabDev& vd, int levelsup, uint64_t* d_wkey, uint64_t* d_nkey, double* d_wts, size_t key_stride, uint32_t* o_words,
                double* o_values, uint32_t* o_nodes, int32_t* o_offsets, uint32_t* o_features, int32_t* o_counts);
void launch_bow_search_one(hipStream_t st, const uint8_t* up, const BowKf* kf, const BowQuerySlot& q, const BowParams& P, int n_feat,
                           BowSlot* slots, BowMatch* lists, int32_t* counts);
orbfe_status vocab_on_device(orbfe_ctx* c, const orbfe_vocab* v, BowVocabDev& out);
orbfe_status check_feature_vector(orbfe_ctx* c, const char* fn, const char* who, int idx, int32_t n, int32_t n_nodes, const uint32_t* nodes,
                                  const int32_t* node_offsets, const uint32_t* features);
namespace orbfe {
void launch_trackref_seed(hipStream_t st, const TrackRefDev& P);
void launch_trackref_check(hipStream_t st, const TrackRefDev& P);
}  // namespace orbfe

static_assert(sizeof(BowMatch) == sizeof(orbfe_bow_match), "BowMatch is orbfe_bow_match");

extern "C" {

orbfe_status orbfe_track_reference_stored(orbfe_ctx* c, int32_t slot, const orbfe_vocab* vocab, orbfe_kfstore* store,
                                          const orbfe_trackref_input* in, const orbfe_trackref_output* out) {
  ApiLock api_lk(c);
  const char* fn = "track_reference_stored";
  if (!c || !store || !in || !out || slot < 0 || slot >= c->cfg.max_images) return fail(c, ORBFE_EBADARG, "%s: NULL argument / bad slot", fn);
  const int n = in->n, nl = c->cfg.n_levels;
  const size_t NF = (size_t)std::max(c->cfg.n_features, 1);
  if (n < 0 || !in->level_sigma2 || !in->level_inv_sigma2 || !in->cam || (n && (!in->good || !in->pos)) || (in->frame_good && !in->frame_pos) ||
      !out->verdict || !out->n_matches || (n && !out->matches) || !out->assigned || !out->n_edges || !out->n_inliers || !out->inlier ||
      !out->final_assigned || !out->pose_se3 || !out->Tcw)
    return fail(c, ORBFE_EBADARG, "%s: NULL array", fn);
  TRY(pose_check_features(c, fn, NF));
  const bool host_fv = in->n_nodes != 0 || in->nodes || in->node_offsets || in->features;
  if ((vocab != nullptr) == host_fv)
    return fail(c, ORBFE_EBADARG, "%s: exactly one of a vocabulary and a host FeatureVector of the frame must be given", fn);
  if (in->levelsup < 0) return fail(c, ORBFE_EBADARG, "%s: levelsup %d", fn, in->levelsup);
  if (host_fv) TRY(check_feature_vector(c, fn, "frame", slot, (int32_t)NF, in->n_nodes, in->nodes, in->node_offsets, in->features));
  TRY(kfstore_check_ctx(c, store, fn));
  if (nl < store->n_levels) return fail(c, ORBFE_EBADARG, "%s: the context has %d levels, the store's octaves go up to %d", fn, nl, store->n_levels - 1);
  const orbfe_camera* cam = in->cam;
  const float scalars[] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->bf, in->ratio, in->bounds[0], in->bounds[1], in->bounds[2], in->bounds[3]};
  TRY(check_finite(c, fn, {{scalars, 10}, {in->Rcw, 9}, {in->tcw, 3}}));
  std::shared_lock<std::shared_timed_mutex> store_lk(store->mu);  // held until the results are down: no erase frees memory under the kernels
  const KfEntry* e = store->map.find(in->kf_id);
  if (!e) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)in->kf_id);
  if (e->n != n) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu has %d features, the call says %d", fn, (unsigned long long)in->kf_id, e->n, n);
  if (!e->has_bow) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu has no FeatureVector (orbfe_kfstore_set_bow)", fn, (unsigned long long)in->kf_id);
  TRY(slots_idle(c, slot, 1, fn));
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  BowVocabDev vd = {};
  if (vocab) TRY(vocab_on_device(c, vocab, vd));
  const bool want_bow = vocab && out->bow;
  const size_t N = (size_t)n, NE = (size_t)e->n_feat, nn = host_fv ? (size_t)in->n_nodes : 0, nfv = host_fv ? (size_t)in->node_offsets[nn] : 0;
  size_t np2 = 1;
  while (np2 < NF) np2 <<= 1;
  // [ upload | the transform's keys, the match slots and the list | the transform's result block | header and results (0 fill) | counts,
  // estimates (0 fill) | edge list ]; the download runs from the header to the inlier flags, with the transform's block in front of it
  // when the caller takes the frame's BoW
  ScratchLayout L;
  ScratchRegion up, bow, zero, down;
  PoseWorkspace W(NF);
  FrameUpload U;
  const size_t o_kf = L.open(up).take<BowKf>(1), o_good = L.take(N), o_pos = L.take<float>(N * 3), o_fg = L.take(NF),
               o_fp = L.take<float>(in->frame_good ? NF * 3 : 0), o_hn = U.take(L, NF, (size_t)nl).take<int32_t>(1),
               o_hnodes = L.take<uint32_t>(nn), o_hoffs = L.take<int32_t>(nn + 1),
               o_hfeat = L.take<uint32_t>(nfv), o_wkey = L.close(up).take<uint64_t>(np2), o_nkey = L.take<uint64_t>(np2),
               o_wts = L.take<double>(np2), o_slots = L.take<BowSlot>(NE), o_list = L.take<BowMatch>(NE), o_ln = L.take<int32_t>(1),
               o_values = L.open(bow).take<double>(NF), o_words = L.take<uint32_t>(NF), o_nodes = L.take<uint32_t>(NF),
               o_feat = L.take<uint32_t>(NF), o_offs = L.take<int32_t>(NF + 1), o_bc = L.take<int32_t>(2),
               o_hdr = L.close(bow).open(zero).open(down).take<int32_t>(4), o_m = L.take<BowMatch>(N), o_asg = L.take<int32_t>(NF),
               o_cur = L.take<int32_t>(NF), o_po = L.take<double>(7), o_tc = L.take<float>(12), o_in = L.take(NF),
               o_cnt = L.close(down).take<int32_t>(1);
  W.take_seed(L), W.take_results(L), L.close(zero), W.take_list(L);
  const ScratchRegion fetch = {want_bow ? bow.begin : down.begin, down.end};
  StagedIo io;
  TRY(io.reserve(c, L.end(), std::max(up.end, fetch.bytes())));
  uint8_t* b = io.d;
  BowKf kf = {};
  kf.kps = e->at<orbfe_keypoint>(e->o_kps), kf.desc = e->at<uint8_t>(e->o_desc);
  kf.nodes = e->bow<uint32_t>(e->o_nodes), kf.offs = e->bow<int32_t>(e->o_offs), kf.feat = e->bow<uint32_t>(e->o_feat);
  kf.o_flags = (uint32_t)o_good, kf.n_nodes = e->n_nodes, kf.n_feat = e->n_feat, kf.slot0 = 0;
  io.put(o_kf, &kf, sizeof kf);
  if (N) {
    io.put(o_good, in->good, N);
    io.put(o_pos, in->pos, N * 12);
  }
  if (in->frame_good) {
    io.put(o_fg, in->frame_good, NF);
    io.put(o_fp, in->frame_pos, NF * 12);
  } else
    std::memset(io.host<uint8_t>(o_fg), 0, NF);
  put_frame(io, U, NF, (size_t)nl, in->right_u, in->level_sigma2, in->level_inv_sigma2);
  if (host_fv) {
    io.put(o_hn, &in->n_nodes, 4);
    io.put(o_hnodes, in->nodes, nn * 4);
    io.put(o_hoffs, in->node_offsets, (nn + 1) * 4);
    io.put(o_hfeat, in->features, nfv * 4);
  }
  hipStream_t st = c->stream;
  HIP_TRY(c, io.upload(up));
  HIP_TRY(c, hipMemsetAsync(b + zero.begin, 0, zero.bytes(), st));
  TrackRefDev P = {};
  P.F = pose_frame(c, slot, b, U);
  pose_frame_camera(P.F, in->Rcw, in->tcw, cam, in->bounds);
  P.E = pose_edges(W, b);
  P.pos = (const float*)(b + o_pos), P.f_good = b + o_fg, P.f_pos = (const float*)(b + o_fp);
  P.n = n, P.min_matches = in->min_matches, P.min_inliers = in->min_inliers;
  P.list = (const BowMatch*)(b + o_list), P.n_list = (const int32_t*)(b + o_ln);
  P.cnt = (int32_t*)(b + o_cnt), P.p_init = (double*)(b + W.o_p0), P.p_opt = (double*)(b + W.o_p1);
  P.hdr = (int32_t*)(b + o_hdr), P.matches = (BowMatch*)(b + o_m), P.assigned = (int32_t*)(b + o_asg), P.cur = (int32_t*)(b + o_cur);
  P.pose_out = (double*)(b + o_po), P.tcw_out = (float*)(b + o_tc), P.inlier = b + o_in;
  BowQuerySlot Q = {};
  Q.kps = P.F.kps, Q.desc = c->d_desc + (size_t)slot * NF * 32, Q.o_flags = (uint32_t)o_fg;
  if (host_fv)
    Q.nodes = (const uint32_t*)(b + o_hnodes), Q.offs = (const int32_t*)(b + o_hoffs), Q.feat = (const uint32_t*)(b + o_hfeat),
    Q.n_nodes = (const int32_t*)(b + o_hn);
  else
    Q.nodes = (const uint32_t*)(b + o_nodes), Q.offs = (const int32_t*)(b + o_offs), Q.feat = (const uint32_t*)(b + o_feat),
    Q.n_nodes = (const int32_t*)(b + o_bc) + 1;
  BowParams BP = {};
  BP.mode = ORBFE_BOW_TRACK, BP.dist_threshold = in->dist_threshold, BP.check_orientation = in->check_orientation ? 1 : 0, BP.n_kf = 1;
  BP.ratio = in->ratio, BP.cap = n;
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, st);
    if (vocab)
      launch_bow(st, Q.desc, 0, P.F.n_kp, 1, 0, 1, (int)NF, vd, in->levelsup, (uint64_t*)(b + o_wkey), (uint64_t*)(b + o_nkey),
                 (double*)(b + o_wts), np2, (uint32_t*)(b + o_words), (double*)(b + o_values), (uint32_t*)(b + o_nodes), (int32_t*)(b + o_offs),
                 (uint32_t*)(b + o_feat), (int32_t*)(b + o_bc));
    launch_bow_search_one(st, b, (const BowKf*)(b + o_kf), Q, BP, e->n_feat, (BowSlot*)(b + o_slots), (BowMatch*)(b + o_list),
                          (int32_t*)(b + o_ln));
    launch_trackref_seed(st, P);
  }
  pose_optimise(c, st, W, b, cam, 0, P.cnt);
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, st);
    launch_trackref_check(st, P);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(fetch));
  drain_timers(c);
  const int32_t* hdr = (const int32_t*)io.got(o_hdr);
  const int v = hdr[TRACKREF_H_VERDICT], nm = hdr[TRACKREF_H_MATCHES];
  if (v < ORBFE_TRACKREF_REJECT_MATCHES || v > ORBFE_TRACKREF_ACCEPT || nm < 0 || nm > n) return fail(c, ORBFE_EDEVICE, "%s: corrupt result", fn);
  int32_t bc[2] = {0, 0}, kept = 0;
  if (want_bow) {
    io.get(bc, o_bc, 8);
    if (bc[0] < 0 || bc[0] > (int)NF || bc[1] < 0 || bc[1] > (int)NF) return fail(c, ORBFE_EDEVICE, "%s: corrupt BoW counts %d %d", fn, bc[0], bc[1]);
    io.get(&kept, o_offs + 4 * (size_t)bc[1], 4);
    if (kept < 0 || kept > (int)NF) return fail(c, ORBFE_EDEVICE, "%s: corrupt BoW feature count %d", fn, kept);
  }
  *out->verdict = v;
  *out->n_matches = nm;
  *out->n_edges = hdr[TRACKREF_H_EDGES];
  *out->n_inliers = hdr[TRACKREF_H_INLIERS];
  io.get(out->matches, o_m, N * sizeof(BowMatch));
  io.get(out->assigned, o_asg, NF * 4);
  io.get(out->final_assigned, o_cur, NF * 4);
  io.get(out->pose_se3, o_po, 56);
  io.get(out->Tcw, o_tc, 48);
  io.get(out->inlier, o_in, NF);
  if (want_bow) {
    const orbfe_bow_out* w = out->bow;
    if (w->words) io.get(w->words, o_words, 4 * (size_t)bc[0]);
    if (w->values) io.get(w->values, o_values, 8 * (size_t)bc[0]);
    if (w->n_words) *w->n_words = bc[0];
    if (w->nodes) io.get(w->nodes, o_nodes, 4 * (size_t)bc[1]);
    if (w->node_offsets) io.get(w->node_offsets, o_offs, 4 * ((size_t)bc[1] + 1));
    if (w->features) io.get(w->features, o_feat, 4 * (size_t)kept);
    if (w->n_nodes) *w->n_nodes = bc[1];
  }
  return ORBFE_OK;
}

}  // extern "C"

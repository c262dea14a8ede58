// orbfe_bowsearch.hip -- host side of orbfe_search_by_bow_stored (include/orbfe.h): argument checks, one upload into the
// context's scratch (the candidate records, every flag array and, for a query given as host arrays, those arrays), the three launches of
// k_bowsearch.hip, one download (match_offsets and the matches).  The candidates' features and FeatureVectors are read where the keyframe
// store keeps them.
#include "orbfe_kfstore.h"

void launch_bow_search(hipStream_t st, const uint8_t* up, const BowKf* kfs, const BowQuery& q, const BowParams& P, int max_feat, BowSlot* slots,
                       BowMatch* lists, int32_t* counts, int32_t* offsets, BowMatch* matches);
void launch_bow_search(hipStream_t st, const uint8_t* up, const BowKf* kfs, const BowQueryStored& q, const BowParams& P, int max_feat,
                       BowSlot* slots, BowMatch* lists, int32_t* counts, int32_t* offsets, BowMatch* matches);
orbfe_status check_feature_vector(orbfe_ctx* c, const char* fn, const char* who, int idx, int32_t n, int32_t n_nodes, const uint32_t* nodes,
                                  const int32_t* node_offsets, const uint32_t* features);

static_assert(sizeof(BowMatch) == sizeof(orbfe_bow_match), "BowMatch is orbfe_bow_match");

extern "C" orbfe_status orbfe_search_by_bow_stored(orbfe_ctx* c, orbfe_kfstore* store, const orbfe_bow_query* q, int32_t n_kf,
                                                   const uint64_t* kf_ids, const uint8_t* const* kf_flags, int32_t mode, float ratio,
                                                   int32_t dist_threshold, int32_t check_orientation, orbfe_bow_match* matches, int64_t cap,
                                                   int64_t* match_offsets) {
  ApiLock api_lk(c);
  const char* fn = "search_by_bow_stored";
  if (!c || !store || !q || !match_offsets || cap < 0 || (cap > 0 && !matches) || (n_kf > 0 && !kf_ids))
    return fail(c, ORBFE_EBADARG, "%s: bad arguments", fn);
  if (n_kf < 0 || n_kf > ORBFE_BOW_SEARCH_MAX_KF) return fail(c, ORBFE_EBADARG, "%s: %d candidate keyframes, 0..%d allowed", fn, n_kf, ORBFE_BOW_SEARCH_MAX_KF);
  if (mode != ORBFE_BOW_TRACK && mode != ORBFE_BOW_LOOP && mode != ORBFE_BOW_ADD) return fail(c, ORBFE_EBADARG, "%s: mode %d", fn, mode);
  TRY(kfstore_check_ctx(c, store, fn));
  std::shared_lock<std::shared_timed_mutex> store_lk(store->mu);  // held until the results are down: no erase frees memory under the kernels

  // the query
  const KfEntry* qe = nullptr;
  int32_t qn = q->n;
  if (q->from_store) {
    qe = store->map.find(q->id);
    if (!qe) return fail(c, ORBFE_EBADARG, "%s: the query keyframe %llu is not in the store", fn, (unsigned long long)q->id);
    if (!qe->has_bow) return fail(c, ORBFE_EBADARG, "%s: the query keyframe %llu has no FeatureVector (orbfe_kfstore_set_bow)", fn, (unsigned long long)q->id);
    if (q->n != qe->n) return fail(c, ORBFE_EBADARG, "%s: the query keyframe %llu has %d features, the query says %d", fn, (unsigned long long)q->id, qe->n, q->n);
  } else {
    if (qn < 0 || qn > ORBFE_BOW_MAX_FEATURES) return fail(c, ORBFE_EBADARG, "%s: %d query features", fn, qn);
    if (qn > 0 && (!q->desc || (check_orientation && !q->angle))) return fail(c, ORBFE_EBADARG, "%s: NULL query array", fn);
    TRY(check_feature_vector(c, fn, "query", 0, qn, q->n_nodes, q->nodes, q->node_offsets, q->features));
  }

  // the candidates
  std::vector<BowKf> kf((size_t)n_kf);
  std::vector<const KfEntry*> ent((size_t)n_kf);
  int32_t n_slots = 0, max_feat = 0, max_n = qn;
  for (int32_t i = 0; i < n_kf; ++i) {
    const KfEntry* e = store->map.find(kf_ids[i]);
    if (!e) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)kf_ids[i]);
    if (!e->has_bow) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu has no FeatureVector (orbfe_kfstore_set_bow)", fn, (unsigned long long)kf_ids[i]);
    ent[(size_t)i] = e;
    BowKf& d = kf[(size_t)i];
    d.kps = e->at<orbfe_keypoint>(e->o_kps), d.desc = e->at<uint8_t>(e->o_desc);
    d.nodes = e->bow<uint32_t>(e->o_nodes), d.offs = e->bow<int32_t>(e->o_offs), d.feat = e->bow<uint32_t>(e->o_feat);
    d.n_nodes = e->n_nodes, d.n_feat = e->n_feat, d.slot0 = n_slots;
    n_slots += e->n_feat;
    max_feat = std::max(max_feat, e->n_feat);
    max_n = std::max(max_n, e->n);
  }
  if (n_kf == 0) {
    match_offsets[0] = 0;
    return ORBFE_OK;
  }

  // the upload: [BowKf x n_kf] | one run of zeros for every NULL flag array | the flag arrays | the host query's arrays
  struct Piece {
    const void* src;
    size_t bytes, off;
  };
  std::vector<Piece> pieces;
  ScratchLayout L;
  ScratchRegion up, down;
  L.open(up).take<BowKf>(kf.size());
  auto place = [&](const void* src, size_t bytes) {
    const size_t off = L.take(bytes);
    pieces.push_back({src, bytes, off});
    return (uint32_t)off;
  };
  const std::vector<uint8_t> zeros((size_t)max_n, 0);
  bool any_null = !q->flags;
  for (int32_t i = 0; i < n_kf; ++i) any_null = any_null || !kf_flags || !kf_flags[i];
  const uint32_t o_zero = any_null ? place(zeros.data(), zeros.size()) : 0;
  for (int32_t i = 0; i < n_kf; ++i)
    kf[(size_t)i].o_flags = (kf_flags && kf_flags[i]) ? place(kf_flags[i], (size_t)ent[(size_t)i]->n) : o_zero;
  const uint32_t o_qflags = q->flags ? place(q->flags, (size_t)qn) : o_zero;
  BowQuery qh = {};
  BowQueryStored qs = {};
  if (qe) {
    qs.kps = qe->at<orbfe_keypoint>(qe->o_kps), qs.desc = qe->at<uint8_t>(qe->o_desc);
    qs.nodes = qe->bow<uint32_t>(qe->o_nodes), qs.offs = qe->bow<int32_t>(qe->o_offs), qs.feat = qe->bow<uint32_t>(qe->o_feat);
    qs.o_flags = o_qflags, qs.n_nodes = qe->n_nodes;
  } else {
    qh.o_desc = place(q->desc, (size_t)qn * 32);
    qh.o_angle = check_orientation ? place(q->angle, (size_t)qn * 4) : 0;
    qh.o_nodes = place(q->nodes, (size_t)q->n_nodes * 4);
    qh.o_offs = place(q->node_offsets, ((size_t)q->n_nodes + 1) * 4);
    qh.o_feat = place(q->features, (size_t)q->node_offsets[q->n_nodes] * 4);
    qh.o_flags = o_qflags, qh.n_nodes = q->n_nodes;
  }
  BowParams P = {};
  P.mode = mode, P.dist_threshold = dist_threshold, P.check_orientation = check_orientation ? 1 : 0, P.n_kf = n_kf, P.ratio = ratio;
  P.cap = (int32_t)std::min<int64_t>(cap, n_slots);
  // device scratch behind the upload: slots, the candidates' own lists, their lengths | the download (offsets, matches)
  const size_t ns = (size_t)n_slots;
  const size_t o_slots = L.close(up).take<BowSlot>(ns), o_lists = L.take<BowMatch>(ns), o_cnt = L.take<int32_t>((size_t)n_kf),
               o_off = L.open(down).take<int32_t>((size_t)n_kf + 1), o_m = L.take<BowMatch>((size_t)P.cap);
  L.close(down);
  HIP_TRY(c, hipSetDevice(c->device));
  StagedIo io;
  TRY(io.reserve(c, L.end(), up.end + down.bytes()));
  io.put(0, kf.data(), kf.size() * sizeof(BowKf));
  for (const Piece& p : pieces) io.put(p.off, p.src, p.bytes);
  HIP_TRY(c, io.upload(up));
  {
    StageTimer tm(c, ORBFE_STAGE_MATCH, c->stream);
    if (qe)
      launch_bow_search(c->stream, io.d, io.dev<BowKf>(0), qs, P, max_feat, io.dev<BowSlot>(o_slots), io.dev<BowMatch>(o_lists),
                        io.dev<int32_t>(o_cnt), io.dev<int32_t>(o_off), io.dev<BowMatch>(o_m));
    else
      launch_bow_search(c->stream, io.d, io.dev<BowKf>(0), qh, P, max_feat, io.dev<BowSlot>(o_slots), io.dev<BowMatch>(o_lists),
                        io.dev<int32_t>(o_cnt), io.dev<int32_t>(o_off), io.dev<BowMatch>(o_m));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down, up.end));  // (behind the staged inputs)
  drain_timers(c);
  const int32_t* off = (const int32_t*)io.got(o_off);
  for (int32_t i = 0; i <= n_kf; ++i)
    if (off[i] < 0 || off[i] > n_slots || (i > 0 && off[i] < off[i - 1])) return fail(c, ORBFE_EDEVICE, "%s: corrupt offsets", fn);
  for (int32_t i = 0; i <= n_kf; ++i) match_offsets[i] = off[i];
  const int64_t total = off[n_kf];
  if (total > cap) return fail(c, ORBFE_ECAPACITY, "%s: %lld matches, room for %lld", fn, (long long)total, (long long)cap);
  io.get(matches, o_m, (size_t)total * sizeof(BowMatch));
  return ORBFE_OK;
}

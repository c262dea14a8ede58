// orbfe_tri.hip -- host side of orbfe_create_new_map_points and orbfe_create_new_map_points_stored (include/orbfe.h): argument checks,
// the baseline test (T7), one upload into the context's scratch, the launch sequence of k_tri.hip, one download.  The stored form
// names its keyframes by their id in a keyframe store (orbfe_kfstore.h) and uploads only the map state; everything behind the keyframe
// records (tri_run) is one text for both.
#include "orbfe_kfstore.h"

void launch_tri(hipStream_t st, const uint8_t* up, const TriKf* kfs, const TriParams& P, int max_feat, TriSlot* slots, int32_t* cnt,
                int32_t* off, int32_t* fill, int32_t* list, int32_t* acc, int32_t* tail_flag, int32_t* pos, int32_t* hdr, TriRec* recs,
                int32_t* tail, uint8_t* consumed);
void launch_tri(hipStream_t st, const uint8_t* up, const TriKfStored* kfs, const TriParams& P, int max_feat, TriSlot* slots, int32_t* cnt,
                int32_t* off, int32_t* fill, int32_t* list, int32_t* acc, int32_t* tail_flag, int32_t* pos, int32_t* hdr, TriRec* recs,
                int32_t* tail, uint8_t* consumed);

// the checks of a FeatureVector in orbfe_bow_out's layout over n features (orbfe_tri_kf, orbfe_kfstore_set_bow)
orbfe_status check_feature_vector(orbfe_ctx* c, const char* fn, const char* who, int idx, int32_t n, int32_t n_nodes, const uint32_t* nodes,
                                  const int32_t* node_offsets, const uint32_t* features) {
  if (n_nodes < 0 || n_nodes > n) return fail(c, ORBFE_EBADARG, "%s: %s %d: %d features, %d nodes", fn, who, idx, n, n_nodes);
  if (!node_offsets || (n_nodes > 0 && (!nodes || !features))) return fail(c, ORBFE_EBADARG, "%s: %s %d: NULL FeatureVector array", fn, who, idx);
  if (node_offsets[0] != 0) return fail(c, ORBFE_EBADARG, "%s: %s %d: node_offsets[0] != 0", fn, who, idx);
  for (int32_t i = 0; i < n_nodes; ++i) {
    if (node_offsets[i + 1] < node_offsets[i] || node_offsets[i + 1] > n)
      return fail(c, ORBFE_EBADARG, "%s: %s %d: node_offsets[%d] out of order or range", fn, who, idx, i + 1);
    if (i > 0 && !(nodes[i] > nodes[i - 1])) return fail(c, ORBFE_EBADARG, "%s: %s %d: nodes not strictly ascending at %d", fn, who, idx, i);
  }
  const int32_t nf = node_offsets[n_nodes];
  for (int32_t i = 0; i < nf; ++i)
    if (features[i] >= (uint32_t)n)
      return fail(c, ORBFE_EBADARG, "%s: %s %d: feature index %u out of range (%d features)", fn, who, idx, features[i], n);
  return ORBFE_OK;
}

namespace {

orbfe_status check_kf(orbfe_ctx* c, const orbfe_tri_kf* k, int32_t n_levels, const char* who, int idx) {
  if (k->n < 0 || k->n > ORBFE_BOW_MAX_FEATURES || k->n_nodes < 0 || k->n_nodes > k->n)
    return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: %d features, %d nodes", who, idx, k->n, k->n_nodes);
  if (k->n > 0 && (!k->kps || !k->desc || !k->flags || !k->depth || !k->right_u))
    return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: NULL array", who, idx);
  TRY(check_feature_vector(c, "create_new_map_points", who, idx, k->n, k->n_nodes, k->nodes, k->node_offsets, k->features));
  for (int32_t i = 0; i < k->n; ++i)
    if (k->kps[i].octave < 0 || k->kps[i].octave >= n_levels)
      return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: feature %d has octave %d outside 0..%d", who, idx, i, k->kps[i].octave, n_levels - 1);
  return ORBFE_OK;
}

static_assert(sizeof(TriKf) == 184, "tools/tri_bench.py counts 184 bytes per keyframe record");

struct Piece {  // an input array and where it goes in the upload
  const void* src;
  size_t bytes, off;
};

// T7: (float)cv::norm(Ow_cur - Ow_nb) < mfBl skips the neighbour (cv::norm in double)
int32_t below_baseline(const float* ow_cur, const float* ow_nb, float bl) {
  double s = 0;
  for (int a = 0; a < 3; ++a) {
    const float df = ow_cur[a] - ow_nb[a];
    s = s + (double)df * (double)df;
  }
  return (float)std::sqrt(s) < bl ? 1 : 0;
}

// Everything behind the keyframe records: L holds the open upload region `up` with the records at offset 0 and the pieces placed; the
// device scratch is laid out behind it, the launch sequence runs and the header, records, tail and consumed flags come down.
template <class KF>
orbfe_status tri_run(orbfe_ctx* c, ScratchLayout& L, ScratchRegion& up, const std::vector<KF>& kf, const std::vector<Piece>& pieces, TriParams& P,
                     int32_t max_feat, orbfe_tri_record* records, int64_t cap, int64_t* n_records, int32_t* tail, int64_t tail_cap,
                     int64_t* n_tail, uint8_t* consumed) {
  const int32_t n_cur = P.n_cur, n_slots = P.n_slots;
  P.rec_cap = (int32_t)std::min<int64_t>(cap, std::min(n_slots, n_cur));
  P.tail_cap = (int32_t)std::min<int64_t>(tail_cap, n_cur);
  // device scratch behind the upload: zeroed counters | offsets, lists, slots, positions | the download (header, records, tail)
  ScratchRegion zero, down;
  const size_t nc = (size_t)n_cur, ns = (size_t)n_slots;
  const size_t o_cnt = L.close(up).open(zero).take<int32_t>(nc), o_fill = L.take<int32_t>(nc), o_acc = L.take<int32_t>(ns),
               o_off = L.close(zero).take<int32_t>(nc + 1),  // k_tri_scan writes the total into off[n_cur]
               o_list = L.take<int32_t>(ns), o_slots = L.take<TriSlot>(ns), o_tf = L.take<int32_t>(nc),
               o_pos = L.take<int32_t>(std::max(nc, ns) + 1),  // k_tri_compact scans n_slots, then n_cur flags into pos[0 .. n]
               o_hdr = L.open(down).take<int32_t>(2), o_rec = L.take<TriRec>((size_t)P.rec_cap), o_tail = L.take<int32_t>((size_t)P.tail_cap),
               o_cons = L.take(nc);
  L.close(down);
  StagedIo io;
  TRY(io.reserve(c, L.end(), up.end + down.bytes()));
  io.put(0, kf.data(), kf.size() * sizeof(KF));
  for (const Piece& p : pieces) io.put(p.off, p.src, p.bytes);
  HIP_TRY(c, io.upload(up));
  HIP_TRY(c, hipMemsetAsync(io.dev<uint8_t>(zero.begin), 0, zero.bytes(), c->stream));
  launch_tri(c->stream, io.d, io.dev<KF>(0), P, max_feat, io.dev<TriSlot>(o_slots), io.dev<int32_t>(o_cnt), io.dev<int32_t>(o_off),
             io.dev<int32_t>(o_fill), io.dev<int32_t>(o_list), io.dev<int32_t>(o_acc), io.dev<int32_t>(o_tf), io.dev<int32_t>(o_pos),
             io.dev<int32_t>(o_hdr), io.dev<TriRec>(o_rec), io.dev<int32_t>(o_tail), io.dev<uint8_t>(o_cons));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down, up.end));  // (behind the staged inputs)
  int32_t h[2];
  io.get(h, o_hdr, sizeof h);
  *n_records = h[0];
  *n_tail = h[1];
  if (h[0] < 0 || h[0] > std::min(n_slots, n_cur) || h[1] < 0 || h[1] > n_cur)
    return fail(c, ORBFE_EDEVICE, "create_new_map_points: corrupt counts %d / %d", h[0], h[1]);
  if (h[0] > cap || h[1] > tail_cap)
    return fail(c, ORBFE_ECAPACITY, "create_new_map_points: %d records (room for %lld), %d tail entries (room for %lld)", h[0], (long long)cap,
                h[1], (long long)tail_cap);
  static_assert(sizeof(TriRec) == sizeof(orbfe_tri_record), "TriRec is orbfe_tri_record");
  io.get(records, o_rec, (size_t)h[0] * sizeof(TriRec));
  io.get(tail, o_tail, (size_t)h[1] * 4);
  io.get(consumed, o_cons, nc);
  return ORBFE_OK;
}

}  // namespace

extern "C" {

orbfe_status orbfe_create_new_map_points(orbfe_ctx* c, const orbfe_tri_kf* cur, int32_t n_nb, const orbfe_tri_kf* nbs, const orbfe_camera* cam,
                                         const float* k_inv, float bl, const float* scale_factors, int32_t n_levels, orbfe_tri_record* records,
                                         int64_t cap, int64_t* n_records, int32_t* tail, int64_t tail_cap, int64_t* n_tail, uint8_t* consumed) {
  ApiLock api_lk(c);
  if (!c || !cur || !cam || !k_inv || !scale_factors || !n_records || !n_tail || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS || cap < 0 ||
      tail_cap < 0 || (cap > 0 && !records) || (tail_cap > 0 && !tail) || (n_nb > 0 && !nbs))
    return fail(c, ORBFE_EBADARG, "create_new_map_points: bad arguments");
  if (n_nb < 0 || n_nb > ORBFE_TRI_MAX_NB) return fail(c, ORBFE_EBADARG, "create_new_map_points: %d neighbours, 0..%d allowed", n_nb, ORBFE_TRI_MAX_NB);
  *n_records = 0;
  *n_tail = 0;
  TRY(check_kf(c, cur, n_levels, "current keyframe", 0));
  if (cur->n > 0 && (!cur->unproc || !cur->unproc_pos)) return fail(c, ORBFE_EBADARG, "create_new_map_points: NULL unprocessed arrays");
  for (int32_t i = 0; i < n_nb; ++i) TRY(check_kf(c, nbs + i, n_levels, "neighbour", i));
  HIP_TRY(c, hipSetDevice(c->device));

  // the upload: [TriKf x (1 + n_nb)] | scale factors | every keyframe's arrays | cur's unprocessed flags and positions
  std::vector<TriKf> kf((size_t)n_nb + 1);
  std::vector<Piece> pieces;
  ScratchLayout L;
  ScratchRegion up;
  L.open(up).take<TriKf>(kf.size());
  auto place = [&](const void* src, size_t bytes, uint32_t* off) {
    *off = (uint32_t)L.take(bytes);
    pieces.push_back({src, bytes, *off});
  };
  TriParams P = {};
  int32_t n_slots = 0, max_feat = 0;
  for (int32_t i = 0; i <= n_nb; ++i) {
    const orbfe_tri_kf& k = i == 0 ? *cur : nbs[i - 1];
    TriKf& d = kf[(size_t)i];
    const size_t n = (size_t)k.n;
    d.n = k.n;
    d.n_nodes = k.n_nodes;
    d.n_feat = k.node_offsets[k.n_nodes];
    std::memcpy(d.Tcw, k.Tcw, sizeof d.Tcw);
    std::memcpy(d.Twc, k.Twc, sizeof d.Twc);
    if (i > 0) {
      d.skip = below_baseline(cur->Ow, k.Ow, bl);
      d.slot0 = n_slots;
      n_slots += d.n_feat;
      max_feat = std::max(max_feat, d.n_feat);
    }
    place(k.kps, n * sizeof(orbfe_keypoint), &d.o_kps);
    place(k.desc, n * 32, &d.o_desc);
    place(k.nodes, (size_t)k.n_nodes * 4, &d.o_nodes);
    place(k.node_offsets, ((size_t)k.n_nodes + 1) * 4, &d.o_offs);
    place(k.features, (size_t)d.n_feat * 4, &d.o_feat);
    place(k.flags, n, &d.o_flags);
    place(k.depth, n * 8, &d.o_depth);
    place(k.right_u, n * 8, &d.o_ru);
  }
  place(scale_factors, (size_t)n_levels * 4, &P.o_sf);
  place(cur->unproc, (size_t)cur->n, &P.o_unproc);
  place(cur->unproc_pos, (size_t)cur->n * 12, &P.o_upos);
  P.fx = cam->fx, P.fy = cam->fy, P.cx = cam->cx, P.cy = cam->cy;
  std::memcpy(P.kinv, k_inv, sizeof P.kinv);
  P.n_nb = n_nb;
  P.n_levels = n_levels;
  P.n_cur = cur->n;
  P.n_slots = n_slots;
  return tri_run(c, L, up, kf, pieces, P, max_feat, records, cap, n_records, tail, tail_cap, n_tail, consumed);
}

orbfe_status orbfe_create_new_map_points_stored(orbfe_ctx* c, orbfe_kfstore* store, uint64_t cur_id, const orbfe_tri_state* cur, int32_t n_nb,
                                                const uint64_t* nb_ids, const orbfe_tri_state* nbs, const orbfe_camera* cam, const float* k_inv,
                                                float bl, const float* scale_factors, int32_t n_levels, orbfe_tri_record* records, int64_t cap,
                                                int64_t* n_records, int32_t* tail, int64_t tail_cap, int64_t* n_tail, uint8_t* consumed) {
  ApiLock api_lk(c);
  const char* fn = "create_new_map_points_stored";
  if (!c || !store || !cur || !cam || !k_inv || !scale_factors || !n_records || !n_tail || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS ||
      cap < 0 || tail_cap < 0 || (cap > 0 && !records) || (tail_cap > 0 && !tail) || (n_nb > 0 && (!nbs || !nb_ids)))
    return fail(c, ORBFE_EBADARG, "%s: bad arguments", fn);
  if (n_nb < 0 || n_nb > ORBFE_TRI_MAX_NB) return fail(c, ORBFE_EBADARG, "%s: %d neighbours, 0..%d allowed", fn, n_nb, ORBFE_TRI_MAX_NB);
  TRY(kfstore_check_ctx(c, store, fn));
  if (n_levels < store->n_levels) return fail(c, ORBFE_EBADARG, "%s: %d scale factors, the store's octaves go up to %d", fn, n_levels, store->n_levels - 1);
  *n_records = 0;
  *n_tail = 0;
  std::shared_lock<std::shared_timed_mutex> store_lk(store->mu);  // held until the results are down: no erase frees memory under the kernels
  std::vector<TriKfStored> kf((size_t)n_nb + 1);
  std::vector<Piece> pieces;
  ScratchLayout L;
  ScratchRegion up;
  L.open(up).take<TriKfStored>(kf.size());
  auto place = [&](const void* src, size_t bytes, uint32_t* off) {
    *off = (uint32_t)L.take(bytes);
    pieces.push_back({src, bytes, *off});
  };
  TriParams P = {};
  int32_t n_slots = 0, max_feat = 0;
  for (int32_t i = 0; i <= n_nb; ++i) {
    const uint64_t id = i == 0 ? cur_id : nb_ids[i - 1];
    const orbfe_tri_state& k = i == 0 ? *cur : nbs[i - 1];
    const KfEntry* e = store->map.find(id);
    if (!e) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)id);
    if (!e->has_bow) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu has no FeatureVector (orbfe_kfstore_set_bow)", fn, (unsigned long long)id);
    if (k.n != e->n) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu has %d features, the state says %d", fn, (unsigned long long)id, e->n, k.n);
    if (e->n > 0 && (!k.flags || (i == 0 && (!k.unproc || !k.unproc_pos)))) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu: NULL array", fn, (unsigned long long)id);
    TriKfStored& d = kf[(size_t)i];
    d.kps = e->at<orbfe_keypoint>(e->o_kps), d.desc = e->at<uint8_t>(e->o_desc);
    d.depth = e->at<double>(e->o_depth), d.ru = e->at<double>(e->o_ru);
    d.nodes = e->bow<uint32_t>(e->o_nodes), d.offs = e->bow<int32_t>(e->o_offs), d.feat = e->bow<uint32_t>(e->o_feat);
    d.n = e->n, d.n_nodes = e->n_nodes, d.n_feat = e->n_feat, d.pad = 0;
    std::memcpy(d.Tcw, k.Tcw, sizeof d.Tcw);
    std::memcpy(d.Twc, k.Twc, sizeof d.Twc);
    if (i > 0) {
      d.skip = below_baseline(cur->Ow, k.Ow, bl);
      d.slot0 = n_slots;
      n_slots += d.n_feat;
      max_feat = std::max(max_feat, d.n_feat);
    }
    place(k.flags, (size_t)e->n, &d.o_flags);
  }
  place(scale_factors, (size_t)n_levels * 4, &P.o_sf);
  place(cur->unproc, (size_t)kf[0].n, &P.o_unproc);
  place(cur->unproc_pos, (size_t)kf[0].n * 12, &P.o_upos);
  P.fx = cam->fx, P.fy = cam->fy, P.cx = cam->cx, P.cy = cam->cy;
  std::memcpy(P.kinv, k_inv, sizeof P.kinv);
  P.n_nb = n_nb;
  P.n_levels = n_levels;
  P.n_cur = kf[0].n;
  P.n_slots = n_slots;
  HIP_TRY(c, hipSetDevice(c->device));
  return tri_run(c, L, up, kf, pieces, P, max_feat, records, cap, n_records, tail, tail_cap, n_tail, consumed);
}

}  // extern "C"

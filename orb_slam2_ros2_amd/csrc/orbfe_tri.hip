// orbfe_tri.hip -- host side of orbfe_create_new_map_points (include/orbfe.h): argument checks, the baseline test (T7), one upload
// into the context's scratch, the launch sequence of k_tri.hip, one download.
#include "orbfe_ctx.h"

void launch_tri(hipStream_t st, const uint8_t* up, const TriKf* kfs, const TriParams& P, int max_feat, TriSlot* slots, int32_t* cnt,
                int32_t* off, int32_t* fill, int32_t* list, int32_t* acc, int32_t* tail_flag, int32_t* pos, int32_t* hdr, TriRec* recs,
                int32_t* tail, uint8_t* consumed);

namespace {

orbfe_status check_kf(orbfe_ctx* c, const orbfe_tri_kf* k, int32_t n_levels, const char* who, int idx) {
  if (k->n < 0 || k->n > ORBFE_BOW_MAX_FEATURES || k->n_nodes < 0 || k->n_nodes > k->n)
    return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: %d features, %d nodes", who, idx, k->n, k->n_nodes);
  if (k->n > 0 && (!k->kps || !k->desc || !k->flags || !k->depth || !k->right_u))
    return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: NULL array", who, idx);
  if (!k->node_offsets || (k->n_nodes > 0 && (!k->nodes || !k->features)))
    return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: NULL FeatureVector array", who, idx);
  if (k->node_offsets[0] != 0) return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: node_offsets[0] != 0", who, idx);
  for (int32_t i = 0; i < k->n_nodes; ++i) {
    if (k->node_offsets[i + 1] < k->node_offsets[i] || k->node_offsets[i + 1] > k->n)
      return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: node_offsets[%d] out of order or range", who, idx, i + 1);
    if (i > 0 && !(k->nodes[i] > k->nodes[i - 1]))
      return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: nodes not strictly ascending at %d", who, idx, i);
  }
  const int32_t nf = k->node_offsets[k->n_nodes];
  for (int32_t i = 0; i < nf; ++i)
    if (k->features[i] >= (uint32_t)k->n)
      return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: feature index %u out of range (%d features)", who, idx, k->features[i], k->n);
  for (int32_t i = 0; i < k->n; ++i)
    if (k->kps[i].octave < 0 || k->kps[i].octave >= n_levels)
      return fail(c, ORBFE_EBADARG, "create_new_map_points: %s %d: feature %d has octave %d outside 0..%d", who, idx, i, k->kps[i].octave, n_levels - 1);
  return ORBFE_OK;
}

static_assert(sizeof(TriKf) == 184, "tools/tri_bench.py counts 184 bytes per keyframe record");

struct Piece {
  const void* src;
  size_t bytes;
  uint32_t* off;
};

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
  ScratchRegion up, zero, down;
  L.open(up).take<TriKf>(kf.size());
  auto place = [&](const void* src, size_t bytes, uint32_t* off) {
    *off = (uint32_t)L.take(bytes);
    pieces.push_back({src, bytes, off});
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
      // T7: (float)cv::norm(Ow_cur - Ow_nb) < mfBl skips the neighbour (cv::norm in double)
      double s = 0;
      for (int a = 0; a < 3; ++a) {
        const float df = cur->Ow[a] - k.Ow[a];
        s = s + (double)df * (double)df;
      }
      d.skip = (float)std::sqrt(s) < bl ? 1 : 0;
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
  P.rec_cap = (int32_t)std::min<int64_t>(cap, std::min(n_slots, cur->n));
  P.tail_cap = (int32_t)std::min<int64_t>(tail_cap, cur->n);

  // device scratch behind the upload: zeroed counters | offsets, lists, slots, positions | the download (header, records, tail)
  const size_t nc = (size_t)cur->n, ns = (size_t)n_slots;
  const size_t o_cnt = L.close(up).open(zero).take<int32_t>(nc), o_fill = L.take<int32_t>(nc), o_acc = L.take<int32_t>(ns),
               o_off = L.close(zero).take<int32_t>(nc + 1),  // k_tri_scan writes the total into off[n_cur]
               o_list = L.take<int32_t>(ns), o_slots = L.take<TriSlot>(ns), o_tf = L.take<int32_t>(nc),
               o_pos = L.take<int32_t>(std::max(nc, ns) + 1),  // k_tri_compact scans n_slots, then n_cur flags into pos[0 .. n]
               o_hdr = L.open(down).take<int32_t>(2), o_rec = L.take<TriRec>((size_t)P.rec_cap), o_tail = L.take<int32_t>((size_t)P.tail_cap),
               o_cons = L.take(nc);
  L.close(down);
  StagedIo io;
  TRY(io.reserve(c, L.end(), up.end + down.bytes()));
  io.put(0, kf.data(), kf.size() * sizeof(TriKf));
  for (const Piece& p : pieces) io.put(*p.off, p.src, p.bytes);
  HIP_TRY(c, io.upload(up));
  HIP_TRY(c, hipMemsetAsync(io.dev<uint8_t>(zero.begin), 0, zero.bytes(), c->stream));
  launch_tri(c->stream, io.d, io.dev<TriKf>(0), P, max_feat, io.dev<TriSlot>(o_slots), io.dev<int32_t>(o_cnt), io.dev<int32_t>(o_off),
             io.dev<int32_t>(o_fill), io.dev<int32_t>(o_list), io.dev<int32_t>(o_acc), io.dev<int32_t>(o_tf), io.dev<int32_t>(o_pos),
             io.dev<int32_t>(o_hdr), io.dev<TriRec>(o_rec), io.dev<int32_t>(o_tail), io.dev<uint8_t>(o_cons));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down, up.end));  // (behind the staged inputs)
  int32_t h[2];
  io.get(h, o_hdr, sizeof h);
  *n_records = h[0];
  *n_tail = h[1];
  if (h[0] < 0 || h[0] > std::min(n_slots, cur->n) || h[1] < 0 || h[1] > cur->n)
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

}  // extern "C"

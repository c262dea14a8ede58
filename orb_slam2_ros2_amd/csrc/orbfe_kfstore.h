// orbfe_kfstore.h -- the keyframe store's record (include/orbfe.h) as its host side (orbfe_kfstore.hip) and the calls
// that read it (orbfe_fuse.hip, orbfe_tri.hip, orbfe_bowsearch.hip, orbfe_sim3search.hip, orbfe_fusepoints.hip) see it.
#pragma once
#include <shared_mutex>

#include "kfstore_alloc.h"
#include "orbfe_ctx.h"

// One keyframe: a block [kps | desc | depth | right_u | cell_off | cell_feat] (every array on a 256-byte boundary, scratch_layout.h's
// rule) and, once set_bow has run, a second block [nodes | node_offsets | features].
struct KfEntry {
  int32_t n = 0;
  AreaGrid ag = {0, 0, 0, 0};
  float bounds[4] = {0, 0, 0, 0};
  KfBlock blk, bow_blk;
  uint8_t *base = nullptr, *bow_base = nullptr;  // device addresses of the two blocks
  size_t o_kps = 0, o_desc = 0, o_depth = 0, o_ru = 0, o_coff = 0, o_cfeat = 0, front = 0;  // front: bytes an insertion uploads
  bool has_bow = false;
  bool has_stereo = false;  // depth and right_u were supplied at insertion (else both are -1 throughout)
  int32_t n_nodes = 0, n_feat = 0;
  size_t o_nodes = 0, o_offs = 0, o_feat = 0;
  template <typename T>
  T* at(size_t off) const { return (T*)(base + off); }
  template <typename T>
  T* bow(size_t off) const { return (T*)(bow_base + off); }
  size_t ncells() const { return (size_t)ag.rows * ag.cols; }
};

struct orbfe_kfstore {
  std::shared_timed_mutex mu;  // add / add_from_slot / set_bow / erase exclusive; fetch / info / size / the stored calls shared
  int device = 0;
  int32_t width = 0, height = 0, n_levels = 0;
  hipStream_t stream = nullptr;  // add / set_bow / fetch (add_from_slot and the stored calls run on their context's stream)
  KfSlabAlloc alloc{0};
  std::vector<uint8_t*> slab_dev;  // device memory of slab i (nullptr: released)
  KfIdMap<KfEntry> map;
  uint8_t* h_io = nullptr;  // page-locked staging of an insertion
  size_t h_bytes = 0;
};

// the context may use the store: same device
static inline orbfe_status kfstore_check_ctx(orbfe_ctx* c, const orbfe_kfstore* s, const char* who) {
  if (c->device != s->device) return fail(c, ORBFE_EBADARG, "%s: the context is on device %d, the keyframe store on device %d", who, c->device, s->device);
  return ORBFE_OK;
}

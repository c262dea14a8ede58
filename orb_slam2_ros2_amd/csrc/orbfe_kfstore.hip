// orbfe_kfstore.hip -- host side of the keyframe store (include/orbfe.h): slabs, the id map, insertion from host arrays
// and from an extraction slot, the FeatureVector, erase, info and fetch.  The bookkeeping is kfstore_alloc.h (no HIP in it), the one
// kernel k_kfstore.hip; the calls that read the store are in orbfe_fuse.hip and orbfe_tri.hip.
#include "orbfe_kfstore.h"

void launch_kfstore_pack(hipStream_t st, KfPack A, size_t grid_lds, bool copy);
orbfe_status check_feature_vector(orbfe_ctx* c, const char* fn, const char* who, int idx, int32_t n, int32_t n_nodes, const uint32_t* nodes,
                                  const int32_t* node_offsets, const uint32_t* features);

namespace {

const size_t kDefaultSlab = (size_t)32 << 20;

// a block of `bytes`, from a new slab if the existing ones have no room
orbfe_status take_block(orbfe_kfstore* s, size_t bytes, KfBlock* b, uint8_t** base) {
  if (!s->alloc.take(bytes, b)) {
    const size_t sz = s->alloc.slab_size_for(bytes);
    uint8_t* p = nullptr;
    if (hipMalloc((void**)&p, sz) != hipSuccess) {
      (void)hipGetLastError();
      return fail(nullptr, ORBFE_ENOMEM, "kfstore: cannot allocate a slab of %zu bytes on device %d", sz, s->device);
    }
    const size_t idx = (size_t)s->alloc.add_slab(sz);
    if (s->slab_dev.size() <= idx) s->slab_dev.resize(idx + 1, nullptr);
    s->slab_dev[idx] = p;
    if (!s->alloc.take(bytes, b)) return fail(nullptr, ORBFE_ENOMEM, "kfstore: a fresh slab of %zu bytes has no room for %zu", sz, bytes);
  }
  *base = s->slab_dev[(size_t)b->slab] + b->off;
  return ORBFE_OK;
}

void give_block(orbfe_kfstore* s, const KfBlock& b) {
  if (b.slab < 0) return;
  if (s->alloc.give(b)) {
    (void)hipFree(s->slab_dev[(size_t)b.slab]);
    s->slab_dev[(size_t)b.slab] = nullptr;
  }
}

orbfe_status stage_reserve(orbfe_kfstore* s, size_t bytes) {
  if (s->h_bytes >= bytes) return ORBFE_OK;
  if (s->h_io) (void)hipHostFree(s->h_io);
  s->h_io = nullptr;
  s->h_bytes = 0;
  const size_t b = std::max<size_t>(bytes + bytes / 2, 1 << 18);
  HIP_TRY(nullptr, hipHostMalloc((void**)&s->h_io, b, hipHostMallocDefault));
  s->h_bytes = b;
  return ORBFE_OK;
}

// the entry's geometry: its grid from the bounds (the rules of orbfe_fuse_into_keyframes), the layout of its block
orbfe_status plan_entry(orbfe_ctx* c, const orbfe_kfstore* s, const char* fn, int32_t n, const float* bounds, KfEntry* e, size_t* total, size_t* grid_lds,
                        int* in_lds) {
  if (!area_grid(s->width, s->height, bounds, &e->ag)) return fail(c, ORBFE_EBADARG, "%s: bad frame bounds", fn);
  const size_t ncells = e->ncells();
  const AreaGridLds g = area_grid_lds(ncells, (size_t)n);
  if (g.refused) return fail(c, ORBFE_EBADSIZE, "%s: %zu grid cells exceed the LDS counters", fn, ncells);
  *in_lds = g.in_lds;
  *grid_lds = g.bytes;
  e->n = n;
  const float whole[4] = {0.f, (float)s->width, 0.f, (float)s->height};
  std::memcpy(e->bounds, bounds ? bounds : whole, sizeof e->bounds);
  ScratchLayout L;
  e->o_kps = L.take<orbfe_keypoint>((size_t)n), e->o_desc = L.take((size_t)n * 32), e->o_depth = L.take<double>((size_t)n),
  e->o_ru = L.take<double>((size_t)n);
  e->front = L.end();
  e->o_coff = L.take<int32_t>(ncells + 1), e->o_cfeat = L.take<int32_t>((size_t)n);
  *total = L.end();
  return ORBFE_OK;
}

KfPack pack_args(const KfEntry& e, int in_lds) {
  KfPack A = {};
  A.kps = e.at<orbfe_keypoint>(e.o_kps), A.desc = e.at<uint8_t>(e.o_desc), A.depth = e.at<double>(e.o_depth), A.right_u = e.at<double>(e.o_ru);
  A.cell_off = e.at<int32_t>(e.o_coff), A.cell_feat = e.at<int32_t>(e.o_cfeat);
  A.n = e.n, A.rows = e.ag.rows, A.cols = e.ag.cols, A.in_lds = in_lds;
  return A;
}

}  // namespace

extern "C" {

orbfe_status orbfe_kfstore_create(int32_t device_id, int32_t width, int32_t height, int32_t n_levels, int64_t slab_bytes, orbfe_kfstore** out) {
  if (!out || width < 1 || height < 1 || width > 65536 || height > 65536 || n_levels < 1 || n_levels > ORBFE_MAX_LEVELS || slab_bytes < 0)
    return fail(nullptr, ORBFE_EBADARG, "orbfe_kfstore_create: bad arguments");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_kfstore_create: no HIP device (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfstore_create: device %d of %d", device_id, ndev);
  std::unique_ptr<orbfe_kfstore> s(new (std::nothrow) orbfe_kfstore());
  if (!s) return fail(nullptr, ORBFE_ENOMEM, "orbfe_kfstore_create: out of memory");
  s->device = device_id;
  s->width = width, s->height = height, s->n_levels = n_levels;
  s->alloc = KfSlabAlloc(slab_bytes ? (size_t)slab_bytes : kDefaultSlab);
  DeviceScope dev(device_id);
  if (dev.err != hipSuccess || hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess)
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_kfstore_create: cannot create a stream on device %d", device_id);
  *out = s.release();
  return ORBFE_OK;
}

void orbfe_kfstore_destroy(orbfe_kfstore* s) {
  if (!s) return;
  DeviceScope dev(s->device);
  for (uint8_t* p : s->slab_dev)
    if (p) (void)hipFree(p);
  if (s->h_io) (void)hipHostFree(s->h_io);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

orbfe_status orbfe_kfstore_add(orbfe_kfstore* s, uint64_t id, int32_t n, const orbfe_keypoint* kps, const uint8_t* desc, const double* depth,
                               const double* right_u, const float* bounds) {
  const char* fn = "orbfe_kfstore_add";
  if (!s || n < 0 || n > ORBFE_BOW_MAX_FEATURES || (n > 0 && (!kps || !desc))) return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", fn);
  for (int32_t i = 0; i < n; ++i)
    if (kps[i].octave < 0 || kps[i].octave >= s->n_levels)
      return fail(nullptr, ORBFE_EBADARG, "%s: feature %d has octave %d outside 0..%d", fn, i, kps[i].octave, s->n_levels - 1);
  KfEntry e;
  size_t total = 0, grid_lds = 0;
  int in_lds = 0;
  TRY(plan_entry(nullptr, s, fn, n, bounds, &e, &total, &grid_lds, &in_lds));
  std::unique_lock<std::shared_timed_mutex> lk(s->mu);
  if (s->map.find(id)) return fail(nullptr, ORBFE_EBADARG, "%s: keyframe %llu is already in the store", fn, (unsigned long long)id);
  DeviceScope dev(s->device);
  HIP_TRY(nullptr, dev.err);
  TRY(stage_reserve(s, e.front));
  TRY(take_block(s, total, &e.blk, &e.base));
  e.has_stereo = depth && right_u;
  const size_t N = (size_t)n;
  if (N) {
    std::memcpy(s->h_io + e.o_kps, kps, N * sizeof(orbfe_keypoint));
    std::memcpy(s->h_io + e.o_desc, desc, N * 32);
    double* hd = (double*)(s->h_io + e.o_depth);
    double* hr = (double*)(s->h_io + e.o_ru);
    for (size_t i = 0; i < N; ++i) hd[i] = depth ? depth[i] : -1.0, hr[i] = right_u ? right_u[i] : -1.0;
  }
  hipError_t err = hipMemcpyAsync(e.base, s->h_io, e.front, hipMemcpyHostToDevice, s->stream);
  if (err == hipSuccess) {
    KfPack A = pack_args(e, in_lds);
    A.s_kps = A.kps, A.s_desc = A.desc;
    launch_kfstore_pack(s->stream, A, grid_lds, false);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
  if (err != hipSuccess) {
    give_block(s, e.blk);
    return fail(nullptr, ORBFE_EDEVICE, "%s: %s", fn, hipGetErrorString(err));
  }
  s->map.insert(id, e);
  return ORBFE_OK;
}

orbfe_status orbfe_kfstore_add_from_slot(orbfe_ctx* c, orbfe_kfstore* s, uint64_t id, int32_t slot, int32_t pair, const float* bounds, int32_t* n_out) {
  ApiLock api_lk(c);
  const char* fn = "kfstore_add_from_slot";
  if (!c || !s || slot < 0 || slot >= c->cfg.max_images || pair >= (c->cfg.max_images + 1) / 2)
    return fail(c, ORBFE_EBADARG, "%s: bad arguments (slot %d, pair %d)", fn, slot, pair);
  TRY(kfstore_check_ctx(c, s, fn));
  if (c->cfg.n_levels > s->n_levels) return fail(c, ORBFE_EBADARG, "%s: the context has %d levels, the store %d", fn, c->cfg.n_levels, s->n_levels);
  TRY(slots_idle(c, slot, 1, fn));
  std::unique_lock<std::shared_timed_mutex> lk(s->mu);
  if (s->map.find(id)) return fail(c, ORBFE_EBADARG, "%s: keyframe %llu is already in the store", fn, (unsigned long long)id);
  HIP_TRY(c, hipSetDevice(c->device));
  TRY(join_stereo(c));
  // the count, behind the slot's pending work: the one download of this call
  const size_t NF = (size_t)c->cfg.n_features;
  StagedIo io;
  TRY(io.reserve(c, 0, 256));
  HIP_TRY(c, hipMemcpyAsync(io.h, c->d_n_kp + slot, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, io.wait());
  int32_t n = 0;
  io.get(&n, 0, 4);
  if (n < 0 || (size_t)n > NF || n > ORBFE_BOW_MAX_FEATURES) return fail(c, ORBFE_EDEVICE, "%s: corrupt count %d", fn, n);
  KfEntry e;
  size_t total = 0, grid_lds = 0;
  int in_lds = 0;
  TRY(plan_entry(c, s, fn, n, bounds, &e, &total, &grid_lds, &in_lds));
  TRY(take_block(s, total, &e.blk, &e.base));
  e.has_stereo = pair >= 0;
  KfPack A = pack_args(e, in_lds);
  A.s_kps = c->d_kps + (size_t)slot * NF;
  A.s_desc = c->d_desc + (size_t)slot * NF * 32;
  A.s_depth = pair >= 0 ? c->d_depth + (size_t)pair * NF : nullptr;
  A.s_right_u = pair >= 0 ? c->d_right_u + (size_t)pair * NF : nullptr;
  launch_kfstore_pack(c->stream, A, grid_lds, true);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
  if (err != hipSuccess) {
    give_block(s, e.blk);
    return fail(c, ORBFE_EDEVICE, "%s: %s", fn, hipGetErrorString(err));
  }
  s->map.insert(id, e);
  if (n_out) *n_out = n;
  return ORBFE_OK;
}

orbfe_status orbfe_kfstore_set_bow(orbfe_kfstore* s, uint64_t id, int32_t n_nodes, const uint32_t* nodes, const int32_t* node_offsets,
                                   const uint32_t* features) {
  const char* fn = "orbfe_kfstore_set_bow";
  if (!s) return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", fn);
  std::unique_lock<std::shared_timed_mutex> lk(s->mu);
  KfEntry* e = s->map.find(id);
  if (!e) return fail(nullptr, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)id);
  TRY(check_feature_vector(nullptr, fn, "keyframe", (int)id, e->n, n_nodes, nodes, node_offsets, features));
  const size_t nn = (size_t)n_nodes, nf = (size_t)node_offsets[n_nodes];
  ScratchLayout L;
  const size_t o_nodes = L.take<uint32_t>(nn), o_offs = L.take<int32_t>(nn + 1), o_feat = L.take<uint32_t>(nf);
  DeviceScope dev(s->device);
  HIP_TRY(nullptr, dev.err);
  TRY(stage_reserve(s, L.end()));
  KfBlock blk;
  uint8_t* base = nullptr;
  TRY(take_block(s, L.end(), &blk, &base));
  if (nn) std::memcpy(s->h_io + o_nodes, nodes, nn * 4);
  std::memcpy(s->h_io + o_offs, node_offsets, (nn + 1) * 4);
  if (nf) std::memcpy(s->h_io + o_feat, features, nf * 4);
  hipError_t err = hipMemcpyAsync(base, s->h_io, L.end(), hipMemcpyHostToDevice, s->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(s->stream);
  if (err != hipSuccess) {
    give_block(s, blk);
    return fail(nullptr, ORBFE_EDEVICE, "%s: %s", fn, hipGetErrorString(err));
  }
  if (e->has_bow) give_block(s, e->bow_blk);  // (exclusive lock: no call reads the old FeatureVector)
  e->has_bow = true;
  e->bow_blk = blk, e->bow_base = base;
  e->n_nodes = n_nodes, e->n_feat = (int32_t)nf;
  e->o_nodes = o_nodes, e->o_offs = o_offs, e->o_feat = o_feat;
  return ORBFE_OK;
}

orbfe_status orbfe_kfstore_erase(orbfe_kfstore* s, int32_t n, const uint64_t* ids) {
  if (!s || n < 0 || (n > 0 && !ids)) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfstore_erase: bad arguments");
  std::unique_lock<std::shared_timed_mutex> lk(s->mu);
  DeviceScope dev(s->device);
  for (int32_t i = 0; i < n; ++i) {
    KfEntry e;
    if (!s->map.erase(ids[i], &e)) continue;
    give_block(s, e.blk);
    if (e.has_bow) give_block(s, e.bow_blk);
  }
  return ORBFE_OK;
}

orbfe_status orbfe_kfstore_size(orbfe_kfstore* s, int64_t* n_keyframes, int64_t* bytes_used, int64_t* bytes_reserved) {
  if (!s) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfstore_size: NULL argument");
  std::shared_lock<std::shared_timed_mutex> lk(s->mu);
  if (n_keyframes) *n_keyframes = (int64_t)s->map.size();
  if (bytes_used) *bytes_used = (int64_t)s->alloc.used_bytes();
  if (bytes_reserved) *bytes_reserved = (int64_t)s->alloc.reserved_bytes();
  return ORBFE_OK;
}

orbfe_status orbfe_kfstore_info_get(orbfe_kfstore* s, uint64_t id, orbfe_kfstore_info* out) {
  if (!s || !out) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfstore_info_get: NULL argument");
  std::shared_lock<std::shared_timed_mutex> lk(s->mu);
  const KfEntry* e = s->map.find(id);
  if (!e) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfstore_info_get: keyframe %llu is not in the store", (unsigned long long)id);
  out->n = e->n;
  out->has_bow = e->has_bow ? 1 : 0;
  out->has_stereo = e->has_stereo ? 1 : 0;
  out->n_nodes = e->n_nodes, out->n_bow_features = e->n_feat;
  out->grid_rows = e->ag.rows, out->grid_cols = e->ag.cols;
  std::memcpy(out->bounds, e->bounds, sizeof out->bounds);
  out->bytes = (int64_t)(e->blk.bytes + (e->has_bow ? e->bow_blk.bytes : 0));
  return ORBFE_OK;
}

orbfe_status orbfe_kfstore_fetch(orbfe_kfstore* s, uint64_t id, orbfe_keypoint* kps, uint8_t* desc, double* depth, double* right_u, int32_t* cell_off,
                                 int32_t* cell_feat, uint32_t* nodes, int32_t* node_offsets, uint32_t* features) {
  const char* fn = "orbfe_kfstore_fetch";
  if (!s) return fail(nullptr, ORBFE_EBADARG, "%s: NULL argument", fn);
  std::shared_lock<std::shared_timed_mutex> lk(s->mu);
  const KfEntry* e = s->map.find(id);
  if (!e) return fail(nullptr, ORBFE_EBADARG, "%s: keyframe %llu is not in the store", fn, (unsigned long long)id);
  if ((nodes || node_offsets || features) && !e->has_bow) return fail(nullptr, ORBFE_EBADARG, "%s: keyframe %llu has no FeatureVector", fn, (unsigned long long)id);
  DeviceScope dev(s->device);
  HIP_TRY(nullptr, dev.err);
  // (every write to an entry was waited for before its insertion returned: plain blocking copies see it)
  const size_t N = (size_t)e->n;
  auto get = [&](void* dst, const void* src, size_t bytes) { return (!dst || !bytes) ? hipSuccess : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); };
  HIP_TRY(nullptr, get(kps, e->at<uint8_t>(e->o_kps), N * sizeof(orbfe_keypoint)));
  HIP_TRY(nullptr, get(desc, e->at<uint8_t>(e->o_desc), N * 32));
  HIP_TRY(nullptr, get(depth, e->at<uint8_t>(e->o_depth), N * 8));
  HIP_TRY(nullptr, get(right_u, e->at<uint8_t>(e->o_ru), N * 8));
  HIP_TRY(nullptr, get(cell_off, e->at<uint8_t>(e->o_coff), (e->ncells() + 1) * 4));
  HIP_TRY(nullptr, get(cell_feat, e->at<uint8_t>(e->o_cfeat), N * 4));
  if (e->has_bow) {
    HIP_TRY(nullptr, get(nodes, e->bow<uint8_t>(e->o_nodes), (size_t)e->n_nodes * 4));
    HIP_TRY(nullptr, get(node_offsets, e->bow<uint8_t>(e->o_offs), ((size_t)e->n_nodes + 1) * 4));
    HIP_TRY(nullptr, get(features, e->bow<uint8_t>(e->o_feat), (size_t)e->n_feat * 4));
  }
  return ORBFE_OK;
}

}  // extern "C"

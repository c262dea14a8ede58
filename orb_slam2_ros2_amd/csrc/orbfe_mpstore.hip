// orbfe_mpstore.hip -- host side of the map-point store (include/orbfe.h): pages and the page table, upsert, erase, fetch,
// size.  The bookkeeping is mpstore_index.h (no HIP in it), the two kernels k_mpstore.hip; the call that reads the store on a
// context's stream is orbfe_track_local_map_stored (orbfe_guided.hip).
#include "orbfe_mpstore.h"

namespace {

const int32_t kMaxIdsPerCall = 1 << 24;

// scratch and staging of one call on the store's stream (io_mu held)
orbfe_status io_reserve(orbfe_mpstore* s, size_t bytes) {
  if (s->io_bytes >= bytes) return ORBFE_OK;
  if (s->d_io) (void)hipFree(s->d_io);
  if (s->h_io) (void)hipHostFree(s->h_io);
  s->d_io = s->h_io = nullptr;
  s->io_bytes = 0;
  const size_t b = std::max<size_t>(bytes + bytes / 2, 1 << 18);
  HIP_TRY(nullptr, hipMalloc((void**)&s->d_io, b));
  HIP_TRY(nullptr, hipHostMalloc((void**)&s->h_io, b, hipHostMallocDefault));
  s->io_bytes = b;
  return ORBFE_OK;
}

// [ ids | the gather's word | one array per field the call names ]: an upsert uploads all of it -- a POS-only update 20 bytes per id,
// not 73 --, an erase only the ids; a fetch (every field) uploads `up` (the ids and the zeroed word) and downloads `down` (the word and
// the arrays).  A field the mask does not name has no array: the scatter does not read it.
struct MpCallLayout {
  size_t o_ids, o_absent, o_pos = 0, o_vd = 0, o_mx = 0, o_mn = 0, o_desc = 0, end;
  ScratchRegion up, down;
  MpCallLayout(size_t N, uint32_t fields) {
    ScratchLayout L;
    o_ids = L.take<uint64_t>(N), o_absent = L.take(8);
    up = {0, L.end()};
    if (fields & ORBFE_MP_POS) o_pos = L.take<float>(N * 3);
    if (fields & ORBFE_MP_NORMAL_DEPTH) o_vd = L.take<float>(N * 3), o_mx = L.take<float>(N), o_mn = L.take<float>(N);
    if (fields & ORBFE_MP_DESC) o_desc = L.take(N * 32);
    end = L.end();
    down = {o_absent, end};
  }
  MpArrays arrays(uint8_t* b) const { return {(float*)(b + o_pos), (float*)(b + o_vd), (float*)(b + o_mx), (float*)(b + o_mn), b + o_desc}; }
};

}  // namespace

extern "C" {

orbfe_status orbfe_mpstore_create(int32_t device_id, int32_t rows_per_page, int32_t max_pages, orbfe_mpstore** out) {
  // (the bounds keep what create itself allocates small: the page table and the host index are 8 + 24 bytes per POSSIBLE page)
  if (!out || rows_per_page < 0 || max_pages < 0 || rows_per_page > ORBFE_MP_MAX_ROWS_PER_PAGE || max_pages > ORBFE_MP_MAX_PAGES)
    return fail(nullptr, ORBFE_EBADARG, "orbfe_mpstore_create: bad arguments (rows_per_page 0..%d, max_pages 0..%d)", ORBFE_MP_MAX_ROWS_PER_PAGE,
                ORBFE_MP_MAX_PAGES);
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_mpstore_create: no HIP device (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, ORBFE_EBADARG, "orbfe_mpstore_create: device %d of %d", device_id, ndev);
  std::unique_ptr<orbfe_mpstore> s(new (std::nothrow) orbfe_mpstore());
  if (!s) return fail(nullptr, ORBFE_ENOMEM, "orbfe_mpstore_create: out of memory");
  s->device = device_id;
  s->idx = MpIndex(rows_per_page ? (uint32_t)rows_per_page : 16384u, max_pages ? (uint32_t)max_pages : 4096u);
  const size_t np = s->idx.max_pages();
  s->page_dev.assign(np, nullptr);
  DeviceScope dev(device_id);
  hipError_t err = dev.err;
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipMalloc((void**)&s->d_table, np * sizeof(uint8_t*));
  if (err == hipSuccess) err = hipMemset(s->d_table, 0, np * sizeof(uint8_t*));
  if (err != hipSuccess) {
    (void)hipGetLastError();
    orbfe_mpstore_destroy(s.release());
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_mpstore_create: %s on device %d", hipGetErrorString(err), device_id);
  }
  *out = s.release();
  return ORBFE_OK;
}

void orbfe_mpstore_destroy(orbfe_mpstore* s) {
  if (!s) return;
  DeviceScope dev(s->device);
  for (uint8_t* p : s->page_dev)
    if (p) (void)hipFree(p);
  if (s->d_table) (void)hipFree(s->d_table);
  if (s->d_io) (void)hipFree(s->d_io);
  if (s->h_io) (void)hipHostFree(s->h_io);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

orbfe_status orbfe_mpstore_upsert(orbfe_mpstore* s, int32_t n, const uint64_t* ids, uint32_t fields, const float* pos, const float* view_dir,
                                  const float* max_dist, const float* min_dist, const uint8_t* desc) {
  const char* fn = "orbfe_mpstore_upsert";
  if (!s || n < 0 || n > kMaxIdsPerCall || (n > 0 && !ids)) return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", fn);
  if (n > 0 && (((fields & ORBFE_MP_POS) && !pos) || ((fields & ORBFE_MP_NORMAL_DEPTH) && (!view_dir || !max_dist || !min_dist)) ||
                ((fields & ORBFE_MP_DESC) && !desc)))
    return fail(nullptr, ORBFE_EBADARG, "%s: an array the field mask %u names is NULL", fn, fields);
  const size_t N = (size_t)n;
  std::unique_lock<std::shared_timed_mutex> lk(s->mu);
  std::vector<uint32_t> new_pages;
  size_t at = 0;
  switch (s->idx.check_upsert(N, ids, fields, &new_pages, &at)) {
    case MpVerdict::ok: break;
    case MpVerdict::bad_mask: return fail(nullptr, ORBFE_EBADARG, "%s: field mask %u", fn, fields);
    case MpVerdict::duplicate: return fail(nullptr, ORBFE_EBADARG, "%s: map point %llu is listed twice", fn, (unsigned long long)ids[at]);
    case MpVerdict::partial_first:
      return fail(nullptr, ORBFE_EBADARG, "%s: map point %llu is not in the store and comes without all three fields", fn, (unsigned long long)ids[at]);
    case MpVerdict::capacity:
      return fail(nullptr, ORBFE_ECAPACITY, "%s: map point %llu is past the store's %llu rows", fn, (unsigned long long)ids[at],
                  (unsigned long long)s->idx.capacity());
  }
  if (n == 0) return ORBFE_OK;
  std::lock_guard<std::mutex> io_lk(s->io_mu);
  DeviceScope dev(s->device);
  HIP_TRY(nullptr, dev.err);
  const MpCallLayout L(N, fields);
  TRY(io_reserve(s, L.end));
  // new pages: presence cleared, then their pointers into the page table -- behind everything that ran before (exclusive lock: no reader
  // is in flight), in front of the scatter on the same stream
  for (uint32_t p : new_pages) {
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, s->idx.page_bytes()) != hipSuccess) {
      (void)hipGetLastError();
      return fail(nullptr, ORBFE_ENOMEM, "%s: cannot allocate a page of %zu bytes on device %d", fn, s->idx.page_bytes(), s->device);
    }
    s->page_dev[p] = d;
    s->idx.add_page(p);  // (an empty page stays if a later step fails: it holds no point)
    HIP_TRY(nullptr, hipMemsetAsync(d + s->idx.presence_offset(), 0, s->idx.rows_per_page(), s->stream));
    HIP_TRY(nullptr, hipMemcpyAsync(s->d_table + p, &s->page_dev[p], sizeof(uint8_t*), hipMemcpyHostToDevice, s->stream));
  }
  StagedIo io(s->d_io, s->h_io, s->stream);
  io.put(L.o_ids, ids, N * 8);
  if (fields & ORBFE_MP_POS) io.put(L.o_pos, pos, N * 12);
  if (fields & ORBFE_MP_NORMAL_DEPTH) {
    io.put(L.o_vd, view_dir, N * 12);
    io.put(L.o_mx, max_dist, N * 4);
    io.put(L.o_mn, min_dist, N * 4);
  }
  if (fields & ORBFE_MP_DESC) io.put(L.o_desc, desc, N * 32);
  HIP_TRY(nullptr, io.upload({0, L.end}));
  launch_mpstore_scatter(s->stream, s->table(), n, io.dev<uint64_t>(L.o_ids), fields, L.arrays(io.d), 1);
  HIP_TRY(nullptr, hipGetLastError());
  HIP_TRY(nullptr, io.wait());  // the rows are on the device: any later call on any stream of it sees them
  s->idx.commit_upsert(N, ids);
  return ORBFE_OK;
}

orbfe_status orbfe_mpstore_erase(orbfe_mpstore* s, int32_t n, const uint64_t* ids) {
  const char* fn = "orbfe_mpstore_erase";
  if (!s || n < 0 || n > kMaxIdsPerCall || (n > 0 && !ids)) return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", fn);
  std::unique_lock<std::shared_timed_mutex> lk(s->mu);
  // the ids the store holds, each once (the scatter writes every presence byte from one thread)
  std::vector<uint64_t> gone;
  for (int32_t i = 0; i < n; ++i)
    if (s->idx.has(ids[i])) gone.push_back(ids[i]);
  std::sort(gone.begin(), gone.end());
  gone.erase(std::unique(gone.begin(), gone.end()), gone.end());
  if (gone.empty()) return ORBFE_OK;
  std::lock_guard<std::mutex> io_lk(s->io_mu);
  DeviceScope dev(s->device);
  HIP_TRY(nullptr, dev.err);
  const MpCallLayout L(gone.size(), 0);
  TRY(io_reserve(s, L.end));
  StagedIo io(s->d_io, s->h_io, s->stream);
  io.put(L.o_ids, gone.data(), gone.size() * 8);
  HIP_TRY(nullptr, io.upload(L.up));
  launch_mpstore_scatter(s->stream, s->table(), (int)gone.size(), io.dev<uint64_t>(L.o_ids), 0, L.arrays(io.d), 0);
  HIP_TRY(nullptr, hipGetLastError());
  HIP_TRY(nullptr, io.wait());
  for (uint64_t id : gone) s->idx.erase(id);  // (after the device: a failed call leaves index and presence bytes agreeing)
  return ORBFE_OK;
}

orbfe_status orbfe_mpstore_fetch(orbfe_mpstore* s, int32_t n, const uint64_t* ids, float* pos, float* view_dir, float* max_dist, float* min_dist,
                                 uint8_t* desc) {
  const char* fn = "orbfe_mpstore_fetch";
  if (!s || n < 0 || n > kMaxIdsPerCall || (n > 0 && !ids)) return fail(nullptr, ORBFE_EBADARG, "%s: bad arguments", fn);
  std::shared_lock<std::shared_timed_mutex> lk(s->mu);
  for (int32_t i = 0; i < n; ++i)
    if (!s->idx.has(ids[i])) return fail(nullptr, ORBFE_EBADARG, "%s: map point %llu is not in the store", fn, (unsigned long long)ids[i]);
  if (n == 0) return ORBFE_OK;
  const size_t N = (size_t)n;
  std::lock_guard<std::mutex> io_lk(s->io_mu);
  DeviceScope dev(s->device);
  HIP_TRY(nullptr, dev.err);
  const MpCallLayout L(N, ORBFE_MP_ALL);
  TRY(io_reserve(s, L.end));
  StagedIo io(s->d_io, s->h_io, s->stream);
  io.put(L.o_ids, ids, N * 8);
  *io.host<uint32_t>(L.o_absent) = 0;
  HIP_TRY(nullptr, io.upload(L.up));
  launch_mpstore_gather(s->stream, s->table(), n, io.dev<uint64_t>(L.o_ids), L.arrays(io.d), nullptr, io.dev<uint32_t>(L.o_absent));
  HIP_TRY(nullptr, hipGetLastError());
  HIP_TRY(nullptr, io.fetch(L.down, L.down.begin));
  if (*(const uint32_t*)io.got(L.o_absent))  // (the host index and the device's presence bytes disagree)
    return fail(nullptr, ORBFE_EDEVICE, "%s: the device holds no row for an id the index lists", fn);
  io.get(pos, L.o_pos, N * 12);
  io.get(view_dir, L.o_vd, N * 12);
  io.get(max_dist, L.o_mx, N * 4);
  io.get(min_dist, L.o_mn, N * 4);
  io.get(desc, L.o_desc, N * 32);
  return ORBFE_OK;
}

orbfe_status orbfe_mpstore_size(orbfe_mpstore* s, int64_t* n_points, int64_t* bytes_used, int64_t* bytes_reserved) {
  if (!s) return fail(nullptr, ORBFE_EBADARG, "orbfe_mpstore_size: NULL argument");
  std::shared_lock<std::shared_timed_mutex> lk(s->mu);
  if (n_points) *n_points = (int64_t)s->idx.n_points();
  if (bytes_used) *bytes_used = (int64_t)(s->idx.n_points() * kMpRowBytes);
  if (bytes_reserved) *bytes_reserved = (int64_t)(s->idx.n_pages() * s->idx.page_bytes());
  return ORBFE_OK;
}

}  // extern "C"

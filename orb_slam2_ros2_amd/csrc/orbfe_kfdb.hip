// orbfe_kfdb.hip -- host side of the keyframe database (include/orbfe.h): the slot table and its mirror, the word / value pools, the
// query's one upload / two launches / one download, and the host-only group filter.  The kernels and the storage: k_kfdb.hip.
#include <unordered_map>
#include <unordered_set>

#include "orbfe_ctx.h"

void launch_kfdb_query(hipStream_t st, const uint32_t* qwords, const double* qvalues, int nq, const KfSlot* slots, int n_slots,
                       const uint32_t* wpool, const double* vpool, const uint32_t* ign, int n_ign, int32_t* counts, KfdbHdr* hdr,
                       int has_min, double min_score, KfdbRec* recs, uint32_t rec_cap);
void launch_kfdb_score_list(hipStream_t st, const uint32_t* qwords, const double* qvalues, int nq, const KfSlot* slots, const uint32_t* wpool,
                            const double* vpool, const uint32_t* list, int n, double* out);
void launch_kfdb_gather(hipStream_t st, const KfSlot* slots, const uint64_t* new_off, int n_slots, const uint32_t* w_old, const double* v_old,
                        uint32_t* w_new, double* v_new);
void launch_kfdb_scatter(hipStream_t st, const uint32_t* idx, const KfSlot* src, int n, KfSlot* slots);

struct orbfe_kfdb {
  std::mutex mu;  // KeyFrameDB::mMutex: add, erase, set_bad and query one at a time
  int device = 0;
  int32_t n_words = 0;
  hipStream_t stream = nullptr;  // add / erase / set_bad (a query runs on its context's stream)
  // the slot table (host mirror of d_slots) and the id of every slot
  std::vector<KfSlot> slots;
  std::vector<uint64_t> slot_id;
  std::vector<int32_t> free_slots;
  std::unordered_map<uint64_t, int32_t> slot_of;
  uint64_t pool_used = 0, pool_dead = 0, pool_cap = 0;  // words
  // device
  KfSlot* d_slots = nullptr;
  int32_t* d_counts = nullptr;
  size_t slot_cap = 0;
  uint32_t* d_words = nullptr;
  double* d_values = nullptr;
  uint8_t* d_io = nullptr;  // a call's upload and results
  size_t io_bytes = 0;
  uint8_t* h_io = nullptr;  // its page-locked staging
  size_t h_bytes = 0;
};

namespace {

orbfe_status kfail(orbfe_ctx* c, orbfe_status st, const char* what) { return fail(c, st, "%s", what); }

orbfe_status io_reserve(orbfe_kfdb* db, orbfe_ctx* c, size_t bytes) {
  if (db->io_bytes < bytes) {
    if (db->d_io) (void)hipFree(db->d_io);
    db->d_io = nullptr;
    db->io_bytes = 0;
    const size_t b = std::max<size_t>(bytes + bytes / 2, 1 << 16);
    HIP_TRY(c, hipMalloc((void**)&db->d_io, b));
    db->io_bytes = b;
  }
  if (db->h_bytes < bytes) {
    if (db->h_io) (void)hipHostFree(db->h_io);
    db->h_io = nullptr;
    db->h_bytes = 0;
    const size_t b = std::max<size_t>(bytes + bytes / 2, 1 << 16);
    HIP_TRY(c, hipHostMalloc((void**)&db->h_io, b, hipHostMallocDefault));
    db->h_bytes = b;
  }
  return ORBFE_OK;
}

// upload the slot records of `idx` (changed by add / erase / set_bad) and scatter them into d_slots
orbfe_status push_slots(orbfe_kfdb* db, const std::vector<uint32_t>& idx) {
  if (idx.empty()) return ORBFE_OK;
  const size_t n = idx.size(), o_src = align_up(n * 4, 256), total = o_src + n * sizeof(KfSlot);
  TRY(io_reserve(db, nullptr, total));
  std::memcpy(db->h_io, idx.data(), n * 4);
  for (size_t i = 0; i < n; ++i) std::memcpy(db->h_io + o_src + i * sizeof(KfSlot), &db->slots[idx[i]], sizeof(KfSlot));
  HIP_TRY(nullptr, hipMemcpyAsync(db->d_io, db->h_io, total, hipMemcpyHostToDevice, db->stream));
  launch_kfdb_scatter(db->stream, (const uint32_t*)db->d_io, (const KfSlot*)(db->d_io + o_src), (int)n, db->d_slots);
  HIP_TRY(nullptr, hipGetLastError());
  HIP_TRY(nullptr, hipStreamSynchronize(db->stream));
  return ORBFE_OK;
}

// room for `n` slots in the device table (the whole table is uploaded again when it moves)
orbfe_status reserve_slots(orbfe_kfdb* db, size_t n) {
  if (n <= db->slot_cap) return ORBFE_OK;
  size_t cap = std::max<size_t>(db->slot_cap * 2, 1024);
  while (cap < n) cap *= 2;
  if (cap > 0x7FFFFFFF) return fail(nullptr, ORBFE_ECAPACITY, "kfdb: more than 2^31 keyframe slots");
  KfSlot* s = nullptr;
  int32_t* cnt = nullptr;
  if (hipMalloc((void**)&s, cap * sizeof(KfSlot)) != hipSuccess || hipMalloc((void**)&cnt, cap * 4) != hipSuccess) {
    if (s) (void)hipFree(s);
    return fail(nullptr, ORBFE_ENOMEM, "kfdb: cannot allocate %zu keyframe slots on device %d", cap, db->device);
  }
  if (!db->slots.empty()) HIP_TRY(nullptr, hipMemcpy(s, db->slots.data(), db->slots.size() * sizeof(KfSlot), hipMemcpyHostToDevice));
  if (db->d_slots) (void)hipFree(db->d_slots);
  if (db->d_counts) (void)hipFree(db->d_counts);
  db->d_slots = s;
  db->d_counts = cnt;
  db->slot_cap = cap;
  return ORBFE_OK;
}

// room for `extra` more words at the end of the pools: when they are full, new pools of twice the live words (plus the extra) receive the
// live slots, packed (k_kfdb_gather); the space of erased and re-added keyframes is given back there
orbfe_status reserve_pool(orbfe_kfdb* db, uint64_t extra) {
  if (db->pool_used + extra <= db->pool_cap) return ORBFE_OK;
  const uint64_t live = db->pool_used - db->pool_dead;
  const uint64_t cap = std::max<uint64_t>(2 * (live + extra), 1 << 20);
  uint32_t* w = nullptr;
  double* v = nullptr;
  uint64_t* d_off = nullptr;
  auto drop = [&]() {
    for (void* p : {(void*)w, (void*)v, (void*)d_off})
      if (p) (void)hipFree(p);
  };
  if (hipMalloc((void**)&w, cap * 4) != hipSuccess || hipMalloc((void**)&v, cap * 8) != hipSuccess ||
      hipMalloc((void**)&d_off, std::max<size_t>(db->slots.size(), 1) * 8) != hipSuccess) {
    drop();
    return fail(nullptr, ORBFE_ENOMEM, "kfdb: cannot allocate pools of %llu words on device %d", (unsigned long long)cap, db->device);
  }
  std::vector<uint64_t> off(db->slots.size(), 0);
  uint64_t at = 0;
  for (size_t s = 0; s < db->slots.size(); ++s)
    if (db->slots[s].flags & KFDB_LIVE) {
      off[s] = at;
      at += db->slots[s].len;
    }
  if (!off.empty()) {
    if (hipMemcpy(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
      drop();
      return fail(nullptr, ORBFE_EDEVICE, "kfdb: upload of the pool offsets failed");
    }
    launch_kfdb_gather(db->stream, db->d_slots, d_off, (int)db->slots.size(), db->d_words, db->d_values, w, v);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(db->stream) != hipSuccess) {
      drop();
      return fail(nullptr, ORBFE_EDEVICE, "kfdb: pool compaction failed");
    }
  }
  (void)hipFree(d_off);
  d_off = nullptr;
  if (db->d_words) (void)hipFree(db->d_words);
  if (db->d_values) (void)hipFree(db->d_values);
  db->d_words = w;
  db->d_values = v;
  db->pool_cap = cap;
  db->pool_used = at;
  db->pool_dead = 0;
  for (size_t s = 0; s < db->slots.size(); ++s)
    if (db->slots[s].flags & KFDB_LIVE) db->slots[s].off = off[s];
  if (!db->slots.empty()) HIP_TRY(nullptr, hipMemcpy(db->d_slots, db->slots.data(), db->slots.size() * sizeof(KfSlot), hipMemcpyHostToDevice));
  return ORBFE_OK;
}

bool words_ok(const uint32_t* w, int64_t n, int32_t n_words) {
  for (int64_t i = 0; i < n; ++i)
    if (w[i] >= (uint32_t)n_words || (i > 0 && w[i] <= w[i - 1])) return false;
  return true;
}

// the query's checks, shared by query and score
orbfe_status check_query(orbfe_ctx* c, orbfe_kfdb* db, const orbfe_kfdb_query_in* q, const char* who) {
  if (!c || !db || !q || q->n_words < 0 || q->n_ignore < 0 || (q->n_words > 0 && (!q->words || !q->values)) || (q->n_ignore > 0 && !q->ignore))
    return fail(c, ORBFE_EBADARG, "%s: bad arguments", who);
  if (q->n_words > ORBFE_BOW_MAX_FEATURES) return fail(c, ORBFE_EBADARG, "%s: %d query words, at most %d", who, q->n_words, ORBFE_BOW_MAX_FEATURES);
  if (c->device != db->device) return fail(c, ORBFE_EBADARG, "%s: the context is on device %d, the database on device %d", who, c->device, db->device);
  if (!words_ok(q->words, q->n_words, db->n_words))
    return fail(c, ORBFE_EBADARG, "%s: query words must be strictly ascending and below %d", who, db->n_words);
  return ORBFE_OK;
}

}  // namespace

extern "C" {

orbfe_status orbfe_kfdb_create(int32_t device_id, int32_t n_words, orbfe_kfdb** out) {
  if (!out || n_words < 0) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_create: bad arguments");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, ORBFE_EDEVICE, "orbfe_kfdb_create: no HIP device (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_create: device %d of %d", device_id, ndev);
  std::unique_ptr<orbfe_kfdb> db(new (std::nothrow) orbfe_kfdb());
  if (!db) return fail(nullptr, ORBFE_ENOMEM, "orbfe_kfdb_create: out of memory");
  db->device = device_id;
  db->n_words = n_words;
  orbfe_status st = ORBFE_OK;
  DeviceScope dev(device_id);
  if (dev.err != hipSuccess || hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess)
    st = fail(nullptr, ORBFE_EDEVICE, "orbfe_kfdb_create: cannot create a stream on device %d", device_id);
  if (st == ORBFE_OK) st = reserve_slots(db.get(), 1024);
  if (st == ORBFE_OK) st = reserve_pool(db.get(), 0);
  if (st != ORBFE_OK) {
    orbfe_kfdb_destroy(db.release());
    return st;
  }
  *out = db.release();
  return ORBFE_OK;
}

void orbfe_kfdb_destroy(orbfe_kfdb* db) {
  if (!db) return;
  DeviceScope dev(db->device);
  for (void* p : {(void*)db->d_slots, (void*)db->d_counts, (void*)db->d_words, (void*)db->d_values, (void*)db->d_io})
    if (p) (void)hipFree(p);
  if (db->h_io) (void)hipHostFree(db->h_io);
  if (db->stream) (void)hipStreamDestroy(db->stream);
  delete db;
}

orbfe_status orbfe_kfdb_add(orbfe_kfdb* db, int32_t n_kf, const uint64_t* ids, const int64_t* offsets, const uint32_t* words, const double* values) {
  if (!db || n_kf < 0 || (n_kf > 0 && (!ids || !offsets))) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_add: bad arguments");
  if (n_kf == 0) return ORBFE_OK;
  if (offsets[0] != 0) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_add: offsets[0] must be 0");
  for (int32_t i = 0; i < n_kf; ++i) {
    const int64_t n = offsets[i + 1] - offsets[i];
    if (n < 0 || n > ORBFE_BOW_MAX_FEATURES)
      return fail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_add: keyframe %d has %lld words (0 .. %d)", i, (long long)n, ORBFE_BOW_MAX_FEATURES);
  }
  const int64_t total = offsets[n_kf];
  if (total > 0 && (!words || !values)) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_add: NULL words / values");
  for (int32_t i = 0; i < n_kf; ++i)
    if (!words_ok(words + offsets[i], offsets[i + 1] - offsets[i], db->n_words))
      return fail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_add: keyframe %d: words must be strictly ascending and below %d", i, db->n_words);
  std::lock_guard<std::mutex> lk(db->mu);
  {
    std::unordered_set<uint64_t> seen;
    for (int32_t i = 0; i < n_kf; ++i)
      if (!seen.insert(ids[i]).second) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_add: id %llu twice in one call", (unsigned long long)ids[i]);
  }
  // the keyframes to add (an id already present is left as it is: the reference's std::set)
  std::vector<int32_t> todo;
  uint64_t extra = 0;
  for (int32_t i = 0; i < n_kf; ++i)
    if (!db->slot_of.count(ids[i])) {
      todo.push_back(i);
      extra += (uint64_t)(offsets[i + 1] - offsets[i]);
    }
  if (todo.empty()) return ORBFE_OK;
  DeviceScope dev(db->device);
  HIP_TRY(nullptr, dev.err);
  const size_t reuse = std::min(todo.size(), db->free_slots.size());
  TRY(reserve_slots(db, db->slots.size() + (todo.size() - reuse)));
  TRY(reserve_pool(db, extra));
  // words / values of the new keyframes, packed, behind the pools' used part
  std::vector<uint32_t> w;
  std::vector<double> v;
  w.reserve(extra);
  v.reserve(extra);
  for (int32_t i : todo) {
    w.insert(w.end(), words + offsets[i], words + offsets[i + 1]);
    v.insert(v.end(), values + offsets[i], values + offsets[i + 1]);
  }
  if (extra) {
    HIP_TRY(nullptr, hipMemcpyAsync(db->d_words + db->pool_used, w.data(), extra * 4, hipMemcpyHostToDevice, db->stream));
    HIP_TRY(nullptr, hipMemcpyAsync(db->d_values + db->pool_used, v.data(), extra * 8, hipMemcpyHostToDevice, db->stream));
  }
  std::vector<uint32_t> changed;
  changed.reserve(todo.size());
  uint64_t at = db->pool_used;
  for (int32_t i : todo) {
    int32_t s;
    if (!db->free_slots.empty()) {
      s = db->free_slots.back();
      db->free_slots.pop_back();
    } else {
      s = (int32_t)db->slots.size();
      db->slots.push_back(KfSlot{0, 0, 0});
      db->slot_id.push_back(0);
    }
    const uint32_t len = (uint32_t)(offsets[i + 1] - offsets[i]);
    db->slots[(size_t)s] = KfSlot{at, len, KFDB_LIVE};
    db->slot_id[(size_t)s] = ids[i];
    db->slot_of[ids[i]] = s;
    at += len;
    changed.push_back((uint32_t)s);
  }
  db->pool_used = at;
  return push_slots(db, changed);  // (its synchronisation also covers the copies above: same stream)
}

orbfe_status orbfe_kfdb_set_bad(orbfe_kfdb* db, int32_t n, const uint64_t* ids, const uint8_t* flags) {
  if (!db || n < 0 || (n > 0 && (!ids || !flags))) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_set_bad: bad arguments");
  std::lock_guard<std::mutex> lk(db->mu);
  for (int32_t i = 0; i < n; ++i)
    if (!db->slot_of.count(ids[i])) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_set_bad: id %llu is not in the database", (unsigned long long)ids[i]);
  std::vector<uint32_t> changed;
  for (int32_t i = 0; i < n; ++i) {
    const int32_t s = db->slot_of[ids[i]];
    KfSlot& sl = db->slots[(size_t)s];
    const uint32_t f = flags[i] ? (sl.flags | KFDB_BAD) : (sl.flags & ~KFDB_BAD);
    if (f != sl.flags) {
      sl.flags = f;
      changed.push_back((uint32_t)s);
    }
  }
  if (changed.empty()) return ORBFE_OK;
  std::sort(changed.begin(), changed.end());
  changed.erase(std::unique(changed.begin(), changed.end()), changed.end());
  DeviceScope dev(db->device);
  HIP_TRY(nullptr, dev.err);
  return push_slots(db, changed);
}

orbfe_status orbfe_kfdb_erase(orbfe_kfdb* db, int32_t n, const uint64_t* ids) {
  if (!db || n < 0 || (n > 0 && !ids)) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_erase: bad arguments");
  std::lock_guard<std::mutex> lk(db->mu);
  std::vector<uint32_t> changed;
  for (int32_t i = 0; i < n; ++i) {
    const auto it = db->slot_of.find(ids[i]);
    if (it == db->slot_of.end()) continue;
    const int32_t s = it->second;
    db->pool_dead += db->slots[(size_t)s].len;
    db->slots[(size_t)s] = KfSlot{0, 0, 0};
    db->slot_of.erase(it);
    db->free_slots.push_back(s);
    changed.push_back((uint32_t)s);
  }
  if (changed.empty()) return ORBFE_OK;
  DeviceScope dev(db->device);
  HIP_TRY(nullptr, dev.err);
  return push_slots(db, changed);
}

orbfe_status orbfe_kfdb_size(orbfe_kfdb* db, int64_t* out) {
  if (!db || !out) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_size: NULL argument");
  std::lock_guard<std::mutex> lk(db->mu);
  *out = (int64_t)db->slot_of.size();
  return ORBFE_OK;
}

orbfe_status orbfe_kfdb_query(orbfe_ctx* c, orbfe_kfdb* db, const orbfe_kfdb_query_in* q, uint64_t* out_ids, int32_t* out_counts,
                              double* out_scores, int64_t cap, int64_t* n_out) {
  ApiLock api_lk(c);
  TRY(check_query(c, db, q, "kfdb_query"));
  if (!n_out || cap < 0) return fail(c, ORBFE_EBADARG, "kfdb_query: bad arguments (cap %lld)", (long long)cap);
  std::lock_guard<std::mutex> lk(db->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  *n_out = 0;
  const int n_slots = (int)db->slots.size();
  // the ignored ids' slots, sorted (ids not in the database are skipped)
  std::vector<uint32_t> ign;
  ign.reserve((size_t)q->n_ignore);
  for (int32_t i = 0; i < q->n_ignore; ++i) {
    const auto it = db->slot_of.find(q->ignore[i]);
    if (it != db->slot_of.end()) ign.push_back((uint32_t)it->second);
  }
  std::sort(ign.begin(), ign.end());
  ign.erase(std::unique(ign.begin(), ign.end()), ign.end());
  // one upload: words | values | ignored slots | header (zeros); one download: header | records
  const size_t nq = (size_t)q->n_words;
  const uint32_t rec_cap = (uint32_t)std::min<int64_t>(cap, (int64_t)db->slot_of.size());
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_w = L.open(up).take<uint32_t>(nq), o_v = L.take<double>(nq), o_i = L.take<uint32_t>(ign.size()),
               o_h = L.open(down).take(sizeof(KfdbHdr)),  // (goes up as zeros, comes down with the counts)
               o_rec = L.close(up).take<KfdbRec>(rec_cap);
  L.close(down);
  TRY(io_reserve(db, c, L.end()));
  StagedIo io(db->d_io, db->h_io, c->stream);
  io.put(o_w, q->words, nq * 4);
  io.put(o_v, q->values, nq * 8);
  io.put(o_i, ign.data(), ign.size() * 4);
  std::memset(io.host<uint8_t>(o_h), 0, sizeof(KfdbHdr));
  HIP_TRY(c, io.upload(up));
  launch_kfdb_query(c->stream, io.dev<uint32_t>(o_w), io.dev<double>(o_v), (int)nq, db->d_slots, n_slots, db->d_words, db->d_values,
                    io.dev<uint32_t>(o_i), (int)ign.size(), db->d_counts, io.dev<KfdbHdr>(o_h), q->min_score ? 1 : 0,
                    q->min_score ? *q->min_score : 0.0, io.dev<KfdbRec>(o_rec), rec_cap);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down, down.begin));
  KfdbHdr hd;
  io.get(&hd, o_h, sizeof hd);
  *n_out = (int64_t)hd.n_out;
  if ((int64_t)hd.n_out > cap) return fail(c, ORBFE_ECAPACITY, "kfdb_query: %u survivors, room for %lld", hd.n_out, (long long)cap);
  if (hd.n_out > rec_cap) return fail(c, ORBFE_EDEVICE, "kfdb_query: corrupt survivor count %u", hd.n_out);
  std::vector<KfdbRec> r(hd.n_out);
  io.get(r.data(), o_rec, (size_t)hd.n_out * sizeof(KfdbRec));
  for (const KfdbRec& x : r)
    if (x.slot >= (uint32_t)n_slots || !(db->slots[x.slot].flags & KFDB_LIVE)) return fail(c, ORBFE_EDEVICE, "kfdb_query: corrupt record (slot %u)", x.slot);
  std::sort(r.begin(), r.end(), [&](const KfdbRec& a, const KfdbRec& b) { return db->slot_id[a.slot] < db->slot_id[b.slot]; });
  for (size_t i = 0; i < r.size(); ++i) {
    if (out_ids) out_ids[i] = db->slot_id[r[i].slot];
    if (out_counts) out_counts[i] = r[i].count;
    if (out_scores) out_scores[i] = r[i].score;
  }
  return ORBFE_OK;
}

orbfe_status orbfe_kfdb_score(orbfe_ctx* c, orbfe_kfdb* db, const orbfe_kfdb_query_in* q, const uint64_t* ids, int32_t n, double* scores) {
  ApiLock api_lk(c);
  TRY(check_query(c, db, q, "kfdb_score"));
  if (n < 0 || (n > 0 && (!ids || !scores))) return fail(c, ORBFE_EBADARG, "kfdb_score: bad arguments");
  std::lock_guard<std::mutex> lk(db->mu);
  std::vector<uint32_t> list((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    const auto it = db->slot_of.find(ids[i]);
    if (it == db->slot_of.end()) return fail(c, ORBFE_EBADARG, "kfdb_score: id %llu is not in the database", (unsigned long long)ids[i]);
    list[(size_t)i] = (uint32_t)it->second;
  }
  if (n == 0) return ORBFE_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t nq = (size_t)q->n_words;
  ScratchLayout L;
  ScratchRegion up, down;
  const size_t o_w = L.open(up).take<uint32_t>(nq), o_v = L.take<double>(nq), o_l = L.take<uint32_t>((size_t)n),
               o_out = L.close(up).open(down).take<double>((size_t)n);
  L.close(down);
  TRY(io_reserve(db, c, L.end()));
  StagedIo io(db->d_io, db->h_io, c->stream);
  io.put(o_w, q->words, nq * 4);
  io.put(o_v, q->values, nq * 8);
  io.put(o_l, list.data(), (size_t)n * 4);
  HIP_TRY(c, io.upload(up));
  launch_kfdb_score_list(c->stream, io.dev<uint32_t>(o_w), io.dev<double>(o_v), (int)nq, db->d_slots, db->d_words, db->d_values,
                         io.dev<uint32_t>(o_l), n, io.dev<double>(o_out));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, io.fetch(down.upto(o_out + (size_t)n * 8), down.begin));
  io.get(scores, o_out, (size_t)n * 8);
  return ORBFE_OK;
}

orbfe_status orbfe_kfdb_group_filter(int64_t n, const uint64_t* ids, const double* scores, const int64_t* conn_offsets, const uint64_t* conn_ids,
                                     uint64_t* out, int64_t* n_out) {
  if (n < 0 || !n_out || (n > 0 && (!ids || !scores || !conn_offsets || !out))) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_group_filter: bad arguments");
  *n_out = 0;
  if (n == 0) return ORBFE_OK;
  if (conn_offsets[0] != 0) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_group_filter: conn_offsets[0] must be 0");
  for (int64_t i = 0; i < n; ++i)
    if (conn_offsets[i + 1] < conn_offsets[i]) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_group_filter: conn_offsets must not decrease");
  if (conn_offsets[n] > 0 && !conn_ids) return kfail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_group_filter: NULL conn_ids");
  std::unordered_map<uint64_t, int64_t> at;  // survivor id -> its index (the reference's kfAndWordNum.find)
  at.reserve((size_t)n * 2);
  for (int64_t i = 0; i < n; ++i)
    if (!at.emplace(ids[i], i).second) return fail(nullptr, ORBFE_EBADARG, "orbfe_kfdb_group_filter: id %llu twice", (unsigned long long)ids[i]);
  std::vector<double> acc((size_t)n);
  std::vector<uint64_t> best((size_t)n);
  double best_acc = 0;
  for (int64_t i = 0; i < n; ++i) {
    uint64_t b = ids[i];
    double b_score = scores[i];
    double a = 0;  // Group::mfAccScore has no initialiser in the reference: here it starts at 0
    a += b_score;
    for (int64_t k = conn_offsets[i]; k < conn_offsets[i + 1]; ++k) {
      const auto it = at.find(conn_ids[k]);
      if (it == at.end()) continue;
      const double s = scores[it->second];
      a += s;
      if (s > b_score) {
        b_score = s;
        b = conn_ids[k];
      }
    }
    acc[(size_t)i] = a;
    best[(size_t)i] = b;
    if (a > best_acc) best_acc = a;
  }
  const double th2 = best_acc * 0.75;
  std::vector<uint64_t> o;
  for (int64_t i = 0; i < n; ++i)
    if (acc[(size_t)i] > th2) o.push_back(best[(size_t)i]);
  std::sort(o.begin(), o.end());
  o.erase(std::unique(o.begin(), o.end()), o.end());
  std::copy(o.begin(), o.end(), out);
  *n_out = (int64_t)o.size();
  return ORBFE_OK;
}

}  // extern "C"

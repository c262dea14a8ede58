// orbfe_mpstore.h -- the map-point store's record (include/orbfe.h) as its host side (orbfe_mpstore.hip) and the call that
// reads it (orbfe_track_local_map_stored, orbfe_guided.hip) see it.
#pragma once
#include <mutex>
#include <shared_mutex>

#include "mpstore_index.h"
#include "orbfe_ctx.h"

static_assert(MP_FIELD_POS == ORBFE_MP_POS && MP_FIELD_NORMAL_DEPTH == ORBFE_MP_NORMAL_DEPTH && MP_FIELD_DESC == ORBFE_MP_DESC &&
                  MP_FIELD_ALL == ORBFE_MP_ALL,
              "mpstore_index.h and orbfe.h name the same fields");

// The device side of the paged index: table[page] is the page's address (nullptr: no such page), its rows first, then one presence byte
// per row.  Passed to the kernels by value.
struct MpTable {
  uint8_t* const* table;
  uint32_t rows_per_page, max_pages;
};
// the row of `id` and its presence byte; nullptr: the id is past the capacity or its page does not exist (k_mpstore.hip's kernels, and
// k_motion.hip's prepare kernel, which reads a position where it lies)
__device__ inline uint8_t* mp_row(const MpTable& t, uint64_t id, uint8_t** presence) {
  if (id >= (uint64_t)t.rows_per_page * t.max_pages) return nullptr;
  uint32_t page, row;
  if ((id >> 32) == 0) {  // (the usual case: a 32-bit division)
    page = (uint32_t)id / t.rows_per_page, row = (uint32_t)id % t.rows_per_page;
  } else {
    page = (uint32_t)(id / t.rows_per_page), row = (uint32_t)(id % t.rows_per_page);
  }
  uint8_t* base = t.table[page];
  if (!base) return nullptr;
  *presence = base + (size_t)t.rows_per_page * kMpRowBytes + row;
  return base + (size_t)row * kMpRowBytes;
}

// The arrays a gather fills / a scatter reads, one entry per listed id, in orbfe_track_input's layout.
struct MpArrays {
  float *pos, *view_dir, *max_dist, *min_dist;
  uint8_t* desc;
};

struct orbfe_mpstore {
  std::shared_timed_mutex mu;  // upsert / erase exclusive; fetch / size / orbfe_track_local_map_stored shared
  std::mutex io_mu;            // the store's own stream, scratch and staging: one upsert, erase or fetch at a time
  int device = 0;
  hipStream_t stream = nullptr;
  MpIndex idx;
  std::vector<uint8_t*> page_dev;  // device address of page p (nullptr: none); d_table is its copy on the device
  uint8_t** d_table = nullptr;
  uint8_t *d_io = nullptr, *h_io = nullptr;  // scratch of a call and its page-locked staging
  size_t io_bytes = 0;
  MpTable table() const { return {d_table, idx.rows_per_page(), idx.max_pages()}; }
};

// the context may use the store: same device
static inline orbfe_status mpstore_check_ctx(orbfe_ctx* c, const orbfe_mpstore* s, const char* who) {
  if (c->device != s->device) return fail(c, ORBFE_EBADARG, "%s: the context is on device %d, the map-point store on device %d", who, c->device, s->device);
  return ORBFE_OK;
}

// k_mpstore.hip.  gather: rows of ids[0..n) into `out`; an id without a row: a zero row, flags[i] = 0 (flags nullptr: none kept) and
// *absent = 1.  scatter: the fields of `in` named by `fields` into the rows of ids[0..n) and `present` into their presence bytes; every
// id has a page and appears once (the host has checked both).
void launch_mpstore_gather(hipStream_t st, MpTable t, int n, const uint64_t* ids, MpArrays out, uint8_t* flags, uint32_t* absent);
void launch_mpstore_scatter(hipStream_t st, MpTable t, int n, const uint64_t* ids, uint32_t fields, MpArrays in, uint8_t present);
